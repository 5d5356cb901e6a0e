"""The argument contract of the six triples of native training entry points, from the table in tests/train_abi.py: every
symbol is exported, listed in ``_native.SYMBOLS`` with the argument types of its row and declared in the header with the
row's argument names, and every entry point refuses the same family of calls before anything is launched.  No GPU."""
import ctypes as C
import os
import re

import pytest

from occlusionenv_amd import _native as nat
from tests import train_abi as T

P = C.c_void_p(4096)  # never dereferenced: every call below that takes it is rejected before a launch
BIG = 1 << 40
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "occlusionenv_amd.h")
CTYPES = {"cfg": C.POINTER(nat.OccEncoderConfig), "ptr": C.c_void_p, "n_env": C.c_int, "bytes": C.c_size_t, "stream": C.c_void_p,
          "out": C.POINTER(C.c_size_t)}
IDS = [T.TRIPLES[name][role][0] for name, role in T.ENTRY_POINTS]


def _cfg(fields):
    cfg = nat.OccEncoderConfig()
    cfg.img, cfg.dilation, cfg.residual, cfg.separable = fields
    return cfg


def _values(args, fields, n=2):
    """A call's arguments with nothing wrong but the config: the pointers present and aligned, the byte sizes huge."""
    fill = {"cfg": lambda: C.byref(_cfg(fields)), "ptr": lambda: P, "n_env": lambda: n, "bytes": lambda: BIG,
            "stream": lambda: None, "out": lambda: C.byref(C.c_size_t())}
    return [fill[a[0]]() for a in args]


def _query(triple, fields, n):
    ws, sc = C.c_size_t(), C.c_size_t()
    rc = getattr(nat.load(), triple["query"][0])(C.byref(_cfg(fields)), n, C.byref(ws), C.byref(sc))
    return rc, (int(ws.value), int(sc.value))


def _pairs(rows):
    """(config, n_env) of rows that are a config (n_env = 2) or already such a pair."""
    return [row if isinstance(row[0], tuple) else (row, 2) for row in rows]


def _refused_calls(triple, role):
    """-> [(what, argument list)]: the family of calls the entry point has to refuse."""
    args = triple[role][1]
    calls = []
    for fields, n in _pairs(triple["refuses"]) + (_pairs(triple["query_refuses"]) if role == "query" else []):
        calls.append((f"config {fields} n_env {n}", _values(args, fields, n)))
    for good in triple["accepts"]:
        need = _query(triple, good, 2)[1]

        def one(i, value):
            changed = _values(args, good)
            changed[i] = value
            return changed

        for i, a in enumerate(args):
            if a[0] in ("cfg", "ptr", "out"):
                calls.append((f"{good}: {a[1]} null", one(i, None)))
            if a[0] == "n_env":
                calls += [(f"{good}: n_env {n}", one(i, n)) for n in (0, 65536)]
            if a[0] == "bytes":
                calls.append((f"{good}: {a[1]} one short", one(i, need[a[2]] - 1)))
            if a[0] == "ptr" and a[2] is not None:
                calls.append((f"{good}: {a[1]} not {a[2]}-byte aligned", one(i, C.c_void_p(4096 + a[2] // 2))))
    return calls


def test_abi_stays_12():
    assert nat.load().occ_abi_version() == 12 == nat.ABI_VERSION


@pytest.mark.parametrize("name,role", T.ENTRY_POINTS, ids=IDS)
def test_symbol_is_exported_listed_and_declared(name, role):
    symbol, args = T.TRIPLES[name][role]
    assert hasattr(C.CDLL(nat.LIB_PATH), symbol)
    # equal rows are equal signatures: the separable entry points take the dense ones' arguments, the batch-statistics
    # forward the joint forward's with bn_stats in front of the stream
    assert nat.SYMBOLS[symbol] == (C.c_int, [CTYPES[a[0]] for a in args])
    header = open(HEADER).read()
    assert f"int {symbol}(" in header
    declared = re.search(r"\bint " + symbol + r"\(([^)]*)\);", header).group(1)
    assert [p.split()[-1].lstrip("*") for p in declared.split(",")] == [a[1] for a in args]


def test_rows_the_forms_share():
    """What the former per-path tests asserted as equal signatures, on the table."""
    t = T.TRIPLES
    for role in T.ROLES:
        assert t["sep_fullnet"][role][1] == t["fullnet"][role][1] and t["sep_encoder"][role][1] == t["encoder"][role][1]
    assert t["fullnet_bn"]["query"][1] == t["fullnet"]["query"][1]
    assert t["fullnet_bn"]["backward"][1] == t["fullnet"]["backward"][1]
    fwd, bn = t["fullnet"]["forward"][1], t["fullnet_bn"]["forward"][1]
    assert [a[:2] for a in bn] == [a[:2] for a in fwd[:-1]] + [("ptr", "bn_stats")] + [fwd[-1][:2]]


@pytest.mark.parametrize("name,role", T.ENTRY_POINTS, ids=IDS)
def test_refused_before_a_launch(name, role):
    triple = T.TRIPLES[name]
    fn = getattr(nat.load(), triple[role][0])
    calls = _refused_calls(triple, role)
    assert len(calls) >= len(triple["refuses"]) + 5 * len(triple["accepts"])
    for what, values in calls:
        assert fn(*values) == 1, what


@pytest.mark.parametrize("name", list(T.TRIPLES))
def test_query_accepts_what_is_supported(name):
    triple = T.TRIPLES[name]
    for fields, n in [(good, 2) for good in triple["accepts"]] + list(triple["query_accepts"]):
        rc, (ws, sc) = _query(triple, fields, n)
        assert rc == 0 and ws > 0 and sc > 0, (fields, n)
