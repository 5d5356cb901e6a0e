"""The masked forwards of the C ABI (occ_encoder_forward_masked, occ_segment_forward_masked) on a GPU-less host: declared in
the header with the unmasked call's arguments plus ``skip`` in front of ``stream``, bound with as many arguments, exported
by the built library, rejected with the unmasked call's argument checks, and additive: OCC_ABI_VERSION is still 12."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "occlusionenv_amd.h")
PAIRS = [("occ_encoder_forward", "occ_encoder_forward_masked"), ("occ_segment_forward", "occ_segment_forward_masked")]


def _params(name):
    """The parameter declarations of ``name`` in the header (comments removed)."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in the header"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


@pytest.mark.parametrize("plain,masked", PAIRS)
def test_header_declares_the_masked_call(plain, masked):
    a, b = _params(plain), _params(masked)
    assert b[:-2] == a[:-1], "the masked call takes the unmasked call's arguments in the same order"
    assert b[-2] == "const int32_t* skip" and b[-1] == a[-1] == "void* stream"


@pytest.mark.parametrize("plain,masked", PAIRS)
def test_binding_and_library_have_the_masked_call(plain, masked):
    from occlusionenv_amd import _native as nat

    assert masked in nat.SYMBOLS
    res, args = nat.SYMBOLS[masked]
    assert res is ctypes.c_int and len(args) == len(_params(masked)) == len(nat.SYMBOLS[plain][1]) + 1
    assert args[:-2] == nat.SYMBOLS[plain][1][:-1] and args[-2:] == [ctypes.c_void_p, ctypes.c_void_p]
    assert hasattr(ctypes.CDLL(nat.LIB_PATH), masked), f"{masked} is not exported by the built library"


def test_abi_version_is_still_12():
    from occlusionenv_amd import _native as nat

    src = open(HEADER).read()
    assert int(re.search(r"#define\s+OCC_ABI_VERSION\s+(\d+)", src).group(1)) == 12
    assert nat.ABI_VERSION == 12 and nat.load().occ_abi_version() == 12


def test_masked_calls_keep_the_argument_checks():
    """Bad arguments are answered with OCC_ERR_ARG (1) before any launch, with or without a mask: no GPU is needed."""
    from occlusionenv_amd import _native as nat

    lib = nat.load()
    p = ctypes.c_void_p(16)
    cfg = ctypes.byref(nat.OccEncoderConfig(64, 2, 1, 1))
    for skip in (None, p):
        assert lib.occ_encoder_forward_masked(cfg, p, p, 1, p, 0, p, skip, None) == 1  # ws too small
        assert lib.occ_encoder_forward_masked(None, p, p, 1, p, 1 << 30, p, skip, None) == 1
        assert lib.occ_encoder_forward_masked(cfg, p, p, 0, p, 1 << 30, p, skip, None) == 1
        assert lib.occ_segment_forward_masked(cfg, p, p, p, 1, p, 0, p, p, None, None, skip, None) == 1  # ws too small
        assert lib.occ_segment_forward_masked(cfg, p, p, p, 1, p, 1 << 30, p, None, None, None, skip, None) == 1  # no prob
        assert lib.occ_segment_forward_masked(cfg, p, p, p, 1, p, 1 << 30, p, ctypes.c_void_p(20), None, None, skip, None) == 1


def test_plain_callable_encoder_is_called_as_before():
    """``BatchedPPO(encoder=...)`` takes any callable obs -> features: such an encoder never sees ``skip`` / ``out``; every
    row is computed and the contract is honoured afterwards.  Only an encoder that says ``takes_skip_mask`` gets them."""
    import torch

    from occlusionenv_amd import ppo
    from occlusionenv_amd.encoder import FrozenEncoder

    assert FrozenEncoder.takes_skip_mask is True
    n = 5
    w = torch.randn(4 * 8 * 8, 256, generator=torch.Generator().manual_seed(0))
    calls = []

    def plain(o):  # one positional argument, as the encoders of tests/test_ppo.py
        calls.append(o.shape[0])
        return o.reshape(o.shape[0], -1) @ w

    agent = ppo.BatchedPPO(device="cpu", seed=0, encoder=plain)
    obs = torch.randn(n, 4, 8, 8, generator=torch.Generator().manual_seed(1))
    ref = agent.features(obs)
    mask = torch.tensor([0, 1, 0, 1, 1], dtype=torch.int32)
    holed = obs.clone()
    holed[mask != 0] = float("nan")
    sentinel = torch.full((n, 256), 0x7FC5A5A5, dtype=torch.int32).view(torch.float32)
    for m in (mask, mask.bool()):
        out = sentinel.clone()
        got = agent.features(holed, skip=m, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(out.view(torch.int32)[mask != 0], sentinel.view(torch.int32)[mask != 0])
        assert torch.equal(out[mask == 0], ref[mask == 0])
        fresh = agent.features(holed, skip=m)
        assert bool((fresh.view(torch.int32)[mask != 0] == 0).all()) and torch.equal(fresh[mask == 0], ref[mask == 0])
    out = sentinel.clone()
    assert torch.equal(agent.features(obs, out=out), ref) and torch.equal(out, ref)
    assert calls == [n] * 6
    gen = torch.Generator().manual_seed(3)
    _f0, a0, _lp0 = agent.select_action(obs, gen)
    state = gen.get_state()
    gen.manual_seed(3)
    f1, a1, _lp1 = agent.select_action(holed, gen, skip=mask)
    assert torch.equal(gen.get_state(), state) and torch.equal(a1[mask == 0], a0[mask == 0]) and bool(torch.isfinite(a1).all())
    for bad in (dict(skip=mask.long()), dict(skip=mask[:-1]), dict(skip=mask, out=torch.empty(n, 255)), dict(out=torch.empty(256, n).t())):
        with pytest.raises(ValueError):
            agent.features(obs, **bad)

    class Masking:  # an encoder that declares the mask gets it handed on
        takes_skip_mask = True

        def __call__(self, o, skip=None, out=None):
            self.seen = (skip, out)
            return plain(o)

    enc = Masking()
    ppo.BatchedPPO(device="cpu", seed=0, encoder=enc).features(obs, skip=mask, out=sentinel.clone())
    assert enc.seen[0] is mask and enc.seen[1] is not None
