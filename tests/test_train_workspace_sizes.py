"""The five training workspace queries against recorded answers.  The encoder's and the joint step's sizes are computed by
one piece of host code for the dense and the separable form (enc_train_ws_layout and full_train_ws_layout,
csrc/occ_encoder_bwd.hpp and csrc/occ_fullnet_bwd.hpp); tests/golden/train_workspace_sizes.json holds what each query
answered before that code was shared (the library of the commit before, asked at img 32 / 96 / 256, n 1 / 3 / 129 and every
dilation, residual and separable value the query accepts).  A caller that sized its buffers then must find them large
enough and no larger now: every pair is equal.  The queries launch nothing.  No GPU."""
import ctypes as C
import json
import os

from occlusionenv_amd import _native as nat

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_workspace_sizes.json")
QUERIES = ("occ_segment_train_workspace_query", "occ_encoder_train_workspace_query", "occ_sep_encoder_train_workspace_query",
           "occ_fullnet_train_workspace_query", "occ_sep_fullnet_train_workspace_query")


def test_every_query_answers_what_it_answered_before():
    lib = nat.load()
    with open(GOLDEN) as f:
        records = json.load(f)
    # 9 shapes x the forms a query accepts: the decoder's takes all 8, a dense one 2 (residual), a separable one 4
    assert len(records) == 9 * (8 + 2 + 4 + 2 + 4)
    assert {r["query"] for r in records} == set(QUERIES)
    assert {(r["img"], r["n"]) for r in records} == {(s, n) for s in (32, 96, 256) for n in (1, 3, 129)}
    for r in records:
        cfg = nat.OccEncoderConfig()
        cfg.img, cfg.dilation, cfg.residual, cfg.separable = r["img"], r["dilation"], r["residual"], r["separable"]
        ws, sc = C.c_size_t(), C.c_size_t()
        assert getattr(lib, r["query"])(C.byref(cfg), r["n"], C.byref(ws), C.byref(sc)) == 0, r
        assert (int(ws.value), int(sc.value)) == (r["ws_bytes"], r["scratch_bytes"]), r
