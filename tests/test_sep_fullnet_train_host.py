"""Host-side checks of the joint training path of the separable network (csrc/occ_fullnet_bwd.hpp,
occlusionenv_amd/sepfullnet.py): the workspace query is the restated layout, the two parts' packed layouts round-trip from
the whole checkpoint, the separable joint f64 model of tests/train_model.py is the inference model of
tests/segmenter_model.py and its joint gradient the sum of its two losses' gradients, the split cases of the GPU test reach
what they claim, and every GPU case keeps its gate band small.  The argument contract of the three entry points is checked
from the table of tests/train_abi.py by tests/test_train_abi_host.py.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from occlusionenv_amd import _native as nat
from tests import decoder_split_model as dsm
from tests import segmenter_model
from tests import train_layout as tl
from tests import train_model as m

BAND_CAP = 0.005
JOINT = m.Net("ppo", True, 2, True, True)  # the sizes and the keys do not depend on the dilation or the residual
DENSE_JOINT = m.Net("ppo", False, 1, True, True)


def _cfg(img=64, dilation=2, residual=1, separable=1):
    cfg = nat.OccEncoderConfig()
    cfg.img, cfg.dilation, cfg.residual, cfg.separable = img, dilation, residual, separable
    return cfg


def _query(lib, img, n, **kw):
    ws, sc = C.c_size_t(), C.c_size_t()
    rc = lib.occ_sep_fullnet_train_workspace_query(C.byref(_cfg(img, **kw)), n, C.byref(ws), C.byref(sc))
    return rc, int(ws.value), int(sc.value)


def test_workspace_query_is_the_restated_layout():
    lib = nat.load()
    pairs = {(s, n) for _w, _d, _r, s, n in m.SEP_JOINT_CASES} | {(64, 4), (64, 1), (256, 128), (512, 64), (1024, 1)}
    assert {(32, 2), (64, 3), (96, 2), (64, 130), (96, 65)} <= pairs
    for img, n in sorted(pairs):
        for d, residual in ((2, 1), (1, 1), (2, 0)):
            rc, ws_b, sc_b = _query(lib, img, n, dilation=d, residual=residual)
            assert rc == 0
            assert ws_b == tl.ws_bytes(JOINT, img, n) == tl.ws_bytes(DENSE_JOINT, img, n), (img, n)
            assert sc_b == tl.scratch_bytes(JOINT, img, n), (img, n)
            assert ws_b % 256 == 0 and sc_b % 256 == 0
        # the workspace is the dense joint one; the scratch the larger of the two single passes'
        f_ws, f_sc = C.c_size_t(), C.c_size_t()
        dense = _cfg(img, dilation=1, separable=0)
        assert lib.occ_fullnet_train_workspace_query(C.byref(dense), n, C.byref(f_ws), C.byref(f_sc)) == 0
        assert ws_b == int(f_ws.value)
        e_ws, e_sc, d_ws, d_sc = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        assert lib.occ_sep_encoder_train_workspace_query(C.byref(_cfg(img)), n, C.byref(e_ws), C.byref(e_sc)) == 0
        assert lib.occ_segment_train_workspace_query(C.byref(_cfg(img)), n, C.byref(d_ws), C.byref(d_sc)) == 0
        assert int(e_ws.value) == tl.encoder_ws_bytes(img, n)
        assert sc_b == max(int(e_sc.value), int(d_sc.value))
        assert ws_b < int(e_ws.value) + int(d_ws.value)  # one encoder pass, 0.94 kept d skip buffers


@pytest.mark.parametrize("weights", ["golden", "seeded"])
def test_pack_round_trips_from_a_whole_checkpoint(weights):
    """Folding and packing the tensors ``TrainableSeparableFullNetwork`` holds, part by part, gives the buffers
    ``FrozenEncoder`` packs from the same checkpoint, and unpacking gives the tensors back: bitwise."""
    from occlusionenv_amd.encoder import DECODER_KEYS, pack_decoder, pack_state_dict
    from occlusionenv_amd.nettrain import decoder_part, fold_bn_vectors, sep_encoder_part

    sd = m.joint_state_dict(weights)
    assert set(m.param_keys(JOINT, head=True)) <= set(sd)
    assert len(m.enc_keys(JOINT)) == 11 * 6 + 5 * 4 and len(m.dec_keys(JOINT)) == 22
    separable, want_enc, _off = pack_state_dict(sd, "encoder.")
    assert separable
    want = [want_enc, pack_decoder(sd, *DECODER_KEYS["ppo"])]
    parts = [sep_encoder_part("ppo"), decoder_part("ppo")]
    assert list(parts[0].stems) == ["encoder." + stem for stem, *_ in m.layers(True)]
    for part, buf in zip(parts, want):
        folded = []
        for stem, leaves in zip(part.stems, part.layer_leaves()):
            scale, shift, _ = fold_bn_vectors(sd[stem + "bn.weight"], sd[stem + "bn.bias"], sd[stem + "bn.running_mean"],
                                              sd[stem + "bn.running_var"])
            folded.append(tuple(sd[stem + leaf] for leaf in leaves[:-2]) + (scale, shift))
        tail = tuple(sd[k] for k in part.tail)
        got = part.pack(folded, tail)
        assert got.dtype == torch.float32 and got.numel() == part.floats and np.array_equal(got.numpy(), buf)
        layers, back_tail = part.unpack(got)
        assert len(layers) == len(folded) and len(back_tail) == len(tail)
        for b, f in zip(layers, folded):
            assert len(b) == len(f) and all(x.shape == y.shape and torch.equal(x, y.float()) for x, y in zip(b, f))
        assert all(torch.equal(x, y) for x, y in zip(back_tail, tail))


@pytest.mark.parametrize("weights,dilation,residual", [("golden", 2, 1), ("golden", 1, 1), ("seeded", 2, 0)])
def test_forward_is_the_inference_model(weights, dilation, residual):
    """Without gates: segmenter_model.full_forward (decode on encode_full, the classifier, the pool), up to the rounding of
    the depthwise pair; with its own gates it is the same function up to rounding; grad_feats alone gives the encoder-only
    net's gradients bitwise and leaves the decoder's exactly zero; both upstream gradients together give the sum of the
    two."""
    obs = m.case_obs((32, 2))
    sd = {k: v.double() for k, v in m.joint_state_dict(weights).items()}
    net = m.Net("ppo", True, dilation, bool(residual), True)
    us = []
    pooled, logit = m.forward_gated(sd, obs, net, None, us)
    assert len(us) == 21 and [u.shape[-1] for u in us[16:]] == [2, 4, 8, 16, 32] and us[15].shape[1:] == (256, 1, 1)
    ref = segmenter_model.full_forward(sd, obs, "ppo", dilation, bool(residual))
    # encode_full's depthwise pair is F.conv2d, the model's the sliced sums: the same function, not the same rounding
    assert torch.allclose(logit, ref["logit"], rtol=1e-12, atol=1e-13) and torch.allclose(pooled, ref["pooled"], rtol=1e-12, atol=1e-13)
    gates = [(u > 0).double() for u in us]
    pooled_g, logit_g = m.forward_gated(sd, obs, net, gates)
    assert torch.allclose(pooled_g, pooled, rtol=1e-12, atol=1e-14) and torch.allclose(logit_g, logit, rtol=1e-12, atol=1e-14)
    # alive: every layer has open and closed gates, the map both classes
    assert all(0.02 < float(g.mean()) < 0.98 for g in gates), [float(g.mean()) for g in gates]
    assert 0.02 < float((logit > 0).double().mean()) < 0.98

    gen = torch.Generator().manual_seed(44)
    gf = torch.randn(2, 256, generator=gen, dtype=torch.float64)
    gp = torch.randn(2, 1, 32, 32, generator=gen, dtype=torch.float64)
    host = m.HostModel(sd, net, obs)
    # grad_prob = 0: the encoder's gradients are the encoder-only net's, the decoder's exactly zero
    a = host.grads((host.forward(gates)[0] * gf).sum())
    enc_host = m.HostModel(sd, net._replace(joint=False), obs)
    want = enc_host.grads((enc_host.feats(gates[:16]) * gf).sum())
    assert set(want) == set(m.enc_keys(net)) and all(torch.equal(a[k], w) for k, w in want.items())
    assert all(float(a[k].abs().max()) == 0.0 for k in m.dec_keys(net))
    # grad_feats = 0: the map's loss reaches every encoder layer (the join) and every decoder level
    b = host.grads((host.forward(gates)[1] * gp).sum())
    assert all(float(b[k].abs().max()) > 0.0 for k in m.param_keys(net))
    # together: the sum of the two
    joint = host.grads((host.forward(gates)[0] * gf).sum() + (host.forward(gates)[1] * gp).sum())
    for k, w in joint.items():
        assert torch.allclose(a[k] + b[k], w, rtol=1e-11, atol=1e-13 * float(w.abs().max())), k


def test_split_cases_reach_what_they_claim():
    """From train_layout.dpw_plans and decoder_split_model.dw_plans alone."""
    assert [(s, n) for _w, _d, _r, s, n in m.SEP_JOINT_SPLIT_CASES] == [(64, 130), (96, 65)]
    enc = tl.dpw_plans(64, 130)
    # the initial layer and both layers of levels 0 (16-pixel tiles, 16 per env) and 1 (8-pixel tiles, 16 per env): 3 tiles
    # per slice, 2080 = 693 x 3 + 1: a last slice of one tile, slices crossing env boundaries
    for p in enc[:3] + enc[4:6]:
        assert p["sep"] and p["tiles_env"] == 16 and p["total_tiles"] == 2080 and p["tps"] == 3 and p["slices"] == 694
        assert p["short_last"] and p["total_tiles"] - 693 * 3 == 1 and p["straddles"]
    assert [enc[i]["T"] for i in (0, 1, 4)] == [16, 16, 8]
    assert not enc[3]["sep"] and enc[3]["tps"] == 5 and enc[3]["straddles"]  # the level-0 down
    # the one-hot envs of the GPU test: the short last slice lies in the last env, and a slice ends in env 1 that began in env 0
    assert (693 * 3) // 16 == 129 and any((s * 3) // 16 == 0 and (s * 3 + 2) // 16 == 1 for s in range(694))
    assert any(p["tps"] >= 2 for p in dsm.dw_plans(64, 130))
    # (96, 65) is the decoder's split shape; the separable layers of levels 3 and 4 straddle envs with a short last slice
    dec = dsm.dw_plans(96, 65)
    assert [p["tps"] for p in dec] == [2, 2, 2, 2, 5]
    assert any(p["short_last"] for p in dec) and sum(p["straddles"] for p in dec) == 3
    enc = tl.dpw_plans(96, 65)
    for i in (10, 11, 13, 14):
        assert enc[i]["sep"] and enc[i]["tps"] >= 2 and enc[i]["straddles"] and enc[i]["short_last"], (i, enc[i])
    assert ("golden", 2, 1, 96, 65) in m.SEP_JOINT_SPLIT_CASES and ("ppo", 96, 65) in dsm.SPLIT_CASES


@pytest.mark.parametrize("weights,dilation,residual,img,n", m.SEP_JOINT_CASES,
                         ids=[f"{w}-d{d}-res{r}-S{s}-N{n}" for w, d, r, s, n in m.SEP_JOINT_CASES])
def test_gate_band_is_small_in_every_gpu_case(weights, dilation, residual, img, n):
    """From the f64 model alone: at most 0.5 % of any layer's pixels have |u| <= 1e-4 max(1, max |u|), so that the 1 % cap
    of the GPU test is met or missed by the kernels and not by the inputs."""
    sd = {k: v.double() for k, v in m.joint_state_dict(weights).items()}
    us = []
    with torch.no_grad():
        m.forward_gated(sd, m.case_obs((img, n)), m.Net("ppo", True, dilation, bool(residual), True), None, us)
    shares = m.band_shares(us)
    assert len(shares) == 21
    assert max(shares) <= BAND_CAP, [f"{s:.4f}" for s in shares]
