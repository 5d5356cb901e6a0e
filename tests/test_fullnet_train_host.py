"""Host-side checks of the joint training path (csrc/occ_fullnet_bwd.hpp, occlusionenv_amd/fullnet.py): the workspace query
is the restated layout, the packed layouts round-trip from a whole checkpoint, and the dense joint f64 model of
tests/train_model.py is the inference models of tests/segmenter_model.py, its joint gradient the sum of the gradients of its
two losses.  The argument contract of the three entry points is checked from the table of
tests/train_abi.py by tests/test_train_abi_host.py.  No GPU."""
import ctypes as C

import numpy as np
import torch

from occlusionenv_amd import _native as nat
from tests import decoder_split_model as dsm
from tests import encoder_model, segmenter_model
from tests import train_layout as tl
from tests import train_model as m

JOINT = m.Net("ppo", False, 1, True, True)  # the sizes do not depend on the preset or the residual


def _cfg(img=64, dilation=1, residual=1, separable=0):
    cfg = nat.OccEncoderConfig()
    cfg.img, cfg.dilation, cfg.residual, cfg.separable = img, dilation, residual, separable
    return cfg


def _query(lib, img, n, **kw):
    ws, sc = C.c_size_t(), C.c_size_t()
    rc = lib.occ_fullnet_train_workspace_query(C.byref(_cfg(img, **kw)), n, C.byref(ws), C.byref(sc))
    return rc, int(ws.value), int(sc.value)


def test_workspace_query_is_the_restated_layout():
    lib = nat.load()
    pairs = {(s, n) for _p, _r, s, n in m.JOINT_GRAD_CASES + m.JOINT_SPLIT_CASES} | {(64, 4), (64, 1), (128, 16), (256, 128), (512, 64), (1024, 1)}
    assert {(32, 2), (64, 3), (96, 2), (32, 129), (96, 65)} <= pairs
    for img, n in sorted(pairs):
        for residual in (0, 1):
            rc, ws_b, sc_b = _query(lib, img, n, residual=residual)
            assert rc == 0
            assert ws_b == tl.ws_bytes(JOINT, img, n), (img, n)
            assert sc_b == tl.scratch_bytes(JOINT, img, n), (img, n)
            assert ws_b % 256 == 0
        # the joint workspace starts with the encoder's, whose size the encoder's own query gives
        e_ws, e_sc = C.c_size_t(), C.c_size_t()
        assert lib.occ_encoder_train_workspace_query(C.byref(_cfg(img)), n, C.byref(e_ws), C.byref(e_sc)) == 0
        assert int(e_ws.value) == tl.encoder_ws_bytes(img, n)
        d_ws, d_sc = C.c_size_t(), C.c_size_t()
        assert lib.occ_segment_train_workspace_query(C.byref(_cfg(img)), n, C.byref(d_ws), C.byref(d_sc)) == 0
        assert sc_b == max(int(e_sc.value), int(d_sc.value))
        # less than the two single workspaces together: one encoder pass, 0.94 kept d skip buffers
        assert ws_b < int(e_ws.value) + int(d_ws.value)
    # the d skip of level 0 is not stored: dlast and levels 1..4 only
    lvl = dsm.level_bytes(256, 8)
    kept = tl.ws_bytes(JOINT, 256, 8) - tl.encoder_ws_bytes(256, 8) - 2 * sum(lvl) - dsm.align(4 * 8 * 256 * 256) - 2 * dsm.align(4 * 8 * 256 * 64)
    assert kept == sum(lvl[:4]) and abs(kept / lvl[4] - 0.9375) < 1e-9


def test_pack_round_trips_from_a_whole_checkpoint():
    """Folding and packing the tensors ``TrainableFullNetwork`` holds gives the buffers ``FrozenEncoder`` packs from the
    same checkpoint, and unpacking gives the tensors back."""
    from occlusionenv_amd.encoder import DECODER_KEYS, pack_decoder, pack_state_dict
    from occlusionenv_amd.enctrain import pack_encoder_buffer, unpack_encoder_buffer
    from occlusionenv_amd.seghead import fold_bn_vectors, pack_decoder_buffer, unpack_decoder_buffer

    for preset in m.JOINT_PRESETS:
        sd = {k: v.float() for k, v in m.state_dict(preset, 12).items()}
        net = JOINT._replace(preset=preset)
        assert set(m.param_keys(net, head=True)) <= set(sd)
        assert len(m.enc_keys(net)) == 64 and len(m.dec_keys(net)) == 22

        def folded(stems):
            out = []
            for st in stems:
                scale, shift, _ = fold_bn_vectors(sd[st + "bn.weight"], sd[st + "bn.bias"], sd[st + "bn.running_mean"],
                                                  sd[st + "bn.running_var"])
                out.append((sd[st + "conv.weight"], sd[st + "conv.bias"], scale, shift))
            return out

        separable, want, _off = pack_state_dict(sd, "encoder.")
        assert not separable
        enc = folded(["encoder." + stem for stem, *_ in m.layers(False)])
        got = pack_encoder_buffer(enc)
        assert np.array_equal(got.numpy(), want)
        assert all(torch.equal(b[0], f[0]) and torch.equal(b[1], f[1]) for b, f in zip(unpack_encoder_buffer(got), enc))
        dp, dc = DECODER_KEYS[preset]
        dec = folded([f"{dp}{j}.up." for j in range(5)])
        got = pack_decoder_buffer(dec, sd[dc + "weight"], sd[dc + "bias"])
        assert np.array_equal(got.numpy(), pack_decoder(sd, dp, dc))
        levels, cw, cb = unpack_decoder_buffer(got)
        assert all(torch.equal(b[0], f[0]) and torch.equal(b[1], f[1]) for b, f in zip(levels, dec))
        assert torch.equal(cw, sd[dc + "weight"]) and torch.equal(cb, sd[dc + "bias"])


def test_forward_is_the_inference_models():
    """Without gates: the map is segmenter_model.decode on segmenter_model.encode_full and pooled the mean of its last down
    output, bitwise; with its own gates it is the same function up to rounding."""
    obs = encoder_model.make_obs(41, 2, 64)
    for preset in m.JOINT_PRESETS:
        for residual in (1, 0):
            sd = m.state_dict(preset)  # the seed of the GPU tests: the liveness below is about them
            p = segmenter_model.PRESETS[preset]
            net = m.Net(preset, False, 1, bool(residual), True)
            us = []
            pooled, logit = m.forward_gated(sd, obs, net, None, us)
            assert len(us) == 21 and [u.shape[-1] for u in us[16:]] == [4, 8, 16, 32, 64] and us[15].shape[1:] == (256, 2, 2)
            x_last, skips = segmenter_model.encode_full(sd, obs, p["prefix"], False, 1, bool(residual))
            feats = segmenter_model.decode(sd, x_last, skips, p["decoder"])
            want = torch.nn.functional.conv2d(feats, sd[p["classifier"] + "weight"], sd[p["classifier"] + "bias"])
            assert torch.equal(logit, want) and torch.equal(pooled, x_last.mean(dim=(2, 3)))
            assert torch.equal(pooled, encoder_model.encode(sd, obs, p["prefix"], False, 1, bool(residual)))
            gates = [(u > 0).double() for u in us]
            pooled_g, logit_g = m.forward_gated(sd, obs, net, gates)
            assert torch.allclose(pooled_g, pooled, rtol=1e-12, atol=1e-14) and torch.allclose(logit_g, logit, rtol=1e-12, atol=1e-14)
            # the fixture's decoder is alive on the dense encoder: every level has open and closed gates, the map both classes
            assert all(0.02 < float(g.mean()) < 0.98 for g in gates), [float(g.mean()) for g in gates]
            assert 0.02 < float((logit > 0).double().mean()) < 0.98


def test_joint_gradient_is_the_sum_of_the_two():
    obs = encoder_model.make_obs(43, 2, 32)
    gen = torch.Generator().manual_seed(44)
    gf = torch.randn(2, 256, generator=gen, dtype=torch.float64)
    gp = torch.randn(2, 1, 32, 32, generator=gen, dtype=torch.float64)
    for preset in m.JOINT_PRESETS:
        net = JOINT._replace(preset=preset)
        host = m.HostModel(m.state_dict(preset, 14), net, obs)
        us = []
        host.forward(None, us)
        gates = [(u > 0).double() for u in us]
        pooled, prob, _pred = host.forward(gates)
        joint = host.grads((pooled * gf).sum() + (prob * gp).sum())
        pooled, prob, _pred = host.forward(gates)
        a = host.grads((pooled * gf).sum())
        pooled, prob, _pred = host.forward(gates)
        b = host.grads((prob * gp).sum())
        assert len(joint) == 86
        for k, w in joint.items():
            assert torch.allclose(a[k] + b[k], w, rtol=1e-11, atol=1e-13 * float(w.abs().max())), k
        # the pooled feature's loss does not reach the decoder; the map's loss reaches every encoder layer (the join)
        assert all(float(a[k].abs().max()) == 0.0 for k in m.dec_keys(net))
        assert all(float(b[k].abs().max()) > 0.0 for k in m.enc_keys(net))
