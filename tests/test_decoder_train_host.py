"""Host-side checks of the decoder training path (csrc/occ_decoder_bwd.hpp, occlusionenv_amd/seghead.py): the workspace
query covers what the backward needs, the mapping between the packed gradient and the parameters is right, and the f64
model and the workspace layout that the GPU tests judge by (tests/train_model.py with the encoder frozen,
tests/train_layout.py) are the inference model's and the library's.  The
argument contract of the three entry points is checked from the table of tests/train_abi.py by
tests/test_train_abi_host.py.  No GPU."""
import ctypes as C

import torch
import torch.nn.functional as F

from occlusionenv_amd import _native as nat


def _cfg(img=64):
    cfg = nat.OccEncoderConfig()
    cfg.img, cfg.dilation, cfg.residual, cfg.separable = img, 2, 1, 1
    return cfg


def _query(lib, img, n):
    ws, sc = C.c_size_t(), C.c_size_t()
    assert lib.occ_segment_train_workspace_query(C.byref(_cfg(img)), n, C.byref(ws), C.byref(sc)) == 0
    return int(ws.value), int(sc.value)


def _kept_bytes(img, n):
    """x_j and r_j of every level, y_4 and prob, as f32."""
    floats = n * 256 * (img // 32) ** 2  # x_0: the encoder's last down output
    for j in range(5):
        c, side = 128 >> j, (img // 16) << j
        y = n * c * side * side
        floats += 2 * y  # r_j, and y_j = x_{j+1} (y_4, the decoder feature, at the last level)
    return 4 * (floats + n * img * img)


def test_workspace_query_covers_the_kept_tensors():
    lib = nat.load()
    prev = 0
    for n in (1, 2, 5, 64):
        ws, sc = _query(lib, 128, n)
        assert ws > prev and sc > 0
        prev = ws
        seg = C.c_size_t()
        assert lib.occ_segment_workspace_query(C.byref(_cfg(128)), n, C.byref(seg)) == 0
        assert ws >= _kept_bytes(128, n) and ws > seg.value
    for img in (32, 96, 512):
        assert _query(lib, img, 3)[0] >= _kept_bytes(img, 3)


def test_packed_gradient_round_trip():
    from occlusionenv_amd.encoder import decoder_packed_floats, decoder_plan
    from occlusionenv_amd.seghead import pack_decoder_buffer, unpack_decoder_buffer

    g = torch.Generator().manual_seed(1)
    buf = torch.randn(decoder_packed_floats(), generator=g)
    levels, cls_w, cls_b = unpack_decoder_buffer(buf)
    assert [tuple(l[0].shape) for l in levels] == [(cin, cout, 3, 3) for _j, cin, cout in decoder_plan()]
    assert cls_w.shape == (1, 8, 1, 1) and cls_b.shape == (1,)
    assert torch.equal(pack_decoder_buffer(levels, cls_w, cls_b), buf)
    # the layout is the one pack_decoder documents: w[ci][ky * 3 + kx][co], then bias | scale | shift
    w0, b0, s0, t0 = levels[0]
    assert float(w0[5, 7, 2, 1]) == float(buf[(5 * 9 + 2 * 3 + 1) * 128 + 7])
    off = 9 * 256 * 128
    assert torch.equal(b0, buf[off:off + 128]) and torch.equal(s0, buf[off + 128:off + 256]) and torch.equal(t0, buf[off + 256:off + 384])
    assert torch.equal(cls_b, buf[-1:]) and torch.equal(cls_w.reshape(-1), buf[-9:-1])


def test_pack_matches_the_encoders_fold():
    """Packing the unfolded tensors with the fold of seghead equals encoder.pack_decoder on the same state dict."""
    import numpy as np

    from occlusionenv_amd.encoder import DECODER_KEYS, LEVELS, pack_decoder
    from occlusionenv_amd.seghead import fold_bn_vectors, pack_decoder_buffer
    from tests.segmenter_model import golden_seg_state_dict
    import os

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segmenter_golden.npz"))
    for preset in ("ppo", "segmenter"):
        sd = {k: v.float() for k, v in golden_seg_state_dict(g, preset).items()}
        dp, dc = DECODER_KEYS[preset]
        levels = []
        for j in range(LEVELS):
            st = f"{dp}{j}.up."
            scale, shift, _ = fold_bn_vectors(sd[st + "bn.weight"], sd[st + "bn.bias"], sd[st + "bn.running_mean"], sd[st + "bn.running_var"])
            levels.append((sd[st + "conv.weight"], sd[st + "conv.bias"], scale, shift))
        got = pack_decoder_buffer(levels, sd[dc + "weight"], sd[dc + "bias"])
        assert np.array_equal(got.numpy(), pack_decoder(sd, dp, dc))


def test_bn_parameter_gradients_against_autograd():
    """dgamma / dbeta from the gradients of the folded affine against f64 autograd through F.batch_norm in eval mode."""
    from occlusionenv_amd.seghead import bn_param_grads, fold_bn_vectors

    g = torch.Generator().manual_seed(2)
    c = 16
    r = torch.relu(torch.randn(3, c, 6, 6, generator=g, dtype=torch.float64))
    gamma = (torch.rand(c, generator=g, dtype=torch.float64) + 0.5).requires_grad_()
    beta = torch.randn(c, generator=g, dtype=torch.float64).requires_grad_()
    mean = torch.randn(c, generator=g, dtype=torch.float64)
    var = torch.rand(c, generator=g, dtype=torch.float64) + 0.1
    up = torch.randn(3, c, 6, 6, generator=g, dtype=torch.float64)
    y = F.batch_norm(r, mean, var, gamma, beta, False, 0.0, 1e-5)
    (y * up).sum().backward()
    scale, shift, _rstd = fold_bn_vectors(gamma.detach(), beta.detach(), mean, var)
    assert torch.allclose(r * scale[None, :, None, None] + shift[None, :, None, None], y.detach(), rtol=1e-13, atol=1e-13)
    dscale, dshift = (up * r).sum((0, 2, 3)), up.sum((0, 2, 3))  # what the kernels produce: sum dY r, sum dY
    dgamma, dbeta = bn_param_grads(dscale, dshift, mean, var)
    assert torch.allclose(dgamma, gamma.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(dbeta, beta.grad, rtol=1e-12, atol=1e-12)


def test_scratch_query_equals_the_split_model():
    """scratch_bytes = max over the levels of (activation partials, weight-gradient partials), tests/decoder_split_model.py."""
    from tests import decoder_split_model as m

    lib = nat.load()
    accepted = 0
    for img in (32, 64, 96, 128, 256, 512):
        for n in (1, 2, 3, 16, 64, 65, 128, 130, 256):
            ws, sc = C.c_size_t(), C.c_size_t()
            rc = lib.occ_segment_train_workspace_query(C.byref(_cfg(img)), n, C.byref(ws), C.byref(sc))
            if rc != 0:  # a rejected combination says nothing about sizes
                continue
            accepted += 1
            assert int(sc.value) == m.scratch_bytes(img, n), (img, n)
            # the gradient buffers at the end of the workspace, after everything _kept_bytes counts
            g = m.level_bytes(img, n)
            assert int(ws.value) >= _kept_bytes(img, n) + g[4] + g[3], (img, n)
    assert accepted == 54  # every one of these is inside the documented contract (img % 32 == 0, 1 <= n <= 65535)


def test_split_model_on_the_table_of_known_shapes():
    """Tiles and tiles per slice of the shapes the GPU tests and the published timing use."""
    from tests import decoder_split_model as m

    def col(img, n, key):
        return [p[key] for p in m.dw_plans(img, n)]

    assert col(32, 1, "total_tiles") == [1, 1, 1, 1, 4] and col(32, 1, "tps") == [1] * 5
    assert col(64, 3, "total_tiles") == [3, 3, 12, 12, 48] and col(64, 3, "tps") == [1] * 5
    assert col(96, 2, "total_tiles") == [2, 8, 18, 18, 72] and col(96, 2, "tps") == [1] * 5
    assert col(256, 128, "total_tiles") == [512, 2048, 8192, 8192, 32768] and col(256, 128, "tps") == [8, 8, 16, 16, 64]
    assert col(128, 16, "tps") == [1, 1, 1, 1, 2]  # the harness test: several tiles per block on the last level only
    for img, n in ((32, 1), (96, 65), (256, 128), (512, 64)):
        for p in m.dw_plans(img, n):
            assert p["slices"] * p["grid_y"] <= m.DW_BLOCKS and (p["slices"] - 1) * p["tps"] < p["total_tiles"] <= p["slices"] * p["tps"]


def _frozen_hosts():
    """(preset, S, N, the state dict, obs, tests/train_model.HostModel of the decoder over the frozen encoder) per case."""
    import numpy as np

    from tests import train_model as tm
    from tests.encoder_model import make_obs
    from tests.segmenter_model import golden_seg_state_dict

    g = np.load(tm.GOLDEN)
    for preset in ("ppo", "segmenter"):
        sd = {k: (v.float().double() if v.is_floating_point() else v) for k, v in golden_seg_state_dict(g, preset).items()}
        for img, n in ((32, 1), (64, 2)):
            obs = make_obs(4000 + img + n, n, img).float().double()
            yield preset, img, n, sd, obs, tm.HostModel(sd, tm.frozen_net(preset), obs)


def test_frozen_encoder_model_is_the_segmenter_model():
    """Without gates the host model of the decoder path (tests/train_model.py, ``frozen_encoder``) is tests/segmenter_model.py:
    decode on encode_full, the classifier, the sigmoid, and the mean of the last down output.  The separable encoder's
    depthwise pair is the same function in another rounding (the tolerances of tests/test_sep_fullnet_train_host.py)."""
    from tests import train_model as tm
    from tests.segmenter_model import full_forward

    for preset, img, n, sd, obs, host in _frozen_hosts():
        assert tm.frozen_net(preset).separable == ("encoder.initial.conv.0.weight" in sd)
        assert len(host.params) == 22 and list(host.params) == tm.dec_keys(host.net)
        with torch.no_grad():
            want = full_forward(sd, obs, preset)
            us = []
            pooled, prob, _pred = host.forward(None, us)
        assert len(us) == 5 and prob.shape == (n, 1, img, img) and pooled.shape == (n, 256)
        assert torch.allclose(prob, want["prob"], rtol=1e-12, atol=1e-13), (preset, img, n)
        assert torch.allclose(pooled, want["pooled"], rtol=1e-12, atol=1e-13), (preset, img, n)
        assert torch.allclose(host.logit()[1].detach(), want["logit"], rtol=1e-12, atol=1e-13), (preset, img, n)


def test_frozen_encoder_model_with_its_own_gates():
    """``u * (u > 0)`` in place of ``relu(u)`` on the decoder's five levels: the same 22 gradients."""
    for preset, img, n, _sd, _obs, host in _frozen_hosts():
        up = torch.randn(n, 1, img, img, generator=torch.Generator().manual_seed(img + n), dtype=torch.float64)
        us = []
        want = host.grads((host.forward(None, us)[1] * up).sum())
        got = host.grads((host.forward([(u > 0).double() for u in us])[1] * up).sum())
        assert len(want) == 22
        for k, w in want.items():
            assert float(w.abs().max()) > 0.0
            assert torch.allclose(got[k], w, rtol=1e-11, atol=1e-13 * float(w.abs().max())), (preset, img, n, k)


def test_layout_of_the_decoder_only_workspace():
    """tests/train_layout.py against the library's queries: the inference decoder's workspace, behind it y_j | r_j per level
    (include/occlusionenv_amd.h), and the whole."""
    from tests import decoder_split_model as m
    from tests import train_layout as tl
    from tests import train_model as tm

    lib = nat.load()
    net = tm.frozen_net("ppo")
    for img, n in ((32, 1), (64, 3), (96, 2), (96, 65), (64, 130), (256, 7)):
        seg = C.c_size_t()
        assert lib.occ_segment_workspace_query(C.byref(_cfg(img)), n, C.byref(seg)) == 0
        assert tl.segment_ws_bytes(img, n) == int(seg.value)
        assert (tl.ws_bytes(net, img, n), tl.scratch_bytes(net, img, n)) == _query(lib, img, n)
        views, off = tl.relu_views(img, n, frozen_encoder=True), int(seg.value)
        assert len(views) == 5
        for j, view in enumerate(views):  # y_j | r_j, each (n, 128 >> j, S/16 << j, S/16 << j) f32 rounded up to 256 bytes
            c, side = 128 >> j, (img // 16) << j
            size = (4 * n * c * side * side + 255) // 256 * 256
            assert view == (off + size, c, side)
            off += 2 * size
        (lo, hi), = tl.only_written(net, img, n)
        assert lo == off + m.align(4 * n * img * img) and hi == tl.ws_bytes(net, img, n)  # prob, then g0 | g1 to the end


def test_split_cases_reach_the_tile_loop():
    """What the split cases of tests/test_gpu_decoder_train.py have to reach, on the model alone: a change of a tile size
    or of the block count that takes the reach away fails here."""
    from tests import decoder_split_model as m

    assert m.SPLIT_CASES == [("ppo", 96, 65), ("segmenter", 64, 130)]
    plans = {(img, n): m.dw_plans(img, n) for _preset, img, n in m.SPLIT_CASES}
    assert [p["tps"] for p in plans[(96, 65)]] == [2, 2, 2, 2, 5]
    assert [p["tps"] for p in plans[(64, 130)]] == [3, 1, 2, 2, 5]
    levels = [[ps[j] for ps in plans.values()] for j in range(m.LEVELS)]
    assert all(any(p["tps"] >= 2 for p in lv) for lv in levels)  # every level runs its tile loop more than once somewhere
    flat = [p for lv in levels for p in lv]
    assert any(p["short_last"] for p in flat)
    assert any(p["straddles"] and p["tps"] >= 2 for p in flat)
    assert any(p["tps"] >= 5 for p in flat)
    # the one-hot envs of test_gradients_of_one_env: env 64 alone fills the short last slice of level 0; the first slices
    # that cross an env boundary on levels 2 to 4 end in env 1
    p96 = plans[(96, 65)]
    assert p96[0]["short_last"] and p96[0]["tiles_env"] == 1 and p96[0]["total_tiles"] - (p96[0]["slices"] - 1) * p96[0]["tps"] == 1
    for j in (2, 3, 4):
        te, tps = p96[j]["tiles_env"], p96[j]["tps"]
        first = next(s for s in range(p96[j]["slices"]) if (s * tps) // te != (s * tps + tps - 1) // te)
        assert (first * tps) // te == 0 and (first * tps + tps - 1) // te == 1
