"""Host-side checks of the encoder training path (csrc/occ_encoder_bwd.hpp, occlusionenv_amd/enctrain.py): the workspace
query grows with n and covers the kept tensors, the packed layout round-trips, the BatchNorm fold's gradients are right, the gated f64 model is plain autograd when given its own gates, and the restated K
split of the weight gradient is what the library's query sizes its scratch for.  The argument contract of the three entry
points is checked from the table of tests/train_abi.py by tests/test_train_abi_host.py.  No GPU."""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from occlusionenv_amd import _native as nat
from tests import encoder_model
from tests import train_layout as tl
from tests import train_model as m

DENSE = m.Net("ppo", False, 1, True)  # the scratch does not depend on the preset or the residual


def _cfg(img=64, dilation=1, residual=0, separable=0):
    cfg = nat.OccEncoderConfig()
    cfg.img, cfg.dilation, cfg.residual, cfg.separable = img, dilation, residual, separable
    return cfg


def _query(lib, img, n, **kw):
    ws, sc = C.c_size_t(), C.c_size_t()
    rc = lib.occ_encoder_train_workspace_query(C.byref(_cfg(img, **kw)), n, C.byref(ws), C.byref(sc))
    return rc, int(ws.value), int(sc.value)


def test_workspace_query_grows_with_n_and_covers_the_kept_tensors():
    lib = nat.load()
    prev = 0
    for n in (1, 2, 5, 64):
        rc, ws_b, sc_b = _query(lib, 128, n)
        assert rc == 0 and ws_b > prev and sc_b > 0
        prev = ws_b
    for img in (32, 40, 96, 256):  # odd intermediate sides included
        for n in (1, 3):
            rc, ws_b, _sc = _query(lib, img, n)
            assert rc == 0 and ws_b % 256 == 0
            # the kept tensors and three gradient buffers of (n, 8, S, S)
            assert ws_b >= tl.kept_bytes(img, n) + 3 * 4 * n * 8 * img * img
    # the size the header states: 30.31 MiB per env at 256^2
    assert abs(_query(lib, 256, 128)[1] / 128 / 2 ** 20 - 30.31) < 0.01


def test_pack_round_trip_against_pack_state_dict():
    from occlusionenv_amd.encoder import pack_state_dict, packed_floats
    from occlusionenv_amd.enctrain import pack_encoder_buffer, unpack_encoder_buffer
    from occlusionenv_amd.seghead import fold_bn_vectors

    buf = torch.randn(packed_floats(False), generator=torch.Generator().manual_seed(1))
    layers = unpack_encoder_buffer(buf)
    assert [tuple(l[0].shape) for l in layers] == [(co, ci, 3, 3) for _s, ci, co, *_ in m.layers(False)]
    assert torch.equal(pack_encoder_buffer(layers), buf)
    w1 = layers[1][0]  # the layout: w[ci][ky * 3 + kx][co]
    off = 9 * 4 * 8 + 3 * 8
    assert float(w1[5, 3, 2, 1]) == float(buf[off + (3 * 9 + 2 * 3 + 1) * 8 + 5])
    for preset in ("predictor", "ppo"):
        sd = {k: v.float() for k, v in m.dense_state_dict(preset, 11).items()}
        prefix = m.preset_keys(preset)["prefix"]
        separable, want, _offsets = pack_state_dict(sd, prefix)
        assert not separable
        folded = []
        for stem, *_ in m.layers(False):
            st = prefix + stem
            scale, shift, _ = fold_bn_vectors(sd[st + "bn.weight"], sd[st + "bn.bias"], sd[st + "bn.running_mean"], sd[st + "bn.running_var"])
            folded.append((sd[st + "conv.weight"], sd[st + "conv.bias"], scale, shift))
        got = pack_encoder_buffer(folded)
        assert np.array_equal(got.numpy(), want)
        back = unpack_encoder_buffer(got)
        assert all(torch.equal(b[0], f[0]) and torch.equal(b[1], f[1]) for b, f in zip(back, folded))


def test_bn_parameter_gradients_against_autograd():
    from occlusionenv_amd.seghead import bn_param_grads, fold_bn_vectors

    g = torch.Generator().manual_seed(3)
    c = 8
    r = torch.relu(torch.randn(2, c, 5, 5, generator=g, dtype=torch.float64))
    gamma = (torch.rand(c, generator=g, dtype=torch.float64) + 0.5).requires_grad_()
    beta = torch.randn(c, generator=g, dtype=torch.float64).requires_grad_()
    mean = torch.randn(c, generator=g, dtype=torch.float64)
    var = torch.rand(c, generator=g, dtype=torch.float64) + 0.1
    up = torch.randn(2, c, generator=g, dtype=torch.float64)
    y = F.batch_norm(r, mean, var, gamma, beta, False, 0.0, 1e-5)
    (y.mean(dim=(2, 3)) * up).sum().backward()  # through the pool, as the encoder's last layer
    scale, shift, _rstd = fold_bn_vectors(gamma.detach(), beta.detach(), mean, var)
    assert torch.allclose(r * scale[None, :, None, None] + shift[None, :, None, None], y.detach(), rtol=1e-13, atol=1e-13)
    dy = (up / 25.0)[:, :, None, None].expand_as(r)
    dgamma, dbeta = bn_param_grads((dy * r).sum((0, 2, 3)), dy.sum((0, 2, 3)), mean, var)
    assert torch.allclose(dgamma, gamma.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(dbeta, beta.grad, rtol=1e-12, atol=1e-12)


def test_gated_model_with_its_own_gates_is_plain_autograd():
    for preset in ("predictor", "ppo"):
        sd = m.dense_state_dict(preset, 21)
        obs = encoder_model.make_obs(22, 2, 40)
        up = torch.randn(2, 256, generator=torch.Generator().manual_seed(23), dtype=torch.float64)
        prefix, residual = m.preset_keys(preset)["prefix"], m.preset_keys(preset)["residual"]
        net = m.Net(preset, False, 1, residual)
        host = m.HostModel(sd, net, obs)
        us = []
        f_plain = host.feats(None, us)
        assert len(us) == 16 and [u.shape[-1] for u in us] == [40, 40, 40, 20, 20, 20, 10, 10, 10, 5, 5, 5, 3, 3, 3, 2]
        # the same function as encoder_model.encode, value and gradient
        ref = {k: v.clone().requires_grad_() if k in host.params else v for k, v in sd.items()}
        f_ref = encoder_model.encode(ref, obs, prefix, False, 1, residual)
        assert torch.equal(f_plain.detach(), f_ref.detach())
        (f_ref * up).sum().backward()
        want = {k: ref[k].grad for k in m.param_keys(net)}
        plain = host.grads((f_plain * up).sum())
        gated = host.grads((host.feats([(u > 0).double() for u in us]) * up).sum())
        assert len(want) == 64
        for k, w in want.items():
            assert torch.equal(plain[k], w), k
            assert torch.allclose(gated[k], w, rtol=1e-12, atol=1e-14 * float(w.abs().max())), k


def test_split_plan_is_what_the_query_sizes_scratch_for():
    lib = nat.load()
    for img in (32, 40, 64, 96, 256, 512):
        for n in (1, 2, 3, 64, 65, 128, 129):
            rc, ws_b, sc_b = _query(lib, img, n, residual=1)
            assert rc == 0
            assert sc_b == tl.scratch_bytes(DENSE, img, n), (img, n)
            for p in tl.dw_plans(img, n):
                assert p["slices"] * p["grid_y"] <= tl.DW_BLOCKS
                assert (p["slices"] - 1) * p["tps"] < p["total_tiles"] <= p["slices"] * p["tps"]
    col = lambda img, n, key: [p[key] for p in tl.dw_plans(img, n)]  # noqa: E731
    assert col(40, 3, "ho") == [40, 40, 40, 20, 20, 20, 10, 10, 10, 5, 5, 5, 3, 3, 3, 2]
    assert col(40, 3, "T") == [8] * 10 + [4] * 6
    assert set(col(32, 2, "tps")) == set(col(40, 3, "tps")) == set(col(96, 2, "tps")) == {1}  # one tile per block there
    # the published timing shapes: 128 x 256^2
    assert col(256, 128, "tps")[:4] == [256, 256, 256, 64] and col(256, 128, "slices")[:4] == [512] * 4


def test_split_case_reaches_the_tile_loop():
    """What the split case of tests/test_gpu_encoder_train.py has to reach, on the model alone."""
    preset, img, n = m.ENCODER_SPLIT_CASE
    assert (preset, img, n) == ("ppo", 32, 129)
    plans = tl.dw_plans(img, n)
    assert [p["tps"] for p in plans] == [5, 5, 5, 2, 2, 2, 1, 1, 1, 1, 1, 1, 2, 3, 3, 5]
    # the three deepest layers (one 4-pixel tile per env): every slice of several tiles crosses env boundaries
    assert all(p["T"] == 4 and p["tiles_env"] == 1 and p["straddles"] for p in plans[12:])
    assert plans[12]["short_last"] and plans[15]["short_last"] and plans[15]["stride"] == 2
    # the level-0 layers: 16 tiles per env, 5 per slice, 413 slices, the last one of 4 tiles, slices crossing envs
    for p in plans[:3]:
        assert p["tiles_env"] == 16 and p["total_tiles"] == 2064 and p["slices"] == 413
        assert p["short_last"] and p["total_tiles"] - 412 * 5 == 4 and p["straddles"]
    assert plans[3]["stride"] == 2 and plans[3]["tps"] == 2  # a stride-2 layer runs its tile loop twice as well
    # the one-hot envs of test_gradients_of_one_env: the short last slice lies in the last env alone; the first slice that
    # crosses an env boundary starts in env 0 and ends in env 1
    te, tps = 16, 5
    assert (412 * tps) // te == n - 1 == (2064 - 1) // te
    first = next(s for s in range(413) if (s * tps) // te != (s * tps + tps - 1) // te)
    assert (first * tps) // te == 0 and (first * tps + tps - 1) // te == 1
