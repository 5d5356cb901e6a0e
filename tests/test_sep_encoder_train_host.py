"""Host-side checks of the separable-encoder training path (csrc/occ_sepenc_bwd.hpp, occlusionenv_amd/septrain.py): the
separable packed layout is ``encoder.pack_state_dict``'s and round-trips, the restated K split of the pointwise weight gradient
is what the library's query sizes its scratch for, the split case of the GPU test reaches what its description claims, and the
decomposition of one separable layer's backward that the kernels implement equals torch autograd in f64.  The argument
contract of the three entry points is checked from the table of tests/train_abi.py by tests/test_train_abi_host.py.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from occlusionenv_amd import _native as nat
from tests import encoder_model
from tests import train_layout as tl
from tests import train_model as m

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_golden.npz")
SEP = m.Net("ppo", True, 2, True)  # the scratch does not depend on the preset, the dilation or the residual


def _cfg(img=64, dilation=2, residual=1, separable=1):
    cfg = nat.OccEncoderConfig()
    cfg.img, cfg.dilation, cfg.residual, cfg.separable = img, dilation, residual, separable
    return cfg


def _query(lib, img, n, **kw):
    ws, sc = C.c_size_t(), C.c_size_t()
    rc = lib.occ_sep_encoder_train_workspace_query(C.byref(_cfg(img, **kw)), n, C.byref(ws), C.byref(sc))
    return rc, int(ws.value), int(sc.value)


def test_queries_equal_the_model():
    lib = nat.load()
    for img in (32, 33, 40, 64, 96, 256, 512):
        for n in (1, 2, 3, 64, 115, 128, 513):
            for d in (1, 2):
                rc, ws_b, sc_b = _query(lib, img, n, dilation=d, residual=d - 1)
                assert rc == 0
                assert sc_b == tl.scratch_bytes(SEP, img, n), (img, n)
                # the workspace is the dense training workspace: the same tensors are kept
                dws, dsc = C.c_size_t(), C.c_size_t()
                dense = _cfg(img, dilation=1, residual=0, separable=0)
                assert lib.occ_encoder_train_workspace_query(C.byref(dense), n, C.byref(dws), C.byref(dsc)) == 0
                assert ws_b == int(dws.value) and ws_b % 256 == 0
                assert ws_b >= tl.kept_bytes(img, n) + 3 * 4 * n * 8 * img * img
            for p in tl.dpw_plans(img, n):
                if p["sep"]:
                    assert p["slices"] * p["grid_y"] <= tl.DPW_BLOCKS
                    assert (p["slices"] - 1) * p["tps"] < p["total_tiles"] <= p["slices"] * p["tps"]
    col = lambda img, n, key: [p[key] for p in tl.dpw_plans(img, n)]  # noqa: E731
    assert col(40, 3, "ho") == [40, 40, 40, 20, 20, 20, 10, 10, 10, 5, 5, 5, 3, 3, 3, 2]
    assert col(40, 3, "T") == [16, 16, 16, 8, 8, 8, 8, 8, 8, 8, 4, 4, 4, 4, 4, 4]
    sep = [i for i, p in enumerate(tl.dpw_plans(40, 3)) if p["sep"]]
    assert sep == [0, 1, 2, 4, 5, 7, 8, 10, 11, 13, 14]
    for img, n in ((32, 2), (40, 3), (96, 2)):  # one tile per block in the small cases of the GPU test
        assert {p["tps"] for p in tl.dpw_plans(img, n)} == {1}
    # the timing shape 128 x 256^2: 256 16-pixel tiles per env at level 0, 32 per slice
    assert col(256, 128, "tps")[:3] == [32, 32, 32] and col(256, 128, "slices")[:3] == [1024] * 3


def test_separable_pack_is_pack_state_dict_and_round_trips():
    from occlusionenv_amd.encoder import pack_state_dict, packed_floats
    from occlusionenv_amd.nettrain import fold_bn_vectors, sep_encoder_part
    from occlusionenv_amd.septrain import pack_sep_encoder_buffer, unpack_sep_encoder_buffer

    sd = {k: v.float() for k, v in encoder_model.golden_state_dict(np.load(GOLDEN), "ppo").items()}
    separable, want, _offsets = pack_state_dict(sd, "encoder.")
    assert separable and want.size == packed_floats(True)
    part = sep_encoder_part("ppo")
    assert part.stems == tuple("encoder." + stem for stem, *_ in m.layers(True))
    assert [len(leaves) for leaves in part.layer_leaves()] == [6] + [6, 6, 4] * 5
    folded = []
    for stem, leaves in zip(part.stems, part.layer_leaves()):
        scale, shift, _ = fold_bn_vectors(sd[stem + "bn.weight"], sd[stem + "bn.bias"], sd[stem + "bn.running_mean"],
                                          sd[stem + "bn.running_var"])
        folded.append(tuple(sd[stem + leaf] for leaf in leaves[:-2]) + (scale, shift))
    got = part.pack(folded, ())
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    back, tail = part.unpack(got)
    assert tail == () and len(back) == 16
    for b, f in zip(back, folded):
        assert len(b) == len(f)
        assert all(x.shape == y.shape and torch.equal(x, y.float()) for x, y in zip(b, f))
    buf = torch.randn(packed_floats(True), generator=torch.Generator().manual_seed(1))
    layers = unpack_sep_encoder_buffer(buf)
    assert torch.equal(pack_sep_encoder_buffer(layers), buf)
    # the layout of Layer 1 of level 1 (16 channels): wv[ci][3] | wh[ci][3] | pw[ci][co]
    off = (6 * 4 + 4 * 8 + 24) + 2 * (6 * 8 + 64 + 24) + (9 * 8 * 16 + 48)
    wv, wh, pw = layers[4][:3]
    assert tuple(wv.shape) == (16, 1, 3, 1) and tuple(wh.shape) == (16, 1, 1, 3) and tuple(pw.shape) == (16, 16, 1, 1)
    assert float(wv[5, 0, 2, 0]) == float(buf[off + 5 * 3 + 2]) and float(wh[5, 0, 0, 1]) == float(buf[off + 48 + 5 * 3 + 1])
    assert float(pw[7, 3, 0, 0]) == float(buf[off + 96 + 3 * 16 + 7])
    with pytest.raises(ValueError):
        unpack_sep_encoder_buffer(buf[:-1])


def test_dense_parts_are_unchanged():
    from occlusionenv_amd.nettrain import LEAVES, decoder_part, encoder_part

    for part in (encoder_part("predictor"), encoder_part("ppo"), decoder_part("ppo")):
        assert part.leaves is None and part.layer_leaves() == (LEAVES,) * len(part.stems)


def test_split_case_reaches_the_tile_loop():
    """What the split case of tests/test_gpu_sep_encoder_train.py has to reach, on the model alone."""
    img, n = m.SEP_ENCODER_SPLIT_CASE
    assert (img, n) == (33, 115)
    plans = tl.dpw_plans(img, n)
    assert [p["ho"] for p in plans] == [33, 33, 33, 17, 17, 17, 9, 9, 9, 5, 5, 5, 3, 3, 3, 2]
    assert [p["tps"] for p in plans if p["sep"]] == [2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1]
    # the initial layer and both layers of levels 0 (16-pixel tiles) and 1 (8-pixel tiles): 9 tiles per env (the last row and
    # column of tiles one pixel wide), 2 per slice, 518 slices, the last one of a single tile, slices crossing envs
    for p in plans[:3] + plans[4:6]:
        assert p["tiles_env"] == 9 and p["total_tiles"] == 1035 and p["slices"] == 518
        assert p["short_last"] and p["total_tiles"] - 517 * 2 == 1 and p["straddles"]
    assert [plans[i]["T"] for i in (0, 1, 4)] == [16, 16, 8]
    # the dense downs keep their own split: the first one loops over tiles as well
    assert not plans[3]["sep"] and plans[3]["tps"] > 1
    # the one-hot envs of test_gradients_of_one_env: the short last slice lies in the last env; the first slice that crosses
    # an env boundary starts in env 0 and ends in env 1
    te, tps = 9, 2
    assert (517 * tps) // te == n - 1 == (1035 - 1) // te
    first = next(s for s in range(518) if (s * tps) // te != (s * tps + tps - 1) // te)
    assert first == 4 and (first * tps) // te == 0 and (first * tps + tps - 1) // te == 1


@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("shape", [(5, 3), (2, 2)], ids=["5x3", "2x2"])
def test_layer_decomposition_equals_autograd(d, shape):
    g = torch.Generator().manual_seed(100 * d + shape[0])
    n, cin, cout = 2, 3, 4
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    x = rnd(n, cin, *shape).requires_grad_()
    wv, wh, pw = rnd(cin, 1, 3, 1).requires_grad_(), rnd(cin, 1, 1, 3).requires_grad_(), rnd(cout, cin, 1, 1).requires_grad_()
    du = rnd(n, cout, *shape)
    h = F.conv2d(F.conv2d(x, wv, None, 1, (d, 0), (d, 1), cin), wh, None, 1, (0, d), (1, d), cin)
    u = F.conv2d(h, pw)
    (u * du).sum().backward()
    dwv, dwh, dpw, dx = m.sep_layer_backward(x.detach(), wv.detach()[:, 0, :, 0], wh.detach()[:, 0, 0, :], pw.detach()[:, :, 0, 0],
                                             du, d)
    for got, want in ((dwv, wv.grad[:, 0, :, 0]), (dwh, wh.grad[:, 0, 0, :]), (dpw, pw.grad[:, :, 0, 0]), (dx, x.grad)):
        assert got.shape == want.shape
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12 * max(1.0, float(want.abs().max())))
    assert float(dwv.abs().max()) > 0 and float(dx.abs().max()) > 0


def test_gated_model_with_its_own_gates_is_plain_autograd():
    sd = encoder_model.golden_state_dict(np.load(GOLDEN), "ppo")
    obs = encoder_model.make_obs(22, 2, 40)
    up = torch.randn(2, 256, generator=torch.Generator().manual_seed(23), dtype=torch.float64)
    for d in (1, 2):
        net = m.Net("ppo", True, d, True)
        host = m.HostModel(sd, net, obs)
        us = []
        f_plain = host.feats(None, us)
        assert len(us) == 16 and [u.shape[-1] for u in us] == [40, 40, 40, 20, 20, 20, 10, 10, 10, 5, 5, 5, 3, 3, 3, 2]
        ref = {k: v.clone().requires_grad_() if k in host.params else v for k, v in sd.items()}
        f_ref = encoder_model.encode(ref, obs, "encoder.", True, d, True)
        assert torch.allclose(f_plain.detach(), f_ref.detach(), rtol=1e-13, atol=1e-13)  # the sliced depthwise pair
        (f_ref * up).sum().backward()
        want = {k: ref[k].grad for k in m.param_keys(net)}
        plain = host.grads((f_plain * up).sum())
        assert len(want) == 11 * 6 + 5 * 4
        gated = host.grads((host.feats([(u > 0).double() for u in us]) * up).sum())
        for k, w in want.items():
            assert torch.allclose(plain[k], w, rtol=1e-11, atol=1e-13 * float(w.abs().max())), k
            assert torch.allclose(gated[k], w, rtol=1e-11, atol=1e-13 * float(w.abs().max())), k
