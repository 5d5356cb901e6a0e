"""GPU tests of ``occ_dataset_pack`` (csrc/occ_datapack.hpp; ``devdata.DeviceDataset.put``) against tests/datapack_model.py,
the numpy model that tests/test_datapack_model.py pins to PIL and to the dataset files.  Every plane is compared bit for
bit.  The kernel tests call the C ABI directly on a store that starts as a seeded pattern and runs GUARD elements past
what the ABI names; frames no slot names, and the guards, are compared afterwards.

Sizes.  The dither pass takes bands of 64 rows, one row per lane, and label bytes in chunks of 8 steps.  S = 8: one partial
band.  S = 64: exactly one band.  S = 72: a band boundary and a short last band.  S = 136: two boundaries.  The point pass
takes 256 pixels per block: 64 pixels are a quarter block, 5184 = 20.25 blocks, 18496 = 72.25 blocks.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import augment_model as am
from tests import datapack_model as dm

pytestmark = pytest.mark.gpu

GUARD = 64
CASES = [(1, 8), (3, 64), (2, 72), (1, 136)]  # (n, S)


@pytest.fixture(scope="module")
def lib():
    from occlusionenv_amd import _native as nat

    return nat.load()


def _p(t, byte_offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + byte_offset)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def make_inputs(n, S, seed, alpha_kind="mixed"):
    """obs (n,4,S,S) and alpha (n,S,S) f32.  Colours in [-0.2, 1.2] with NaN, +-inf and exact 0 / 0.5 / 1 in them; depth of
    -1 (background), [0, 5], values whose product with 51 passes 255, negatives and NaN; alpha soft over a third of the
    image, hard 0 / 1 elsewhere, with values below 0, above 1 and NaN -- or the constant 128 / 255 or 129 / 255."""
    rng = np.random.default_rng(seed)
    obs = rng.uniform(-0.2, 1.2, (n, 4, S, S)).astype(np.float32)
    obs[:, :3, 0, ::3] = np.nan
    obs[:, 0, 1, ::2], obs[:, 1, 1, ::2], obs[:, 2, 1, ::2] = 0.0, 0.5, 1.0
    obs[:, 0, 2, 1::4], obs[:, 1, 2, 1::4] = np.inf, -np.inf
    d = rng.uniform(0.0, 5.0, (n, S, S)).astype(np.float32)
    kind = rng.integers(0, 6, (n, S, S))
    d = np.where(kind == 0, -1.0, d)
    d = np.where(kind == 1, rng.uniform(5.0, 9.0, (n, S, S)), d)
    d = np.where(kind == 2, -0.7, d).astype(np.float32)
    d[:, 3, ::5] = np.nan
    d[:, 4, ::5] = 1e30
    d[:, 5 % S, ::5] = 5.0  # 255 exactly
    obs[:, 3] = d
    if alpha_kind == "mixed":
        a = rng.uniform(-0.1, 1.1, (n, S, S)).astype(np.float32)
        hard = (rng.random((n, S, S)) < 0.5).astype(np.float32)
        a[:, :, S // 3:] = hard[:, :, S // 3:]
        a[:, S // 2, ::4] = np.nan
        a[:, -1, :] = 0.5  # 127.5 rounds to the even level 128; the threshold rule gives 0
    else:
        a = np.full((n, S, S), {"c128": 128, "c129": 129}[alpha_kind] / 255.0, np.float32)
    return obs, a


def pattern(words, seed, dtype):
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, words, dtype=dtype, endpoint=True)


def run_pack(lib, obs, alpha, stride, slots, M, mode, seed=99, rc_want=0, overrides=None):
    """One occ_dataset_pack on a pattern-filled, guarded store -> (words (M,S,S) u32, depth (M,S,S) i16, the same two as
    they were before).  ``stride`` 4 embeds alpha as channel 3 of an (n,S,S,4) image of noise.  ``overrides``: argument
    index -> value, for the calls that must be refused."""
    n, S = obs.shape[0], obs.shape[-1]
    w0, d0 = pattern(M * S * S + GUARD, seed, np.int32), pattern(M * S * S + GUARD, seed + 1, np.int16)
    d_w, d_d = torch.from_numpy(w0.copy()).cuda(), torch.from_numpy(d0.copy()).cuda()
    d_obs = torch.from_numpy(obs).cuda()
    if stride == 4:
        fs = np.random.default_rng(seed + 2).random((n, S, S, 4)).astype(np.float32)
        fs[..., 3] = alpha
        d_a, off = torch.from_numpy(fs).cuda(), 12
    else:
        d_a, off = torch.from_numpy(alpha).cuda(), 0
    d_slot = torch.from_numpy(np.asarray(slots, np.int64)).cuda()
    args = [_p(d_obs), _p(d_a, off), stride, n, S, _p(d_slot), _p(d_w), _p(d_d), M, mode, _stream()]
    for i, v in (overrides or {}).items():
        args[i] = v
    rc = lib.occ_dataset_pack(*args)
    torch.cuda.synchronize()
    assert rc == rc_want, (rc, rc_want)
    w1, d1 = d_w.cpu().numpy(), d_d.cpu().numpy()
    assert np.array_equal(w1[M * S * S:], w0[M * S * S:]) and np.array_equal(d1[M * S * S:], d0[M * S * S:]), "guards were written"
    shape = (M, S, S)
    return (w1[: M * S * S].view(np.uint32).reshape(shape), d1[: M * S * S].reshape(shape),
            w0[: M * S * S].view(np.uint32).reshape(shape), d0[: M * S * S].reshape(shape))


def unpack(words):
    rgb = np.stack([words & 255, (words >> 8) & 255, (words >> 16) & 255], -1).astype(np.uint8)
    return rgb, (words >> 24).astype(np.uint8)


def assert_frames(words, depth, frames, want, what=""):
    """Frames ``frames`` of the store hold the model's planes ``want`` = (rgb, depth, label), env by env."""
    rgb, label = unpack(words[frames])
    for name, g, w in (("rgb", rgb, want[0]), ("depth", depth[frames], want[1]), ("label", label, want[2])):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype)
        bad = g != w
        assert not bad.any(), f"{what} {name}: {int(bad.sum())} of {bad.size} differ, first at {tuple(np.argwhere(bad)[0])}"


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("n,S", CASES)
def test_kernel_equals_model(lib, n, S, stride):
    for kind in ("mixed", "c128", "c129"):
        obs, alpha = make_inputs(n, S, 100 * S + n, kind)
        for mode in (dm.LABEL_DITHER, dm.LABEL_THRESHOLD):
            want = dm.pack_model(obs, alpha, mode)
            words, depth, _, _ = run_pack(lib, obs, alpha, stride, np.arange(n), n, mode)
            assert_frames(words, depth, np.arange(n), want, f"{kind} mode {mode}")
        if kind == "mixed":
            assert not np.array_equal(want[2], dm.pack_model(obs, alpha, dm.LABEL_DITHER)[2])  # the two rules differ
            assert want[1].min() == 0 and want[1].max() == 255 and want[0].min() == 0 and want[0].max() == 255
    # a constant just above the threshold dithers to a pattern that is neither all 0 nor all 1
    lab = dm.pack_model(obs, alpha, dm.LABEL_DITHER)[2]
    assert 0 < lab.mean() < 1


def test_slots_skip_permute_and_leave_the_rest(lib):
    n, S, M = 5, 72, 7
    obs, alpha = make_inputs(n, S, 7)
    slots = np.array([4, -1, 0, M, 6])  # envs 1 and 3 are skipped (-1 and m_frames); frames 1, 2, 3, 5 are not named
    for mode in (dm.LABEL_DITHER, dm.LABEL_THRESHOLD):
        want = dm.pack_model(obs, alpha, mode)
        words, depth, w0, d0 = run_pack(lib, obs, alpha, 4, slots, M, mode)
        envs = np.array([0, 2, 4])
        assert_frames(words, depth, slots[envs], tuple(p[envs] for p in want), f"mode {mode}")
        rest = np.array([1, 2, 3, 5])
        assert np.array_equal(words[rest], w0[rest]) and np.array_equal(depth[rest], d0[rest])
    # nothing but skipped envs, slots far outside included: the store keeps its pattern
    words, depth, w0, d0 = run_pack(lib, obs, alpha, 1, [-1, M, -2 ** 62, 2 ** 62, M + 1], M, dm.LABEL_DITHER)
    assert np.array_equal(words, w0) and np.array_equal(depth, d0)


def test_two_calls_give_the_same_bits(lib):
    obs, alpha = make_inputs(2, 72, 8)
    a = run_pack(lib, obs, alpha, 4, [1, 0], 2, dm.LABEL_DITHER)
    b = run_pack(lib, obs, alpha, 4, [1, 0], 2, dm.LABEL_DITHER)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # a second call on a store that already holds labels (not the pattern) gives the same frames again
    from occlusionenv_amd.devdata import DeviceDataset

    ds = DeviceDataset.empty(2, 72, "cuda")
    fs = torch.from_numpy(alpha).cuda()
    ds.put(torch.from_numpy(obs).cuda(), fs, [1, 0])
    first = (ds.rgbl.clone(), ds.depth.clone())
    ds.put(torch.from_numpy(obs).cuda(), fs, [1, 0])
    assert torch.equal(ds.rgbl, first[0]) and torch.equal(ds.depth, first[1])
    assert np.array_equal(ds.rgbl.cpu().numpy().view(np.uint32), a[0])


def test_refused_calls_leave_the_store(lib):
    obs, alpha = make_inputs(2, 8, 9)
    # occ_dataset_pack(obs, alpha, alpha_stride, n, img, slot, rgbl, depth, m_frames, label_mode, stream)
    bad = [{i: None} for i in (0, 1, 5, 6, 7)]
    bad += [{2: 0}, {2: -1}, {3: 0}, {3: -1}, {3: 65536}, {4: 0}, {4: -8}, {4: 4097}, {8: 0}, {8: -2}, {9: 2}, {9: -1}]
    for o in bad:
        words, depth, w0, d0 = run_pack(lib, obs, alpha, 1, [0, 1], 2, dm.LABEL_DITHER, rc_want=1, overrides=o)
        assert np.array_equal(words, w0) and np.array_equal(depth, d0), o


def test_put_then_batch_through_the_python_layer():
    from occlusionenv_amd import _native as nat
    from occlusionenv_amd.devdata import DeviceDataset

    n, S, M = 3, 72, 5
    obs, alpha = make_inputs(n, S, 10)
    rng = np.random.default_rng(11)
    fs = rng.random((n, S, S, 4)).astype(np.float32)
    fs[..., 3] = alpha
    pos, grad = rng.normal(size=(n, 2)).astype(np.float32), rng.normal(size=(n, 2)).astype(np.float32)
    for label, mode in (("dither", dm.LABEL_DITHER), ("threshold", dm.LABEL_THRESHOLD)):
        ds = DeviceDataset.empty(M, S, "cuda", split="val")
        slots = torch.tensor([3, -1, 0])  # a host tensor; env 1 is skipped, its pos / grad rows too
        ds.put(torch.from_numpy(obs).cuda(), torch.from_numpy(fs).cuda(), slots, pos=pos, grad=torch.from_numpy(grad).cuda(), label=label)
        rgb, depth, lab = dm.pack_model(obs, alpha, mode)
        store = [np.zeros((M,) + p.shape[1:], p.dtype) for p in (rgb, depth, lab)] + [np.zeros((M, 2), np.float32), np.zeros((M, 2), np.float32)]
        for env, f in ((0, 3), (2, 0)):
            for dst, src in zip(store, (rgb, depth, lab, pos, grad)):
                dst[f] = src[env]
        got = ds.batch(range(M), None, normalize=False)
        want = am.batch(*store, np.arange(M), None, False)
        for name, g, w in zip(("img", "label", "grad", "pos"), got, want):
            assert np.array_equal(g.cpu().numpy().view(np.uint32), w.view(np.uint32)), (label, name)
        # the model's planes over 255: what the network is fed
        f32 = np.float32
        img = got[0].cpu().numpy()
        assert np.array_equal(img[3, :3], np.transpose(rgb[0], (2, 0, 1)).astype(f32) / f32(255))
        assert np.array_equal(img[3, 3], depth[0].astype(f32) / f32(255)) and np.array_equal(got[1].cpu().numpy()[0, 0], lab[2].astype(f32))
    # device slots, an (n,S,S) alpha image
    ds.put(torch.from_numpy(obs).cuda(), torch.from_numpy(alpha).cuda(), torch.tensor([1, 2, 4], device="cuda"), label="threshold")
    assert np.array_equal(ds.unpack(4)[2], lab[2]) and np.array_equal(ds.unpack(1)[1], depth[0])
    with pytest.raises(ValueError):
        ds.put(torch.zeros(1, 4, 64, 64, device="cuda"), torch.zeros(1, 64, 64, 4, device="cuda"), [0])
    with pytest.raises(nat.NativeError):
        DeviceDataset.empty(2, S, "cpu").put(torch.from_numpy(obs[:1]), torch.from_numpy(fs[:1]), [0])
