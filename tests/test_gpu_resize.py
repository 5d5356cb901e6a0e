"""GPU tests of ``occ_dataset_resize`` (csrc/occ_resize.hpp; ``devdata.DeviceDataset.put(resize=True)`` and ``resized``)
against tests/resize_model.py, the numpy model that tests/test_resize_model.py pins to PIL and to the dataset files.  Every
plane is compared bit for bit, and so are the tables the call leaves in its workspace.  The kernel tests call the C ABI
directly on a destination and a workspace that start as a seeded pattern and run GUARD elements past what the ABI names;
frames no slot names, and the guards, are compared afterwards.

Sizes.  The kernel takes 32 x 32 output tiles and at most 72 x 72 input windows.  16 -> 8: one partial tile, every window
clipped at both borders.  40 -> 23: a non-integer ratio, the tap count varies from output to output.  24 -> 40: upscaling,
a tile boundary with a short last tile.  9 -> 1: one output, a ratio far above 2 on a small source.  64 -> 32: exactly one
tile.  72 -> 36: scale 2 across a tile boundary with a short last tile; the first tile's window is the largest the kernel
takes on the low side, the last tile's is clipped.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import augment_model as am
from tests import datapack_model as dm
from tests import resize_model as rm
from tests.test_gpu_datapack import GUARD, _p, _stream, assert_frames, make_inputs, pattern

pytestmark = pytest.mark.gpu

CASES = [(1, 16, 8), (2, 40, 23), (1, 24, 40), (2, 9, 1), (1, 64, 32), (2, 72, 36)]  # (n, R, S)


@pytest.fixture(scope="module")
def lib():
    from occlusionenv_amd import _native as nat

    return nat.load()


def make_store(n, R, seed, depth_kind="levels"):
    """(rgb (n,R,R,3) u8, depth (n,R,R) int16, label (n,R,R) u8): noise in the left half, 3 x 3 blocks of hard 0 / 255 in the
    right half (both ends of the 8-bit clip); depth in [-300, 600], or blocks of the two ends of int16."""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (n, R, R, 3), dtype=np.uint8)
    b = (R + 2) // 3
    blocks = np.kron(rng.integers(0, 2, (n, b, b, 3)), np.ones((1, 3, 3, 1), np.int64))[:, :R, :R]
    rgb[:, :, R // 2:] = (blocks[:, :, R // 2:] * 255).astype(np.uint8)
    if depth_kind == "levels":
        depth = rng.integers(-300, 601, (n, R, R)).astype(np.int16)
        depth[:, R // 2:] = np.where(blocks[:, R // 2:, :, 0] > 0, 600, -300)
    else:
        depth = np.where(blocks[..., 1] > 0, 32767, -32768).astype(np.int16)
    label = (rng.random((n, R, R)) < 0.5).astype(np.uint8)
    label[:, : R // 3] = blocks[:, : R // 3, :, 2]
    return rgb, depth, label


def words_of(rgb, label):
    c = rgb.astype(np.uint32)
    return c[..., 0] | c[..., 1] << 8 | c[..., 2] << 16 | label.astype(np.uint32) << 24


def run_resize(lib, store, slots, M, S, seed=99, rc_want=0, overrides=None):
    """One occ_dataset_resize from ``store`` (make_store) into a pattern-filled, guarded destination of M frames ->
    (words (M,S,S) u32, depth (M,S,S) i16, the same two as they were before, the workspace as bytes)."""
    rgb, depth, label = store
    n, R = rgb.shape[0], rgb.shape[1]
    need = C.c_size_t()
    assert lib.occ_dataset_resize_query(R, S, n, C.byref(need)) == 0 and need.value % 4 == 0
    w0, d0 = pattern(M * S * S + GUARD, seed, np.int32), pattern(M * S * S + GUARD, seed + 1, np.int16)
    ws0 = pattern(need.value // 4 + GUARD, seed + 2, np.int32)
    d_w, d_d, d_ws = torch.from_numpy(w0.copy()).cuda(), torch.from_numpy(d0.copy()).cuda(), torch.from_numpy(ws0.copy()).cuda()
    s_w = torch.from_numpy(words_of(rgb, label).view(np.int32)).cuda()
    s_d = torch.from_numpy(depth).cuda()
    d_slot = torch.from_numpy(np.asarray(slots, np.int64)).cuda()
    assert d_ws.data_ptr() % 8 == 0
    args = [_p(s_w), _p(s_d), n, R, _p(d_slot), _p(d_w), _p(d_d), M, S, _p(d_ws), _stream()]
    for i, v in (overrides or {}).items():
        args[i] = v
    rc = lib.occ_dataset_resize(*args)
    torch.cuda.synchronize()
    assert rc == rc_want, (rc, rc_want)
    w1, d1, ws1 = d_w.cpu().numpy(), d_d.cpu().numpy(), d_ws.cpu().numpy()
    assert np.array_equal(w1[M * S * S:], w0[M * S * S:]) and np.array_equal(d1[M * S * S:], d0[M * S * S:]), "guards were written"
    assert np.array_equal(ws1[need.value // 4:], ws0[need.value // 4:]), "the workspace guard was written"
    assert np.array_equal(s_w.cpu().numpy().view(np.uint32), words_of(rgb, label)) and np.array_equal(s_d.cpu().numpy(), depth)
    if rc_want:
        assert np.array_equal(ws1, ws0), "a refused call wrote its workspace"
    shape = (M, S, S)
    return (w1[: M * S * S].view(np.uint32).reshape(shape), d1[: M * S * S].reshape(shape),
            w0[: M * S * S].view(np.uint32).reshape(shape), d0[: M * S * S].reshape(shape), ws1[: need.value // 4].tobytes())


def assert_tables(ws_bytes, R, S):
    """The workspace holds the model's tables in the documented layout: k, kk, bounds, nearest."""
    k, kk, bounds, nearest = rm.tables(R, S)
    K = rm.taps(R, S)
    assert len(ws_bytes) == S * K * 12 + S * 12
    at = 0
    for name, want in (("k", k), ("kk", kk), ("bounds", bounds), ("nearest", nearest)):
        got = np.frombuffer(ws_bytes, want.dtype, want.size, at).reshape(want.shape)
        at += want.nbytes
        bits = "u8" if want.dtype == np.float64 else "u4"
        assert np.array_equal(got.view(bits), want.view(bits)), f"{R} -> {S} table {name}"


@pytest.mark.parametrize("n,R,S", CASES)
def test_kernel_equals_model(lib, n, R, S):
    store = make_store(n, R, 1000 * R + S)
    want = rm.resize_model(*store, S)
    M = n + 2
    slots = np.arange(n)[::-1] + 1  # reversed, frame 0 and frame n + 1 not named
    words, depth, w0, d0, ws = run_resize(lib, store, slots, M, S)
    assert_frames(words, depth, slots, want, f"{R} -> {S}")
    rest = np.array([0, n + 1])
    assert np.array_equal(words[rest], w0[rest]) and np.array_equal(depth[rest], d0[rest])
    assert_tables(ws, R, S)
    if S > 1 and R > 9:
        assert want[0].min() == 0 and want[0].max() == 255 and (want[1].min() < -300 or want[1].max() > 600)  # the lobes overshoot


def test_slots_skip_and_leave_the_rest(lib):
    n, R, S, M = 3, 40, 23, 4
    store = make_store(n, R, 7)
    want = rm.resize_model(*store, S)
    slots = np.array([2, -1, M])  # frames 1 and 2 of the source are skipped (-1 and m_frames)
    words, depth, w0, d0, _ = run_resize(lib, store, slots, M, S)
    assert_frames(words, depth, np.array([2]), tuple(p[:1] for p in want))
    rest = np.array([0, 1, 3])
    assert np.array_equal(words[rest], w0[rest]) and np.array_equal(depth[rest], d0[rest])
    # nothing but skipped frames, slots far outside included: the store keeps its pattern
    words, depth, w0, d0, ws = run_resize(lib, store, [-2 ** 62, 2 ** 62, M + 1], M, S)
    assert np.array_equal(words, w0) and np.array_equal(depth, d0)
    assert_tables(ws, R, S)


def test_depth_saturates_to_int16(lib):
    """Inputs at the two ends of int16: PIL's int32 result leaves int16 at the edges, the store holds it saturated."""
    n, R, S = 1, 16, 8
    store = make_store(n, R, 8, "ends")
    d32 = rm.resize32(store[1][0], S)
    assert d32.max() > 32767 and d32.min() < -32768
    want = rm.resize_model(*store, S)
    assert np.array_equal(want[1][0], np.clip(d32, -32768, 32767)) and want[1].max() == 32767 and want[1].min() == -32768
    words, depth, _, _, _ = run_resize(lib, store, [0], 1, S)
    assert_frames(words, depth, np.array([0]), want)


def test_two_calls_give_the_same_bits(lib):
    store = make_store(2, 72, 9)
    a = run_resize(lib, store, [1, 0], 2, 36)
    b = run_resize(lib, store, [1, 0], 2, 36)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[4] == b[4]


def test_refused_calls_leave_the_store(lib):
    store = make_store(2, 16, 10)
    # occ_dataset_resize(src_rgbl, src_depth, n, src_img, slot, dst_rgbl, dst_depth, m_frames, dst_img, workspace, stream)
    bad = [{i: None} for i in (0, 1, 4, 5, 6, 9)]
    bad += [{2: 0}, {2: -1}, {2: 65536}, {3: 0}, {3: -16}, {3: 4097}, {3: 80}, {7: 0}, {7: -2}, {8: 0}, {8: -8}, {8: 4097}]
    for o in bad:
        words, depth, w0, d0, _ = run_resize(lib, store, [0, 1], 2, 8, rc_want=1, overrides=o)
        assert np.array_equal(words, w0) and np.array_equal(depth, d0), o


def test_put_resize_and_resized_through_the_python_layer():
    from occlusionenv_amd import _native as nat
    from occlusionenv_amd.devdata import DeviceDataset

    n, R, S, M = 3, 72, 36, 5
    obs, alpha = make_inputs(n, R, 10)
    rng = np.random.default_rng(11)
    fs = rng.random((n, R, R, 4)).astype(np.float32)
    fs[..., 3] = alpha
    pos, grad = rng.normal(size=(n, 2)).astype(np.float32), rng.normal(size=(n, 2)).astype(np.float32)
    for label, mode in (("dither", dm.LABEL_DITHER), ("threshold", dm.LABEL_THRESHOLD)):
        ds = DeviceDataset.empty(M, S, "cuda", split="val")
        slots = torch.tensor([3, -1, 0])  # env 1 is skipped, its pos / grad rows too
        ds.put(torch.from_numpy(obs).cuda(), torch.from_numpy(fs).cuda(), slots, pos=pos, grad=grad, label=label, resize=True)
        packed = dm.pack_model(obs, alpha, mode)
        rgb, depth, lab = rm.resize_model(*packed, S)
        store = [np.zeros((M,) + p.shape[1:], p.dtype) for p in (rgb, depth, lab)] + [np.zeros((M, 2), np.float32), np.zeros((M, 2), np.float32)]
        for env, f in ((0, 3), (2, 0)):
            for dst, src in zip(store, (rgb, depth, lab, pos, grad)):
                dst[f] = src[env]
        for f in range(M):
            for name, g, w in zip(("rgb", "depth", "label"), ds.unpack(f), store):
                assert g.dtype == w.dtype and np.array_equal(g, w[f]), (label, f, name)
        # a batch from the resized store
        got = ds.batch(range(M), None, normalize=False)
        want = am.batch(*store, np.arange(M), None, False)
        for name, g, w in zip(("img", "label", "grad", "pos"), got, want):
            assert np.array_equal(g.cpu().numpy().view(np.uint32), w.view(np.uint32)), (label, name)
        assert list(ds._staging) == [(n, R)]
    # the same staging store serves the next put; device slots, an (n,R,R) alpha image
    ds.put(torch.from_numpy(obs).cuda(), torch.from_numpy(alpha).cuda(), torch.tensor([1, 2, 4], device="cuda"), label="threshold", resize=True)
    assert list(ds._staging) == [(n, R)] and np.array_equal(ds.unpack(4)[2], lab[2]) and np.array_equal(ds.unpack(1)[1], depth[0])
    # R == S with resize=True is the plain pack
    at_r = DeviceDataset.empty(n, R, "cuda")
    at_r.put(torch.from_numpy(obs).cuda(), torch.from_numpy(fs).cuda(), [0, 1, 2], label="threshold", resize=True)
    assert not at_r._staging and np.array_equal(at_r.unpack(2)[1], packed[1][2])
    # resized(): the whole store, labels carried over; a jittered batch from it
    at_r.pos[:], at_r.grad[:] = torch.from_numpy(pos).cuda(), torch.from_numpy(grad).cuda()
    small = at_r.resized(S)
    assert len(small) == n and small.size == S and small.split == at_r.split and small.device == at_r.device
    assert torch.equal(small.pos, at_r.pos) and torch.equal(small.grad, at_r.grad) and small.pos.data_ptr() != at_r.pos.data_ptr()
    for f in range(n):
        for name, g, w in zip(("rgb", "depth", "label"), small.unpack(f), (rgb, depth, lab)):
            assert np.array_equal(g, w[f]), (f, name)
    up = small.resized(40)  # 36 -> 40: upscaling through the same call
    want_up = rm.resize_model(rgb, depth, lab, 40)
    for name, g, w in zip(("rgb", "depth", "label"), up.unpack(1), want_up):
        assert np.array_equal(g, w[1]), name
    with pytest.raises(ValueError):
        ds.put(torch.zeros(1, 4, 64, 64, device="cuda"), torch.zeros(1, 64, 64, 4, device="cuda"), [0])  # resize=False
    with pytest.raises(ValueError, match="supported"):
        DeviceDataset.empty(1, 16, "cuda").put(torch.zeros(1, 4, 160, 160, device="cuda"), torch.zeros(1, 160, 160, device="cuda"), [0], resize=True)
    with pytest.raises(nat.NativeError):
        DeviceDataset.empty(2, S, "cpu").put(torch.from_numpy(obs[:1]), torch.from_numpy(fs[:1]), [0], resize=True)
