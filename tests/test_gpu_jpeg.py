"""GPU tests of ``occ_dataset_jpeg`` (csrc/occ_jpeg.hpp; ``devdata.DeviceDataset.jpeg`` and ``put(jpeg=)``) against
tests/jpeg_model.py, the numpy model that tests/test_jpeg_model.py pins to PIL and to the dataset files.  Every colour byte
is compared bit for bit.  The kernel tests call the C ABI directly on a store and a workspace that sit between GUARD
elements of a seeded pattern on both sides; frames no slot names, the label bytes, the workspace planes of skipped entries
and the guards are compared afterwards.

Sizes.  The kernel takes 32 x 32 tiles (2 x 2 MCUs of 16 x 16).  8: one block, every edge in it.  16: one MCU.  23: odd,
the crop and the input row replicated to an even height.  24: 8 mod 16, the chroma planes padded with their own last row
and a luminance block row without a chroma partner.  40: a tile boundary, 8 mod 16 again.  136: 5 x 5 tiles, the last one
short, 8 mod 16.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import datapack_model as dm
from tests import jpeg_model as jm
from tests import resize_model as rm
from tests.test_gpu_datapack import GUARD, _p, _stream, make_inputs, pattern
from tests.test_jpeg_model import contents

pytestmark = pytest.mark.gpu

CASES = [(S, q) for S in (8, 16, 23, 24, 40, 136) for q in (75, 95)] + [(24, 1), (24, 100)]
M = 7
SLOTS = [4, -1, 0, 6, M, 2, 5]  # entries 1 and 4 are skipped; frames 1 and 3 are not named


@pytest.fixture(scope="module")
def lib():
    from occlusionenv_amd import _native as nat

    return nat.load()


def make_store(S, seed):
    """(rgb (M,S,S,3) u8, label (M,S,S) u8): the named frames hold the five kinds of input, the other two noise; the label
    byte is any byte."""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (M, S, S, 3), dtype=np.uint8)
    named = [s for s in SLOTS if 0 <= s < M]
    for f, (_, img) in zip(named, contents(S, S, rng)):
        rgb[f] = img
    return rgb, rng.integers(0, 256, (M, S, S), dtype=np.uint8)


def words_of(rgb, label):
    c = rgb.astype(np.uint32)
    return c[..., 0] | c[..., 1] << 8 | c[..., 2] << 16 | label.astype(np.uint32) << 24


def run_jpeg(lib, store, slots, S, q, seed=99, rc_want=0, overrides=None):
    """One occ_dataset_jpeg on the guarded store -> (words (M,S,S) u32 afterwards, the workspace (n,cs,cs) u16 afterwards,
    the workspace as it was)."""
    n = len(slots)
    need = C.c_size_t()
    assert lib.occ_dataset_jpeg_query(S, n, q if 1 <= q <= 100 else 75, C.byref(need)) == 0
    cs = (S + 15) // 16 * 8
    assert need.value == n * cs * cs * 2
    w0 = pattern(M * S * S + 2 * GUARD, seed, np.int32)
    w0[GUARD:GUARD + M * S * S] = words_of(*store).reshape(-1).view(np.int32)
    ws0 = pattern(need.value // 2 + 2 * GUARD, seed + 1, np.int16)
    d_w, d_ws = torch.from_numpy(w0.copy()).cuda(), torch.from_numpy(ws0.copy()).cuda()
    d_slot = torch.from_numpy(np.asarray(slots, np.int64)).cuda()
    args = [_p(d_w, 4 * GUARD), M, S, _p(d_slot), n, q, _p(d_ws, 2 * GUARD), _stream()]
    for i, v in (overrides or {}).items():
        args[i] = v
    rc = lib.occ_dataset_jpeg(*args)
    torch.cuda.synchronize()
    assert rc == rc_want, (rc, rc_want)
    w1, ws1 = d_w.cpu().numpy(), d_ws.cpu().numpy()
    assert np.array_equal(w1[:GUARD], w0[:GUARD]) and np.array_equal(w1[GUARD + M * S * S:], w0[GUARD + M * S * S:]), "store guards"
    assert np.array_equal(ws1[:GUARD], ws0[:GUARD]) and np.array_equal(ws1[-GUARD:], ws0[-GUARD:]), "workspace guards"
    if rc_want:
        assert np.array_equal(w1, w0) and np.array_equal(ws1, ws0), "a refused call wrote"
    return (w1[GUARD:GUARD + M * S * S].view(np.uint32).reshape(M, S, S), ws1[GUARD:-GUARD].view(np.uint16).reshape(n, cs, cs),
            ws0[GUARD:-GUARD].view(np.uint16).reshape(n, cs, cs))


def unpack(words):
    return np.stack([words & 255, (words >> 8) & 255, (words >> 16) & 255], -1).astype(np.uint8), (words >> 24).astype(np.uint8)


@pytest.mark.parametrize("S,q", CASES)
def test_kernel_equals_model(lib, S, q):
    store = make_store(S, 1000 * S + q)
    rgb, label = store
    words, ws, ws0 = run_jpeg(lib, store, SLOTS, S, q)
    got, got_label = unpack(words)
    assert np.array_equal(got_label, label), "a label byte changed"
    for entry, f in enumerate(SLOTS):
        if 0 <= f < M:
            want = jm.roundtrip(rgb[f], q)
            bad = got[f] != want
            assert not bad.any(), f"S {S} q {q} frame {f}: {int(bad.sum())} of {bad.size} bytes differ, first at {tuple(np.argwhere(bad)[0])}"
        else:
            assert np.array_equal(ws[entry], ws0[entry]), "the workspace plane of a skipped entry was written"
    for f in (1, 3):
        assert np.array_equal(got[f], rgb[f]), "a frame no slot names changed"
    if S >= 16 and q < 100:
        assert any(not np.array_equal(got[f], rgb[f]) for f in (0, 2, 4)), "the round trip is lossy"
    again, _, _ = run_jpeg(lib, store, SLOTS, S, q)  # a fresh copy
    assert np.array_equal(again, words)


def test_only_skipped_entries_leave_everything(lib):
    S = 24
    store = make_store(S, 5)
    words, ws, ws0 = run_jpeg(lib, store, [-1, M, -2 ** 62, 2 ** 62], S, 75)
    assert np.array_equal(words, words_of(*store)) and np.array_equal(ws, ws0)


def test_refused_calls_leave_the_store(lib):
    S = 16
    store = make_store(S, 6)
    # occ_dataset_jpeg(rgbl, m_frames, img, slot, n, quality, workspace, stream)
    bad = [{i: None} for i in (0, 3, 6)] + [{1: 0}, {1: -1}, {2: 0}, {2: -16}, {2: 4097}, {4: 0}, {4: -1}, {4: 65536}, {5: 0}, {5: 101}]
    for o in bad:
        words, _, _ = run_jpeg(lib, store, SLOTS, S, 75, rc_want=1, overrides=o)
        assert np.array_equal(words, words_of(*store)), o


def test_jpeg_and_put_through_the_python_layer():
    from occlusionenv_amd import _native as nat
    from occlusionenv_amd.devdata import DeviceDataset

    n, R, S, Mf = 3, 40, 23, 5
    obs, alpha = make_inputs(n, R, 12)
    packed = dm.pack_model(obs, alpha, dm.LABEL_DITHER)
    jpg = np.stack([jm.roundtrip(packed[0][i], 95) for i in range(n)])
    d_obs, d_alpha = torch.from_numpy(obs).cuda(), torch.from_numpy(alpha).cuda()
    # put(jpeg=) at the store's size: on the named slots
    ds = DeviceDataset.empty(Mf, R, "cuda")
    ds.rgbl[1] = 0x01030507
    ds.put(d_obs, d_alpha, torch.tensor([3, -1, 0]), jpeg=95)
    for env, f in ((0, 3), (2, 0)):
        for name, g, w in zip(("rgb", "depth", "label"), ds.unpack(f), (jpg, packed[1], packed[2])):
            assert np.array_equal(g, w[env]), (f, name)
    assert (ds.rgbl[1] == 0x01030507).all() and not ds.rgbl[2].any() and not ds.rgbl[4].any()
    # put(resize=True, jpeg=): on the staging store, before the resize
    small = DeviceDataset.empty(Mf, S, "cuda")
    small.put(d_obs, d_alpha, torch.tensor([3, -1, 0]), resize=True, jpeg=95)
    want = rm.resize_model(jpg, packed[1], packed[2], S)
    for env, f in ((0, 3), (2, 0)):
        for name, g, w in zip(("rgb", "depth", "label"), small.unpack(f), want):
            assert np.array_equal(g, w[env]), (f, name)
    assert not small.rgbl[1].any() and list(small._staging) == [(n, R)]
    # jpeg=None is the plain pack; jpeg() afterwards, on some frames and then on the rest, is put(jpeg=)
    plain = DeviceDataset.empty(n, R, "cuda")
    plain.put(d_obs, d_alpha, [0, 1, 2])
    for name, g, w in zip(("rgb", "depth", "label"), plain.unpack(1), packed):
        assert np.array_equal(g, w[1]), name
    plain.pos[:], plain.grad[:] = 3.0, -2.0
    depth0 = plain.depth.clone()
    plain.jpeg(95, frames=[2, 0])
    assert np.array_equal(plain.unpack(0)[0], jpg[0]) and np.array_equal(plain.unpack(2)[0], jpg[2])
    assert np.array_equal(plain.unpack(1)[0], packed[0][1])
    plain.jpeg(95, frames=torch.tensor([1]))
    for i in range(n):
        for name, g, w in zip(("rgb", "depth", "label"), plain.unpack(i), (jpg, packed[1], packed[2])):
            assert np.array_equal(g, w[i]), (i, name)
    assert torch.equal(plain.depth, depth0) and (plain.pos == 3.0).all() and (plain.grad == -2.0).all()
    whole = DeviceDataset.empty(n, R, "cuda")
    whole.put(d_obs, d_alpha, [0, 1, 2])
    whole.jpeg(95)
    assert torch.equal(whole.rgbl, plain.rgbl)
    with pytest.raises(ValueError):
        whole.jpeg(0)
    with pytest.raises(ValueError):
        whole.put(d_obs, d_alpha, [0, 1, 2], jpeg=101)
    with pytest.raises(nat.NativeError):
        DeviceDataset.empty(2, R, "cpu").jpeg(75)
