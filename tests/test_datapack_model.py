"""tests/datapack_model.py, the yardstick of ``occ_dataset_pack`` (csrc/occ_datapack.hpp), against PIL and against the
files: its dither is PIL's ``convert("1")``, its three planes are what ``dataset_io.RunWriter`` writes and
``devdata.DeviceDataset.from_directory`` reads back at the same size (the JPEG apart), and the entry point is declared,
bound and exported.  No GPU.
"""
import ctypes as C
import os

import numpy as np
import pytest
from PIL import Image

from occlusionenv_amd import _native as nat
from occlusionenv_amd import dataset_io, devdata
from tests import datapack_model as dm

SHAPES = [(1, 1), (1, 7), (5, 1), (8, 8), (16, 16), (33, 47), (64, 64), (72, 72), (64, 130)]  # (H, W)


def blurred_disc(H, W):
    """A soft silhouette edge: a disc whose alpha falls from 1 to 0 over a third of its radius."""
    y, x = np.mgrid[:H, :W]
    r = np.hypot(y - (H - 1) / 2.0, x - (W - 1) / 2.0)
    R = 0.35 * max(H, W) + 0.5
    return np.clip(np.rint(255.0 * np.clip((R - r) / (R / 3.0), 0.0, 1.0)), 0, 255).astype(np.uint8)


def contents(H, W, rng):
    yield "random", rng.integers(0, 256, (H, W), dtype=np.uint8)
    yield "four levels", (rng.integers(0, 4, (H, W)) * 85).astype(np.uint8)
    yield "noise around 128", np.clip(np.rint(128 + rng.normal(0, 4, (H, W))), 0, 255).astype(np.uint8)
    for v in (0, 255, 128, 129):
        yield "all %d" % v, np.full((H, W), v, np.uint8)
    yield "horizontal ramp", np.broadcast_to(np.linspace(0, 255, W).astype(np.uint8)[None, :], (H, W)).copy()
    yield "vertical ramp", np.broadcast_to(np.linspace(0, 255, H).astype(np.uint8)[:, None], (H, W)).copy()
    yield "blurred disc", blurred_disc(H, W)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_dither_is_pils_convert_1(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    for name, a in contents(*shape, rng):
        want = np.asarray(Image.fromarray(a).convert("1")).astype(np.uint8)
        got = dm.dither(a)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, shape)


def test_dither_is_not_a_threshold_on_a_soft_edge():
    a = blurred_disc(64, 64)
    d = dm.dither(a)
    assert set(np.unique(d)) == {0, 1} and not np.array_equal(d, (a > 128).astype(np.uint8))


def test_out_of_range_values_are_defined():
    f32 = np.float32
    x = np.array([-0.5, -0.0, 0.0, 0.5 / 255, 1.5 / 255, 2.5 / 255, 0.5, 1.0, 1.5, np.nan, np.inf, -np.inf], f32)
    want = dataset_io._ubyte(x[:8])
    assert np.array_equal(dm.ubyte(x), np.concatenate([want, [255, 0, 255, 0]]).astype(np.uint8))
    assert dm.ubyte(np.array([0.5], f32)).tolist() == [128]  # 127.5, the one tie an f32 in [0, 1] can hit: to the even level
    d = np.array([-1.0, 0.0, 1.0, 4.99, 5.0, 5.01, 1e30, -0.3, np.nan, np.inf, -np.inf, 1.0 / 51.0], f32)
    got = dm.depth_levels(d)
    assert got.dtype == np.int16
    assert got.tolist() == [0, 0, 51, int(f32(4.99) * f32(51)), 255, 255, 255, 0, 0, 255, 0, int(f32(1.0 / 51.0) * f32(51))]
    # inside the byte the rule is the writer's cast
    inside = np.linspace(0, 4.99, 1000).astype(f32)
    assert np.array_equal(dm.depth_levels(inside), (inside * 51).astype(np.uint8).astype(np.int16))


def synthetic_frames(n, S, seed):
    """obs in [0,1] with depth in {-1} u [0,5], a soft alpha in [0,1]."""
    rng = np.random.default_rng(seed)
    obs = rng.random((n, 4, S, S)).astype(np.float32)
    obs[:, 3] = np.where(rng.random((n, S, S)) < 0.4, -1.0, 5.0 * obs[:, 3]).astype(np.float32)
    alpha = rng.random((n, S, S)).astype(np.float32)
    alpha[:, : S // 2] = np.clip(alpha[:, : S // 2] * 3.0 - 1.0, 0.0, 1.0)  # patches of exact 0 and 1
    return obs, alpha


def test_model_equals_the_files(tmp_path):
    """RunWriter -> from_directory at the writer's size -> unpack: depth and label bit for bit; RGB before the JPEG is
    ``_ubyte`` with the channel swap (the JPEG itself is lossy and is not compared)."""
    S, F = 16, 3
    obs, alpha = synthetic_frames(F, S, 5)
    w = dataset_io.RunWriter(str(tmp_path), 0)
    for j in range(F):
        w.write_frame(j, obs[j], alpha[j], 0.1 * j, -0.2 * j, (1.0 + j, 2.0 - j))
    w.close()
    ds = devdata.DeviceDataset.from_directory(str(tmp_path), "", (S, S), device="cpu")
    rgb, depth, label = dm.pack_model(obs, alpha, dm.LABEL_DITHER)
    assert rgb.dtype == np.uint8 and depth.dtype == np.int16 and label.dtype == np.uint8
    assert set(np.unique(label)) == {0, 1} and depth.max() > 200 and (depth == 0).any()
    for j in range(F):
        _, f_depth, f_label = ds.unpack(j)
        assert np.array_equal(f_depth, depth[j]), j
        assert np.array_equal(f_label, label[j]), j
        hwc = np.transpose(obs[j], (1, 2, 0))
        assert np.array_equal(rgb[j], dataset_io._ubyte(hwc[..., :3])[..., ::-1]), j  # what the writer hands the JPEG
    thr = dm.pack_model(obs, alpha, dm.LABEL_THRESHOLD)
    assert np.array_equal(thr[0], rgb) and np.array_equal(thr[1], depth)
    assert np.array_equal(thr[2], (alpha > 0.5).astype(np.uint8)) and not np.array_equal(thr[2], label)


def test_symbol_declared_bound_and_exported():
    lib = C.CDLL(nat.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "occlusionenv_amd.h")).read()
    assert hasattr(lib, "occ_dataset_pack") and "occ_dataset_pack" in nat.SYMBOLS and "int occ_dataset_pack(" in header
    assert len(nat.SYMBOLS["occ_dataset_pack"][1]) == 11
    assert "occ_datapack.hpp" in open(os.path.join(root, "occlusionenv_amd", "csrc", "occ_kernels.hip")).read()
    assert nat.load().occ_abi_version() == 12 == nat.ABI_VERSION
    assert devdata.LABEL_MODES == {"dither": dm.LABEL_DITHER, "threshold": dm.LABEL_THRESHOLD}


def test_argument_checks_need_no_gpu():
    lib = nat.load()
    P = C.c_void_p(4096)  # never dereferenced: every call below is rejected before a launch
    # occ_dataset_pack(obs, alpha, alpha_stride, n, img, slot, rgbl, depth, m_frames, label_mode, stream)
    full = [P, P, 1, 2, 16, P, P, P, 4, 0, None]
    for i in (0, 1, 5, 6, 7):
        args = list(full)
        args[i] = None
        assert lib.occ_dataset_pack(*args) == 1, i
    for i, bad in ((2, 0), (2, -4), (3, 0), (3, -1), (3, 65536), (4, 0), (4, -2), (4, 4097), (4, 1 << 16), (8, 0), (8, -1),
                   (9, 2), (9, -1)):
        args = list(full)
        args[i] = bad
        assert lib.occ_dataset_pack(*args) == 1, (i, bad)


def test_host_side_of_put_and_empty():
    ds = devdata.DeviceDataset.empty(3, 8, "cpu", split="val")
    assert len(ds) == 3 and ds.size == 8 and ds.split == "val" and not ds.rgbl.any() and not ds.depth.any()
    import torch

    obs, fs = torch.zeros(2, 4, 8, 8), torch.zeros(2, 8, 8, 4)
    with pytest.raises(ValueError):
        ds.put(torch.zeros(2, 4, 16, 16), torch.zeros(2, 16, 16, 4), [0, 1])
    with pytest.raises(ValueError):
        ds.put(obs, fs, [0, 1], label="round")
    with pytest.raises(ValueError):
        ds.put(obs, fs, [0, 1, 2])
    with pytest.raises(ValueError):
        ds.put(obs, torch.zeros(2, 8, 8, 3), [0, 1])
    with pytest.raises(nat.NativeError, match="no CPU path"):
        ds.put(obs, fs, [0, 1])
    with pytest.raises(ValueError):
        devdata.DeviceDataset.empty(0, 8, "cpu")
