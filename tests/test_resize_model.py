"""tests/resize_model.py, the yardstick of ``occ_dataset_resize`` (csrc/occ_resize.hpp), against PIL and against the
files: its three resamplers are ``PIL.Image.resize`` without a filter argument in modes "RGB", "I" and "1" bit for bit,
``pack_model`` at R followed by ``resize_model`` is what ``dataset_io.RunWriter`` at R and
``devdata.DeviceDataset.from_directory`` at S give (the JPEG apart), the host side of ``put(resize=True)``, ``resized`` and
``generate_resident(size=)`` refuses what it must, and the entry points are declared, bound, exported and refuse bad
arguments without a GPU.  No GPU.
"""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch
from PIL import Image

from occlusionenv_amd import _native as nat
from occlusionenv_amd import dataset_io, devdata
from tests import datapack_model as dm
from tests import resize_model as rm
from tests.test_datapack_model import synthetic_frames

PAIRS = [(8, 4), (16, 8), (64, 32), (7, 3), (5, 8), (40, 23), (24, 40), (72, 36), (130, 64), (512, 256), (33, 32), (9, 1),
         (1, 3)]  # (R, S)


def contents(R, rng):
    """(name, rgb (R,R,3) u8, depth (R,R) int32, label (R,R) bool)."""
    yield ("random", rng.integers(0, 256, (R, R, 3), dtype=np.uint8), rng.integers(-300, 601, (R, R)).astype(np.int32),
           rng.random((R, R)) < 0.5)
    # hard 0 / 255 edges: the bicubic lobes overshoot both ends of the 8-bit clip; depth steps across its whole range
    blocks = rng.integers(0, 2, ((R + 2) // 3, (R + 2) // 3, 3))
    edges = (np.kron(blocks, np.ones((3, 3, 1), np.int64))[:R, :R] * 255).astype(np.uint8)
    steps = np.where(edges[..., 0] > 0, 600, -300).astype(np.int32)
    yield "edges", edges, steps, edges[..., 1] > 0
    y, x = np.mgrid[:R, :R]
    ramp = np.stack([(x * 255) // max(R - 1, 1), (y * 255) // max(R - 1, 1), ((x + y) % 2) * 255], -1).astype(np.uint8)
    yield "ramps and a checkerboard", ramp, (-300 + (900 * ((x * y) % 7)) // 6).astype(np.int32), (x + y) % 2 == 0


@pytest.mark.parametrize("R,S", PAIRS, ids=lambda v: str(v))
def test_model_is_pils_resize(R, S):
    rng = np.random.default_rng(1000 * R + S)
    tab = rm.tables(R, S)
    assert tab[0].shape == (S, rm.taps(R, S)) and (tab[2][:, 0] >= 0).all() and (tab[2].sum(1) <= R).all()
    for name, rgb, depth, label in contents(R, rng):
        want = np.asarray(Image.fromarray(rgb).resize((S, S)))
        assert np.array_equal(rm.resize8(rgb, S, tab), want), (name, "RGB")
        assert np.array_equal(rm.resize8(rgb[..., 0], S), np.asarray(Image.fromarray(rgb[..., 0]).resize((S, S), Image.BICUBIC))), (name, "L")
        want = np.asarray(Image.fromarray(depth).resize((S, S)))
        got = rm.resize32(depth, S, tab)
        assert got.dtype == np.int32 and np.array_equal(got, want), (name, "I")
        one = Image.fromarray(label).convert("1")
        assert one.mode == "1" and np.array_equal(np.asarray(one), label)
        assert np.array_equal(rm.resize_nearest(label, S, tab), np.asarray(one.resize((S, S)))), (name, "1")
        if name == "edges" and R >= 7 and S >= 3 and R != S:
            assert (want < -300).any() or (want > 600).any(), "the depth edges overshoot"


def test_resize_model_saturates_and_stacks():
    rng = np.random.default_rng(3)
    R, S, n = 16, 8, 2
    rgb = rng.integers(0, 256, (n, R, R, 3), dtype=np.uint8)
    depth = np.kron(rng.choice(np.array([-32768, 32767], np.int64), (n, R // 4, R // 4)), np.ones((1, 4, 4), np.int64))  # hard edges
    label = rng.integers(0, 2, (n, R, R), dtype=np.uint8)
    out = rm.resize_model(rgb, depth, label, S)
    assert [o.dtype for o in out] == [np.uint8, np.int16, np.uint8] and [o.shape for o in out] == [(n, S, S, 3), (n, S, S), (n, S, S)]
    d32 = np.asarray(Image.fromarray(depth[1].astype(np.int32)).resize((S, S))).astype(np.int64)
    assert d32.max() > 32767 and d32.min() < -32768  # PIL's int32 leaves int16 here; the store saturates
    assert np.array_equal(out[1][1], np.clip(d32, -32768, 32767))
    assert np.array_equal(out[0][0], np.asarray(Image.fromarray(rgb[0]).resize((S, S))))
    same = rm.resize_model(rgb, depth, label, R)  # R == S: the identity
    assert np.array_equal(same[0], rgb) and np.array_equal(same[1], depth) and np.array_equal(same[2], label)


@pytest.mark.parametrize("mode", [dm.LABEL_DITHER, dm.LABEL_THRESHOLD])
def test_pack_then_resize_equals_the_files(tmp_path, mode):
    """RunWriter at R -> from_directory at S -> unpack: depth and label bit for bit (the dither runs at R, the resize picks
    from its result).  The writer stores the 8-bit alpha; for the threshold rule it is handed the 0 / 1 label, which the
    reader's ``convert("1")`` leaves as it is."""
    R, S, F = 16, 8, 3
    obs, alpha = synthetic_frames(F, R, 6)
    rgb, depth, label = dm.pack_model(obs, alpha, mode)
    w = dataset_io.RunWriter(str(tmp_path), 0)
    for j in range(F):
        a = alpha[j] if mode == dm.LABEL_DITHER else label[j].astype(np.float32)
        w.write_frame(j, obs[j], a, 0.1 * j, -0.2 * j, (1.0 + j, 2.0 - j))
    w.close()
    ds = devdata.DeviceDataset.from_directory(str(tmp_path), "", (S, S), device="cpu")
    m_rgb, m_depth, m_label = rm.resize_model(rgb, depth, label, S)
    assert m_depth.dtype == np.int16 and set(np.unique(m_label)) == {0, 1}
    for j in range(F):
        _, f_depth, f_label = ds.unpack(j)
        assert np.array_equal(f_depth, m_depth[j]), j
        assert np.array_equal(f_label, m_label[j]), j
        assert np.array_equal(m_rgb[j], np.asarray(Image.fromarray(rgb[j]).resize((S, S)))), j  # the JPEG apart


# ---- the host side ---------------------------------------------------------------------------------------------------
def fake_venv(S, device="cpu", n=2):
    return types.SimpleNamespace(engine=types.SimpleNamespace(S=S, device=torch.device(device)), num_envs=n)


def test_bad_arguments_are_value_errors():
    ds = devdata.DeviceDataset.empty(3, 8, "cpu")
    obs, fs = torch.zeros(2, 4, 16, 16), torch.zeros(2, 16, 16, 4)
    with pytest.raises(ValueError):
        ds.put(obs, fs, [0, 1])  # resize=False: another size is still refused
    with pytest.raises(ValueError):
        ds.put(obs, fs, [0, 1], resize=True, label="round")
    with pytest.raises(ValueError):
        ds.put(obs, fs, [0, 1, 2], resize=True)
    with pytest.raises(ValueError):
        ds.put(torch.zeros(2, 4, 16, 12), torch.zeros(2, 16, 12, 4), [0, 1], resize=True)  # not square
    with pytest.raises(ValueError):
        ds.put(obs, torch.zeros(2, 8, 8, 4), [0, 1], resize=True)  # full_state at another size than obs
    with pytest.raises(ValueError, match="supported"):
        ds.put(torch.zeros(1, 4, 80, 80), torch.zeros(1, 80, 80), [0], resize=True)  # 80 -> 8: a ratio of 10
    for size in (0, -4, 4097, 2.5, "8"):
        with pytest.raises(ValueError):
            ds.resized(size)
    with pytest.raises(ValueError, match="supported"):
        devdata.DeviceDataset.empty(1, 640, "cpu").resized(256)  # 2.5
    for size in (0, -1, 4097, 100):
        with pytest.raises(ValueError):
            devdata.generate_resident(fake_venv(512), 2, num_frames=2, size=size)


def test_a_cpu_store_has_no_resize():
    ds = devdata.DeviceDataset.empty(3, 8, "cpu", split="val")
    with pytest.raises(nat.NativeError, match="no CPU path"):
        ds.put(torch.zeros(2, 4, 16, 16), torch.zeros(2, 16, 16, 4), [0, 1], resize=True)
    with pytest.raises(nat.NativeError, match="no CPU path"):
        ds.put(torch.zeros(2, 4, 8, 8), torch.zeros(2, 8, 8, 4), [0, 1], resize=True)  # R == S: today's pack
    with pytest.raises(nat.NativeError, match="no CPU path"):
        ds.resized(4)
    with pytest.raises(nat.NativeError, match="no CPU path"):
        devdata.generate_resident(fake_venv(16), 2, num_frames=2, size=8)
    ds.pos[1, 0] = 3.0
    same = ds.resized(8)  # a copy needs no kernel
    assert same is not ds and same.split == "val" and same.size == 8 and torch.equal(same.pos, ds.pos)
    assert same.rgbl.data_ptr() != ds.rgbl.data_ptr() and same.pos.data_ptr() != ds.pos.data_ptr()


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_symbols_declared_bound_and_exported():
    lib = C.CDLL(nat.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "occlusionenv_amd.h")).read()
    for name, nargs in (("occ_dataset_resize_query", 4), ("occ_dataset_resize", 11)):
        assert hasattr(lib, name) and name in nat.SYMBOLS and "int %s(" % name in header
        assert len(nat.SYMBOLS[name][1]) == nargs
    assert len(nat.SYMBOLS["occ_dataset_pack"][1]) == 11
    assert "occ_resize.hpp" in open(os.path.join(root, "occlusionenv_amd", "csrc", "occ_kernels.hip")).read()
    assert nat.load().occ_abi_version() == 12 == nat.ABI_VERSION


def test_query_gives_the_documented_layout():
    lib = nat.load()
    need = C.c_size_t()
    assert lib.occ_dataset_resize_query(130, 64, 7, C.byref(need)) == 1  # 2.03: a tile's window would not fit
    for R, S in [p for p in PAIRS if p != (130, 64)] + [(80, 40), (4096, 4096), (4096, 2048), (1, 4096), (72, 1)]:
        assert lib.occ_dataset_resize_query(R, S, 7, C.byref(need)) == 0, (R, S)
        assert need.value == S * rm.taps(R, S) * 12 + S * 12, (R, S)


def test_argument_checks_need_no_gpu():
    lib = nat.load()
    need = C.c_size_t()
    # occ_dataset_resize_query(src_img, dst_img, n, &workspace_bytes)
    assert lib.occ_dataset_resize_query(16, 8, 2, None) == 1
    for bad in ((0, 8, 2), (16, 0, 2), (-16, 8, 2), (16, -8, 2), (4097, 4096, 2), (16, 4097, 2), (16, 8, 0), (16, 8, -1),
                (16, 8, 65536), (80, 8, 2), (640, 256, 2), (4096, 1, 2), (146, 64, 2)):
        assert lib.occ_dataset_resize_query(*bad, C.byref(need)) == 1, bad
    P = C.c_void_p(4096)  # never dereferenced: every call below is rejected before a launch
    # occ_dataset_resize(src_rgbl, src_depth, n, src_img, slot, dst_rgbl, dst_depth, m_frames, dst_img, workspace, stream)
    full = [P, P, 2, 16, P, P, P, 4, 8, P, None]
    for i in (0, 1, 4, 5, 6, 9):
        args = list(full)
        args[i] = None
        assert lib.occ_dataset_resize(*args) == 1, i
    for i, bad in ((2, 0), (2, -1), (2, 65536), (3, 0), (3, -16), (3, 4097), (3, 80), (3, 1 << 16), (7, 0), (7, -1), (8, 0),
                   (8, -8), (8, 4097), (9, C.c_void_p(4100))):
        args = list(full)
        args[i] = bad
        assert lib.occ_dataset_resize(*args) == 1, (i, bad)
