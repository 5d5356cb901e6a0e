"""Numpy model of ``occ_dataset_pack`` (csrc/occ_datapack.hpp, include/occlusionenv_amd.h "Packing rendered frames into
the resident dataset"): what ``dataset_io.RunWriter.write_frame`` followed by ``devdata.DeviceDataset.from_directory`` at
the same size does to a frame, per pixel, without the JPEG.  tests/test_datapack_model.py pins ``dither`` to PIL's
``convert("1")`` and the three planes to the files.  Numpy only.
"""
import numpy as np

LABEL_DITHER, LABEL_THRESHOLD = 0, 1


def ubyte(a) -> np.ndarray:
    """``dataset_io._ubyte`` with the cases the cast leaves open defined: ``clip(rint((double)x * 255.0), 0, 255)``,
    round-half-even, NaN -> 0."""
    v = np.rint(np.asarray(a, dtype=np.float32).astype(np.float64) * 255.0)
    v = np.where(np.isnan(v), 0.0, v)
    return np.clip(v, 0.0, 255.0).astype(np.uint8)


def depth_levels(d) -> np.ndarray:
    """``depth[depth == -1] = 0; (depth * 51).astype(uint8)`` with one f32 product, truncated toward zero; outside the
    cast's range: ``t <= 0`` or NaN -> 0, ``t >= 255`` -> 255.  int16."""
    d = np.asarray(d, dtype=np.float32)
    d = np.where(d == np.float32(-1.0), np.float32(0.0), d)
    with np.errstate(over="ignore", invalid="ignore"):
        t = (d * np.float32(51.0)).astype(np.float32)
    inside = (t > 0) & (t < 255)  # False for NaN
    out = np.where(inside, np.trunc(np.where(inside, t, 0)), np.where(t >= 255, 255.0, 0.0))
    return out.astype(np.int16)


def dither(a8) -> np.ndarray:
    """PIL's ``convert("1")`` of an (H, W) uint8 image (Convert.c ``tobilevel``: Floyd-Steinberg error diffusion, one
    ``errors`` row of W + 1 ints that persists across rows) -> (H, W) uint8 of 0 / 1."""
    a8 = np.asarray(a8)
    assert a8.dtype == np.uint8 and a8.ndim == 2
    H, W = a8.shape
    rows = a8.astype(np.int64).tolist()
    errors = [0] * (W + 1)
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        row, o = rows[y], out[y]
        l = l0 = l1 = 0
        for x in range(W):
            s = l + errors[x + 1]
            q = s // 16 if s >= 0 else -((-s) // 16)  # C division: toward zero
            l = row[x] + q
            l = 0 if l < 0 else (255 if l > 255 else l)
            if l > 128:
                o[x] = 1
                l -= 255
            l2 = l
            d2 = l + l
            l += d2
            errors[x] = l + l0
            l += d2
            l0 = l + l1
            l1 = l2
            l += d2
        errors[W] = l0
    return out


def pack_model(obs, alpha, label_mode=LABEL_DITHER):
    """``obs`` (n,4,S,S) f32, ``alpha`` (n,S,S) f32 -> ``(rgb_u8 (n,S,S,3), depth_i16 (n,S,S), label_u8 (n,S,S))``: the
    planes ``DeviceDataset.unpack`` returns for the frames ``occ_dataset_pack`` writes.  The colours are swapped (the
    writer saves BGR, the reader opens RGB): R = u8(obs[2]), G = u8(obs[1]), B = u8(obs[0])."""
    obs = np.asarray(obs, dtype=np.float32)
    alpha = np.asarray(alpha, dtype=np.float32)
    n, S = obs.shape[0], obs.shape[-1]
    assert obs.shape == (n, 4, S, S) and alpha.shape == (n, S, S) and label_mode in (LABEL_DITHER, LABEL_THRESHOLD)
    rgb = np.stack([ubyte(obs[:, 2]), ubyte(obs[:, 1]), ubyte(obs[:, 0])], -1)
    depth = depth_levels(obs[:, 3])
    if label_mode == LABEL_THRESHOLD:
        with np.errstate(invalid="ignore"):
            label = (alpha > np.float32(0.5)).astype(np.uint8)
    else:
        a8 = ubyte(alpha)
        label = np.stack([dither(a8[i]) for i in range(n)])
    return rgb, depth, label
