"""Numpy model of ``occ_dataset_jpeg`` (csrc/occ_jpeg.hpp, include/occlusionenv_amd.h "JPEG round trip in the resident
store"): what ``Image.save(format="JPEG", quality=q)`` followed by ``Image.open(...).convert("RGB")`` does to the pixels
of an RGB image.  Entropy coding is lossless, so the round trip is a function of the pixels and the two quantisation
tables: libjpeg's defaults (YCbCr, 2x2 luminance sampling, slow-integer DCT, fancy upsampling), all in integers.
tests/test_jpeg_model.py pins it to PIL bit for bit.  Numpy only; int64 arrays hold values that fit int32 throughout, and
``>>`` on them is the arithmetic shift.
"""
import numpy as np

# JPEG specification, Annex K, tables K.1 and K.2, in natural (row-major) order
LUMA_BASE = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], np.int64).reshape(8, 8)
CHROMA_BASE = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], np.int64).reshape(8, 8)

A, B, C, D_, E, F, G, H, I, J, K, L = 2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172


def tables(quality: int):
    """``(luma (8,8), chroma (8,8))`` int64: the quantisation tables of ``quality`` (jcparam.c jpeg_set_quality)."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality: 1 .. 100")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (LUMA_BASE, CHROMA_BASE))


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _odd(t4, t5, t6, t7):
    """The odd part both transforms share: the four sums before the final descale (o7, o5, o3, o1 of the forward
    transform, the new t0 .. t3 of the inverse)."""
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F
    t4, t5, t6, t7 = t4 * A, t5 * J, t6 * L, t7 * G
    z1, z2 = z1 * -E, z2 * -K
    z3, z4 = z3 * -I + z5, z4 * -B + z5
    return t4 + z1 + z3, t5 + z2 + z4, t6 + z2 + z3, t7 + z1 + z4


def fdct_1d(d, row_pass: bool):
    """jfdctint.c on the last axis (8 samples) of an int64 array."""
    d = [d[..., k] for k in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if row_pass else 15
    if row_pass:
        o0, o4 = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o0, o4 = descale(t10 + t11, 2), descale(t10 - t11, 2)
    z = (t12 + t13) * C
    o2, o6 = descale(z + t13 * D_, n), descale(z - t12 * H, n)
    s7, s5, s3, s1 = _odd(t4, t5, t6, t7)
    return np.stack([o0, descale(s1, n), o2, descale(s3, n), o4, descale(s5, n), o6, descale(s7, n)], -1)


def idct_1d(d, n: int):
    """jidctint.c on the last axis (8 coefficients), descaled by ``n`` bits."""
    d = [d[..., k] for k in range(8)]
    z = (d[2] + d[6]) * C
    t2, t3 = z - d[6] * H, z + d[2] * D_
    t0, t1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = _odd(d[7], d[5], d[3], d[1])
    out = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([descale(o, n) for o in out], -1)


def block_roundtrip(plane, qt):
    """An (8h, 8w) plane of samples 0 .. 255 through forward DCT, quantisation by ``qt``, dequantisation and inverse
    DCT, 8 x 8 block by block; the result clipped to 0 .. 255."""
    h, w = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.astype(np.int64).reshape(h, 8, w, 8).transpose(0, 2, 1, 3) - 128  # (h, w, row, col)
    b = fdct_1d(b, True)                                     # along rows: the last axis is the column index
    b = fdct_1d(b.swapaxes(-1, -2), False).swapaxes(-1, -2)  # along columns
    q8 = qt * 8
    c = np.where(b >= 0, (b + q8 // 2) // q8, -((-b + q8 // 2) // q8))  # truncating division of a magnitude
    b = c * qt
    b = idct_1d(b.swapaxes(-1, -2), 11).swapaxes(-1, -2)     # along columns
    b = idct_1d(b, 18)                                       # along rows
    return np.clip(b + 128, 0, 255).transpose(0, 2, 1, 3).reshape(h * 8, w * 8)


def _pad_rows(plane, rows):
    """The plane's own last row replicated down to ``rows`` rows."""
    return np.concatenate([plane, np.repeat(plane[-1:], rows - plane.shape[0], 0)], 0) if rows > plane.shape[0] else plane


def forward_planes(rgb):
    """``(Y, Cb, Cr)`` as the encoder hands them to the DCT: Y padded to multiples of 8 rows and 16 columns, the chroma
    planes downsampled and padded to multiples of 8 both ways."""
    rgb = np.asarray(rgb)
    Hh, W = rgb.shape[:2]
    W16 = (W + 15) // 16 * 16
    p = rgb.astype(np.int64)
    p = np.concatenate([p, np.repeat(p[:, -1:], W16 - W, 1)], 1)   # right edge: to a multiple of 16 columns
    p = _pad_rows(p, Hh + (Hh & 1))                                # bottom edge of the input: to an even height only
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    bias = np.tile(np.array([1, 2], np.int64), W16 // 4)
    down = [(c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2 for c in (cb, cr)]
    y = _pad_rows(y[:Hh], (Hh + 7) // 8 * 8)                      # every plane: its own last row, to a multiple of 8
    ch = (down[0].shape[0] + 7) // 8 * 8
    return y, _pad_rows(down[0], ch), _pad_rows(down[1], ch)


def upsample(c, Hh, W):
    """jdsample.c h2v2_fancy_upsample of the chroma plane ``c`` cropped to ``ceil(H/2) x ceil(W/2)``; result H x W."""
    c = c[:(Hh + 1) // 2, :(W + 1) // 2].astype(np.int64)
    up, dn = np.concatenate([c[:1], c[:-1]], 0), np.concatenate([c[1:], c[-1:]], 0)
    s = np.empty((2 * c.shape[0], c.shape[1]), np.int64)
    s[0::2], s[1::2] = 3 * c + up, 3 * c + dn
    left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
    return out[:Hh, :W]


def roundtrip(rgb, quality: int):
    """``rgb`` (H,W,3) uint8 written as a baseline 4:2:0 JPEG of ``quality`` and decoded again: (H,W,3) uint8."""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("rgb: (H,W,3) uint8")
    Hh, W = rgb.shape[:2]
    ql, qc = tables(quality)
    y, cb, cr = forward_planes(rgb)
    y = block_roundtrip(y, ql)[:Hh, :W]
    u = upsample(block_roundtrip(cb, qc), Hh, W) - 128
    v = upsample(block_roundtrip(cr, qc), Hh, W) - 128
    r = y + ((91881 * v + 32768) >> 16)
    b = y + ((116130 * u + 32768) >> 16)
    g = y + ((-22554 * u - 46802 * v + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
