"""Numpy model of the device input pipeline (csrc/occ_augment.hpp, include/occlusionenv_amd.h "The pretraining input
pipeline"): the colour jitter of torchvision's PIL path (ImageEnhance.Brightness / Contrast / Color and the hue shift
through PIL's HSV mode), the flip, and the conversion to the network's input, with every rounding of PIL's C code
written out.  tests/test_augment_model.py checks it against PIL alone; the GPU tests compare the kernels with it bit for
bit.  Images are (H, W, 3) uint8 arrays.
"""
import numpy as np

F32 = np.float32
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3

#: the record OccAugmentParams of the C ABI, 32 bytes
PARAMS_DTYPE = np.dtype([("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"), ("hue_shift", "<i4"),
                         ("order", "<i4"), ("jitter", "<i4"), ("flip", "<i4"), ("pad", "<i4")])


def pack_order(ops) -> int:
    """Four op codes, the first op in the low bits."""
    assert sorted(ops) == [0, 1, 2, 3]
    return int(sum(int(o) << (2 * k) for k, o in enumerate(ops)))


def unpack_order(order: int):
    return [(int(order) >> (2 * k)) & 3 for k in range(4)]


def make_params(n: int) -> np.ndarray:
    """n records that change nothing: factors 1, no hue shift, order 0 1 2 3, jitter and flip off."""
    p = np.zeros(n, PARAMS_DTYPE)
    p["brightness"] = p["contrast"] = p["saturation"] = 1.0
    p["order"] = pack_order([0, 1, 2, 3])
    return p


def hue_shift_of(hue_factor: float) -> int:
    """torchvision's np.int32(hue_factor * 255).astype(np.uint8): truncation toward zero, then the wrap."""
    return int(hue_factor * 255) & 255


def luminance(rgb: np.ndarray) -> np.ndarray:
    """PIL's convert("L")."""
    c = rgb.astype(np.int64)
    return (c[..., 0] * 19595 + c[..., 1] * 38470 + c[..., 2] * 7471 + 0x8000) >> 16


def blend(deg, x, f) -> np.ndarray:
    """PIL's ImagingBlend(deg, x, f) per channel: f32, multiply and add rounded separately, truncated; clipped only when
    f is outside [0, 1]."""
    f = F32(f)
    deg = np.asarray(deg, np.int32)
    x = np.asarray(x, np.int32)
    t = deg.astype(F32) + f * (x - deg).astype(F32)
    assert t.dtype == F32
    if F32(0) <= f <= F32(1):
        return t.astype(np.int32).astype(np.uint8)
    out = np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32)))
    return out.astype(np.uint8)


def brightness(rgb, f):
    return blend(np.zeros_like(rgb, np.int32), rgb, f)


def mean_luminance(rgb) -> int:
    """int(ImageStat.Stat(im.convert("L")).mean[0] + 0.5)."""
    L = luminance(rgb)
    return int(int(L.sum()) / float(L.size) + 0.5)


def contrast(rgb, f, mean=None):
    mean = mean_luminance(rgb) if mean is None else int(mean)
    return blend(np.full(rgb.shape, mean, np.int32), rgb, f)


def saturation(rgb, f):
    return blend(np.repeat(luminance(rgb)[..., None], 3, -1), rgb, f)


def rgb_to_hsv(rgb: np.ndarray) -> np.ndarray:
    """PIL's convert("HSV") of an RGB image."""
    c = rgb.astype(np.int32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    mx, mn = c.max(-1), c.min(-1)
    grey = mx == mn
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (mx - mn).astype(F32)
        s = cr / mx.astype(F32)
        rc, gc, bc = ((mx - ch).astype(F32) / cr for ch in (r, g, b))
        h_r = bc - gc
        h_g = (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(F32)
        h_b = (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(F32)
        h = np.where(r == mx, h_r, np.where(g == mx, h_g, h_b))
        x = h.astype(np.float64) / 6.0 + 1.0
        h = (x - np.floor(x)).astype(F32)  # fmod(x, 1.0) for x > 0
        uh = (h.astype(np.float64) * 255.0)
        us = (s.astype(np.float64) * 255.0)
    uh = np.clip(np.where(grey, 0, np.nan_to_num(uh)).astype(np.int64), 0, 255)
    us = np.clip(np.where(grey, 0, np.nan_to_num(us)).astype(np.int64), 0, 255)
    return np.stack([uh, us, mx], -1).astype(np.uint8)


def hsv_to_rgb(hsv: np.ndarray) -> np.ndarray:
    """PIL's convert("RGB") of an HSV image."""
    c = hsv.astype(np.int32)
    h, s, v = c[..., 0], c[..., 1], c[..., 2]
    one = F32(1)
    fh = h.astype(F32) * F32(6) / F32(255)
    i = np.floor(fh)
    f = fh - i
    fs = s.astype(F32) / F32(255)
    vf = v.astype(F32)

    def rnd(a):
        assert a.dtype == F32
        return np.clip(np.floor(a + F32(0.5)).astype(np.int32), 0, 255)

    p = rnd(vf * (one - fs))
    q = rnd(vf * (one - fs * f))
    t = rnd(vf * (one - fs * (one - f)))
    sel = i.astype(np.int32) % 6
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = np.zeros(c.shape, np.int32)
    for k, cols in enumerate(table):
        m = sel == k
        for ch in range(3):
            out[..., ch] = np.where(m, cols[ch], out[..., ch])
    out = np.where((s == 0)[..., None], v[..., None], out)
    return out.astype(np.uint8)


def hue(rgb, shift: int):
    hsv = rgb_to_hsv(rgb).astype(np.int32)
    hsv[..., 0] = (hsv[..., 0] + int(shift)) & 255
    return hsv_to_rgb(hsv.astype(np.uint8))


def jitter(rgb, p) -> np.ndarray:
    """The four ops on one image in the order of the record ``p`` (one element of a PARAMS_DTYPE array)."""
    for op in unpack_order(p["order"]):
        if op == OP_BRIGHTNESS:
            rgb = brightness(rgb, p["brightness"])
        elif op == OP_CONTRAST:
            rgb = contrast(rgb, p["contrast"])
        elif op == OP_SATURATION:
            rgb = saturation(rgb, p["saturation"])
        else:
            rgb = hue(rgb, p["hue_shift"])
    return rgb


def batch(rgb, depth, label, pos, grad, idx, params=None, normalize=True):
    """occ_augment_batch: rgb (M,S,S,3) u8, depth (M,S,S) i16, label (M,S,S) 0/1, pos / grad (M,2) f32, idx (n,).
    Returns out_img (n,4,S,S), out_label (n,1,S,S), out_grad (n,2), out_pos (n,2), all f32."""
    idx = np.asarray(idx, np.int64)
    n, S = len(idx), rgb.shape[1]
    out_img = np.empty((n, 4, S, S), F32)
    out_label = np.empty((n, 1, S, S), F32)
    for i, m in enumerate(idx):
        c, d, l = rgb[m], depth[m], label[m]
        if params is not None:
            if params[i]["jitter"]:
                c = jitter(c, params[i])
            if params[i]["flip"]:
                c, d, l = c[:, ::-1], d[:, ::-1], l[:, ::-1]
        x = np.concatenate([c.astype(F32) / F32(255), (d.astype(F32) / F32(255))[..., None]], -1)
        if normalize:
            x = (x - F32(0.5)) / F32(0.25)
        assert x.dtype == F32
        out_img[i] = np.transpose(x, (2, 0, 1))
        out_label[i, 0] = (l != 0).astype(F32)
    return out_img, out_label, np.asarray(grad, F32)[idx].copy(), np.asarray(pos, F32)[idx].copy()


def mean_edge_image(S: int, k: int, below: bool) -> np.ndarray:
    """A grey (S,S,3) image whose mean luminance is exactly k + 0.5 (``below``: k + 0.5 - 1 / S^2); S even.  Grey g has
    L = g, so half the pixels at k and half at k + 1 give k + 0.5, and one pixel lowered by one level the value below."""
    assert S % 2 == 0 and 1 <= k < 254
    g = np.full(S * S, k, np.uint8)
    g[::2] = k + 1
    if below:
        g[0] = k  # g[0] was k + 1
    img = np.repeat(g.reshape(S, S)[..., None], 3, -1)
    assert int(luminance(img).sum()) * 2 == (2 * k + 1) * S * S - (2 if below else 0)
    return img
