"""tests/augment_model.py, the yardstick of the device input pipeline (csrc/occ_augment.hpp), against PIL alone: the calls
below are what torchvision's ColorJitter makes for a PIL image (ImageEnhance.Brightness / Contrast / Color; for the hue
split, wrap-add on the H band, merge, convert back).  Every comparison is exact.  No GPU.
"""
import itertools

import numpy as np
import pytest
from PIL import Image, ImageEnhance

from tests import augment_model as am

BLEND_FACTORS = [0.7, 0.8613, 1.0, 1.1377, 1.3]
HUE_FACTORS = [-0.1, -0.0371, 0.0, 0.0642, 0.1]


def _image(seed, S=32):
    return np.random.default_rng(seed).integers(0, 256, (S, S, 3), dtype=np.uint8)


def _colours():
    """2^18 seeded random colours and the 16-step lattice (with 255), as one (512, W, 3) image."""
    rnd = np.random.default_rng(5).integers(0, 256, (1 << 18, 3), dtype=np.uint8)
    steps = np.array(list(range(0, 256, 16)) + [255], np.uint8)
    lattice = np.stack(np.meshgrid(steps, steps, steps, indexing="ij"), -1).reshape(-1, 3)
    pad = (-len(lattice)) % 512
    both = np.concatenate([rnd, lattice, np.zeros((pad, 3), np.uint8)])
    return np.ascontiguousarray(both.reshape(512, -1, 3))


def pil_hue(rgb, hue_factor):
    """torchvision's adjust_hue for a PIL image."""
    h, s, v = Image.fromarray(rgb).convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.int32(hue_factor * 255).astype(np.uint8)
    return np.asarray(Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB"))


PIL_OPS = {
    am.OP_BRIGHTNESS: lambda rgb, p: np.asarray(ImageEnhance.Brightness(Image.fromarray(rgb)).enhance(float(p["brightness"]))),
    am.OP_CONTRAST: lambda rgb, p: np.asarray(ImageEnhance.Contrast(Image.fromarray(rgb)).enhance(float(p["contrast"]))),
    am.OP_SATURATION: lambda rgb, p: np.asarray(ImageEnhance.Color(Image.fromarray(rgb)).enhance(float(p["saturation"]))),
}


def test_rgb_to_hsv_is_pils():
    cols = _colours()
    want = np.asarray(Image.fromarray(cols).convert("HSV"))
    assert int((am.rgb_to_hsv(cols) != want).any(-1).sum()) == 0


def test_hsv_to_rgb_is_pils():
    cols = _colours()
    want = np.asarray(Image.fromarray(cols, "HSV").convert("RGB"))
    assert int((am.hsv_to_rgb(cols) != want).any(-1).sum()) == 0


@pytest.mark.parametrize("f", BLEND_FACTORS)
def test_blend_ops_are_image_enhance(f):
    for seed in (1, 2):
        img = _image(seed)
        img[0, :4] = 0
        img[1, :4] = 255
        p = am.make_params(1)[0]
        p["brightness"] = p["contrast"] = p["saturation"] = f
        assert np.array_equal(am.brightness(img, p["brightness"]), PIL_OPS[am.OP_BRIGHTNESS](img, p))
        assert np.array_equal(am.contrast(img, p["contrast"]), PIL_OPS[am.OP_CONTRAST](img, p))
        assert np.array_equal(am.saturation(img, p["saturation"]), PIL_OPS[am.OP_SATURATION](img, p))


@pytest.mark.parametrize("hf", HUE_FACTORS)
def test_hue_op_is_the_h_band_shift(hf):
    img = _image(3)
    assert np.array_equal(am.hue(img, am.hue_shift_of(hf)), pil_hue(img, hf))


def test_hue_shift_is_truncation_then_wrap():
    assert [am.hue_shift_of(h) for h in (0.0, 0.1, -0.1, 0.0039, -0.0039, 0.5, -0.5)] == [0, 25, 231, 0, 0, 127, 129]
    for h in HUE_FACTORS:
        assert am.hue_shift_of(h) == int(np.int32(h * 255).astype(np.uint8))


def test_all_24_orders_of_the_chain():
    img = _image(4)
    p = am.make_params(1)[0]
    p["brightness"], p["contrast"], p["saturation"], p["jitter"] = 1.21, 0.77, 1.13, 1
    hf = -0.083
    p["hue_shift"] = am.hue_shift_of(hf)
    seen = set()
    for ops in itertools.permutations(range(4)):
        p["order"] = am.pack_order(ops)
        assert am.unpack_order(p["order"]) == list(ops)
        want = img
        for op in ops:
            want = pil_hue(want, hf) if op == am.OP_HUE else PIL_OPS[op](want, p)
        got = am.jitter(img, p)
        assert np.array_equal(got, want), ops
        seen.add(got.tobytes())
    assert len(seen) > 12  # the order matters: the test would not notice a model that ignored it otherwise


@pytest.mark.parametrize("S", [32, 40])
@pytest.mark.parametrize("below", [False, True])
def test_contrast_mean_rounding_edge(S, below):
    """Mean L exactly k + 0.5 rounds up to k + 1; one level less in one pixel, k + 0.5 - 1 / S^2, rounds down to k."""
    k = 101
    img = am.mean_edge_image(S, k, below)
    assert am.mean_luminance(img) == (k if below else k + 1)
    for f in (0.7, 1.3):
        p = am.make_params(1)[0]
        p["contrast"] = f
        assert np.array_equal(am.contrast(img, f), PIL_OPS[am.OP_CONTRAST](img, p))
    # the two means give different images, so the comparison above tells them apart
    assert not np.array_equal(am.contrast(img, 0.7, mean=k), am.contrast(img, 0.7, mean=k + 1))


def test_batch_converts_flips_and_gathers():
    rng = np.random.default_rng(6)
    M, S = 3, 8
    rgb = rng.integers(0, 256, (M, S, S, 3), dtype=np.uint8)
    depth = rng.integers(-20, 301, (M, S, S)).astype(np.int16)
    label = rng.integers(0, 2, (M, S, S)).astype(np.uint8)
    pos, grad = rng.normal(size=(M, 2)).astype(np.float32), rng.normal(size=(M, 2)).astype(np.float32)
    p = am.make_params(2)
    p["flip"] = [0, 1]
    img, lab, g, q = am.batch(rgb, depth, label, pos, grad, [2, 2], p, normalize=False)
    assert img.dtype == np.float32 and img.shape == (2, 4, S, S) and lab.shape == (2, 1, S, S)
    assert np.array_equal(img[0, :3], np.transpose(rgb[2], (2, 0, 1)).astype(np.float32) / np.float32(255))
    assert np.array_equal(img[0, 3], depth[2].astype(np.float32) / np.float32(255))
    assert np.array_equal(img[1], img[0][..., ::-1]) and np.array_equal(lab[1], lab[0][..., ::-1])
    assert np.array_equal(g, grad[[2, 2]]) and np.array_equal(q, pos[[2, 2]])
    norm = am.batch(rgb, depth, label, pos, grad, [2, 2], p, normalize=True)[0]
    assert np.array_equal(norm, (img - np.float32(0.5)) / np.float32(0.25))
