"""The host model of the segmentation decoder (tests/segmenter_model.py) against the fixture the reference's own model.py
produced (tests/golden/segmenter_golden.npz), a hand-computed transposed convolution, the decoder loader's parsing,
validation and BatchNorm folding, and the argument checks of the decoder's C entry points.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from occlusionenv_amd import encoder as E
from tests.encoder_model import make_obs
from tests.segmenter_model import PRESETS, exempt_band, full_forward, golden_seg_state_dict, tr_conv, up_conv

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segmenter_golden.npz")
F32 = 2.0 ** -23  # relative rounding of the values the fixture stores as float32


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _close(got, want, tol):
    return np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("preset", ["ppo", "segmenter"])
def test_host_model_matches_reference_fixture(golden, preset):
    sd = golden_seg_state_dict(golden, preset)
    for n, img, seed in golden["inputs"]:
        out = full_forward(sd, make_obs(int(seed), int(n), int(img)), preset)
        assert out["prob"].shape == (n, 1, img, img) and out["features"].shape == (n, 8, img, img)
        key = f"{preset}_logit_{img}"
        if key in golden.files:
            assert golden[key].dtype == np.float64 and _close(out["logit"].numpy(), golden[key], 1e-10)
        else:  # stored as the float32 rounding of the f64 result
            assert _close(out["logit"].numpy(), golden[key + "_f32"].astype(np.float64), F32)
        assert _close(out["prob"].numpy(), golden[f"{preset}_prob_{img}_f32"].astype(np.float64), F32)
        key = f"{preset}_features_{img}_f32"
        if key in golden.files:
            assert _close(out["features"].numpy(), golden[key].astype(np.float64), F32)
        # the fixture's thresholded map is not trivial and (almost) nowhere undecided
        share = float((out["logit"] > 0).double().mean())
        assert 0.1 <= share <= 0.9 and float(exempt_band(out["logit"]).double().mean()) <= 1e-3
    assert "segmenter_features_64_f32" in golden.files


def test_fixture_is_small_and_holds_no_weights(golden):
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert not any(k.endswith("weight") for k in golden.files)
    assert "segmenter.0.features.0.up.conv.weight" in set(golden["ppo_keys"]) and "segmenter.1.bias" in set(golden["ppo_keys"])
    assert "decoder.features.4.up.conv.weight" in set(golden["segmenter_keys"]) and "classifier.weight" in set(golden["segmenter_keys"])
    assert [tuple(r) for r in golden["inputs"]] == [(2, 64, 101), (1, 96, 104), (1, 128, 103)]


def test_transposed_conv_known_answer():
    """ConvTranspose2d(1, 1, 3, stride 2, padding 1, output_padding 1) on a 2 x 2 input with nine distinct taps, every one
    of the 16 outputs written out by hand: out[oy][ox] = sum over x[iy][ix] * w[ky][kx] with oy = 2 iy - 1 + ky,
    ox = 2 ix - 1 + kx.  A flipped or transposed kernel index changes these numbers."""
    x = torch.tensor([[1.0, 2.0], [3.0, 4.0]], dtype=torch.float64).reshape(1, 1, 2, 2)
    w = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]], dtype=torch.float64).reshape(1, 1, 3, 3)  # w[ky][kx]
    a, b, c, d = 1.0, 2.0, 3.0, 4.0
    w00, w01, w02, w10, w11, w12, w20, w21, w22 = range(1, 10)
    want = [
        [a * w11, a * w12 + b * w10, b * w11, b * w12],
        [a * w21 + c * w01, a * w22 + b * w20 + c * w02 + d * w00, b * w21 + d * w01, b * w22 + d * w02],
        [c * w11, c * w12 + d * w10, d * w11, d * w12],
        [c * w21, c * w22 + d * w20, d * w21, d * w22],
    ]
    assert want == [[5, 14, 10, 12], [14, 36, 24, 30], [15, 34, 20, 24], [24, 55, 32, 36]]
    sd = {"u.conv.weight": w, "u.conv.bias": torch.tensor([0.5], dtype=torch.float64),
          "u.bn.weight": torch.tensor([2.0], dtype=torch.float64), "u.bn.bias": torch.tensor([-1.0], dtype=torch.float64),
          "u.bn.running_mean": torch.tensor([3.0], dtype=torch.float64), "u.bn.running_var": torch.tensor([4.0], dtype=torch.float64)}
    got = up_conv(x, sd, "u.")
    assert got.shape == (1, 1, 4, 4)
    assert torch.equal(got[0, 0], torch.tensor(want, dtype=torch.float64) + 0.5)
    # TrConv: BN after the ReLU
    full = tr_conv(x, sd, "u.")[0, 0]
    ref = (torch.relu(torch.tensor(want, dtype=torch.float64) + 0.5) - 3.0) / np.sqrt(4.0 + 1e-5) * 2.0 - 1.0
    assert torch.allclose(full, ref, rtol=1e-14, atol=0)


def test_packed_up_layer_feeds_the_quad_formula(golden):
    """The packed layout w[ci][ky * 3 + kx][co] read the way the kernel reads it (a thread's 2 x 2 output quad from the
    four inputs a, b, c, d and nine taps, each used once) reproduces conv_transpose2d, including the zero row / column beyond
    the edge."""
    sd = golden_seg_state_dict(golden, "ppo")
    buf = E.pack_decoder(sd, "segmenter.0.features.", "segmenter.1.")
    j, cin, cout = E.decoder_plan()[4]
    off = sum(9 * ci * co + 3 * co for _, ci, co in E.decoder_plan()[:4])
    w = torch.from_numpy(buf[off:off + 9 * cin * cout].astype(np.float64)).reshape(cin, 9, cout)
    x = torch.randn(1, cin, 5, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    xp = F.pad(x, (0, 1, 0, 1))[0]  # zero beyond the edge
    a, b, c, d = xp[:, :5, :5], xp[:, :5, 1:], xp[:, 1:, :5], xp[:, 1:, 1:]
    t = lambda v, k: torch.einsum("iyx,io->oyx", v, w[:, k])  # noqa: E731
    out = torch.zeros(cout, 10, 10, dtype=torch.float64)
    out[:, 0::2, 0::2] = t(a, 4)
    out[:, 0::2, 1::2] = t(a, 5) + t(b, 3)
    out[:, 1::2, 0::2] = t(a, 7) + t(c, 1)
    out[:, 1::2, 1::2] = t(a, 8) + t(b, 6) + t(c, 2) + t(d, 0)
    w32 = sd[f"segmenter.0.features.{j}.up.conv.weight"].float().double()
    want = F.conv_transpose2d(x, w32, None, stride=2, padding=1, output_padding=1)[0]
    assert torch.allclose(out, want, rtol=1e-12, atol=1e-12)


def test_packed_size_and_argument_checks_need_no_gpu():
    from occlusionenv_amd import _native as nat

    lib = nat.load()
    assert E.decoder_packed_floats() == sum(9 * 2 * c * c + 3 * c for c in (128, 64, 32, 16, 8)) + 9
    for sep in (0, 1):
        assert lib.occ_decoder_packed_floats(ctypes.byref(nat.OccEncoderConfig(64, 2, 1, sep))) == E.decoder_packed_floats()
    assert lib.occ_decoder_packed_floats(ctypes.byref(nat.OccEncoderConfig(64, 2, 1, 3))) == -1
    assert lib.occ_decoder_packed_floats(None) == -1
    nbytes, enc_bytes = ctypes.c_size_t(), ctypes.c_size_t()
    cfg = nat.OccEncoderConfig(256, 2, 1, 1)
    assert lib.occ_segment_workspace_query(ctypes.byref(cfg), 4, ctypes.byref(nbytes)) == 0
    buf = 4 * 8 * 256 * 256 * 4
    # two activation buffers, the skips (1 + 1/2 + 1/4 + 1/8 + 1/16 buffers), the last down output, one 8x8 pool tile per env
    assert nbytes.value == 2 * buf + (buf + buf // 2 + buf // 4 + buf // 8 + buf // 16) + 4 * 256 * 8 * 8 * 4 + 4 * 256 * 4
    assert lib.occ_encoder_workspace_query(ctypes.byref(cfg), 4, ctypes.byref(enc_bytes)) == 0
    assert enc_bytes.value == 3 * buf + 4 * 256 * 4  # the encoder's own workspace is what it was
    for bad in (nat.OccEncoderConfig(100, 2, 1, 1), nat.OccEncoderConfig(48, 2, 1, 1), nat.OccEncoderConfig(1056, 2, 1, 1),
                nat.OccEncoderConfig(64, 3, 1, 1)):
        assert lib.occ_segment_workspace_query(ctypes.byref(bad), 4, ctypes.byref(nbytes)) == 1
    assert lib.occ_segment_workspace_query(ctypes.byref(cfg), 0, ctypes.byref(nbytes)) == 1
    assert lib.occ_segment_workspace_query(ctypes.byref(cfg), 4, None) == 1
    p = ctypes.c_void_p(16)
    big = 1 << 40
    ok = nat.OccEncoderConfig(64, 2, 1, 1)
    fwd = lib.occ_segment_forward
    assert fwd(ctypes.byref(ok), p, p, p, 1, p, 0, p, p, None, None, None) == 1  # workspace too small
    assert fwd(None, p, p, p, 1, p, big, p, p, None, None, None) == 1
    assert fwd(ctypes.byref(nat.OccEncoderConfig(100, 2, 1, 1)), p, p, p, 1, p, big, p, p, None, None, None) == 1  # S % 32
    for hole in range(6):  # each required pointer in turn: enc_packed, dec_packed, obs, ws, feats, prob
        a = [p] * 6
        a[hole] = None
        assert fwd(ctypes.byref(ok), a[0], a[1], a[2], 1, a[3], big, a[4], a[5], None, None, None) == 1
    assert fwd(ctypes.byref(ok), p, p, p, 0, p, big, p, p, None, None, None) == 1
    assert fwd(ctypes.byref(ok), p, p, p, 1, p, big, p, ctypes.c_void_p(20), None, None, None) == 1  # misaligned map
    met = lib.occ_seg_metrics
    assert met(None, p, 1, 1, 64, p, None) == 1 and met(p, None, 1, 1, 64, p, None) == 1 and met(p, p, 1, 1, 64, None, None) == 1
    assert met(p, p, 0, 1, 64, p, None) == 1 and met(p, p, 1, 0, 64, p, None) == 1 and met(p, p, 1, 1, 0, p, None) == 1


def test_pack_decoder_layout_and_bn_folding(golden):
    for preset in ("ppo", "segmenter"):
        sd = golden_seg_state_dict(golden, preset)
        prefix, cls = E.DECODER_KEYS[preset]
        assert (prefix, cls) == (PRESETS[preset]["decoder"], PRESETS[preset]["classifier"])
        buf = E.pack_decoder(sd, prefix, cls)
        assert buf.dtype == np.float32 and buf.size == E.decoder_packed_floats()
        off = 0
        for j, cin, cout in E.decoder_plan():
            stem = f"{prefix}{j}.up."
            w = buf[off:off + 9 * cin * cout].reshape(cin, 3, 3, cout); off += 9 * cin * cout
            np.testing.assert_array_equal(w.transpose(0, 3, 1, 2), sd[stem + "conv.weight"].float().numpy())
            bias, scale, shift = (buf[off + i * cout:off + (i + 1) * cout] for i in range(3))
            off += 3 * cout
            np.testing.assert_array_equal(bias, sd[stem + "conv.bias"].float().numpy())
            # the fold is the eval-mode BN after the ReLU, as F.batch_norm computes it
            r = torch.relu(torch.linspace(-2, 3, 7 * cout, dtype=torch.float64)).reshape(7, cout, 1, 1)
            bn = F.batch_norm(r, sd[stem + "bn.running_mean"], sd[stem + "bn.running_var"], sd[stem + "bn.weight"],
                              sd[stem + "bn.bias"], False, 0.0, 1e-5)
            mine = r * torch.from_numpy(scale.astype(np.float64)).reshape(1, cout, 1, 1) + torch.from_numpy(
                shift.astype(np.float64)).reshape(1, cout, 1, 1)
            assert torch.allclose(mine, bn, rtol=1e-5, atol=1e-6)
        np.testing.assert_array_equal(buf[off:off + 8], sd[cls + "weight"].float().numpy().reshape(-1))
        np.testing.assert_array_equal(buf[off + 8:off + 9], sd[cls + "bias"].float().numpy())
        assert off + 9 == buf.size


def test_dead_net_layers_are_not_needed(golden):
    """TrConvBlock.forward returns self.up(x): a state dict without the decoder blocks' net.* keys packs to the same bytes."""
    sd = golden_seg_state_dict(golden, "ppo")
    dead = [k for k in sd if k.startswith("segmenter.0.features.") and ".net." in k]
    assert len(dead) >= 5 * 2 * 7
    lean = {k: v for k, v in sd.items() if k not in dead}
    a = E.pack_decoder(sd, "segmenter.0.features.", "segmenter.1.")
    b = E.pack_decoder(lean, "segmenter.0.features.", "segmenter.1.")
    assert a.tobytes() == b.tobytes()
    # and garbage in them changes nothing
    for k in dead:
        if sd[k].is_floating_point():
            sd[k] = sd[k] * 0 + 7.0
    assert E.pack_decoder(sd, "segmenter.0.features.", "segmenter.1.").tobytes() == a.tobytes()


def _broken(golden, how):
    sd = dict(golden_seg_state_dict(golden, "ppo"))
    up = "segmenter.0.features.%d.up."
    if how == "missing_up":
        del sd[up % 2 + "conv.weight"]
    elif how == "missing_bn":
        del sd[up % 3 + "bn.running_var"]
    elif how == "channels":
        sd[up % 1 + "conv.weight"] = torch.zeros(128, 32, 3, 3, dtype=torch.float64)
    elif how == "k5":
        sd[up % 4 + "conv.weight"] = torch.zeros(16, 8, 5, 5, dtype=torch.float64)
    elif how == "level6":
        sd[up % 5 + "conv.weight"] = torch.zeros(8, 4, 3, 3, dtype=torch.float64)
    elif how == "levels4":
        sd = {k: v for k, v in sd.items() if not k.startswith("segmenter.0.features.4.")}
    elif how == "no_classifier":
        del sd["segmenter.1.weight"]
    elif how == "classifier_shape":
        sd["segmenter.1.weight"] = torch.zeros(2, 8, 1, 1, dtype=torch.float64)
    return sd


@pytest.mark.parametrize("how,match", [("missing_up", "missing key 'segmenter.0.features.2.up.conv.weight'"), ("missing_bn", "missing key"),
                                       ("channels", "128 -> 32 channels, expected 128 -> 64"), ("k5", "expected"),
                                       ("level6", "levels"), ("levels4", "levels"), ("no_classifier", "missing key"),
                                       ("classifier_shape", "expected")])
def test_loader_rejections(golden, how, match):
    with pytest.raises(ValueError, match=match):
        E.pack_decoder(_broken(golden, how), "segmenter.0.features.", "segmenter.1.")
    with pytest.raises(ValueError, match=match):
        E.FrozenEncoder.from_state_dict(_broken(golden, how), preset="ppo", device="cpu")


def test_presets_and_checkpoints_without_decoder(golden):
    from occlusionenv_amd._native import NativeError

    assert E.PRESETS["segmenter"] == ("encoder.", None, False, 1, True)
    with pytest.raises(ValueError, match="no key starts with"):
        E.pack_decoder({"encoder.x": 0}, "segmenter.0.features.", "segmenter.1.")
    # a Segmenter state dict parses up to the device check (the CPU has no native path)
    with pytest.raises(NativeError):
        E.FrozenEncoder.from_state_dict(golden_seg_state_dict(golden, "segmenter"), preset="segmenter", device="cpu")
    # a FullNetwork state dict is not a Segmenter's, although both keep the encoder under "encoder."
    with pytest.raises(ValueError, match="use preset='ppo'"):
        E.FrozenEncoder.from_state_dict(golden_seg_state_dict(golden, "ppo"), preset="segmenter", device="cpu")
    # a FullNetwork checkpoint without the decoder still loads: parsing reaches the device check
    sd = {k: v for k, v in golden_seg_state_dict(golden, "ppo").items() if not k.startswith("segmenter.")}
    with pytest.raises(NativeError):
        E.FrozenEncoder.from_state_dict(sd, preset="ppo", device="cpu")


def test_image_sides_the_decoder_rejects():
    """S % 32 != 0: ValueError from segment before anything native is touched (checked on an object without a device)."""
    enc = object.__new__(E.FrozenEncoder)
    enc.dec_packed = torch.zeros(1)
    enc.packed = torch.zeros(1)

    class FakeCuda(torch.Tensor):
        is_cuda = True

    for side in (48, 100, 1056):
        obs = torch.zeros(1, 4, side, side).as_subclass(FakeCuda)
        with pytest.raises(ValueError, match="multiple of 32"):
            enc._segment(obs, False, False)
    enc.dec_packed = None
    with pytest.raises(ValueError, match="no segmentation decoder"):
        enc._segment(torch.zeros(1, 4, 64, 64).as_subclass(FakeCuda), False, False)
