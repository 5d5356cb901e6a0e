"""The host model of the frozen encoder (tests/encoder_model.py) against the fixture the reference's own model.py produced
(tests/golden/encoder_golden.npz), and the encoder loader's parsing, validation and BatchNorm folding.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from occlusionenv_amd import encoder as E
from tests.encoder_model import golden_state_dict, make_obs, preset_forward

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("preset", ["ppo", "predictor"])
def test_host_model_matches_reference_fixture(golden, preset):
    sd = golden_state_dict(golden, preset)
    for n, img, seed in golden["inputs"]:
        f, gpred = preset_forward(sd, make_obs(int(seed), int(n), int(img)), preset)
        want_f, want_g = golden[f"{preset}_feat_{img}"], golden[f"{preset}_grad_{img}"]
        assert f.shape == (n, 256) and gpred.shape == (n, 2)
        assert np.abs(f.numpy() - want_f).max() <= 1e-10 * max(1.0, np.abs(want_f).max())
        assert np.abs(gpred.numpy() - want_g).max() <= 1e-10 * max(1.0, np.abs(want_g).max())


def test_fixture_is_small_and_holds_no_weights(golden):
    assert os.path.getsize(GOLDEN) < 100_000
    assert not any(k.endswith("weight") for k in golden.files)
    assert golden["ppo_keys"][0].startswith("encoder.") and "gradPredictor.weight" in set(golden["ppo_keys"])
    assert golden["predictor_keys"][0].startswith("features.") and "output.weight" in set(golden["predictor_keys"])


def test_packed_size_matches_library():
    from occlusionenv_amd import _native as nat

    lib = nat.load()
    for sep in (0, 1):
        cfg = nat.OccEncoderConfig(64, 2, 1, sep)
        assert lib.occ_encoder_packed_floats(ctypes.byref(cfg)) == E.packed_floats(bool(sep))
    assert E.packed_floats(True) < E.packed_floats(False)
    bad = nat.OccEncoderConfig(64, 2, 1, 3)
    assert lib.occ_encoder_packed_floats(ctypes.byref(bad)) == -1
    nbytes = ctypes.c_size_t()
    assert lib.occ_encoder_workspace_query(ctypes.byref(nat.OccEncoderConfig(256, 2, 1, 1)), 4, ctypes.byref(nbytes)) == 0
    assert nbytes.value == 3 * 4 * 8 * 256 * 256 * 4 + 4 * 256 * 4  # three level-0 buffers + one 8x8 tile per env
    for cfg in (nat.OccEncoderConfig(31, 2, 1, 1), nat.OccEncoderConfig(1025, 2, 1, 1), nat.OccEncoderConfig(64, 3, 1, 1)):
        assert lib.occ_encoder_workspace_query(ctypes.byref(cfg), 4, ctypes.byref(nbytes)) == 1
    p = ctypes.c_void_p(16)
    assert lib.occ_encoder_forward(ctypes.byref(nat.OccEncoderConfig(64, 2, 1, 1)), p, p, 1, p, 0, p, None) == 1  # ws too small
    assert lib.occ_encoder_forward(None, p, p, 1, p, 1 << 30, p, None) == 1


def _unpack(buf, separable, sd, prefix):
    """Every layer of the packed buffer back in state-dict form; the BN scale / shift checked against the f64 fold."""
    off = 0
    for stem, cin, cout, sep, _ in E.layer_plan(separable):
        stem = prefix + stem
        if sep:
            dv = buf[off:off + 3 * cin].reshape(cin, 3); off += 3 * cin
            dh = buf[off:off + 3 * cin].reshape(cin, 3); off += 3 * cin
            pw = buf[off:off + cin * cout].reshape(cin, cout); off += cin * cout
            np.testing.assert_array_equal(dv, sd[stem + "conv.0.weight"][:, 0, :, 0].float().numpy())
            np.testing.assert_array_equal(dh, sd[stem + "conv.1.weight"][:, 0, 0, :].float().numpy())
            np.testing.assert_array_equal(pw.T, sd[stem + "conv.2.weight"][:, :, 0, 0].float().numpy())
            bias_key = stem + "conv.2.bias"
        else:
            w = buf[off:off + 9 * cin * cout].reshape(cin, 3, 3, cout); off += 9 * cin * cout
            np.testing.assert_array_equal(w.transpose(3, 0, 1, 2), sd[stem + "conv.weight"].float().numpy())
            bias_key = stem + "conv.bias"
        bias, scale, shift = (buf[off + i * cout:off + (i + 1) * cout] for i in range(3))
        off += 3 * cout
        np.testing.assert_array_equal(bias, sd[bias_key].float().numpy())
        g, b = sd[stem + "bn.weight"].numpy(), sd[stem + "bn.bias"].numpy()
        m, v = sd[stem + "bn.running_mean"].numpy(), sd[stem + "bn.running_var"].numpy()
        s64 = g / np.sqrt(v + 1e-5)
        np.testing.assert_allclose(scale, s64, rtol=1e-7)
        np.testing.assert_allclose(shift, b - m * s64, rtol=1e-6, atol=1e-7)
        # the fold is the eval-mode BN: relu(x) * scale + shift == (relu(x) - mean) / sqrt(var + eps) * gamma + beta
        x = np.linspace(-2, 3, cout)
        r = np.maximum(x, 0)
        np.testing.assert_allclose(r * scale + shift, (r - m) / np.sqrt(v + 1e-5) * g + b, rtol=1e-5, atol=1e-6)
    assert off == buf.size


@pytest.mark.parametrize("preset", ["ppo", "predictor"])
def test_packing_and_bn_folding(golden, preset):
    sd = golden_state_dict(golden, preset)
    prefix = E.PRESETS[preset][0]
    sep, buf, offsets = E.pack_state_dict(sd, prefix)
    assert sep == (preset == "ppo") and buf.dtype == np.float32 and buf.size == E.packed_floats(sep)
    assert len(offsets) == 16 and offsets[0] == 0
    _unpack(buf, sep, sd, prefix)


def test_key_prefixes_of_the_presets(golden):
    ppo, pred = golden_state_dict(golden, "ppo"), golden_state_dict(golden, "predictor")
    assert E.pack_state_dict(ppo, "encoder.")[0] is True
    assert E.pack_state_dict(pred, "features.")[0] is False
    with pytest.raises(ValueError, match="no key starts with 'features.'"):
        E.pack_state_dict(ppo, "features.")
    with pytest.raises(ValueError, match="no key starts with 'encoder.'"):
        E.pack_state_dict(pred, "encoder.")
    with pytest.raises(ValueError, match="unknown preset"):
        E.FrozenEncoder.from_state_dict(ppo, preset="segmenter")


def _broken(golden, how):
    sd = dict(golden_state_dict(golden, "ppo"))
    if how == "ch":
        sd["encoder.initial.conv.2.weight"] = torch.zeros(16, 4, 1, 1, dtype=torch.float64)
    elif how == "levels6":
        sd["encoder.features.5.down.conv.weight"] = torch.zeros(512, 256, 3, 3, dtype=torch.float64)
    elif how == "levels4":
        sd = {k: v for k, v in sd.items() if not k.startswith("encoder.features.4.")}
    elif how == "layer3":
        sd["encoder.features.0.net.Layer 3.conv.0.weight"] = torch.zeros(8, 1, 3, 1, dtype=torch.float64)
    elif how == "k5":
        sd["encoder.features.0.down.conv.weight"] = torch.zeros(16, 8, 5, 5, dtype=torch.float64)
    elif how == "k5sep":
        sd["encoder.features.1.net.Layer 2.conv.0.weight"] = torch.zeros(16, 1, 5, 1, dtype=torch.float64)
    elif how == "missing":
        del sd["encoder.features.2.net.Layer 1.bn.running_var"]
    elif how == "missing_initial":
        sd = {k: v for k, v in sd.items() if not k.startswith("encoder.initial.conv")}
    return sd


@pytest.mark.parametrize("how,match", [("ch", "ch = 16"), ("levels6", "levels"), ("levels4", "levels"), ("layer3", "layers"),
                                       ("k5", "k=3"), ("k5sep", "k=3"), ("missing", "missing key"),
                                       ("missing_initial", "missing key")])
def test_loader_rejects_what_does_not_give_256_features(golden, how, match):
    with pytest.raises(ValueError, match=match):
        E.pack_state_dict(_broken(golden, how), "encoder.")
    with pytest.raises(ValueError, match=match):
        E.FrozenEncoder.from_state_dict(_broken(golden, how), preset="ppo", device="cpu")


def test_cpu_device_raises_native_error(golden):
    from occlusionenv_amd._native import NativeError

    with pytest.raises(NativeError):
        E.FrozenEncoder.from_state_dict(golden_state_dict(golden, "ppo"), device="cpu")
