"""Generates tests/golden/segmenter_golden.npz from the reference's own model.py: FullNetwork(8, dilation=2,
separable=True) and Segmenter(8), built in f64 eval mode.  Run once, at authoring time only, with the reference's
directory given (its model.py is imported from there, nothing of it is copied):

    python tests/golden/make_segmenter_golden.py /path/to/reference

Weights, BN statistics and inputs come from numpy.random.default_rng seeds in state-dict key order
(tests/segmenter_model.py: make_seg_state_dict; tests/encoder_model.py: make_obs), so only key names, shapes, the seeds and
gains and the outputs are stored; the tests regenerate the rest.  To stay under the size limit of a committed file the
logits are stored in f64 for S = 64 and 96 and as the float32 rounding of the f64 result for S = 128; the probabilities
(a function of the logits) and the Segmenter's (N,8,S,S) features (S = 64 only) as float32 roundings as well.  Keys ending
in ``_f32`` say so.

A fixture on which the decoder is dead or swamped by the skips would let a broken transposed conv pass, so per decoder
level and per input this script asserts: 20-80 % of the up conv's pre-ReLU values are positive; the RMS of the up term is
within [0.25, 4] x the RMS of the skip term; at least 10 % of the final logits lie on each side of 0; at most 0.1 % of the
pixels have |logit| <= 1e-4 * max(1, max |logit|) (the only pixels on which a thresholded f32 map may differ).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, sys.argv[1])
import model as ref_model  # noqa: E402

from tests.encoder_model import make_obs  # noqa: E402
from tests.segmenter_model import PRESETS, decode, encode_full, exempt_band, make_seg_state_dict  # noqa: E402

# preset: (seed, gain, up_gain, cls_gain, cls_bias or nan = as drawn).  With the classifier bias as drawn 99.7 % of the
# Segmenter's logits were positive (its thresholded map would test nothing); -0.6 puts 34-39 % of them above 0.
WEIGHTS = {"ppo": (20261020, 0.5, 1.0, 1.0, float("nan")), "segmenter": (20261021, 0.5, 1.0, 1.0, -0.6)}
INPUTS = [(2, 64, 101), (1, 96, 104), (1, 128, 103)]  # (N, S, seed)
torch.set_grad_enabled(False)
out = {"inputs": np.array(INPUTS)}
for preset, (seed, gain, up_gain, cls_gain, cls_bias) in WEIGHTS.items():
    net = ref_model.FullNetwork(8, dilation=2, separable=True) if preset == "ppo" else ref_model.Segmenter(8)
    net = net.double().eval()
    ref_sd = net.state_dict()
    keys = list(ref_sd)
    shapes = [tuple(v.shape) for v in ref_sd.values()]
    sd = make_seg_state_dict(keys, shapes, int(seed), gain, up_gain, cls_gain, None if cls_bias != cls_bias else cls_bias)
    net.load_state_dict(sd)
    p = PRESETS[preset]
    out[f"{preset}_keys"] = np.array(keys)
    out[f"{preset}_shapes"] = np.array([",".join(map(str, s)) for s in shapes])
    out[f"{preset}_weights"] = np.array([seed, gain, up_gain, cls_gain, cls_bias], dtype=np.float64)
    for n, img, iseed in INPUTS:
        obs = make_obs(iseed, n, img)
        if preset == "ppo":
            _pooled, prob, _grad = net(obs)
            logit = net.segmenter(net.encoder(obs))
            feats = None
        else:
            feats, prob = net(obs)
            logit = net.classifier(feats)
        assert torch.equal(torch.sigmoid(logit), prob)
        stats = []
        x, skips = encode_full(sd, obs, p["prefix"], preset == "ppo", p["dilation"], p["residual"])
        mine = decode(sd, x, skips, p["decoder"], stats)
        if feats is not None:
            assert torch.allclose(mine, feats, rtol=1e-12, atol=1e-12)
        pos, ratio = [], []
        for j, (pre, up, skip) in enumerate(stats):
            pos.append(float((pre > 0).double().mean()))
            ratio.append(float(up.pow(2).mean().sqrt() / skip.pow(2).mean().sqrt()))
            assert 0.2 <= pos[-1] <= 0.8, (preset, img, j, pos[-1])
            assert 0.25 <= ratio[-1] <= 4.0, (preset, img, j, ratio[-1])
        share_pos = float((logit > 0).double().mean())
        band = float(exempt_band(logit).double().mean())
        print(preset, n, img, "pre-ReLU positive", [round(v, 2) for v in pos], "up/skip RMS", [round(v, 2) for v in ratio],
              "logits > 0: %.3f" % share_pos, "max|logit| %.3g" % float(logit.abs().max()), "exempt band %.4f %%" % (100 * band))
        assert 0.1 <= share_pos <= 0.9, (preset, img, share_pos)
        assert band <= 1e-3, (preset, img, band)
        if img <= 96:
            out[f"{preset}_logit_{img}"] = logit.numpy()
        else:
            out[f"{preset}_logit_{img}_f32"] = logit.numpy().astype(np.float32)
        out[f"{preset}_prob_{img}_f32"] = prob.numpy().astype(np.float32)
        if feats is not None and img == 64:
            out[f"{preset}_features_{img}_f32"] = feats.numpy().astype(np.float32)
path = os.path.join(HERE, "segmenter_golden.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
assert os.path.getsize(path) < 1 << 20
