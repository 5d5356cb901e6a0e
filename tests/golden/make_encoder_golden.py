"""Generates tests/golden/encoder_golden.npz from the reference's own model.py (FullNetwork and PredictorNet, built in
f64 eval mode).  Run once, in the authoring container only:

    python tests/golden/make_encoder_golden.py

Weights, BN statistics and inputs come from numpy.random.default_rng seeds in state-dict key order
(tests/encoder_model.py: make_state_dict, make_obs), so only key names, shapes, the configuration and the outputs are
stored; the tests regenerate the rest.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, "/root/reference")
import model as ref_model  # noqa: E402

from tests.encoder_model import encode, make_obs, make_state_dict  # noqa: E402

SEEDS = {"ppo": 20261016, "predictor": 20261017}
GAINS = {"ppo": 0.5, "predictor": 2.0}
INPUTS = [(2, 64, 101), (1, 100, 102), (1, 128, 103)]  # (N, S, seed)
torch.set_grad_enabled(False)
out = {"inputs": np.array(INPUTS)}
for preset, seed in SEEDS.items():
    net = ref_model.FullNetwork(8, dilation=2, separable=True) if preset == "ppo" else ref_model.PredictorNet(8)
    net = net.double().eval()
    ref_sd = net.state_dict()
    keys = list(ref_sd)
    shapes = [tuple(v.shape) for v in ref_sd.values()]
    sd = make_state_dict(keys, shapes, seed, GAINS[preset])
    net.load_state_dict(sd)
    prefix = "encoder." if preset == "ppo" else "features."
    out[f"{preset}_keys"] = np.array(keys)
    out[f"{preset}_shapes"] = np.array([",".join(map(str, s)) for s in shapes])
    out[f"{preset}_config"] = np.array([seed, 2 if preset == "ppo" else 1, preset == "ppo", preset == "ppo"], dtype=np.int64)
    out[f"{preset}_gain"] = np.array(GAINS[preset])
    for n, img, iseed in INPUTS:
        obs = make_obs(iseed, n, img)
        if preset == "ppo":
            enc_out, _feats = net.encoder(obs)
            pooled = net.pool(enc_out).reshape(n, 256)
            grad = net.gradPredictor(pooled)
        else:
            enc_out, _feats = net.features(obs)
            pooled = net.pool(enc_out).reshape(n, 256)
            grad = torch.tanh(net.output(pooled))
        # the activations must stay alive: 20-80 % of every level's pre-ReLU values positive
        pre = []
        mine = encode(sd, obs, prefix, preset == "ppo", 2 if preset == "ppo" else 1, preset == "ppo", pre_relu=pre)
        assert torch.allclose(mine, pooled, rtol=1e-12, atol=1e-12)
        for lv in range(-1, 5):
            vals = torch.cat([t.reshape(-1) for l, t in pre if l == lv])
            frac = float((vals > 0).double().mean())
            assert 0.2 <= frac <= 0.8, (preset, img, lv, frac)
        print(preset, n, img, "max|f|", float(pooled.abs().max()), "grad", grad.reshape(n, 2)[0].tolist(),
              "pos", [round(float((torch.cat([t.reshape(-1) for l, t in pre if l == lv]) > 0).double().mean()), 2) for lv in range(-1, 5)])
        out[f"{preset}_feat_{img}"] = pooled.numpy()
        out[f"{preset}_grad_{img}"] = grad.reshape(n, 2).numpy()
path = os.path.join(HERE, "encoder_golden.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
