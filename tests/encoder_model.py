"""Host model of the frozen encoder (model.py:8-101 in eval mode), restated in torch functional ops from a state dict.

f64 on the CPU is the yardstick of the native encoder (occlusionenv_amd/encoder.py); the same code in f32 on the GPU is
the PyTorch-ROCm baseline of scripts/encoder_bench.py.  Also here: the seeded weights and obs-like inputs of the
fixture tests/golden/encoder_golden.npz, so that tests regenerate them instead of committing them.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

LEVELS = 5
PRESETS = {"ppo": dict(prefix="encoder.", grad="gradPredictor.", tanh=False, dilation=2, residual=True),
           "predictor": dict(prefix="features.", grad="output.", tanh=True, dilation=1, residual=False)}


def conv_bn_relu(x, sd, stem, separable, dilation, stride):
    """Conv.forward: bn(relu(conv(x))) (model.py:8-23); separable = depthwise (3,1) | depthwise (1,3) | pointwise."""
    p = (3 + dilation - 1) // 2
    if separable:
        c = x.shape[1]
        x = F.conv2d(x, sd[stem + "conv.0.weight"], None, 1, (p, 0), (dilation, 1), c)
        x = F.conv2d(x, sd[stem + "conv.1.weight"], None, 1, (0, p), (1, dilation), c)
        x = F.conv2d(x, sd[stem + "conv.2.weight"], sd[stem + "conv.2.bias"])
    else:
        x = F.conv2d(x, sd[stem + "conv.weight"], sd[stem + "conv.bias"], stride, p, dilation)
    x = torch.relu(x)
    return F.batch_norm(x, sd[stem + "bn.running_mean"], sd[stem + "bn.running_var"], sd[stem + "bn.weight"],
                        sd[stem + "bn.bias"], False, 0.0, 1e-5)


def encode(sd, obs, prefix="encoder.", separable=True, dilation=2, residual=True, pre_relu=None):
    """(N,4,S,S) -> (N,256): the average pool of the last down output.  ``pre_relu``: a list that receives, per
    level (initial = -1), the conv outputs before the ReLU (the fixture generator checks them)."""
    def layer(x, stem, sep, d, s, level):
        if pre_relu is not None:
            pre_relu.append((level, _conv_only(x, sd, stem, sep, d, s)))
        return conv_bn_relu(x, sd, stem, sep, d, s)

    x = layer(obs, prefix + "initial.", separable, 1, 1, -1)
    for lv in range(LEVELS):
        stem = f"{prefix}features.{lv}."
        y = layer(x, stem + "net.Layer 1.", separable, dilation, 1, lv)
        y = layer(y, stem + "net.Layer 2.", separable, dilation, 1, lv)
        if residual:
            y = y + x
        x = layer(y, stem + "down.", False, 1, 2, lv)
    return x.mean(dim=(2, 3))


def _conv_only(x, sd, stem, separable, dilation, stride):
    p = (3 + dilation - 1) // 2
    if separable:
        c = x.shape[1]
        x = F.conv2d(x, sd[stem + "conv.0.weight"], None, 1, (p, 0), (dilation, 1), c)
        x = F.conv2d(x, sd[stem + "conv.1.weight"], None, 1, (0, p), (1, dilation), c)
        return F.conv2d(x, sd[stem + "conv.2.weight"], sd[stem + "conv.2.bias"])
    return F.conv2d(x, sd[stem + "conv.weight"], sd[stem + "conv.bias"], stride, p, dilation)


def preset_forward(sd, obs, preset):
    """-> (pooled (N,256), grad prediction (N,2)) of FullNetwork / PredictorNet."""
    p = PRESETS[preset]
    sep = (p["prefix"] + "initial.conv.0.weight") in sd
    f = encode(sd, obs, p["prefix"], sep, p["dilation"], p["residual"])
    g = F.linear(f, sd[p["grad"] + "weight"], sd[p["grad"] + "bias"])
    return f, (torch.tanh(g) if p["tanh"] else g)


# ---- seeded fixtures -----------------------------------------------------------------------------------------------
def make_state_dict(keys, shapes, seed, gain=2.0, dtype=torch.float64):
    """Weights in state-dict key order from numpy.random.default_rng(seed), scaled so that activations stay O(1) through
    all five levels (``gain``: the weight variance times fan-in; the residual preset needs less); BN stats non-trivial
    (var in [0.5, 2], mean != 0, gamma != 1)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for k, shp in zip(keys, shapes):
        shp = tuple(int(s) for s in shp)
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(100, dtype=torch.int64)
            continue
        if ".bn." in k:
            leaf = k.rsplit(".", 1)[1]
            v = {"weight": lambda: rng.uniform(0.6, 1.4, shp), "bias": lambda: rng.normal(0.0, 0.2, shp),
                 "running_mean": lambda: rng.uniform(0.2, 0.8, shp), "running_var": lambda: rng.uniform(0.5, 2.0, shp)}[leaf]()
        elif len(shp) >= 2:
            fan_in = int(np.prod(shp[1:]))
            if len(shp) == 4 and shp[1] == 1:  # depthwise: one tap row per channel
                fan_in = max(shp[2], shp[3])
            v = rng.normal(0.0, 1.0, shp) * np.sqrt(gain / fan_in)
        else:
            v = rng.normal(0.0, 0.1, shp)
        sd[k] = torch.tensor(v, dtype=dtype)
    return sd


def make_obs(seed, n, img, dtype=torch.float64):
    """Observation-like inputs (what venv.step returns): RGB in [0,1] and a depth channel on an elliptic object, RGB = 1
    and depth = -1 on the background."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(img) + 0.5, np.arange(img) + 0.5, indexing="ij")
    out = np.empty((n, 4, img, img))
    for i in range(n):
        cy, cx = rng.uniform(0.3, 0.7, 2) * img
        ry, rx = rng.uniform(0.15, 0.35, 2) * img
        inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0
        shade = 0.5 + 0.5 * np.cos((xx - cx) / rx * 2.0) * np.sin((yy - cy) / ry * 1.5)
        for c in range(3):
            out[i, c] = np.where(inside, np.clip(shade * rng.uniform(0.3, 1.0) + rng.uniform(0, 0.2, (img, img)), 0, 1), 1.0)
        out[i, 3] = np.where(inside, 3.0 + (yy - cy) / img + rng.uniform(-0.05, 0.05, (img, img)), -1.0)
    return torch.tensor(out, dtype=dtype)


def golden_state_dict(g, preset):
    """The full state dict (FullNetwork / PredictorNet keys) of the fixture ``g`` = np.load(encoder_golden.npz)."""
    shapes = [tuple(int(x) for x in s.split(",")) if s else () for s in g[f"{preset}_shapes"]]
    return make_state_dict(list(g[f"{preset}_keys"]), shapes, int(g[f"{preset}_config"][0]), float(g[f"{preset}_gain"]))
