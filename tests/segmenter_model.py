"""Host model of the segmentation decoder (model.py:25-33,52-67,109-166 in eval mode) on top of the encoder's host model
(tests/encoder_model.py), restated in torch functional ops from a state dict.

f64 on the CPU is the yardstick of the native decoder (occlusionenv_amd/encoder.py: segment, forward_full); the same code
in f32 on the GPU is the PyTorch-ROCm baseline of scripts/segmenter_bench.py.  Also here: the seeded weights of the
fixture tests/golden/segmenter_golden.npz.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests.encoder_model import LEVELS, conv_bn_relu, make_state_dict

PRESETS = {"ppo": dict(prefix="encoder.", decoder="segmenter.0.features.", classifier="segmenter.1.", grad="gradPredictor.",
                       dilation=2, residual=True),
           "segmenter": dict(prefix="encoder.", decoder="decoder.features.", classifier="classifier.", grad=None, dilation=1,
                             residual=True)}


def encode_full(sd, obs, prefix="encoder.", separable=True, dilation=2, residual=True):
    """Encoder.forward (model.py:97-107): -> (last down output (N,256,S/32,S/32), [the five per-level features]).  A
    level's feature is Layer 2's output plus the residual when there is one (ConvBlock.forward returns y after y += x)."""
    x = conv_bn_relu(obs, sd, prefix + "initial.", separable, 1, 1)
    skips = []
    for lv in range(LEVELS):
        stem = f"{prefix}features.{lv}."
        y = conv_bn_relu(x, sd, stem + "net.Layer 1.", separable, dilation, 1)
        y = conv_bn_relu(y, sd, stem + "net.Layer 2.", separable, dilation, 1)
        if residual:
            y = y + x
        skips.append(y)
        x = conv_bn_relu(y, sd, stem + "down.", False, 1, 2)
    return x, skips


def up_conv(x, sd, stem):
    """The ConvTranspose2d of a TrConv (model.py:29) alone, before the ReLU."""
    return F.conv_transpose2d(x, sd[stem + "conv.weight"], sd[stem + "conv.bias"], stride=2, padding=1, output_padding=1)


def tr_conv(x, sd, stem):
    """TrConv.forward: bn(relu(conv(x))) (model.py:32-33)."""
    x = torch.relu(up_conv(x, sd, stem))
    return F.batch_norm(x, sd[stem + "bn.running_mean"], sd[stem + "bn.running_var"], sd[stem + "bn.weight"],
                        sd[stem + "bn.bias"], False, 0.0, 1e-5)


def decode(sd, x_last, skips, prefix="segmenter.0.features.", stats=None):
    """Decoder.forward (model.py:118-125): x = block(x) + y, deepest feature first; a block is its ``up`` alone
    (TrConvBlock.forward returns self.up(x), model.py:63-67: the ``net`` layers do not reach the output).  ``stats``: a
    list that receives per level (pre-ReLU values of the up conv, the up term, the skip term)."""
    x = x_last
    for j, y in enumerate(skips[::-1]):
        stem = f"{prefix}{j}.up."
        up = tr_conv(x, sd, stem)
        if stats is not None:
            stats.append((up_conv(x, sd, stem), up, y))
        x = up + y
    return x


def full_forward(sd, obs, preset, dilation=None, residual=None):
    """-> dict(pooled (N,256), features (N,8,S,S), logit (N,1,S,S), prob (N,1,S,S), grad (N,2) or None): FullNetwork.forward
    (model.py:156-166) / Segmenter.forward (model.py:135-140)."""
    p = PRESETS[preset]
    sep = (p["prefix"] + "initial.conv.0.weight") in sd
    x, skips = encode_full(sd, obs, p["prefix"], sep, p["dilation"] if dilation is None else dilation,
                           p["residual"] if residual is None else residual)
    feats = decode(sd, x, skips, p["decoder"])
    logit = F.conv2d(feats, sd[p["classifier"] + "weight"], sd[p["classifier"] + "bias"])
    pooled = x.mean(dim=(2, 3))
    grad = F.linear(pooled, sd[p["grad"] + "weight"], sd[p["grad"] + "bias"]) if p["grad"] else None
    return dict(pooled=pooled, features=feats, logit=logit, prob=torch.sigmoid(logit), grad=grad)


def exempt_band(logit64):
    """Pixels whose thresholded value an f32 evaluation may flip: |logit| <= 1e-4 * max(1, max |logit|)."""
    return logit64.abs() <= 1e-4 * max(1.0, float(logit64.abs().max()))


# ---- seeded fixtures -----------------------------------------------------------------------------------------------
def make_seg_state_dict(keys, shapes, seed, gain, up_gain=1.0, cls_gain=1.0, cls_bias=None, dtype=torch.float64):
    """encoder_model.make_state_dict, then the knobs of the decoder.  make_state_dict takes a fan-in from shape[1:], which
    for a transposed conv's (2c, c, 3, 3) weight is off by about 2x, so the ``up`` weights can be given ``up_gain`` and the
    classifier ``cls_gain`` (factors on the drawn weights); ``cls_bias`` replaces the classifier's drawn bias so that the
    logits straddle 0.  The fixture generator asserts that the resulting decoder is alive (make_segmenter_golden.py)."""
    sd = make_state_dict(keys, shapes, seed, gain, dtype)
    for k in keys:
        if k.endswith(".up.conv.weight"):
            sd[k] = sd[k] * up_gain
        elif k in ("segmenter.1.weight", "classifier.weight"):
            sd[k] = sd[k] * cls_gain
        elif k in ("segmenter.1.bias", "classifier.bias") and cls_bias is not None:
            sd[k] = torch.full_like(sd[k], cls_bias)
    return sd


def golden_seg_state_dict(g, preset):
    """The full state dict of the fixture ``g`` = np.load(segmenter_golden.npz)."""
    shapes = [tuple(int(x) for x in s.split(",")) if s else () for s in g[f"{preset}_shapes"]]
    seed, gain, up_gain, cls_gain, cls_bias = (float(v) for v in g[f"{preset}_weights"])
    return make_seg_state_dict(list(g[f"{preset}_keys"]), shapes, int(seed), gain, up_gain, cls_gain,
                               None if cls_bias != cls_bias else cls_bias)
