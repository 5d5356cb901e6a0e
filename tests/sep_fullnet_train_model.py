"""Host model of the native joint backward of the separable network (csrc/occ_sepfull_bwd.hpp,
occlusionenv_amd/sepfullnet.py): the separable encoder of tests/sep_encoder_train_model.encode_gated (16 gates) composed with
the gated decoder of tests/fullnet_train_model.forward_gated (5 gates), the skips being the encoder's level outputs, with
torch autograd over every parameter, in f64 on the CPU (tests/test_sep_fullnet_train_host.py holds the composition to its two
constituents, bitwise); the two sets of weights of the GPU test; the joint workspace and scratch sizes in plain integers;
and the share of every layer's pixels that lie in the gate band.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import decoder_split_model as dsm
from tests import fullnet_train_model as ftm
from tests import sep_encoder_train_model as stm
from tests.encoder_model import make_obs
from tests.segmenter_model import PRESETS as SEG_PRESETS
from tests.segmenter_model import golden_seg_state_dict, make_seg_state_dict

GOLDEN = ftm.GOLDEN
LEVELS = 5
PRESET = "ppo"
TOL = 1e-4
# the GPU cases of tests/test_gpu_sep_fullnet_train.py: (weights, dilation, residual, S, N)
GRAD_CASES = [("golden", 2, 1, 32, 2), ("golden", 2, 1, 64, 3), ("golden", 2, 1, 96, 2), ("golden", 1, 1, 64, 3),
              ("seeded", 2, 0, 32, 2), ("seeded", 2, 0, 64, 3)]
SPLIT_CASES = [("golden", 2, 1, 64, 130), ("golden", 2, 1, 96, 65)]
CASES = GRAD_CASES + SPLIT_CASES
SEEDED = dict(seed=57, gain=2.0, dec_seed=58, dec_gain=2.0, up_gain=1.4, cls_gain=1.0, cls_bias=-0.3)

ws_bytes = ftm.ws_bytes            # the separable training workspace is the dense one
encoder_ws_bytes = ftm.encoder_ws_bytes
relu_views = ftm.relu_views
kept_relu = ftm.kept_relu


def obs_seed(img, n):
    return 9000 + img + n


def case_obs(img, n):
    """The f64 observation of a GPU case (rounded to f32 by the test before either side sees it)."""
    return make_obs(obs_seed(img, n), n, img).float().double()


def scratch_bytes(img, n):
    return max(stm.scratch_bytes(img, n), dsm.scratch_bytes(img, n))


def dec_keys():
    return ftm.dec_keys(PRESET)


def enc_keys():
    return stm.param_keys(PRESET)


def head_keys():
    return ftm.head_keys(PRESET)


def golden_state_dict():
    """The reference's own separable d = 2 network with its decoder (the fixture segmenter_golden.npz), rounded to f32."""
    return {k: v.float() for k, v in golden_seg_state_dict(np.load(GOLDEN), PRESET).items()}


def seeded_state_dict():
    """sep_encoder_train_model.sep_state_dict plus a seeded decoder and classifier, rounded to f32; used without the
    residual."""
    sd = stm.sep_state_dict(PRESET, SEEDED["seed"], SEEDED["gain"])
    p = SEG_PRESETS[PRESET]
    keys, shapes = [], []
    for j in range(LEVELS):
        cout = dsm.level_channels(j)
        keys += [f"{p['decoder']}{j}.up.{leaf}" for leaf in ftm.LEAVES + stm.STATS]
        shapes += [(2 * cout, cout, 3, 3)] + [(cout,)] * 5
    keys += [p["classifier"] + "weight", p["classifier"] + "bias"]
    shapes += [(1, dsm.CH, 1, 1), (1,)]
    sd.update(make_seg_state_dict(keys, shapes, SEEDED["dec_seed"], SEEDED["dec_gain"], SEEDED["up_gain"], SEEDED["cls_gain"],
                                  SEEDED["cls_bias"]))
    return {k: v.float() for k, v in sd.items()}


def state_dict(weights):
    return golden_state_dict() if weights == "golden" else seeded_state_dict()


def kind(key):
    """The parameter kind a gradient error is reported under."""
    p = SEG_PRESETS[PRESET]
    if key.startswith(p["classifier"]):
        return "classifier " + key.rsplit(".", 1)[-1]
    if key.startswith(p["grad"]):
        return "head " + key.rsplit(".", 1)[-1]
    if key.startswith(p["decoder"]):
        return "decoder " + ".".join(key.rsplit(".", 2)[-2:])
    tail = key[key.index(".conv.") + 1:] if ".conv." in key else key[key.index(".bn.") + 1:]
    return ("down " if ".down." in key else "encoder ") + tail


def forward_gated(sd, obs, dilation, residual, gates=None, us=None):
    """-> (pooled (N,256), logit (N,1,S,S)).  ``gates``: 21 tensors, the 16 encoder layers in packed order then the
    decoder's five levels; ``relu(u)`` is replaced by ``u * gates[i]``.  ``us`` receives every layer's detached u in that
    order.  The encoder is sep_encoder_train_model.encode_gated's, layer by layer, kept here for its level outputs."""
    p = SEG_PRESETS[PRESET]
    i = [0]

    def act(u):
        if us is not None:
            us.append(u.detach())
        r = torch.relu(u) if gates is None else u * gates[i[0]]
        i[0] += 1
        return r

    def layer(x, stem, sep, d, stride):
        st = p["prefix"] + stem
        if sep:
            u = F.conv2d(stm._depthwise_pair(x, sd[st + "conv.0.weight"], sd[st + "conv.1.weight"], d), sd[st + "conv.2.weight"],
                         sd[st + "conv.2.bias"])
        else:
            u = F.conv2d(x, sd[st + "conv.weight"], sd[st + "conv.bias"], stride, 1, 1)
        return ftm._bn(act(u), sd, st)

    x = layer(obs, "initial.", True, 1, 1)
    skips = []
    for lv in range(LEVELS):
        stem = f"features.{lv}."
        y = layer(x, stem + "net.Layer 1.", True, dilation, 1)
        y = layer(y, stem + "net.Layer 2.", True, dilation, 1)
        if residual:
            y = y + x
        skips.append(y)
        x = layer(y, stem + "down.", False, 1, 2)
    pooled = x.mean(dim=(2, 3))
    for j, y in enumerate(skips[::-1]):  # fullnet_train_model.forward_gated's decoder
        st = f"{p['decoder']}{j}.up."
        u = F.conv_transpose2d(x, sd[st + "conv.weight"], sd[st + "conv.bias"], stride=2, padding=1, output_padding=1)
        x = ftm._bn(act(u), sd, st) + y
    return pooled, F.conv2d(x, sd[p["classifier"] + "weight"], sd[p["classifier"] + "bias"])


class HostModel:
    """``forward(gates)`` -> (pooled, prob, grad_pred) with autograd through the 86 + 22 parameters and the head's two."""

    def __init__(self, sd, dilation, residual, obs64):
        self.sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        self.dilation, self.residual, self.obs = int(dilation), bool(residual), obs64
        self.keys = enc_keys() + dec_keys() + head_keys()
        self.params = {k: self.sd[k].clone().requires_grad_() for k in self.keys}
        self.sd.update(self.params)

    def forward(self, gates=None, us=None):
        pooled, logit = forward_gated(self.sd, self.obs, self.dilation, self.residual, gates, us)
        g = SEG_PRESETS[PRESET]["grad"]
        return pooled, torch.sigmoid(logit), F.linear(pooled, self.sd[g + "weight"], self.sd[g + "bias"])

    def grads(self, loss, head=False):
        for v in self.params.values():
            v.grad = None
        loss.backward()
        keys = self.keys if head else enc_keys() + dec_keys()
        return {k: (self.params[k].grad.clone() if self.params[k].grad is not None else torch.zeros_like(self.params[k]))
                for k in keys}


def band_shares(us):
    """Per layer, the share of its pixels whose gate an f32 evaluation may flip: |u| <= 1e-4 max(1, max |u|)."""
    return [float((u.abs() <= TOL * max(1.0, float(u.abs().max()))).double().mean()) for u in us]
