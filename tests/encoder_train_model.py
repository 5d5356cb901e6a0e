"""Host model of the native encoder backward (csrc/occ_encoder_bwd.hpp, occlusionenv_amd/enctrain.py): the dense encoder of
tests/encoder_model.py restated so that every layer's ReLU can take a given gate (``u * gate`` in place of ``relu(u)``), with
torch autograd over every parameter, in f64 on the CPU; and a restatement in plain integers of the K split of the weight
gradient and of the scratch size (``enc_dw_plan`` / ``enc_train_ws_layout``), which the host test holds to the library's
workspace query and from which the split case of the GPU test is chosen.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests.encoder_model import make_state_dict

LEVELS = 5
# name: (key prefix, grad head prefix, tanh on the head, residual, gain of make_state_dict); both dense at dilation 1
PRESETS = {"predictor": ("features.", "output.", True, False, 2.0),
           "ppo": ("encoder.", "gradPredictor.", False, True, 1.0)}
LEAVES = ("conv.weight", "conv.bias", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var")


def layers():
    """[(stem relative to the prefix, cin, cout, stride)] x 16 in packed order."""
    out = [("initial.", 4, 8, 1)]
    for lv in range(LEVELS):
        c = 8 << lv
        out += [(f"features.{lv}.net.Layer 1.", c, c, 1), (f"features.{lv}.net.Layer 2.", c, c, 1), (f"features.{lv}.down.", c, 2 * c, 2)]
    return out


def dense_state_dict(preset, seed, dtype=torch.float64):
    """A seeded dense checkpoint under the preset's keys (encoder_model.make_state_dict), head included."""
    prefix, head, _tanh, _res, gain = PRESETS[preset]
    keys, shapes = [], []
    for stem, cin, cout, _s in layers():
        for leaf in LEAVES:
            keys.append(prefix + stem + leaf)
            shapes.append((cout, cin, 3, 3) if leaf == "conv.weight" else (cout,))
    keys += [head + "weight", head + "bias"]
    shapes += [(2, 256), (2,)]
    return make_state_dict(keys, shapes, seed, gain, dtype)


def param_keys(preset, head=False):
    prefix, hd = PRESETS[preset][0], PRESETS[preset][1]
    keys = [prefix + stem + leaf for stem, _ci, _co, _s in layers() for leaf in LEAVES[:4]]
    return keys + ([hd + "weight", hd + "bias"] if head else [])


def encode_gated(sd, obs, preset, gates=None, us=None):
    """encoder_model.encode for a dense preset with ``relu(u)`` replaced by ``u * gates[i]`` when gates are given;
    ``us`` receives every layer's detached u in packed order."""
    prefix, residual = PRESETS[preset][0], PRESETS[preset][3]
    i = [0]

    def layer(x, stem, stride):
        st = prefix + stem
        u = F.conv2d(x, sd[st + "conv.weight"], sd[st + "conv.bias"], stride, 1, 1)
        if us is not None:
            us.append(u.detach())
        r = torch.relu(u) if gates is None else u * gates[i[0]]
        i[0] += 1
        return F.batch_norm(r, sd[st + "bn.running_mean"], sd[st + "bn.running_var"], sd[st + "bn.weight"], sd[st + "bn.bias"],
                            False, 0.0, 1e-5)

    x = layer(obs, "initial.", 1)
    for lv in range(LEVELS):
        stem = f"features.{lv}."
        y = layer(x, stem + "net.Layer 1.", 1)
        y = layer(y, stem + "net.Layer 2.", 1)
        if residual:
            y = y + x
        x = layer(y, stem + "down.", 2)
    return x.mean(dim=(2, 3))


class HostModel:
    """``feats(gates)`` / ``predict(gates)`` with autograd through the 64 encoder parameters and the head's two."""

    def __init__(self, sd, preset, obs64):
        self.sd, self.preset, self.obs = dict(sd), preset, obs64
        self.params = {k: sd[k].clone().requires_grad_() for k in param_keys(preset, head=True)}
        self.sd.update(self.params)

    def feats(self, gates=None, us=None):
        return encode_gated(self.sd, self.obs, self.preset, gates, us)

    def predict(self, gates=None):
        _p, hd, tanh, _r, _g = PRESETS[self.preset]
        g = F.linear(self.feats(gates), self.sd[hd + "weight"], self.sd[hd + "bias"])
        return torch.tanh(g) if tanh else g

    def grads(self, loss, head=False):
        for v in self.params.values():
            v.grad = None
        loss.backward()
        return {k: self.params[k].grad.clone() for k in param_keys(self.preset, head)}


# ---- the K split of the weight gradient and the scratch size, in plain integers -------------------------------------------
DW_BLOCKS = 512
ACT_CHUNK = 4096
SPLIT_CASE = ("ppo", 32, 129)  # chosen from dw_plans below; what it reaches is asserted in test_encoder_train_host.py


def sides(img):
    """[H_0 .. H_5]: the sides halve with ceiling."""
    out = [img]
    for _ in range(LEVELS):
        out.append((out[-1] + 1) // 2)
    return out


def dw_plans(img, n):
    """One dict per layer in packed order: the (ci, co) tile, the pixel tile, tiles per slice, slices, partial rows."""
    hs = sides(img)
    plans = []
    for i, (_stem, cin, cout, stride) in enumerate(layers()):
        lv = 0 if i == 0 else (i - 1) // 3
        ho = hs[lv + 1] if stride == 2 else hs[lv]
        cib, cob = min(cin, 64), min(cout, 32)
        t = 4 if cib == 64 else 8
        q = cib * (cob // 8)
        pb = 256 // max(q, 64)
        grid_y = (cin // cib) * (cout // cob)
        tiles_x = -(-ho // t)
        total = n * tiles_x * tiles_x
        want = DW_BLOCKS // grid_y
        tps = -(-total // want)
        slices = -(-total // tps)
        te = tiles_x * tiles_x
        plans.append(dict(cin=cin, cout=cout, stride=stride, ho=ho, T=t, cib=cib, cob=cob, pb=pb, grid_y=grid_y, tiles_env=te,
                          total_tiles=total, tps=tps, slices=slices, short_last=total % tps != 0,
                          straddles=any((s * tps) // te != (min(s * tps + tps, total) - 1) // te for s in range(slices)),
                          part_bytes=slices * pb * cin * 9 * cout * 4))
    return plans


def scratch_bytes(img, n):
    """max over the layers of (activation partials, weight-gradient partials), rounded up to 256."""
    need = 0
    for p in dw_plans(img, n):
        chunks = -(-(p["ho"] * p["ho"]) // ACT_CHUNK)
        need = max(need, p["cout"] * n * chunks * 3 * 8, p["part_bytes"])
    return (need + 255) & ~255


def kept_bytes(img, n):
    """obs, every layer's input and every layer's r, as f32 (a lower bound of the workspace: no alignment, no gradients)."""
    hs = sides(img)
    floats = n * 4 * img * img + n * 8 * img * img  # obs, r_init
    for lv in range(LEVELS):
        c, h, ho = 8 << lv, hs[lv], hs[lv + 1]
        floats += 5 * n * c * h * h + n * 2 * c * ho * ho  # a, r1, b, r2, cc; rd
    return 4 * floats
