"""Host model of the native joint backward (csrc/occ_fullnet_bwd.hpp, occlusionenv_amd/fullnet.py): the dense encoder of
tests/encoder_train_model.encode_gated composed with the decoder of tests/segmenter_model.decode, restated so that the ReLU
of each of the 21 layers can take a given gate (``u * gate`` in place of ``relu(u)``), with torch autograd over every
parameter, in f64 on the CPU (tests/test_fullnet_train_host.py holds the restatement to those two, bitwise); seeded dense
checkpoints with a decoder; and a restatement in plain integers of the joint workspace and scratch sizes, which the host test
holds to the library's query.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import decoder_split_model as dsm
from tests import encoder_train_model as etm
from tests.segmenter_model import PRESETS as SEG_PRESETS
from tests.segmenter_model import golden_seg_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segmenter_golden.npz")
LEVELS = 5
LEAVES = ("conv.weight", "conv.bias", "bn.weight", "bn.bias")
PRESETS = ("ppo", "segmenter")
# the GPU cases of tests/test_gpu_fullnet_train.py: (preset, residual, S, N)
GRAD_CASES = [(p, r, s, n) for s, n in ((32, 2), (64, 3), (96, 2)) for p in PRESETS for r in (1, 0)]
SPLIT_CASES = [("ppo", 1, 32, 129), ("ppo", 1, 96, 65)]  # the encoder's and the decoder's existing split shapes


def state_dict(preset, seed=31):
    """A dense checkpoint under the preset's keys: the seeded dense encoder (and gradPredictor head for "ppo") of
    encoder_train_model.dense_state_dict, the decoder and classifier of the fixture segmenter_golden.npz.  f64."""
    sd = {k: v for k, v in etm.dense_state_dict("ppo", seed).items() if preset == "ppo" or not k.startswith("gradPredictor.")}
    p = SEG_PRESETS[preset]
    gold = golden_seg_state_dict(np.load(GOLDEN), preset)
    sd.update({k: v.double() for k, v in gold.items() if k.startswith((p["decoder"], p["classifier"]))})
    if preset == "segmenter":  # the fixture's -0.6 suits its own encoder; on this one it leaves the logits below 0
        sd[p["classifier"] + "bias"] = torch.full_like(sd[p["classifier"] + "bias"], 0.1)
    return sd


def enc_keys(preset):
    return [SEG_PRESETS[preset]["prefix"] + stem + leaf for stem, _ci, _co, _s in etm.layers() for leaf in LEAVES]


def dec_keys(preset):
    p = SEG_PRESETS[preset]
    return [f"{p['decoder']}{j}.up.{leaf}" for j in range(LEVELS) for leaf in LEAVES] + [p["classifier"] + "weight", p["classifier"] + "bias"]


def head_keys(preset):
    g = SEG_PRESETS[preset]["grad"]
    return [g + "weight", g + "bias"] if g else []


def kind(preset, key):
    """The parameter kind a gradient error is reported under."""
    p = SEG_PRESETS[preset]
    if key.startswith(p["classifier"]):
        return "classifier " + key.rsplit(".", 1)[-1]
    if p["grad"] and key.startswith(p["grad"]):
        return "head " + key.rsplit(".", 1)[-1]
    return ("decoder " if key.startswith(p["decoder"]) else "encoder ") + ".".join(key.rsplit(".", 2)[-2:])


def _bn(r, sd, st):
    return F.batch_norm(r, sd[st + "bn.running_mean"], sd[st + "bn.running_var"], sd[st + "bn.weight"], sd[st + "bn.bias"], False,
                        0.0, 1e-5)


def forward_gated(sd, obs, preset, residual, gates=None, us=None):
    """-> (pooled (N,256), logit (N,1,S,S)).  ``gates``: 21 tensors, the 16 encoder layers in packed order then the decoder's
    five levels; ``relu(u)`` is replaced by ``u * gates[i]``.  ``us`` receives every layer's detached u in that order."""
    p = SEG_PRESETS[preset]
    i = [0]

    def act(u):
        if us is not None:
            us.append(u.detach())
        r = torch.relu(u) if gates is None else u * gates[i[0]]
        i[0] += 1
        return r

    def layer(x, stem, stride):  # encoder_train_model.encode_gated's layer
        st = p["prefix"] + stem
        return _bn(act(F.conv2d(x, sd[st + "conv.weight"], sd[st + "conv.bias"], stride, 1, 1)), sd, st)

    x = layer(obs, "initial.", 1)
    skips = []
    for lv in range(LEVELS):
        stem = f"features.{lv}."
        y = layer(x, stem + "net.Layer 1.", 1)
        y = layer(y, stem + "net.Layer 2.", 1)
        if residual:
            y = y + x
        skips.append(y)
        x = layer(y, stem + "down.", 2)
    pooled = x.mean(dim=(2, 3))
    for j, y in enumerate(skips[::-1]):  # segmenter_model.decode
        st = f"{p['decoder']}{j}.up."
        u = F.conv_transpose2d(x, sd[st + "conv.weight"], sd[st + "conv.bias"], stride=2, padding=1, output_padding=1)
        x = _bn(act(u), sd, st) + y
    return pooled, F.conv2d(x, sd[p["classifier"] + "weight"], sd[p["classifier"] + "bias"])


class HostModel:
    """``forward(gates)`` -> (pooled, prob, grad_pred or None) with autograd through the 86 parameters and the head's two."""

    def __init__(self, sd, preset, residual, obs64):
        self.sd, self.preset, self.residual, self.obs = dict(sd), preset, bool(residual), obs64
        self.keys = enc_keys(preset) + dec_keys(preset) + head_keys(preset)
        self.params = {k: sd[k].clone().requires_grad_() for k in self.keys}
        self.sd.update(self.params)

    def forward(self, gates=None, us=None):
        pooled, logit = forward_gated(self.sd, self.obs, self.preset, self.residual, gates, us)
        g = SEG_PRESETS[self.preset]["grad"]
        pred = F.linear(pooled, self.sd[g + "weight"], self.sd[g + "bias"]) if g else None
        return pooled, torch.sigmoid(logit), pred

    def grads(self, loss, head=False):
        for v in self.params.values():
            v.grad = None
        loss.backward()
        keys = self.keys if head else enc_keys(self.preset) + dec_keys(self.preset)
        return {k: (self.params[k].grad.clone() if self.params[k].grad is not None else torch.zeros_like(self.params[k]))
                for k in keys}


# ---- the joint workspace and scratch, in plain integers (include/occlusionenv_amd.h) ----------------------------------------
def _tiles(h):
    t = 16 if h >= 16 else 8
    return (-(-h // t)) ** 2


def encoder_ws_bytes(img, n):
    """The workspace of occ_encoder_train_forward: obs | r_init | per level a, r1, b, r2, cc, rd | pool partials | g0..g2."""
    a = dsm.align
    hs = etm.sides(img)
    total = a(4 * n * 4 * img * img) + a(4 * n * 8 * img * img)
    for lv in range(LEVELS):
        c = 8 << lv
        total += 5 * a(4 * n * c * hs[lv] ** 2) + a(4 * n * 2 * c * hs[lv + 1] ** 2)
    return total + a(4 * n * _tiles(hs[LEVELS]) * 256) + 3 * a(4 * n * 8 * img * img)


def ws_bytes(img, n):
    """+ last | y_j, r_j per decoder level | prob | dlast | dskip of levels 1..4 (the sizes of y_3 .. y_0)."""
    a = dsm.align
    lvl = dsm.level_bytes(img, n)
    last = a(4 * n * 256 * (img // 32) ** 2)
    return encoder_ws_bytes(img, n) + last + 2 * sum(lvl) + a(4 * n * img * img) + last + sum(lvl[:4])


def scratch_bytes(img, n):
    return max(etm.scratch_bytes(img, n), dsm.scratch_bytes(img, n))


def relu_views(img, n):
    """[(byte offset, channels, side)] x 21: where the joint workspace keeps r = relu(u) of the 16 encoder layers in packed
    order and of the decoder's five levels (the layout of include/occlusionenv_amd.h)."""
    a = dsm.align
    hs = etm.sides(img)
    off = a(4 * n * 4 * img * img)  # obs
    out = [(off, 8, img)]
    off += a(4 * n * 8 * img * img)
    for lv in range(LEVELS):
        c, act = 8 << lv, a(4 * n * (8 << lv) * hs[lv] ** 2)
        out += [(off + act, c, hs[lv]), (off + 3 * act, c, hs[lv]), (off + 5 * act, 2 * c, hs[lv + 1])]  # a r1 b r2 cc rd
        off += 5 * act + a(4 * n * 2 * c * hs[lv + 1] ** 2)
    off = encoder_ws_bytes(img, n) + a(4 * n * 256 * (img // 32) ** 2)  # past the encoder's part and last
    for j, size in enumerate(dsm.level_bytes(img, n)):
        out.append((off + size, 128 >> j, (img // 16) << j))  # y_j | r_j
        off += 2 * size
    return out


def kept_relu(net, i):
    """The kept r of layer i of the latest forward of a ``TrainableFullNetwork``, a view of its workspace."""
    n, img = net._latest
    ws, _scratch = net._train_buffers(n, img)
    off, c, side = relu_views(img, n)[i]
    return ws[off:off + 4 * n * c * side * side].view(torch.float32).view(n, c, side, side)
