"""The f64 host model of every native training path, once: the encoder backward (csrc/occ_encoder_bwd.hpp,
occlusionenv_amd/enctrain.py), the separable encoder backward (csrc/occ_sepenc_bwd.hpp, septrain.py), the joint step in both
forms (csrc/occ_fullnet_bwd.hpp, fullnet.py, sepfullnet.py), the joint step with batch-statistics BatchNorm
(csrc/occ_bn_train.hpp, ``from_encoder(enc, batch_stats=True)``) and the decoder over the frozen encoder
(csrc/occ_decoder_bwd.hpp, seghead.py).

A ``Net`` says which network is meant.  ``forward_gated`` is the one walk through it: the encoder of tests/encoder_model.py
(dense 3x3 layers, or a depthwise pair plus a pointwise conv with dense downs), then, for a joint net, the decoder of
tests/segmenter_model.decode on the encoder's level outputs and the classifier; the ``test_*_train_host.py`` modules hold it
to those two inference models, which the reference's golden fixtures pin.  ``HostModel`` puts torch autograd over every
parameter, on the CPU, in f64 (the oracle) or in f32 (PyTorch's own single-precision run, which conditions the
batch-statistics cases).  With ``frozen_encoder`` the parameters are the decoder's and the classifier's 22: the encoder runs
once per ``HostModel``, without autograd, and the walk enters the decoder loop with its kept outputs.

What a gate is.  The ReLU of each of the 16 encoder layers and 5 decoder levels can take a given gate: ``u * gate`` in place
of ``relu(u)``, ``u`` being the layer's pre-activation.  With ``gate = (u > 0)`` that is the same function and the same
gradient.  The GPU tests evaluate the oracle with the *device's* gates (``r > 0`` of the relu outputs it kept), so that a
borderline pixel which f32 puts on the other side of zero is judged once, by the gate test (it may differ only inside the
band |u64| <= 1e-4 max(1, max |u64|)), and is not smeared into every weight sum behind it.  ``u * gate`` and not
``relu(u) * gate``: where the device's gate is open and the f64 u slightly negative, the device did pass that value on.

Why the weights are rounded to f32.  A checkpoint on disk holds f32, and so do the device's buffers; the host model uses
exactly those values in f64, so that the comparison is about the arithmetic and not about the inputs.  ``HostModel`` casts
the floating tensors it is given to its dtype, which leaves an f64 state dict as it is.

With ``batch_stats`` every ``F.batch_norm`` runs in training mode (momentum 0.1, eps 1e-5) on ``running``, a moving copy of
the checkpoint's statistics, as ``nn.BatchNorm2d`` does; otherwise on the checkpoint's running statistics.

Also here: the seeded checkpoints of the GPU tests; the decomposition of one separable layer's backward that the kernels
implement (dH, the nine correlation sums G and the two depthwise gradients from them, dX with the flipped dilated stencil,
dPW from the rebuilt h) and the A / B / C form of the BatchNorm backward, in plain tensor ops; the share of a layer's pixels
inside the gate band; and the case tables that a host test and a GPU test share.  The workspace, scratch and K-split
restatements in plain integers are in tests/train_layout.py.
"""
from __future__ import annotations

import functools
import os
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from tests import decoder_split_model as dsm
from tests.encoder_model import PRESETS as ENC_PRESETS
from tests.encoder_model import make_obs, make_state_dict
from tests.segmenter_model import PRESETS as SEG_PRESETS
from tests.segmenter_model import golden_seg_state_dict, make_seg_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segmenter_golden.npz")
LEVELS = 5
EPS = 1e-5
MOMENTUM = 0.1
SEP_LEAVES = ("conv.0.weight", "conv.1.weight", "conv.2.weight", "conv.2.bias", "bn.weight", "bn.bias")
DENSE_LEAVES = ("conv.weight", "conv.bias", "bn.weight", "bn.bias")
STATS = ("bn.running_mean", "bn.running_var")


class Net(NamedTuple):
    preset: str                # "ppo", "predictor" (encoder only) or "segmenter" (joint only)
    separable: bool            # Layer 1 / Layer 2 and the initial layer are separable; the downs are always dense
    dilation: int              # of Layer 1 / Layer 2 (a dense net has 1)
    residual: bool
    joint: bool = False        # the decoder and the classifier run
    batch_stats: bool = False  # BatchNorm in training mode
    frozen_encoder: bool = False  # a joint net whose encoder gets no gradient: the parameters and the gates are the decoder's


def preset_keys(preset):
    """The key prefixes of a preset: segmenter_model's entry (decoder, classifier) over encoder_model's (tanh on the head)."""
    return {"tanh": False, **ENC_PRESETS.get(preset, {}), **SEG_PRESETS.get(preset, {})}


# ---- keys ---------------------------------------------------------------------------------------------------------------------
def layers(separable):
    """[(stem relative to the prefix, cin, cout, separable, stride)] x 16 in packed order: the downs are dense."""
    out = [("initial.", 4, 8, separable, 1)]
    for lv in range(LEVELS):
        c = 8 << lv
        out += [(f"features.{lv}.net.Layer 1.", c, c, separable, 1), (f"features.{lv}.net.Layer 2.", c, c, separable, 1),
                (f"features.{lv}.down.", c, 2 * c, False, 2)]
    return out


def enc_keys(net):
    prefix = preset_keys(net.preset)["prefix"]
    return [prefix + stem + leaf for stem, _ci, _co, sep, _s in layers(net.separable) for leaf in (SEP_LEAVES if sep else DENSE_LEAVES)]


def dec_keys(net):
    """The decoder's and the classifier's keys of a joint net."""
    p = preset_keys(net.preset)
    return [f"{p['decoder']}{j}.up.{leaf}" for j in range(LEVELS) for leaf in DENSE_LEAVES] + [p["classifier"] + "weight", p["classifier"] + "bias"]


def head_keys(net):
    g = preset_keys(net.preset)["grad"]
    return [g + "weight", g + "bias"] if g else []


def param_keys(net, head=False):
    """Every tensor that receives a gradient, in packed order; ``head``: and the grad head's two (which sit on the pooled
    feature: a frozen encoder leaves them none)."""
    if net.frozen_encoder:
        return dec_keys(net)
    return enc_keys(net) + (dec_keys(net) if net.joint else []) + (head_keys(net) if head else [])


def bn_stems(net):
    """The BatchNorm layers' state-dict stems in packed order: 16, and the decoder's 5 for a joint net."""
    p = preset_keys(net.preset)
    stems = [p["prefix"] + stem for stem, *_ in layers(net.separable)]
    return stems + ([f"{p['decoder']}{j}.up." for j in range(LEVELS)] if net.joint else [])


def frozen_net(preset):
    """The decoder over the frozen encoder of a segmenter_model preset ("ppo": separable, d = 2; "segmenter": dense)."""
    p = SEG_PRESETS[preset]
    return Net(preset, preset == "ppo", p["dilation"], p["residual"], True, frozen_encoder=True)


def kind(net, key):
    """The parameter kind a gradient error is reported under (the ``WORST`` dictionaries and the printed lines of the GPU
    tests are keyed by it, so each path keeps the names it has always printed)."""
    if net.frozen_encoder:  # the key's last two parts: "conv.weight", "bn.bias", and "1.weight" / "classifier.weight"
        return ".".join(key.rsplit(".", 2)[-2:])
    p = preset_keys(net.preset)
    leaf = key.rsplit(".", 1)[-1]
    if net.joint and key.startswith(p["classifier"]):
        return "classifier " + leaf
    if p["grad"] and key.startswith(p["grad"]):
        return "head " + leaf if net.joint else "head." + leaf if net.separable else key
    tail = key[key.index(".conv." if ".conv." in key else ".bn.") + 1:]
    if not net.joint:
        return tail
    if key.startswith(p["decoder"]):
        return "decoder " + tail
    return ("down " if ".down." in key and (net.separable or net.batch_stats) else "encoder ") + tail


# ---- the forward ----------------------------------------------------------------------------------------------------------------
def _depthwise_pair(x, wv, wh, d):
    """conv2d(conv2d(x, wv, padding (d,0), dilation (d,1), groups c), wh, padding (0,d), dilation (1,d), groups c) as two
    3-tap sums over slices of the zero-padded input: the same function (held to F.conv2d in the host test), many times faster
    than torch's dilated depthwise f64 convolution on the CPU."""
    H, W = x.shape[2:]
    xp = F.pad(x, (0, 0, d, d))
    v = sum(wv[:, 0, k, 0].view(1, -1, 1, 1) * xp[:, :, k * d:k * d + H, :] for k in range(3))
    vp = F.pad(v, (d, d, 0, 0))
    return sum(wh[:, 0, 0, k].view(1, -1, 1, 1) * vp[:, :, :, k * d:k * d + W] for k in range(3))


def _layer_ops(sd, net, gates=None, us=None, running=None, stats=None):
    """-> (layer, act_bn) of one walk: ``layer(x, stem, separable, dilation, stride)`` is an encoder layer, ``act_bn(u, stem)``
    the gated ReLU and the BatchNorm behind any layer's pre-activation u.  Both count the layers they have seen, which is how
    ``gates`` is indexed; the other arguments are ``forward_gated``'s."""
    assert net.separable or net.dilation == 1
    p = preset_keys(net.preset)
    train, mv = running is not None, sd if running is None else running
    i = [0]

    def act_bn(u, st):
        if us is not None:
            us.append(u.detach())
        r = torch.relu(u) if gates is None else u * gates[i[0]]
        i[0] += 1
        if stats is not None:
            rd = r.detach()
            stats.append((rd.mean(dim=(0, 2, 3)), rd.var(dim=(0, 2, 3), unbiased=False)))
        return F.batch_norm(r, mv[st + "bn.running_mean"], mv[st + "bn.running_var"], sd[st + "bn.weight"], sd[st + "bn.bias"],
                            train, MOMENTUM if train else 0.0, EPS)

    def layer(x, stem, sep, d, stride):
        st = p["prefix"] + stem
        if sep:
            u = F.conv2d(_depthwise_pair(x, sd[st + "conv.0.weight"], sd[st + "conv.1.weight"], d), sd[st + "conv.2.weight"],
                         sd[st + "conv.2.bias"])
        else:
            u = F.conv2d(x, sd[st + "conv.weight"], sd[st + "conv.bias"], stride, 1, 1)
        return act_bn(u, st)

    return layer, act_bn


def encode(sd, obs, net, layer=None):
    """-> (the last down output (N,256,S/32,S/32), [the five level features]): the encoder, through ``layer`` of a walk that
    is under way, or with plain ReLUs on the state dict's running statistics."""
    layer = layer or _layer_ops(sd, net)[0]
    x = layer(obs, "initial.", net.separable, 1, 1)
    skips = []
    for lv in range(LEVELS):
        stem = f"features.{lv}."
        y = layer(x, stem + "net.Layer 1.", net.separable, net.dilation, 1)
        y = layer(y, stem + "net.Layer 2.", net.separable, net.dilation, 1)
        if net.residual:
            y = y + x
        skips.append(y)
        x = layer(y, stem + "down.", False, 1, 2)
    return x, skips


def forward_gated(sd, obs, net, gates=None, us=None, running=None, stats=None, encoded=None):
    """-> (pooled (N,256), logit (N,1,S,S) or None when the net is no joint one).  ``gates``: one tensor per layer, the 16
    encoder layers in packed order then the decoder's five levels; ``relu(u)`` is replaced by ``u * gates[i]``.  ``us``
    receives every layer's detached u in that order, ``stats`` every layer's detached (mean, biased variance) of r.
    ``running`` ({stem + "bn.running_mean" / "bn.running_var"}) given: BatchNorm in training mode on it, updated in place as
    nn.BatchNorm2d does; otherwise on the state dict's running statistics.  ``encoded``: what ``encode`` returned; given, the
    encoder does not run (``obs`` is not read), and the layers that ``gates``, ``us`` and ``stats`` count are the decoder's
    five."""
    p = preset_keys(net.preset)
    layer, act_bn = _layer_ops(sd, net, gates, us, running, stats)
    x, skips = encode(sd, obs, net, layer) if encoded is None else encoded
    pooled = x.mean(dim=(2, 3))
    if not net.joint:
        return pooled, None
    for j, y in enumerate(skips[::-1]):  # segmenter_model.decode
        st = f"{p['decoder']}{j}.up."
        u = F.conv_transpose2d(x, sd[st + "conv.weight"], sd[st + "conv.bias"], stride=2, padding=1, output_padding=1)
        x = act_bn(u, st) + y
    return pooled, F.conv2d(x, sd[p["classifier"] + "weight"], sd[p["classifier"] + "bias"])


class HostModel:
    """The network ``net`` on the weights ``sd`` (cast to ``dtype``) with autograd through every parameter and the head's
    two.  With ``net.batch_stats`` every forward moves ``running`` (a copy of the checkpoint's statistics) and records
    ``stats``.  With ``net.frozen_encoder`` the encoder runs here, once and without autograd, and every forward is the
    decoder on its outputs ``encoded``."""

    def __init__(self, sd, net, obs, dtype=torch.float64):
        self.sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        self.net, self.obs = net, obs.to(dtype)
        self.keys = param_keys(net, head=True)
        self.params = {k: self.sd[k].clone().requires_grad_() for k in self.keys}
        self.sd.update(self.params)
        self.running = {st + leaf: self.sd[st + leaf].clone() for st in bn_stems(net) for leaf in STATS} if net.batch_stats else None
        self.stats = None
        self.encoded = None
        if net.frozen_encoder:
            with torch.no_grad():
                self.encoded = encode(self.sd, self.obs, net)

    def logit(self, gates=None, us=None, obs=None):
        """-> (pooled, logit or None): ``forward`` before the sigmoid and the head."""
        assert obs is None or self.encoded is None
        self.stats = [] if self.net.batch_stats else None
        return forward_gated(self.sd, self.obs if obs is None else obs, self.net, gates, us, self.running, self.stats, self.encoded)

    def forward(self, gates=None, us=None, obs=None):
        """-> (pooled, prob or None, the head's prediction or None)."""
        pooled, logit = self.logit(gates, us, obs)
        p = preset_keys(self.net.preset)
        pred = None
        if p["grad"]:
            pred = F.linear(pooled, self.sd[p["grad"] + "weight"], self.sd[p["grad"] + "bias"])
            pred = torch.tanh(pred) if p["tanh"] else pred
        return pooled, None if logit is None else torch.sigmoid(logit), pred

    def feats(self, gates=None, us=None):
        return self.forward(gates, us)[0]

    def predict(self, gates=None):
        return self.forward(gates)[2]

    def grads(self, loss, head=False):
        """{key: gradient}; a parameter of a joint net that the loss does not reach gives zeros."""
        for v in self.params.values():
            v.grad = None
        loss.backward()
        out = {}
        for k in param_keys(self.net, head):
            g = self.params[k].grad
            assert g is not None or self.net.joint, k
            out[k] = torch.zeros_like(self.params[k]) if g is None else g.clone()
        return out

    def packed_stats(self):
        """``bn_stats`` of the latest forward: mean[c] | var_biased[c] per layer, packed order."""
        return torch.cat([t for mean, var in self.stats for t in (mean, var)])


# ---- the checkpoints of the GPU tests --------------------------------------------------------------------------------------------
def _encoder_state_dict(preset, separable, seed, gain, dtype):
    p = ENC_PRESETS[preset]
    keys, shapes = [], []
    for stem, cin, cout, sep, _s in layers(separable):
        keys += [p["prefix"] + stem + leaf for leaf in (SEP_LEAVES if sep else DENSE_LEAVES) + STATS]
        shapes += ([(cin, 1, 3, 1), (cin, 1, 1, 3), (cout, cin, 1, 1)] if sep else [(cout, cin, 3, 3)]) + [(cout,)] * 5
    keys += [p["grad"] + "weight", p["grad"] + "bias"]
    shapes += [(2, 256), (2,)]
    return make_state_dict(keys, shapes, seed, gain, dtype)


DENSE_GAIN = {"predictor": 2.0, "ppo": 1.0}  # make_state_dict's gain of the dense checkpoints: less where the residual adds


def dense_state_dict(preset, seed, gain=None, dtype=torch.float64):
    """A seeded dense checkpoint under the preset's keys (encoder_model.make_state_dict), head included; ``gain``:
    DENSE_GAIN's unless given."""
    return _encoder_state_dict(preset, False, seed, DENSE_GAIN[preset] if gain is None else gain, dtype)


def sep_state_dict(preset, seed, gain=2.0, dtype=torch.float64):
    """A seeded separable checkpoint under the preset's keys (encoder_model.make_state_dict), head included."""
    return _encoder_state_dict(preset, True, seed, gain, dtype)


def state_dict(preset, seed=31):
    """A dense checkpoint with a decoder under the preset's keys ("ppo" or "segmenter"): the seeded dense encoder (and
    gradPredictor head for "ppo") of dense_state_dict, the decoder and classifier of the fixture segmenter_golden.npz.  f64."""
    sd = {k: v for k, v in dense_state_dict("ppo", seed).items() if preset == "ppo" or not k.startswith("gradPredictor.")}
    p = SEG_PRESETS[preset]
    gold = golden_seg_state_dict(np.load(GOLDEN), preset)
    sd.update({k: v.double() for k, v in gold.items() if k.startswith((p["decoder"], p["classifier"]))})
    if preset == "segmenter":  # the fixture's -0.6 suits its own encoder; on this one it leaves the logits below 0
        sd[p["classifier"] + "bias"] = torch.full_like(sd[p["classifier"] + "bias"], 0.1)
    return sd


SEEDED = dict(seed=57, gain=2.0, dec_seed=58, dec_gain=2.0, up_gain=1.4, cls_gain=1.0, cls_bias=-0.3)


def golden_state_dict():
    """The reference's own separable d = 2 network with its decoder (the fixture segmenter_golden.npz), rounded to f32."""
    return {k: v.float() for k, v in golden_seg_state_dict(np.load(GOLDEN), "ppo").items()}


def seeded_state_dict():
    """sep_state_dict plus a seeded decoder and classifier, rounded to f32; used without the residual."""
    sd = sep_state_dict("ppo", SEEDED["seed"], SEEDED["gain"])
    p = SEG_PRESETS["ppo"]
    keys, shapes = [], []
    for j in range(LEVELS):
        cout = dsm.level_channels(j)
        keys += [f"{p['decoder']}{j}.up.{leaf}" for leaf in DENSE_LEAVES + STATS]
        shapes += [(2 * cout, cout, 3, 3)] + [(cout,)] * 5
    keys += [p["classifier"] + "weight", p["classifier"] + "bias"]
    shapes += [(1, dsm.CH, 1, 1), (1,)]
    sd.update(make_seg_state_dict(keys, shapes, SEEDED["dec_seed"], SEEDED["dec_gain"], SEEDED["up_gain"], SEEDED["cls_gain"],
                                  SEEDED["cls_bias"]))
    return {k: v.float() for k, v in sd.items()}


def joint_state_dict(weights, separable=True):
    """The f32 "ppo" checkpoints of the joint tests.  Separable: "golden" = the fixture's own FullNetwork(8, dilation=2,
    separable=True), "seeded" = seeded_state_dict.  Dense "golden" = the seeded dense encoder with the fixture's decoder
    (``state_dict``)."""
    if not separable:
        assert weights == "golden"
        return {k: v.float() for k, v in state_dict("ppo").items()}
    return golden_state_dict() if weights == "golden" else seeded_state_dict()


# ---- one separable layer's backward as the kernels decompose it -------------------------------------------------------------
def _shift(t, dy, dx):
    """s[.., y, x] = t[.., y + dy, x + dx], zero outside."""
    H, W = t.shape[-2:]
    out = torch.zeros_like(t)
    ys, ye = max(0, -dy), min(H, H - dy)
    xs, xe = max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        out[..., ys:ye, xs:xe] = t[..., ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def sep_layer_backward(x, wv, wh, pw, du, d):
    """x (n,cin,H,W); wv (cin,3), wh (cin,3), pw (cout,cin); du = d loss / d u (n,cout,H,W) with u = pw h + bias ->
    (dwv (cin,3), dwh (cin,3), dpw (cout,cin), dx), formed as csrc/occ_sepenc_bwd.hpp forms them."""
    cin = x.shape[1]
    h = torch.zeros_like(x)  # the 9-tap stencil on zero-padded x
    for kv in range(3):
        for kh in range(3):
            h = h + (wv[:, kv] * wh[:, kh]).view(1, cin, 1, 1) * _shift(x, (kv - 1) * d, (kh - 1) * d)
    dpw = torch.einsum("nihw,nohw->oi", h, du)
    dh = torch.einsum("oi,nohw->nihw", pw, du)
    G = torch.stack([torch.stack([(dh * _shift(x, (kv - 1) * d, (kh - 1) * d)).sum(dim=(0, 2, 3)) for kh in range(3)], dim=1)
                     for kv in range(3)], dim=1)  # (cin, kv, kh)
    dwv = torch.einsum("ih,ivh->iv", wh, G)
    dwh = torch.einsum("iv,ivh->ih", wv, G)
    dx = torch.zeros_like(x)
    for kv in range(3):
        for kh in range(3):
            dx = dx + (wv[:, kv] * wh[:, kh]).view(1, cin, 1, 1) * _shift(dh, -(kv - 1) * d, -(kh - 1) * d)
    return dwv, dwh, dpw, dx


# ---- the A / B / C form of the BatchNorm backward (csrc/occ_bn_train.hpp) ---------------------------------------------------
def bn_backward_abc(r, dy, gamma):
    """(dR, dgamma, dbeta) of y = gamma (r - mu) rstd + beta over (N, C, H, W) from the per-channel sums, as the kernels
    form them: dR = A dY + C r + B."""
    m = r.numel() // r.shape[1]
    mu = r.mean(dim=(0, 2, 3))
    v = (r * r).mean(dim=(0, 2, 3)) - mu * mu
    rstd = 1.0 / torch.sqrt(v + EPS)
    dbeta = dy.sum(dim=(0, 2, 3))
    dgamma = rstd * ((dy * r).sum(dim=(0, 2, 3)) - mu * dbeta)
    s = gamma * rstd
    a, c = s, -s * rstd * dgamma / m
    b = -s * dbeta / m - c * mu
    shape = (1, -1, 1, 1)
    return a.view(shape) * dy + c.view(shape) * r + b.view(shape), dgamma, dbeta


# ---- the cases that a host test and a GPU test share ---------------------------------------------------------------------------
TOL = 1e-4
ENCODER_SPLIT_CASE = ("ppo", 32, 129)  # chosen from train_layout.dw_plans; what it reaches is asserted in test_encoder_train_host.py
SEP_ENCODER_SPLIT_CASE = (33, 115)  # (S, N), from train_layout.dpw_plans; what it reaches: test_sep_encoder_train_host.py

# tests/test_gpu_fullnet_train.py: (preset, residual, S, N)
JOINT_PRESETS = ("ppo", "segmenter")
JOINT_GRAD_CASES = [(p, r, s, n) for s, n in ((32, 2), (64, 3), (96, 2)) for p in JOINT_PRESETS for r in (1, 0)]
JOINT_SPLIT_CASES = [("ppo", 1, 32, 129), ("ppo", 1, 96, 65)]  # the encoder's and the decoder's existing split shapes

# tests/test_gpu_sep_fullnet_train.py: (weights, dilation, residual, S, N)
SEP_JOINT_GRAD_CASES = [("golden", 2, 1, 32, 2), ("golden", 2, 1, 64, 3), ("golden", 2, 1, 96, 2), ("golden", 1, 1, 64, 3),
                        ("seeded", 2, 0, 32, 2), ("seeded", 2, 0, 64, 3)]
SEP_JOINT_SPLIT_CASES = [("golden", 2, 1, 64, 130), ("golden", 2, 1, 96, 65)]
SEP_JOINT_CASES = SEP_JOINT_GRAD_CASES + SEP_JOINT_SPLIT_CASES

# tests/test_gpu_bn_train.py: (weights, form, dilation, residual, S, N): the cases whose gradients are judged, and the one
# that is not (M = 2 at the deepest layer: PyTorch's f32 run itself misses the f64 model by 3e-3 to 4e-3 there)
E32_CAP = 1e-4   # a judged case: PyTorch's f32 run is within this of the f64 model, for every tensor
MARGIN = 4.0     # two independent f32 evaluations; the gates are forced on the native side only
BN_GRAD_CASES = [("golden", "separable", 2, 1, 64, 3), ("golden", "dense", 1, 1, 64, 4), ("seeded", "separable", 2, 0, 96, 2)]
BN_FORWARD_ONLY = ("golden", "separable", 2, 1, 32, 2)
BN_CASES = BN_GRAD_CASES + [BN_FORWARD_ONLY]
BN_IDS = [f"{w}-{f}-d{d}-res{r}-S{s}-N{n}" for w, f, d, r, s, n in BN_CASES]
# The observation seed of a case where it is not obs_seed's: a batch-statistics case must be well conditioned (e32 <= 1e-4
# for every tensor, below) and keep the gate band of every layer at or below 1 % of its pixels, both properties of the host
# model alone, settled before any GPU run.  The shapes and the weights stay.
#   golden separable S=64 N=3: seed 9067 gives e32 = 2.5e-4 on the initial layer's pointwise bias (8 elements; a gate that
#     the f32 run flips at a 2 x 2 plane moves statistics of M = 12 values).  Of 20001..20006, tried in order, 20004 (4.3e-5)
#     and 20006 (1.6e-5) meet the condition; 20006 is used.
#   seeded separable S=96 N=2: seed 9098 is well conditioned (4.7e-5) but 6.7 % of Layer 2 of level 0 lies in the band.  Of
#     20001..20004, 20003 meets both (e32 1.7e-5, band 0.34 %); 20001 has e32 1.9e-2, 20002 and 20004 a band of 2 % and 6.9 %.
OBS_SEEDS = {("golden", "separable", 2, 1, 64, 3): 20006, ("seeded", "separable", 2, 0, 96, 2): 20003}
BAND_CAP = 0.01


def obs_seed(img, n):
    return 9000 + img + n


def case_obs(case):
    """The f64 observation of a joint case, a tuple that ends in (S, N) (rounded to f32 before either side sees it)."""
    img, n = case[-2:]
    return make_obs(OBS_SEEDS.get(tuple(case), obs_seed(img, n)), n, img).float().double()


def upstream(img, n):
    """The randn (grad_feats, grad_prob) of a batch-statistics case, f32."""
    gen = torch.Generator().manual_seed(obs_seed(img, n) + 1)
    return torch.randn(n, 256, generator=gen), torch.randn(n, 1, img, img, generator=gen)


def bn_net(case):
    _weights, form, d, res, _img, _n = case
    return Net("ppo", form == "separable", int(d), bool(res), True, True)


def bn_state_dict(case):
    return joint_state_dict(case[0], case[1] == "separable")


@functools.lru_cache(maxsize=None)
def plain_f64(case):
    """(HostModel after one forward, its gradients for the case's randn upstream, its 21 u's) with its own relu gates;
    ``host.first`` = that forward's detached (pooled, prob).  Shared between tests: left as it is."""
    host = HostModel(bn_state_dict(case), bn_net(case), case_obs(case).float())
    us = []
    pooled, prob, _pred = host.forward(None, us)
    host.first = (pooled.detach(), prob.detach())
    gf, gp = upstream(*case[-2:])
    return host, host.grads((pooled * gf.double()).sum() + (prob * gp.double()).sum()), us


@functools.lru_cache(maxsize=None)
def e32(case):
    """{key: max |g32 - g64| / max |g64|}: PyTorch's f32 CPU autograd run of the case against the plain f64 model."""
    _host, want, _us = plain_f64(case)
    h32 = HostModel(bn_state_dict(case), bn_net(case), case_obs(case).float(), torch.float32)
    pooled, prob, _pred = h32.forward()
    gf, gp = upstream(*case[-2:])
    got = h32.grads((pooled * gf).sum() + (prob * gp).sum())
    return {k: float((got[k].double() - w).abs().max()) / float(w.abs().max()) for k, w in want.items()}


def bar(case, key):
    """The relative bar of one gradient tensor of a batch-statistics case: max(1e-4, 4 e32)."""
    return max(TOL, MARGIN * e32(case)[key])


def band_shares(us):
    """Per layer, the share of its pixels whose gate an f32 evaluation may flip: |u| <= 1e-4 max(1, max |u|)."""
    return [float((u.abs() <= TOL * max(1.0, float(u.abs().max()))).double().mean()) for u in us]
