"""Host model of the native separable-encoder backward (csrc/occ_sepenc_bwd.hpp, occlusionenv_amd/septrain.py): the
separable encoder of tests/encoder_model.py restated so that every layer's ReLU can take a given gate (``u * gate`` in place
of ``relu(u)``), with torch autograd over every parameter, in f64 on the CPU (it mirrors encoder_train_model.HostModel); the
decomposition of one separable layer's backward that the kernels implement (dH, the nine correlation sums G and the two
depthwise gradients from them, dX with the flipped dilated stencil, dPW from the rebuilt h) in plain tensor ops; and a
restatement in plain integers of the K split of the pointwise weight gradient and of the scratch size (``sep_dpw_plan`` /
``sep_train_ws_layout``), which the host test holds to the library's workspace query and from which the split case of the GPU
test is chosen.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests import encoder_train_model as etm
from tests.encoder_model import make_state_dict

LEVELS = 5
# name: (key prefix, grad head prefix, tanh on the head, dilation, residual)
PRESETS = {"ppo": ("encoder.", "gradPredictor.", False, 2, True),
           "predictor": ("features.", "output.", True, 1, False)}
SEP_LEAVES = ("conv.0.weight", "conv.1.weight", "conv.2.weight", "conv.2.bias", "bn.weight", "bn.bias")
DENSE_LEAVES = ("conv.weight", "conv.bias", "bn.weight", "bn.bias")
STATS = ("bn.running_mean", "bn.running_var")


def layers():
    """[(stem relative to the prefix, cin, cout, separable, stride)] x 16 in packed order: the downs are dense."""
    return [(stem, cin, cout, stride == 1, stride) for stem, cin, cout, stride in etm.layers()]


def leaf_shapes(cin, cout, sep):
    if sep:
        return [(cin, 1, 3, 1), (cin, 1, 1, 3), (cout, cin, 1, 1)] + [(cout,)] * 5
    return [(cout, cin, 3, 3)] + [(cout,)] * 5


def sep_state_dict(preset, seed, gain=2.0, dtype=torch.float64):
    """A seeded separable checkpoint under the preset's keys (encoder_model.make_state_dict), head included."""
    prefix, head = PRESETS[preset][0], PRESETS[preset][1]
    keys, shapes = [], []
    for stem, cin, cout, sep, _s in layers():
        keys += [prefix + stem + leaf for leaf in (SEP_LEAVES if sep else DENSE_LEAVES) + STATS]
        shapes += leaf_shapes(cin, cout, sep)
    keys += [head + "weight", head + "bias"]
    shapes += [(2, 256), (2,)]
    return make_state_dict(keys, shapes, seed, gain, dtype)


def param_keys(preset, head=False):
    prefix, hd = PRESETS[preset][0], PRESETS[preset][1]
    keys = [prefix + stem + leaf for stem, _ci, _co, sep, _s in layers() for leaf in (SEP_LEAVES if sep else DENSE_LEAVES)]
    return keys + ([hd + "weight", hd + "bias"] if head else [])


def _depthwise_pair(x, wv, wh, d):
    """conv2d(conv2d(x, wv, padding (d,0), dilation (d,1), groups c), wh, padding (0,d), dilation (1,d), groups c) as two
    3-tap sums over slices of the zero-padded input: the same function (held to F.conv2d in the host test), many times faster
    than torch's dilated depthwise f64 convolution on the CPU."""
    H, W = x.shape[2:]
    xp = F.pad(x, (0, 0, d, d))
    v = sum(wv[:, 0, k, 0].view(1, -1, 1, 1) * xp[:, :, k * d:k * d + H, :] for k in range(3))
    vp = F.pad(v, (d, d, 0, 0))
    return sum(wh[:, 0, 0, k].view(1, -1, 1, 1) * vp[:, :, :, k * d:k * d + W] for k in range(3))


def encode_gated(sd, obs, prefix, dilation, residual, gates=None, us=None):
    """encoder_model.encode(separable=True) with ``relu(u)`` replaced by ``u * gates[i]`` when gates are given; ``us``
    receives every layer's detached u in packed order."""
    i = [0]

    def layer(x, stem, sep, d, stride):
        st = prefix + stem
        if sep:
            u = F.conv2d(_depthwise_pair(x, sd[st + "conv.0.weight"], sd[st + "conv.1.weight"], d), sd[st + "conv.2.weight"],
                         sd[st + "conv.2.bias"])
        else:
            u = F.conv2d(x, sd[st + "conv.weight"], sd[st + "conv.bias"], stride, 1, 1)
        if us is not None:
            us.append(u.detach())
        r = torch.relu(u) if gates is None else u * gates[i[0]]
        i[0] += 1
        return F.batch_norm(r, sd[st + "bn.running_mean"], sd[st + "bn.running_var"], sd[st + "bn.weight"], sd[st + "bn.bias"],
                            False, 0.0, 1e-5)

    x = layer(obs, "initial.", True, 1, 1)
    for lv in range(LEVELS):
        stem = f"features.{lv}."
        y = layer(x, stem + "net.Layer 1.", True, dilation, 1)
        y = layer(y, stem + "net.Layer 2.", True, dilation, 1)
        if residual:
            y = y + x
        x = layer(y, stem + "down.", False, 1, 2)
    return x.mean(dim=(2, 3))


class HostModel:
    """``feats(gates)`` / ``predict(gates)`` with autograd through the encoder's parameters and the head's two.  The dilation
    and the residual flag default to the preset's."""

    def __init__(self, sd, preset, obs64, dilation=None, residual=None):
        self.sd, self.preset, self.obs = dict(sd), preset, obs64
        self.dilation = PRESETS[preset][3] if dilation is None else dilation
        self.residual = PRESETS[preset][4] if residual is None else residual
        self.params = {k: sd[k].clone().requires_grad_() for k in param_keys(preset, head=True)}
        self.sd.update(self.params)

    def feats(self, gates=None, us=None):
        return encode_gated(self.sd, self.obs, PRESETS[self.preset][0], self.dilation, self.residual, gates, us)

    def predict(self, gates=None):
        _p, hd, tanh, _d, _r = PRESETS[self.preset]
        g = F.linear(self.feats(gates), self.sd[hd + "weight"], self.sd[hd + "bias"])
        return torch.tanh(g) if tanh else g

    def grads(self, loss, head=False):
        for v in self.params.values():
            v.grad = None
        loss.backward()
        return {k: self.params[k].grad.clone() for k in param_keys(self.preset, head)}


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


# ---- the K split of the pointwise weight gradient and the scratch size, in plain integers ---------------------------------
DPW_BLOCKS = 1024
ACT_CHUNK = 4096
SPLIT_CASE = (33, 115)  # (S, N), chosen from dpw_plans below; what it reaches is asserted in test_sep_encoder_train_host.py


def dpw_plans(img, n):
    """One dict per layer in packed order.  Separable layers: the (ci, co) tile, the pixel tile, tiles per slice, slices and
    partial rows of the pointwise weight gradient; downs: encoder_train_model.dw_plans' entry (the dense kernels run)."""
    hs = etm.sides(img)
    dense = etm.dw_plans(img, n)
    plans = []
    for i, (_stem, cin, cout, sep, _stride) in enumerate(layers()):
        if not sep:
            plans.append(dict(dense[i], sep=False))
            continue
        h = hs[0 if i == 0 else (i - 1) // 3]
        cib, cob = min(cin, 64), min(cout, 32)
        t = 16 if cib <= 8 else 4 if cib == 64 else 8
        q = cib * (cob // 8)
        pb = 256 // max(q, 64)
        grid_y = (cin // cib) * (cout // cob)
        tiles_x = -(-h // t)
        total = n * tiles_x * tiles_x
        want = DPW_BLOCKS // grid_y
        tps = -(-total // want)
        slices = -(-total // tps)
        te = tiles_x * tiles_x
        plans.append(dict(sep=True, cin=cin, cout=cout, ho=h, T=t, cib=cib, cob=cob, pb=pb, grid_y=grid_y, tiles_env=te,
                          total_tiles=total, tps=tps, slices=slices, short_last=total % tps != 0,
                          straddles=any((s * tps) // te != (min(s * tps + tps, total) - 1) // te for s in range(slices)),
                          part_bytes=slices * pb * cin * cout * 4))
    return plans


def scratch_bytes(img, n):
    """max over the layers of (activation partials, weight-gradient partials, a separable layer's G partials: nine f64 sums
    per (input channel, env, chunk)), rounded up to 256.  The G partials are not split further: one block per chunk."""
    need = 0
    for p in dpw_plans(img, n):
        chunks = -(-(p["ho"] * p["ho"]) // ACT_CHUNK)
        need = max(need, p["cout"] * n * chunks * 3 * 8, p["part_bytes"])
        if p["sep"]:
            need = max(need, p["cin"] * n * chunks * 9 * 8)
    return (need + 255) & ~255
