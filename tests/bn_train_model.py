"""Host model of the native joint training step with batch-statistics BatchNorm (csrc/occ_bn_train.hpp,
``from_encoder(enc, batch_stats=True)``): the joint network of tests/fullnet_train_model.py (dense encoder) and
tests/sep_fullnet_train_model.py (separable encoder) with every ``F.batch_norm`` in training mode (momentum 0.1, eps 1e-5),
torch autograd over every parameter, on the CPU, in f64 (the oracle) or in f32 (PyTorch's own single-precision run, which
conditions the cases).  The ReLU of each of the 21 layers can take a given gate (``u * gate`` in place of ``relu(u)``).  Also:
the A / B / C form of the BatchNorm backward the kernels use, the layout of ``bn_stats``, and the workspace of
``occ_fullnet_bn_train_workspace_query`` in plain integers.
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

from tests import decoder_split_model as dsm
from tests import fullnet_train_model as ftm
from tests import sep_encoder_train_model as stm
from tests import sep_fullnet_train_model as sfm
from tests.encoder_model import make_obs
from tests.segmenter_model import PRESETS as SEG_PRESETS

PRESET = "ppo"
LEVELS = 5
TOL = 1e-4
EPS = 1e-5
MOMENTUM = 0.1
E32_CAP = 1e-4   # a judged case: PyTorch's f32 run is within this of the f64 model, for every tensor
MARGIN = 4.0     # two independent f32 evaluations; the gates are forced on the native side only
# (weights, form, dilation, residual, S, N): the cases whose gradients are judged, and the one that is not (M = 2 at the
# deepest layer: PyTorch's f32 run itself misses the f64 model by 3e-3 to 4e-3 there)
GRAD_CASES = [("golden", "separable", 2, 1, 64, 3), ("golden", "dense", 1, 1, 64, 4), ("seeded", "separable", 2, 0, 96, 2)]
FORWARD_ONLY = ("golden", "separable", 2, 1, 32, 2)
CASES = GRAD_CASES + [FORWARD_ONLY]
IDS = [f"{w}-{f}-d{d}-res{r}-S{s}-N{n}" for w, f, d, r, s, n in CASES]

obs_seed = sfm.obs_seed
# The observation seed of a case where it is not sep_fullnet_train_model's: a case must be well conditioned (e32 <= 1e-4
# for every tensor, below) and keep the gate band of every layer at or below 1 % of its pixels, both properties of the host
# models alone, settled before any GPU run.  The shapes and the weights stay.
#   golden separable S=64 N=3: seed 9067 gives e32 = 2.5e-4 on the initial layer's pointwise bias (8 elements; a gate that
#     the f32 run flips at a 2 x 2 plane moves statistics of M = 12 values).  Of 20001..20006, tried in order, 20004 (4.3e-5)
#     and 20006 (1.6e-5) meet the condition; 20006 is used.
#   seeded separable S=96 N=2: seed 9098 is well conditioned (4.7e-5) but 6.7 % of Layer 2 of level 0 lies in the band.  Of
#     20001..20004, 20003 meets both (e32 1.7e-5, band 0.34 %); 20001 has e32 1.9e-2, 20002 and 20004 a band of 2 % and 6.9 %.
OBS_SEEDS = {("golden", "separable", 2, 1, 64, 3): 20006, ("seeded", "separable", 2, 0, 96, 2): 20003}
BAND_CAP = 0.01


def case_obs(case):
    """The f64 observation of a case (rounded to f32 before either side sees it)."""
    _w, _f, _d, _r, img, n = case
    return make_obs(OBS_SEEDS.get(tuple(case), obs_seed(img, n)), n, img).float().double()


relu_views = ftm.relu_views  # the joint workspace is a prefix of the batch-statistics one


def state_dict(weights, form):
    """f32: "golden" separable = the fixture's own FullNetwork(8, dilation=2, separable=True); "golden" dense = the seeded
    dense encoder with the fixture's decoder (fullnet_train_model.state_dict); "seeded" separable = sep_fullnet_train_model's."""
    if form == "dense":
        assert weights == "golden"
        return {k: v.float() for k, v in ftm.state_dict(PRESET).items()}
    return sfm.state_dict(weights)


def enc_keys(form):
    return ftm.enc_keys(PRESET) if form == "dense" else stm.param_keys(PRESET)


def dec_keys():
    return ftm.dec_keys(PRESET)


def head_keys():
    return ftm.head_keys(PRESET)


def bn_stems(form):
    """The 21 BatchNorm layers' state-dict stems in packed order."""
    p = SEG_PRESETS[PRESET]
    stems = [p["prefix"] + "initial."]
    for lv in range(LEVELS):
        stems += [p["prefix"] + f"features.{lv}.net.Layer 1.", p["prefix"] + f"features.{lv}.net.Layer 2.",
                  p["prefix"] + f"features.{lv}.down."]
    return stems + [f"{p['decoder']}{j}.up." for j in range(LEVELS)]


def kind(key):
    return sfm.kind(key)


def layer_shapes(img):
    """[(channels, side)] of the 21 layers' outputs in packed order."""
    out, h = [(8, img)], img
    for lv in range(LEVELS):
        out += [(8 << lv, h), (8 << lv, h), (16 << lv, (h + 1) // 2)]
        h = (h + 1) // 2
    return out + [(128 >> j, (img // 16) << j) for j in range(LEVELS)]


def forward_gated(sd, running, obs, form, dilation, residual, gates=None, us=None, stats=None):
    """-> (pooled (N,256), logit (N,1,S,S)) in train mode.  ``running``: {stem + "bn.running_mean" / "bn.running_var"},
    updated in place as nn.BatchNorm2d does.  ``gates`` / ``us`` as in fullnet_train_model.forward_gated; ``stats`` receives
    every layer's detached (mean, biased variance) of r."""
    p = SEG_PRESETS[PRESET]
    i = [0]

    def act_bn(u, st):
        if us is not None:
            us.append(u.detach())
        r = torch.relu(u) if gates is None else u * gates[i[0]]
        i[0] += 1
        if stats is not None:
            rd = r.detach()
            stats.append((rd.mean(dim=(0, 2, 3)), rd.var(dim=(0, 2, 3), unbiased=False)))
        return F.batch_norm(r, running[st + "bn.running_mean"], running[st + "bn.running_var"], sd[st + "bn.weight"],
                            sd[st + "bn.bias"], True, MOMENTUM, EPS)

    def layer(x, stem, sep, d, stride):
        st = p["prefix"] + stem
        if sep:
            u = F.conv2d(stm._depthwise_pair(x, sd[st + "conv.0.weight"], sd[st + "conv.1.weight"], d), sd[st + "conv.2.weight"],
                         sd[st + "conv.2.bias"])
        else:
            u = F.conv2d(x, sd[st + "conv.weight"], sd[st + "conv.bias"], stride, 1, 1)
        return act_bn(u, st)

    sep = form == "separable"
    x = layer(obs, "initial.", sep, 1, 1)
    skips = []
    for lv in range(LEVELS):
        stem = f"features.{lv}."
        y = layer(x, stem + "net.Layer 1.", sep, dilation, 1)
        y = layer(y, stem + "net.Layer 2.", sep, dilation, 1)
        if residual:
            y = y + x
        skips.append(y)
        x = layer(y, stem + "down.", False, 1, 2)
    pooled = x.mean(dim=(2, 3))
    for j, y in enumerate(skips[::-1]):
        st = f"{p['decoder']}{j}.up."
        u = F.conv_transpose2d(x, sd[st + "conv.weight"], sd[st + "conv.bias"], stride=2, padding=1, output_padding=1)
        x = act_bn(u, st) + y
    return pooled, F.conv2d(x, sd[p["classifier"] + "weight"], sd[p["classifier"] + "bias"])


class HostModel:
    """The network in train mode in ``dtype``.  ``forward(gates)`` -> (pooled, prob, grad_pred) with autograd through every
    parameter; every forward moves ``running`` (a copy of the checkpoint's statistics) and records ``stats``."""

    def __init__(self, sd32, form, dilation, residual, obs, dtype=torch.float64):
        self.sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd32.items()}
        self.form, self.dilation, self.residual, self.obs = form, int(dilation), bool(residual), obs.to(dtype)
        self.keys = enc_keys(form) + dec_keys() + head_keys()
        self.params = {k: self.sd[k].clone().requires_grad_() for k in self.keys}
        self.sd.update(self.params)
        self.running = {st + leaf: self.sd[st + leaf].clone() for st in bn_stems(form)
                        for leaf in ("bn.running_mean", "bn.running_var")}
        self.stats = None

    def forward(self, gates=None, us=None, obs=None):
        self.stats = []
        pooled, logit = forward_gated(self.sd, self.running, self.obs if obs is None else obs, self.form, self.dilation,
                                      self.residual, gates, us, self.stats)
        g = SEG_PRESETS[PRESET]["grad"]
        return pooled, torch.sigmoid(logit), F.linear(pooled, self.sd[g + "weight"], self.sd[g + "bias"])

    def grads(self, loss, head=False):
        for v in self.params.values():
            v.grad = None
        loss.backward()
        keys = self.keys if head else enc_keys(self.form) + dec_keys()
        return {k: (self.params[k].grad.clone() if self.params[k].grad is not None else torch.zeros_like(self.params[k]))
                for k in keys}

    def packed_stats(self):
        """``bn_stats`` of the latest forward: mean[c] | var_biased[c] per layer, packed order."""
        return torch.cat([t for mean, var in self.stats for t in (mean, var)])


def upstream(img, n):
    """The randn (grad_feats, grad_prob) of a case, f32."""
    gen = torch.Generator().manual_seed(obs_seed(img, n) + 1)
    return torch.randn(n, 256, generator=gen), torch.randn(n, 1, img, img, generator=gen)


@functools.lru_cache(maxsize=None)
def plain_f64(case):
    """(HostModel after one forward, its gradients for the case's randn upstream, its 21 u's) with its own relu gates;
    ``host.first`` = that forward's detached (pooled, prob).  Shared between tests: left as it is."""
    weights, form, d, res, img, n = case
    host = HostModel(state_dict(weights, form), form, d, res, case_obs(case).float())
    us = []
    pooled, prob, _pred = host.forward(None, us)
    host.first = (pooled.detach(), prob.detach())
    gf, gp = upstream(img, n)
    return host, host.grads((pooled * gf.double()).sum() + (prob * gp.double()).sum()), us


@functools.lru_cache(maxsize=None)
def e32(case):
    """{key: max |g32 - g64| / max |g64|}: PyTorch's f32 CPU autograd run of the case against the plain f64 model."""
    weights, form, d, res, img, n = case
    _host, want, _us = plain_f64(case)
    h32 = HostModel(state_dict(weights, form), form, d, res, case_obs(case).float(), torch.float32)
    pooled, prob, _pred = h32.forward()
    gf, gp = upstream(img, n)
    got = h32.grads((pooled * gf).sum() + (prob * gp).sum())
    return {k: float((got[k].double() - w).abs().max()) / float(w.abs().max()) for k, w in want.items()}


def bar(case, key):
    """The relative bar of one gradient tensor: max(1e-4, 4 e32)."""
    return max(TOL, MARGIN * e32(case)[key])


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


# ---- the workspace of occ_fullnet_bn_train_workspace_query in plain integers (include/occlusionenv_amd.h) -------------------
CHANNELS = 1248  # 1000 encoder + 248 decoder


def chunks(plane):
    return -(-plane // 4096)


def extra_ws_bytes(img, n):
    """coef (per channel s, t f32 and mu, rstd f64) | abc (A | B | C, 256 f32 each) | the forward's partials (the largest
    layer's c n chunks 2 doubles), every part 256-byte aligned."""
    a = dsm.align
    part = max(c * n * chunks(side * side) * 2 * 8 for c, side in layer_shapes(img))
    return a(24 * CHANNELS) + a(3 * 256 * 4) + a(part)


def ws_bytes(img, n):
    return ftm.ws_bytes(img, n) + extra_ws_bytes(img, n)


def scratch_bytes(form, img, n):
    return ftm.scratch_bytes(img, n) if form == "dense" else sfm.scratch_bytes(img, n)


band_shares = sfm.band_shares


def kept_relu(net, i):
    """The kept r of layer i of the latest train-mode forward of a joint net, a view of its workspace."""
    n, img = net._latest
    ws, _scratch = net._train_buffers(n, img, True)
    off, c, side = relu_views(img, n)[i]
    return ws[off:off + 4 * n * c * side * side].view(torch.float32).view(n, c, side, side)
