"""f64 host model of the pretrainer's segmentation criterion (pretrainer.py:89,127-141,176-189; loss.py:24-39;
nn.BCELoss): the per-env sums and counts of csrc/occ_criterion.hpp, the losses formed from them and the gradients with
respect to the prediction.

Everything is a function of the GIVEN f32 ``pred`` and ``target`` (converted to f64 exactly), so the -100 clamp of the logs
and the 0.5 threshold are decided on the same numbers the kernels see.  Also here: the seeded inputs of the fixture
tests/golden/criterion_golden.npz.
"""
from __future__ import annotations

import numpy as np
import torch


def _flat64(x):
    x = torch.as_tensor(x).detach().cpu()
    # f32: the inputs the kernels see; f64: the maps of an f64 network chain (tests/segmenter_model.py)
    assert x.dtype in (torch.float32, torch.float64), "the model is a function of the given f32 (or f64) inputs"
    if x.dim() == 4:
        x = x[:, 0]
    return x.reshape(x.shape[0], -1)


def sums(pred, target):
    """-> dict of (N,) tensors: f64 s_pt, s_pp, s_tt, s_bce; int64 correct, intersection, union."""
    p32, t32 = _flat64(pred), _flat64(target)
    p, t = p32.double(), t32.double()
    lp = torch.log(p).clamp_min(-100.0)
    lq = torch.log(1.0 - p).clamp_min(-100.0)
    a, b = p32 > 0.5, t32 > 0.5
    return dict(s_pt=(p * t).sum(1), s_pp=(p * p).sum(1), s_tt=(t * t).sum(1), s_bce=(-(t * lp + (1.0 - t) * lq)).sum(1),
                correct=(a == b).sum(1), intersection=(a & b).sum(1), union=(a | b).sum(1))


def dice_loss(pred, target, smooth=1.0, reduction="mean"):
    s = sums(pred, target)
    loss = 1.0 - (s["s_pt"] + smooth) / (s["s_pp"] + s["s_tt"] + smooth)
    return {"mean": loss.mean(), "sum": loss.sum(), "none": loss}[reduction]


def bce_loss(pred, target):
    s = sums(pred, target)
    return s["s_bce"].sum() / _flat64(pred).numel()


def dice_grad(pred, target, smooth=1.0, reduction="mean", upstream=1.0):
    """d reduction(loss) / d pred x upstream, (N,S,S) f64; ``upstream`` a scalar, or (N,) for reduction "none"."""
    p, t = _flat64(pred).double(), _flat64(target).double()
    n = p.shape[0]
    num = (p * t).sum(1) + smooth
    den = (p * p).sum(1) + (t * t).sum(1) + smooth
    u = torch.as_tensor(upstream, dtype=torch.float64).expand(n) / (n if reduction == "mean" else 1)
    g = (-u / den)[:, None] * t + (2.0 * u * num / (den * den))[:, None] * p
    return g.reshape(torch.as_tensor(pred).shape)


def bce_grad(pred, target, upstream=1.0):
    """nn.BCELoss's backward: upstream / numel x (p - t) / max(p (1 - p), 1e-12)."""
    p, t = _flat64(pred).double(), _flat64(target).double()
    g = (float(upstream) / p.numel()) * (p - t) / (p * (1.0 - p)).clamp_min(1e-12)
    return g.reshape(torch.as_tensor(pred).shape)


def grad_loss(grad_pred, grad, use_l1=False):
    """nn.MSELoss() / nn.SmoothL1Loss(beta=0.01) (pretrainer.py:90) in f64."""
    d = torch.as_tensor(grad_pred).double().cpu() - torch.as_tensor(grad).double().cpu()
    if not use_l1:
        return (d * d).mean()
    a, beta = d.abs(), 0.01
    return torch.where(a < beta, 0.5 * a * a / beta, a - 0.5 * beta).mean()


def validation(pred, grad_pred, target, grad, use_dice=True, use_l1=False):
    """One batch of PreTrainer.val() (pretrainer.py:176-189): loss, segm_loss, grad_loss, accuracy and iou (fractions)."""
    s = sums(pred, target)
    segm = dice_loss(pred, target) if use_dice else bce_loss(pred, target)
    gl = grad_loss(grad_pred, grad, use_l1)
    return dict(loss=float(gl + segm), segm_loss=float(segm), grad_loss=float(gl),
                accuracy=float(s["correct"].sum()) / _flat64(pred).numel(),
                iou=float(s["intersection"].sum().double() / s["union"].sum().double()),
                correct=int(s["correct"].sum()), intersection=int(s["intersection"].sum()), union=int(s["union"].sum()))


# ---- seeded inputs ---------------------------------------------------------------------------------------------------
def make_maps(seed: int, n: int, img: int, soft: bool):
    """(pred, target) f32 (n,img,img).  pred: a smooth blob pattern plus noise, clipped to [0,1], so that both sides of 0.5
    are well populated, with a few entries set to exactly 0.0, 1.0 and 0.5 in every env (0 and 1 hit the -100 clamp and
    the 1e-12 floor of the BCE gradient; 0.5 is not above the threshold).  target: a shifted blob pattern, binary, or
    soft in [0,1] (blurred edges plus noise)."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(-1, 1, img), np.linspace(-1, 1, img), indexing="ij")
    pred = np.empty((n, img, img))
    target = np.empty((n, img, img))
    for i in range(n):
        cx, cy, r = rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(0.55, 0.75)
        d = np.sqrt((x - cx) ** 2 + (y - cy) ** 2)
        pred[i] = np.clip(0.5 + 0.6 * (r - d) + 0.12 * rng.standard_normal((img, img)), 0.0, 1.0)
        d2 = np.sqrt((x - cx - 0.15) ** 2 + (y - cy + 0.1) ** 2)
        if soft:
            target[i] = np.clip(0.5 + 2.5 * (r - d2) + 0.1 * rng.standard_normal((img, img)), 0.0, 1.0)
        else:
            target[i] = (d2 < r).astype(np.float64)
        idx = rng.choice(img * img, 9, replace=False)
        flat = pred[i].reshape(-1)
        flat[idx[:3]], flat[idx[3:6]], flat[idx[6:]] = 0.0, 1.0, 0.5
    return torch.from_numpy(pred.astype(np.float32)), torch.from_numpy(target.astype(np.float32))


def make_grad_pairs(seed: int, n: int):
    """(grad_pred, grad) f64 (n,2) with differences on both sides of SmoothL1Loss's beta = 0.01."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.standard_normal((n, 2)) * 0.008), torch.from_numpy(rng.standard_normal((n, 2)) * 0.008)
