"""Everything that consumes a predicted occlusion map (csrc/occ_criterion.hpp, ``occ_seg_metrics``): the accuracy / IoU
counts of pretrainer.py:127-141 (``seg_counts``, ``occlusion_metrics``), the pretrainer's segmentation criterion
(pretrainer.py:89; loss.py's ``BinaryDiceLoss``, ``nn.BCELoss``) as ``seg_criterion``, ``binary_dice_loss`` and
``binary_cross_entropy`` for callers that train ``model.py`` with PyTorch-ROCm autograd, and one batch of
``PreTrainer.val()`` (``validation_losses``).  ``encoder.FrozenEncoder`` and ``ops`` hand these on under their old names.
"""
from __future__ import annotations

import torch

from . import _native as nat

MAX_ENVS_PER_CALL = 65535  # the grid limit of occ_seg_metrics, occ_seg_criterion and occ_seg_criterion_grad


def _maps(t: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise nat.NativeError("occlusion_metrics needs CUDA/ROCm tensors; there is no CPU fallback")
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3 or t.shape[1] != t.shape[2]:
        raise ValueError(f"{what} must be (N,S,S) or (N,1,S,S), got {tuple(t.shape)}")
    return t if t.dtype == torch.float32 else t.to(torch.float32)


def _map_pair(pred: torch.Tensor, target: torch.Tensor):
    """-> (pred (N,S,S) f32 contiguous, target (N,S,S) f32, the target's pixel stride k), checked before any native call.
    A target whose pixels lie k floats apart in an otherwise dense (N,S,S) order, such as ``full_state[..., 3]``, is read
    in place; any other layout is made contiguous (k = 1)."""
    pred, target = _maps(pred, "pred").detach().contiguous(), _maps(target, "target").detach()
    if pred.shape != target.shape or pred.device != target.device:
        raise ValueError(f"pred {tuple(pred.shape)} on {pred.device} and target {tuple(target.shape)} on {target.device} differ")
    img = int(pred.shape[1])
    if img > 1024:
        raise ValueError(f"image side {img} above 1024")
    k = target.stride(2)
    if not (k >= 1 and target.stride(1) == k * img and target.stride(0) == k * img * img):
        target, k = target.contiguous(), 1
    return pred, target, int(k)


def seg_counts(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """(N,3) int64 on the device: per env #(p == t), #(p and t), #(p or t) with p = pred > 0.5, t = target > 0.5
    (occ_seg_metrics)."""
    pred, target, k = _map_pair(pred, target)
    n, img = int(pred.shape[0]), int(pred.shape[1])
    counts = torch.empty(n, 3, dtype=torch.int64, device=pred.device)
    if n == 0:
        return counts
    st = nat.stream_ptr(pred.device)
    for lo, m in nat.row_chunks(n, MAX_ENVS_PER_CALL):
        nat.check(nat.load().occ_seg_metrics(nat.ptr(pred[lo:]), nat.ptr(target[lo:]), k, m, img, nat.ptr(counts[lo:]), st),
                  "occ_seg_metrics")
    return counts


@torch.no_grad()
def occlusion_metrics(pred: torch.Tensor, target: torch.Tensor) -> dict:
    """``FrozenEncoder.occlusion_metrics``."""
    c = seg_counts(pred, target)
    total = c.sum(0).to(torch.float64)
    n, img = int(c.shape[0]), int(pred.shape[-1])
    return dict(correct=c[:, 0], intersection=c[:, 1], union=c[:, 2], accuracy=total[0] / float(n * img * img),
                iou=total[1] / total[2])


def _seg_criterion(pred: torch.Tensor, target: torch.Tensor, k: int):
    """(sums (N,4) f64, counts (N,3) int64) of checked arguments: one occ_seg_criterion per 65 535 envs."""
    lib = nat.load()
    n, img = int(pred.shape[0]), int(pred.shape[1])
    sums = torch.empty(n, 4, dtype=torch.float64, device=pred.device)
    counts = torch.empty(n, 3, dtype=torch.int64, device=pred.device)
    if n == 0:
        return sums, counts
    st = nat.stream_ptr(pred.device)
    scratch = torch.empty(int(lib.occ_seg_criterion_scratch_bytes(min(n, MAX_ENVS_PER_CALL), img)) // 8, dtype=torch.float64,
                          device=pred.device)
    for lo, m in nat.row_chunks(n, MAX_ENVS_PER_CALL):
        nat.check(lib.occ_seg_criterion(nat.ptr(pred[lo:]), nat.ptr(target[lo:]), k, m, img, nat.ptr(sums[lo:]),
                                        nat.ptr(counts[lo:]), nat.ptr(scratch), st), "occ_seg_criterion")
    return sums, counts


@torch.no_grad()
def seg_criterion(pred: torch.Tensor, target: torch.Tensor) -> dict:
    """Everything the pretrainer's segmentation criterion and its metrics need (pretrainer.py:127-141), per env, from one
    read of the maps: f64 ``s_pt`` = sum p t, ``s_pp`` = sum p^2, ``s_tt`` = sum t^2, ``s_bce`` = the sum of nn.BCELoss's
    per-pixel terms (logs clamped at -100), and the int64 ``correct``, ``intersection``, ``union`` of
    ``FrozenEncoder.occlusion_metrics``; all (N,) on the device.  pred (N,1,S,S) or (N,S,S); target likewise, soft or
    binary; a strided view such as ``full_state[..., 3]`` is read in place.  Takes no gradient: see ``binary_dice_loss``
    and ``binary_cross_entropy``.  A per-env result does not depend, bitwise, on the batch around it."""
    pred, target, k = _map_pair(pred, target)
    sums, counts = _seg_criterion(pred, target, k)
    return dict(s_pt=sums[:, 0], s_pp=sums[:, 1], s_tt=sums[:, 2], s_bce=sums[:, 3], correct=counts[:, 0],
                intersection=counts[:, 1], union=counts[:, 2])


def dice_from_sums(s_pt, s_pp, s_tt, smooth=1.0):
    """loss.py:29-32 per env from the sums: (loss, num, den) with loss = 1 - num / den."""
    num, den = s_pt + smooth, s_pp + s_tt + smooth
    return 1.0 - num / den, num, den


def _criterion_grad(pred, target, k, mode, coef):
    lib = nat.load()
    n, img = int(pred.shape[0]), int(pred.shape[1])
    grad = torch.empty_like(pred)
    coef = coef.to(torch.float64).contiguous()
    st = nat.stream_ptr(pred.device)
    for lo, m in nat.row_chunks(n, MAX_ENVS_PER_CALL):
        nat.check(lib.occ_seg_criterion_grad(nat.ptr(pred[lo:]), nat.ptr(target[lo:]), k, m, img, mode, nat.ptr(coef[lo:]),
                                             nat.ptr(grad[lo:]), st), "occ_seg_criterion_grad")
    return grad


class _BinaryDiceLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, smooth, reduction):
        p, t, k = _map_pair(pred, target)
        sums, _counts = _seg_criterion(p, t, k)
        loss, num, den = dice_from_sums(sums[:, 0], sums[:, 1], sums[:, 2], smooth)
        ctx.save_for_backward(p, t, num, den)
        ctx.cfg = (k, reduction, pred.shape, pred.dtype)
        out = loss.mean() if reduction == "mean" else loss.sum() if reduction == "sum" else loss
        return out.to(p.dtype)

    @staticmethod
    def backward(ctx, g):
        p, t, num, den = ctx.saved_tensors
        k, reduction, shape, dtype = ctx.cfg
        n = int(p.shape[0])
        if n == 0:
            return torch.zeros(shape, dtype=dtype, device=p.device), None, None, None
        u = g.to(torch.float64).expand(n) if reduction == "none" else g.to(torch.float64).reshape(1).expand(n)
        if reduction == "mean":
            u = u / n
        coef = torch.stack([-u / den, 2.0 * u * num / (den * den)], 1)  # d(1 - num/den)/dp = -t/den + 2 p num/den^2
        return _criterion_grad(p, t, k, nat.CRITERION_DICE, coef).reshape(shape).to(dtype), None, None, None


class _BinaryCrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        p, t, k = _map_pair(pred, target)
        sums, _counts = _seg_criterion(p, t, k)
        ctx.save_for_backward(p, t)
        ctx.cfg = (k, pred.shape, pred.dtype)
        return (sums[:, 3].sum() / max(p.numel(), 1)).to(p.dtype)

    @staticmethod
    def backward(ctx, g):
        p, t = ctx.saved_tensors
        k, shape, dtype = ctx.cfg
        n = int(p.shape[0])
        if n == 0:
            return torch.zeros(shape, dtype=dtype, device=p.device), None
        coef = torch.zeros(n, 2, dtype=torch.float64, device=p.device)
        coef[:, 0] = g.to(torch.float64) / p.numel()
        return _criterion_grad(p, t, k, nat.CRITERION_BCE, coef).reshape(shape).to(dtype), None


def binary_dice_loss(pred: torch.Tensor, target: torch.Tensor, smooth: float = 1.0, reduction: str = "mean", p: int = 2) -> torch.Tensor:
    """loss.py's ``BinaryDiceLoss(smooth, p=2, reduction)(pred, target)`` (pretrainer.py:89,128): per env
    1 - (sum p t + smooth) / (sum p^2 + sum t^2 + smooth), then ``"mean"`` over the batch, ``"sum"``, or ``"none"`` ->
    (N,).  Differentiable w.r.t. ``pred`` only; one native pass forward (``seg_criterion``'s) and one backward.  The loss
    is formed in f64 and returned in pred's dtype."""
    if p != 2:
        raise ValueError(f"binary_dice_loss: only p = 2 (the reference's default and only use) is supported, got {p}")
    if reduction not in ("mean", "sum", "none"):
        raise ValueError("Unexpected reduction {}".format(reduction))
    return _BinaryDiceLoss.apply(pred, target, float(smooth), reduction)


def binary_cross_entropy(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """``nn.BCELoss()(pred, target)`` (pretrainer.py:89): the mean over all pixels of -(t log p + (1 - t) log(1 - p)) with
    both logs clamped at -100; backward (p - t) / max(p (1 - p), 1e-12) / numel.  Differentiable w.r.t. ``pred`` only."""
    return _BinaryCrossEntropy.apply(pred, target)


@torch.no_grad()
def validation_losses(segm: torch.Tensor, grad_pred: torch.Tensor, occlusion: torch.Tensor, grad: torch.Tensor,
                      use_dice: bool = True, use_l1: bool = False) -> dict:
    """``FrozenEncoder.validation_losses``."""
    c = seg_criterion(segm, occlusion)
    n, pixels = int(c["s_pt"].shape[0]), int(segm.shape[-1]) * int(segm.shape[-2])
    if use_dice:
        segm_loss = dice_from_sums(c["s_pt"], c["s_pp"], c["s_tt"])[0].mean()
    else:
        segm_loss = c["s_bce"].sum() / float(n * pixels)
    gp, g = grad_pred.to(torch.float32), grad.to(grad_pred.device, torch.float32)
    if gp.shape != g.shape:
        raise ValueError(f"grad_pred {tuple(gp.shape)} and grad {tuple(g.shape)} differ")
    grad_loss = (torch.nn.functional.smooth_l1_loss(gp, g, beta=0.01) if use_l1 else torch.nn.functional.mse_loss(gp, g)).double()
    correct, inter, union = c["correct"], c["intersection"], c["union"]
    return dict(loss=grad_loss + segm_loss, segm_loss=segm_loss, grad_loss=grad_loss,
                accuracy=correct.sum().double() / float(n * pixels), iou=inter.sum().double() / union.sum().double(),
                correct=correct, intersection=inter, union=union)
