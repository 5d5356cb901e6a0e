"""The fused pretrainer criterion (occlusionenv_amd/segmentation.py: seg_criterion + binary_dice_loss forward and backward,
csrc/occ_criterion.hpp) against the same expressions as PyTorch-ROCm ops with autograd (loss.py's formula restated, plus
the accuracy / IoU lines of pretrainer.py:133-141), in one process with interleaved repeats.

    python scripts/criterion_bench.py --out profiles/criterion_bench.json

Shape: 128 x 256^2, the pretrainer's batch.  What one sample times is what one training step spends on the criterion: the
metrics, the loss, and the gradient with respect to the prediction.  Each sample is ``--calls`` such steps between two HIP
events (one step is a fraction of a millisecond); after ``--warmup`` samples of each path, ``--iters`` samples alternate between
the two paths.  All samples are kept; medians are compared, with the larger of the two min-max spreads as the margin.  The
least HBM traffic of a step (pred and target read once for the sums, once for the gradient, the gradient written once) is
counted from the shape; the share of peak uses 8.0 TB/s.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import benchlib as bl  # noqa: E402
from occlusionenv_amd import ops  # noqa: E402
from tests import criterion_model as cm  # noqa: E402


def native_step(pred, target):
    pred.grad = None
    c = ops.seg_criterion(pred, target)
    loss = ops.binary_dice_loss(pred, target)
    loss.backward()
    return loss, c["correct"].sum(), c["intersection"].sum(), c["union"].sum()


def torch_step(pred, target):
    pred.grad = None
    p, t = pred.contiguous().view(pred.shape[0], -1), target.contiguous().view(target.shape[0], -1)
    num = torch.sum(torch.mul(p, t), dim=1) + 1
    den = torch.sum(p.pow(2) + t.pow(2), dim=1) + 1
    loss = (1 - num / den).mean()
    loss.backward()
    with torch.no_grad():
        pm, bt = pred > 0.5, target > 0.5
        correct = (pm == bt).sum()
        inter = (pm * bt).sum()
        union = ((pm + bt) > 0.5).sum()
    return loss, correct, inter, union


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50, help="steps per timed sample")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "criterion_bench needs a GPU"
    base_p, base_t = cm.make_maps(7, 8, args.img, soft=False)
    idx = torch.arange(args.n) % 8
    pred = base_p[idx][:, None].cuda().requires_grad_(True)
    target = base_t[idx][:, None].cuda()

    nat = lambda: native_step(pred, target)  # noqa: E731
    ref = lambda: torch_step(pred, target)  # noqa: E731
    want, got = ref(), None
    want_grad = pred.grad.clone()
    got = nat()
    diff = dict(loss=abs(float(want[0].detach()) - float(got[0].detach())), grad_rel_to_max=float((pred.grad - want_grad).abs().max() / want_grad.abs().max()),
                counts_equal=all(int(a) == int(b) for a, b in zip(want[1:], got[1:])))
    ms = bl.interleaved(dict(native=nat, torch=ref), args.warmup, args.iters, args.calls)
    pixels = args.n * args.img * args.img
    # native: the metrics pass and the loss's forward each read both maps, the backward reads both and writes one
    native_bytes = 4 * pixels * (2 + 2 + 3)
    least_bytes = 4 * pixels * (2 + 3)
    r = dict(device=torch.cuda.get_device_name(0), n_env=args.n, img=args.img, warmup=args.warmup, iters=args.iters,
             calls_per_sample=args.calls, **bl.named(bl.compare(ms["native"], ms["torch"]), bl.ONE_RIVAL_NOT_SLOWER))
    r.update(native_bytes_per_step=native_bytes, least_bytes_per_step=least_bytes,
             native_frac_hbm_peak=native_bytes / bl.PEAK_HBM / (r["native_ms"] * 1e-3), diff_vs_torch_f32=diff)
    bl.emit(r)
    bl.write(r, args.out)


if __name__ == "__main__":
    main()
