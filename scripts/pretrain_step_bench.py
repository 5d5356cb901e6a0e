"""One WHOLE step of the pretrainer on the device, optimizer included: ``zero_grad``, ``net(obs)``, Dice + MSE, ``backward``,
``optimizer.step()``, for the two optimizers of ``harness.pretrain_epoch``:

  per_key  ``torch.optim.AdamW`` on the ~110 parameters under the checkpoint's keys (every step folds 21 BatchNorm layers,
           packs both parts, slices the packed gradient back per key, then the optimizer walks the tensors);
  packed   ``netoptim.PackedAdamW``: the parameters stay in the packed layout, the optimizer is one native launch
           (csrc/occ_adamw.hpp).

    python scripts/pretrain_step_bench.py --out profiles/pretrain_step_bench.json

Both encoder forms (dense at dilation 1, separable at dilation 2, the "ppo" preset with the residual, running-statistics
BatchNorm) at 128 x 256^2, the shape of the other train benches, and at 8 x 64^2, where the device work is small and the
host path decides.  Method of the other train benches: one process, each sample is ``--calls`` steps between two HIP
events, ``--warmup`` samples of each path, then ``--iters`` samples alternating between the paths; all samples are kept,
medians are compared, the larger min-max spread of the two paths is the margin.  Device launches per step: the kernel
events (and, apart, the copies and memsets) of one step under ``torch.profiler``, after the timing.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import benchlib as bl  # noqa: E402
from tests import train_model as tm  # noqa: E402

FORMS = {"dense": 1, "separable": 2}  # form -> dilation


def step_fn(net, opt, obs, occl, grad):
    from occlusionenv_amd import segmentation

    def step():
        opt.zero_grad(set_to_none=True)
        _pooled, segm, pred = net(obs)
        loss = segmentation.binary_dice_loss(segm, occl) + F.mse_loss(pred, grad)
        loss.backward()
        opt.step()
        return loss

    return step


def run_case(form, n, img, warmup, iters, calls):
    from occlusionenv_amd.encoder import FrozenEncoder
    from occlusionenv_amd.fullnet import TrainableFullNetwork
    from occlusionenv_amd.netoptim import PackedAdamW
    from occlusionenv_amd.sepfullnet import TrainableSeparableFullNetwork

    sd32 = tm.joint_state_dict("golden", form == "separable")
    enc = FrozenEncoder.from_state_dict(sd32, preset="ppo", dilation=FORMS[form], residual=True)
    cls = TrainableFullNetwork if form == "dense" else TrainableSeparableFullNetwork
    obs, occl, grad, _target = (t.cuda() for t in bl.train_inputs(n, img))
    per_key_net, packed_net = cls.from_encoder(enc), cls.from_encoder(enc)
    steps = dict(per_key=step_fn(per_key_net, torch.optim.AdamW(per_key_net.parameters(), lr=1e-3, weight_decay=1e-5), obs, occl, grad),
                 packed=step_fn(packed_net, PackedAdamW(packed_net, lr=1e-3, weight_decay=1e-5), obs, occl, grad))
    first = {k: float(fn().detach()) for k, fn in steps.items()}
    ms = bl.interleaved(steps, warmup, iters, calls)
    out = dict(form=form, dilation=FORMS[form], n_env=n, img=img, first_loss=first)
    out.update(bl.named(bl.compare(ms["packed"], ms["per_key"]), bl.OPTIMIZERS, n="packed", r="per_key"))
    out.update(bl.launch_counts(steps))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x256,8x64")
    ap.add_argument("--forms", default="dense,separable")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--calls", type=int, default=3, help="steps per timed sample")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pretrain_step_bench needs a GPU"
    cases = []
    for form in args.forms.split(","):
        for n, img in bl.parse_shapes(args.shapes):
            r = run_case(form, n, img, args.warmup, args.iters, args.calls)
            bl.emit(r)
            cases.append(r)
            torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, iters=args.iters, calls_per_sample=args.calls,
               what="whole step: zero_grad, forward, Dice + MSE, backward, optimizer step; per_key = torch.optim.AdamW on the "
                    "parameters under the checkpoint's keys, packed = netoptim.PackedAdamW; same build, interleaved samples",
               cases=cases)
    bl.write(out, args.out)


if __name__ == "__main__":
    main()
