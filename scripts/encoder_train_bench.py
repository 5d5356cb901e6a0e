"""One training step of the gradient predictor, native (occlusionenv_amd/enctrain.py: ``net.predict_grad(obs)`` ->
``F.mse_loss`` -> ``backward``; csrc/occ_encoder_bwd.hpp) against the same expressions of tests/encoder_model.py as
PyTorch-ROCm ops in f32 with torch autograd, in one process with interleaved samples.

    python scripts/encoder_train_bench.py --out profiles/encoder_train_bench.json

Shapes: 128 x 256^2 and 64 x 512^2, preset "predictor".  Both paths compute the gradients of the 64 encoder parameters and of
the head; neither runs an optimizer.  The torch path runs BatchNorm with its running statistics, as the native one does.
Each sample is ``--calls`` steps between two HIP events; after ``--warmup`` samples of each path, ``--iters`` samples alternate
between the two.  All samples are kept; medians are compared, with the larger of the two min-max spreads as the margin.
``--native-only``: the native step alone, for a kernel trace.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from occlusionenv_amd.encoder import FrozenEncoder  # noqa: E402
from occlusionenv_amd.enctrain import TrainableEncoder  # noqa: E402
from tests.encoder_model import make_obs, preset_forward  # noqa: E402
from tests.train_model import dense_state_dict  # noqa: E402


def sample(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def torch_step_fn(sd, params, obs, target):
    sdp = dict(sd)
    sdp.update(params)

    def step():
        for v in params.values():
            v.grad = None
        _f, g = preset_forward(sdp, obs, "predictor")
        loss = F.mse_loss(g, target)
        loss.backward()
        return loss

    return step


def native_step_fn(net, obs, target):
    def step():
        net.zero_grad(set_to_none=True)
        loss = F.mse_loss(net.predict_grad(obs), target)
        loss.backward()
        return loss

    return step


def run_shape(sd32, enc, n, img, warmup, iters, calls, native_only):
    base = make_obs(31, 8, img).float()
    obs = base[torch.arange(n) % 8].cuda()
    target = F.normalize(torch.randn(n, 2, generator=torch.Generator().manual_seed(7)), dim=1).cuda()
    net = TrainableEncoder.from_encoder(enc)
    nat = native_step_fn(net, obs, target)
    if native_only:
        for _ in range(warmup):
            sample(nat, calls)
        nms = [sample(nat, calls) for _ in range(iters)]
        return dict(n_env=n, img=img, native_ms=statistics.median(nms), native_ms_all=nms)
    sd = {k: v.cuda() for k, v in sd32.items()}
    params = {k: sd[k].clone().requires_grad_() for k, _p in net.named_parameters()}
    ref = torch_step_fn(sd, params, obs, target)
    lw, lg = float(ref().detach()), float(nat().detach())
    rel = {}
    for k, p in net.named_parameters():
        kind = ".".join(k.split(".")[-2:])
        err = float((p.grad - params[k].grad).abs().max() / params[k].grad.abs().max())
        rel[kind] = max(rel.get(kind, 0.0), err)
    for _ in range(warmup):
        sample(nat, calls), sample(ref, calls)
    nms, tms = [], []
    for _ in range(iters):
        nms.append(sample(nat, calls))
        tms.append(sample(ref, calls))
    med, tmed = statistics.median(nms), statistics.median(tms)
    margin = max(max(nms) - min(nms), max(tms) - min(tms))
    return dict(n_env=n, img=img, native_ms=med, native_ms_all=nms, torch_ms=tmed, torch_ms_all=tms,
                native_spread_ms=max(nms) - min(nms), torch_spread_ms=max(tms) - min(tms), margin_ms=margin, speedup=tmed / med,
                faster_by_more_than_margin=bool(med + margin < tmed), loss_native=lg, loss_torch_f32=lw,
                grad_rel_to_max_vs_torch_f32=rel)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x256,64x512")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--calls", type=int, default=3, help="steps per timed sample")
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "encoder_train_bench needs a GPU"
    sd32 = {k: v.float() for k, v in dense_state_dict("predictor", 32).items()}
    enc = FrozenEncoder.from_state_dict(sd32, preset="predictor")
    shapes = []
    for s in args.shapes.split(","):
        n, img = (int(v) for v in s.split("x"))
        r = run_shape(sd32, enc, n, img, args.warmup, args.iters, args.calls, args.native_only)
        print(json.dumps({k: v for k, v in r.items() if not k.endswith("_all")}), flush=True)
        shapes.append(r)
    out = dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, iters=args.iters, calls_per_sample=args.calls, shapes=shapes)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
