"""One training step of the gradient predictor on a separable encoder, native (occlusionenv_amd/septrain.py:
``net.predict_grad(obs)`` -> ``F.mse_loss`` -> ``backward``; csrc/occ_sepenc_bwd.hpp) against the same expressions of
tests/encoder_model.py as PyTorch-ROCm ops in f32 with torch autograd, in one process with interleaved samples.

    python scripts/sep_encoder_train_bench.py --out profiles/sep_encoder_train_bench.json

Shapes: 128 x 256^2 and 64 x 512^2.  Weights: "ppo" = the separable FullNetwork fixture tests/golden/encoder_golden.npz
(dilation 2, residual, gradPredictor head) and "predictor" = tests/train_model.sep_state_dict("predictor", 32, gain 1.25)
(dilation 1, no residual, tanh head).  Both paths compute the gradients of the 86 encoder parameters and of the head; neither
runs an optimizer.  The torch path runs BatchNorm with its running statistics, as the native one does.  Each sample is
``--calls`` steps between two HIP events; after ``--warmup`` samples of each path, ``--iters`` samples alternate between the
two.  All samples are kept; medians are compared, with the larger of the two min-max spreads as the margin.
``--native-only``: the native step alone, for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o sep -- \\
        python scripts/sep_encoder_train_bench.py --native-only --warmup 1 --iters 3 --calls 1
    python scripts/sep_encoder_train_bench.py --stats-from DIR/.../sep_kernel_stats.csv --stats-steps 4 \\
        --out profiles/sep_encoder_train_kernel_stats.json
"""
import argparse
import csv
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.encoder_model import golden_state_dict, make_obs, preset_forward  # noqa: E402
from tests.train_model import sep_state_dict  # noqa: E402


def sample(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def torch_step_fn(sd, params, obs, target, preset):
    sdp = dict(sd)
    sdp.update(params)

    def step():
        for v in params.values():
            v.grad = None
        _f, g = preset_forward(sdp, obs, preset)
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


def weights(preset):
    if preset == "ppo":
        g = np.load(os.path.join(ROOT, "tests", "golden", "encoder_golden.npz"))
        return {k: v.float() for k, v in golden_state_dict(g, "ppo").items() if v.is_floating_point()}
    return {k: v.float() for k, v in sep_state_dict("predictor", 32, gain=1.25).items()}


def run_shape(preset, sd32, enc, n, img, warmup, iters, calls, native_only):
    from occlusionenv_amd.septrain import TrainableSeparableEncoder

    base = make_obs(31, 8, img).float()
    obs = base[torch.arange(n) % 8].cuda()
    target = F.normalize(torch.randn(n, 2, generator=torch.Generator().manual_seed(7)), dim=1).cuda()
    net = TrainableSeparableEncoder.from_encoder(enc)
    nat = native_step_fn(net, obs, target)
    head = dict(preset=preset, dilation=enc.dilation, residual=enc.residual, n_env=n, img=img)
    if native_only:
        for _ in range(warmup):
            sample(nat, calls)
        nms = [sample(nat, calls) for _ in range(iters)]
        return dict(head, native_ms=statistics.median(nms), native_ms_all=nms)
    sd = {k: v.cuda() for k, v in sd32.items()}
    params = {k: sd[k].clone().requires_grad_() for k, _p in net.named_parameters()}
    ref = torch_step_fn(sd, params, obs, target, preset)
    lw, lg = float(ref().detach()), float(nat().detach())
    rel = {}
    for k, p in net.named_parameters():
        kind = k[k.index(".conv.") + 1:] if ".conv." in k else ".".join(k.split(".")[-2:])
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
    return dict(head, native_ms=med, native_ms_all=nms, torch_ms=tmed, torch_ms_all=tms, native_spread_ms=max(nms) - min(nms),
                torch_spread_ms=max(tms) - min(tms), margin_ms=margin, speedup=tmed / med,
                faster_by_more_than_margin=bool(med + margin < tmed), loss_native=lg, loss_torch_f32=lw,
                grad_rel_to_max_vs_torch_f32=rel)


def kernel_stats(path, steps, note):
    """The per-kernel table of a ``rocprofv3 --kernel-trace --stats`` CSV (*_kernel_stats.csv), template arguments kept,
    the signature dropped; ``steps``: the native steps of every traced (preset, shape) pair."""
    kernels, total = {}, 0.0
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Name"].split("(")[0].replace("void ", "").replace("occ::", "")
            us = float(row["TotalDurationNs"]) / 1e3
            k = kernels.setdefault(name, dict(calls=0, total_us=0.0))
            k["calls"] += int(row["Calls"])
            k["total_us"] = round(k["total_us"] + us, 1)
            total += us
    for k in kernels.values():
        k["us_per_step_of_every_config"] = round(k["total_us"] / steps, 1)
    native = {n: k for n, k in kernels.items() if n.startswith("occ_")}
    other = round(sum(k["total_us"] for n, k in kernels.items() if n not in native) / steps, 1)
    ordered = dict(sorted(native.items(), key=lambda kv: -kv[1]["total_us"]))
    return dict(note=note, native_steps_traced_per_config=steps, total_kernel_us_per_step_of_every_config=round(total / steps, 1),
                torch_ops_us_per_step_of_every_config=other, kernels=ordered)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x256,64x512")
    ap.add_argument("--presets", default="ppo,predictor")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--calls", type=int, default=3, help="steps per timed sample")
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--stats-from", default=None, help="summarise a rocprofv3 *_kernel_stats.csv instead of timing")
    ap.add_argument("--stats-steps", type=int, default=4, help="native steps traced per (preset, shape)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.stats_from:
        out = kernel_stats(args.stats_from, args.stats_steps,
                           "rocprofv3 --kernel-trace --stats of scripts/sep_encoder_train_bench.py --native-only, a run of its own; "
                           "the presets and shapes share one trace, so times are per one step of every (preset, shape) pair")
    else:
        from occlusionenv_amd.encoder import FrozenEncoder

        assert torch.cuda.is_available(), "sep_encoder_train_bench needs a GPU"
        shapes = []
        for preset in args.presets.split(","):
            sd32 = weights(preset)
            enc = FrozenEncoder.from_state_dict(sd32, preset=preset)
            assert enc.separable
            for s in args.shapes.split(","):
                n, img = (int(v) for v in s.split("x"))
                r = run_shape(preset, sd32, enc, n, img, args.warmup, args.iters, args.calls, args.native_only)
                print(json.dumps({k: v for k, v in r.items() if not k.endswith("_all")}), flush=True)
                shapes.append(r)
        out = dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, iters=args.iters, calls_per_sample=args.calls,
                   shapes=shapes)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
