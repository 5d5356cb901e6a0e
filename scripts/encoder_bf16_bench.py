"""The frozen encoder's bf16 inference mode against its f32 mode (occlusionenv_amd.encoder.FrozenEncoder, ``precision=``),
same process, same build, same weights (the golden "ppo" network) and observations.

    python scripts/encoder_bf16_bench.py --out profiles/encoder_bf16_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o enc16 -- python scripts/encoder_bf16_bench.py --trace --iters 4
    python scripts/encoder_bf16_bench.py --trace-from DIR/.../enc16_kernel_trace.csv --iters 4 --out profiles/encoder_bf16_kernel_stats.json

Shapes: 256 envs x 256^2 and 64 x 512^2.  Method of scripts/benchlib.py: ``--warmup`` rounds, then ``--iters`` interleaved
samples of ``--calls`` calls of ``enc(obs, out=feats)`` each between two device events (ms per call); the medians are compared and the larger
min-max spread is the margin: ``faster_by_more_than_margin`` is the bar.  Also written: the workspace bytes of both modes
and the largest difference of the two modes' features on the bench's observations (the accuracy tests are
tests/test_gpu_encoder_bf16.py).  ``--trace``: both modes run ``--iters`` calls and nothing else (for a kernel trace, taken
in a run of its own, without counters).  ``--trace-from``: no GPU work; the trace's encoder kernels, in start order, are cut
into calls of 17 launches (per shape first the bf16 calls, then the f32 calls, as ``--trace`` issues them) and every launch
is reported as the median over the calls after the first, both modes side by side per layer.
"""
import argparse
import csv
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import benchlib as bl  # noqa: E402
from occlusionenv_amd import _native as nat  # noqa: E402
from occlusionenv_amd import encoder as E  # noqa: E402
from tests.encoder_model import golden_state_dict, make_obs  # noqa: E402


def workspace_bytes(enc, n, img):
    query = "occ_encoder_bf16_workspace_query" if enc.precision == "bf16" else "occ_encoder_workspace_query"
    nbytes = C.c_size_t()
    nat.check(getattr(nat.load(), query)(C.byref(enc._cfg(img)), n, C.byref(nbytes)), query)
    return int(nbytes.value)


LAYERS = ["initial"] + [f"L{lv}.{k}" for lv in range(E.LEVELS) for k in ("layer1", "layer2", "down")] + ["pool"]


def trace_summary(path, shapes, iters):
    """The per-launch table of both modes from a ``rocprofv3 --kernel-trace`` CSV of a ``--trace --iters iters`` run."""
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"].split("(")[0].replace("void ", "").replace("occ::", "")
            if name.startswith("occ_enc"):
                rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), name))
    rows.sort()
    per_call = len(LAYERS)
    assert len(rows) == len(shapes) * 2 * iters * per_call, (len(rows), "encoder launches in the trace; expected",
                                                              len(shapes) * 2 * iters * per_call)
    out, at = [], 0
    for n, img in shapes:
        modes = {}
        for mode in ("bf16", "f32"):
            calls = [rows[at + c * per_call:at + (c + 1) * per_call] for c in range(iters)]
            at += iters * per_call
            launches = []
            for i, layer in enumerate(LAYERS):
                assert len({c[i][2] for c in calls}) == 1
                us = statistics.median((c[i][1] - c[i][0]) / 1e3 for c in calls[1:])
                launches.append(dict(layer=layer, kernel=calls[0][i][2], us=round(us, 1)))
            total = sum(l["us"] for l in launches)
            for l in launches:
                l["share"] = round(l["us"] / total, 4)
            modes[mode] = dict(kernel_sum_ms=round(total / 1e3, 3), per_launch=launches)
        side = [dict(layer=a["layer"], f32_us=a["us"], bf16_us=b["us"], f32_over_bf16=round(a["us"] / b["us"], 2))
                for a, b in zip(modes["f32"]["per_launch"], modes["bf16"]["per_launch"])]
        out.append(dict(n_env=n, img=img, calls=iters, **modes, per_layer=side))
    return dict(source=f"rocprofv3 --kernel-trace --stats of scripts/encoder_bf16_bench.py --trace --iters {iters} (no counters in the "
                       "run); per launch the median over the calls after the first", shapes=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x256,64x512", help="comma-separated NxS")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--calls", type=int, default=3, help="calls per sample")
    ap.add_argument("--trace", action="store_true", help="run the calls only, --iters per mode and shape (for a kernel trace)")
    ap.add_argument("--trace-from", default=None, help="summarise the *_kernel_trace.csv of a --trace run (same --shapes, --iters)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_from:
        return bl.write(trace_summary(args.trace_from, bl.parse_shapes(args.shapes), args.iters), args.out)
    assert torch.cuda.is_available(), "encoder_bf16_bench needs a GPU"
    sd = golden_state_dict(np.load(os.path.join(ROOT, "tests", "golden", "encoder_golden.npz")), "ppo")
    f32 = E.FrozenEncoder.from_state_dict(sd, preset="ppo")
    bf16 = f32.with_precision("bf16")
    results = []
    for n, img in bl.parse_shapes(args.shapes):
        base = make_obs(5, 8, img, dtype=torch.float32).cuda()
        obs = base[torch.arange(n) % 8].contiguous()
        out32, out16 = torch.zeros(n, E.FEATURES, device="cuda"), torch.zeros(n, E.FEATURES, device="cuda")
        paths = dict(bf16=lambda: bf16(obs, out=out16), f32=lambda: f32(obs, out=out32))
        if args.trace:
            for fn in paths.values():
                for _ in range(args.iters):
                    fn()
            torch.cuda.synchronize()
            continue
        ms = bl.interleaved(paths, args.warmup, args.iters, args.calls)
        r = dict(n_env=n, img=img, launches_per_call=17, calls_per_sample=args.calls)
        r.update(bl.named(bl.compare(ms["bf16"], ms["f32"]), bl.ONE_RIVAL, n="bf16", r="f32"))
        r["workspace_bytes_f32"], r["workspace_bytes_bf16"] = workspace_bytes(f32, n, img), workspace_bytes(bf16, n, img)
        r["max_abs_diff_bf16_vs_f32"] = float((out16 - out32).abs().max())
        r["max_abs_feature_f32"] = float(out32.abs().max())
        bl.emit(r)
        results.append(r)
    if not args.trace:
        bl.write(dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, iters=args.iters, results=results), args.out)


if __name__ == "__main__":
    main()
