"""Native frozen encoder (occlusionenv_amd.encoder.FrozenEncoder) against the same network in PyTorch-ROCm
(tests/encoder_model.encode in f32 on the GPU under no_grad, same weights), in one process.

    python scripts/encoder_bench.py --out profiles/encoder_bench.json
    rocprofv3 --kernel-trace --stats -d DIR -o enc -- python scripts/encoder_bench.py --native-only --iters 3

Shapes: 256 envs x 256^2 (config 5 per rank) and 64 x 512^2.  Timing: 5 warm-ups, then the median of 20 HIP-event
timings per call.  MACs, FLOPs and the least HBM traffic (every layer reads its input once and writes its output once)
are counted from the shapes; shares of peak use 157.3 TF f32 and 8.0 TB/s.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import benchlib as bl  # noqa: E402
from occlusionenv_amd import encoder as E  # noqa: E402
from tests.encoder_model import encode, golden_state_dict, make_obs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x256,64x512", help="comma-separated NxS")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--native-only", action="store_true", help="skip the PyTorch path (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "encoder_bench needs a GPU"
    g = np.load(os.path.join(ROOT, "tests", "golden", "encoder_golden.npz"))
    sd64 = golden_state_dict(g, "ppo")
    enc = E.FrozenEncoder.from_state_dict(sd64, preset="ppo")
    sd32 = {k: v.to("cuda", torch.float32) if v.is_floating_point() else v for k, v in sd64.items()}
    results = []
    for n, img in bl.parse_shapes(args.shapes):
        base = make_obs(5, 8, img, dtype=torch.float32).cuda()
        obs = base[torch.arange(n) % 8].contiguous()
        macs, nbytes = bl.encoder_work(img, True, True)
        r = dict(n_env=n, img=img, launches_per_call=17, mac_per_env=macs, gflop_per_call=2 * macs * n / 1e9,
                 least_bytes_per_env=nbytes)
        med, ms = bl.timed(lambda: enc(obs), args.warmup, args.iters)
        r["native_ms"], r["native_ms_all"] = med, ms
        t_flop, t_byte = 2 * macs * n / bl.PEAK_F32, nbytes * n / bl.PEAK_HBM
        r["native_frac_f32_peak"] = t_flop / (med * 1e-3)
        r["native_frac_hbm_peak"] = t_byte / (med * 1e-3)
        if not args.native_only:
            with torch.no_grad():
                ref = lambda: encode(sd32, obs, "encoder.", True, 2, True)  # noqa: E731
                tmed, tms = bl.timed(ref, args.warmup, args.iters)
                diff = float((ref() - enc(obs)).abs().max())
            r["torch_ms"], r["torch_ms_all"], r["speedup"] = tmed, tms, tmed / med
            r["max_abs_diff_vs_torch_f32"] = diff
        bl.emit(r)
        results.append(r)
    bl.write(dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, iters=args.iters, results=results), args.out)


if __name__ == "__main__":
    main()
