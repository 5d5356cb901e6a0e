"""Native frozen encoder (occlusionenv_amd.encoder.FrozenEncoder) against the same network in PyTorch-ROCm
(tests/encoder_model.encode in f32 on the GPU under no_grad, same weights), in one process.

    python scripts/encoder_bench.py --out profiles/encoder_bench.json
    rocprofv3 --kernel-trace --stats -d DIR -o enc -- python scripts/encoder_bench.py --native-only --iters 3

Shapes: 256 envs x 256^2 (config 5 per rank) and 64 x 512^2.  Timing: 5 warm-ups, then the median of 20 HIP-event
timings per call.  MACs, FLOPs and the least HBM traffic (every layer reads its input once and writes its output once)
are counted from the shapes; shares of peak use 157.3 TF f32 and 8.0 TB/s.

The masked forward at 256 envs x 256^2, when that shape is among ``--shapes`` and not under ``--native-only``
(``enc(obs, skip=mask, out=feats)``: the same 17 launches on the same grids, the blocks of a skipped env
return at once) with 0 %, 50 %, 90 % and all but one of the envs skipped, the skipped envs a seeded random subset: benchlib's
interleaved samples (``--masked-calls`` calls each), first of the unmasked call and the 0 % mask alone, then of the unmasked
call and the other three masks (a sample that follows a much shorter one measured some 4 % longer here, so the pair that is
compared runs with nothing short beside it).  The 0 % row must be within the margin (the larger min-max spread) of the
unmasked call; the others say what the empty blocks cost, against the active share of the full time.
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


MASKED_SHAPE = (256, 256)  # the masked rows are measured at this shape of --shapes only


def masked_rows(enc, obs, warmup, iters, calls):
    """The masked forward at 0 %, 50 %, 90 % and all but one of the envs skipped, interleaved with the unmasked call."""
    n = int(obs.shape[0])
    order = torch.randperm(n, generator=torch.Generator().manual_seed(3))
    feats = torch.zeros(n, E.FEATURES, device=obs.device)
    paths, skipped = {}, {}
    for name, k in (("skip_0", 0), ("skip_50", n // 2), ("skip_90", (9 * n) // 10), ("skip_all_but_one", n - 1)):
        mask = torch.zeros(n, dtype=torch.int32)
        mask[order[:k]] = 1
        mask = mask.to(obs.device)
        paths[name], skipped[name] = (lambda m=mask: enc(obs, skip=m, out=feats)), k
    unmasked = lambda: enc(obs, out=feats)  # noqa: E731
    ms = bl.interleaved(dict(unmasked=unmasked, skip_0=paths.pop("skip_0")), warmup, iters, calls)
    rest = bl.interleaved(dict(unmasked=unmasked, **paths), warmup, iters, calls)
    ms.update({k: v for k, v in rest.items() if k != "unmasked"})
    full = bl.compare(ms["skip_0"], ms["unmasked"])
    out = dict(calls_per_sample=calls, unmasked_ms=full["rival_ms"], unmasked_ms_all=ms["unmasked"], unmasked_spread_ms=full["rival_spread_ms"],
               margin_ms=full["margin_ms"], skip_0_within_margin_of_unmasked=full["not_slower"],
               unmasked_beside_the_short_rows_ms=bl.compare(rest["unmasked"], ms["unmasked"])["native_ms"],
               unmasked_beside_the_short_rows_ms_all=rest["unmasked"], rows=[])
    for name, k in skipped.items():
        med = bl.compare(ms[name], ms["unmasked"])["native_ms"]
        out["rows"].append(dict(name=name, skipped=k, active=n - k, ms=med, ms_all=ms[name], spread_ms=max(ms[name]) - min(ms[name]),
                                share_of_unmasked=med / full["rival_ms"], active_share=(n - k) / n))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x256,64x512", help="comma-separated NxS")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--native-only", action="store_true", help="skip the PyTorch path (for a kernel trace)")
    ap.add_argument("--masked-calls", type=int, default=3, help="calls per sample of the masked rows at 256x256 (0: leave them out)")
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
        if args.masked_calls and (n, img) == MASKED_SHAPE and not args.native_only:  # (a kernel trace holds the plain forward alone)
            r["masked"] = masked_rows(enc, obs, args.warmup, args.iters, args.masked_calls)
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
