"""Native ``FrozenEncoder.forward_full`` (encoder + segmentation decoder, occlusionenv_amd/encoder.py) against the same
network in PyTorch-ROCm (tests/segmenter_model.full_forward in f32 on the GPU under no_grad, same weights), in one process.

    python scripts/segmenter_bench.py --out profiles/segmenter_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o seg -- python scripts/segmenter_bench.py --native-only --iters 3
    python scripts/segmenter_bench.py --merge-trace DIR/.../seg_kernel_trace.csv --out profiles/segmenter_bench.json

Shapes: 256 envs x 256^2 and 64 x 512^2.  Timing: 5 warm-ups, then 20 HIP-event timings per call, all kept; medians are
compared, with the larger of the two runs' min-max spreads as the margin.  MACs and the least HBM traffic (every layer
reads its inputs once and writes its output once) are counted from the shapes for the decoder alone and for the whole
pass; shares of peak use 157.3 TF f32 and 8.0 TB/s.  ``--merge-trace`` adds the decoder kernels' share of the native
kernel time from a kernel trace (a run of its own, no counters) to an existing result file; no GPU needed.
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import benchlib as bl  # noqa: E402
from occlusionenv_amd import encoder as E  # noqa: E402
from tests.encoder_model import make_obs  # noqa: E402
from tests.segmenter_model import full_forward, golden_seg_state_dict  # noqa: E402

LEVEL0_BW = 2.0e12  # what the level-0 encoder kernels reach: the yardstick of the decoder's added time


def decoder_work(img: int):
    """(MACs, least bytes) per env of the five up layers + classifier; per level [(macs, bytes)]."""
    levels, h = [], img // 32
    for j, cin, cout in E.decoder_plan():
        macs = h * h * 9 * cin * cout  # nine taps per input pixel, each used once
        out = 4 * cout * (2 * h) ** 2
        nbytes = 4 * cin * h * h + out + (out if j < 4 else 0)  # input, skip, output (the last level's stays in registers)
        if j == 4:
            macs += (2 * h) ** 2 * cout
            nbytes += 4 * (2 * h) ** 2  # the probability map
        levels.append((macs, nbytes))
        h *= 2
    return sum(m for m, _ in levels), sum(b for _, b in levels), levels


def merge_trace(path, out):
    d = json.load(open(out))
    rows = list(csv.DictReader(open(path)))
    name = next(k for k in rows[0] if k.lower() in ("kernel_name", "kernelname", "name"))
    t0 = next(k for k in rows[0] if k.lower().startswith("start"))
    t1 = next(k for k in rows[0] if k.lower().startswith("end"))
    dec = enc = 0.0
    per, full_calls, all_calls = {}, 0, 0
    for r in rows:
        dt = (int(r[t1]) - int(r[t0])) / 1e3
        if "occ_dec_" in r[name]:
            dec += dt
            full_calls += "true>" in r[name]  # the fused last level: one per forward_full
        elif "occ_enc_" in r[name]:
            enc += dt
            all_calls += "occ_enc_pool_kernel" in r[name]  # one per forward_full and per enc(obs)
        else:
            continue
        key = r[name].split("(")[0]
        per[key] = per.get(key, 0.0) + dt
    # the traced run calls forward_full and enc(obs) equally often on the same inputs: forward_full's part of the encoder
    # kernels' time is their total times its share of the calls
    enc_full = enc * full_calls / all_calls
    d["kernel_trace"] = dict(source="rocprofv3 --kernel-trace --stats, scripts/segmenter_bench.py --native-only --iters 3 (both "
                             "shapes, warm-ups included)", forward_full_calls=full_calls, encoder_calls=all_calls, decoder_us=dec,
                             encoder_us_all_calls=enc, encoder_us_in_forward_full=enc_full, decoder_share=dec / (dec + enc_full),
                             per_kernel_us=per)
    json.dump(d, open(out, "w"), indent=1)
    print(json.dumps(d["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x256,64x512", help="comma-separated NxS")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--native-only", action="store_true", help="skip the PyTorch path (for a kernel trace)")
    ap.add_argument("--merge-trace", default=None, help="kernel trace CSV to summarise into --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.merge_trace:
        return merge_trace(args.merge_trace, args.out)
    assert torch.cuda.is_available(), "segmenter_bench needs a GPU"
    g = np.load(os.path.join(ROOT, "tests", "golden", "segmenter_golden.npz"))
    sd64 = golden_seg_state_dict(g, "ppo")
    enc = E.FrozenEncoder.from_state_dict(sd64, preset="ppo")
    sd32 = {k: v.to("cuda", torch.float32) if v.is_floating_point() else v for k, v in sd64.items()}
    results = []
    for n, img in bl.parse_shapes(args.shapes):
        base = make_obs(5, 8, img, dtype=torch.float32).cuda()
        obs = base[torch.arange(n) % 8].contiguous()
        emacs, ebytes = bl.encoder_work(img, True, True)
        ebytes += 4 * 256 * (img // 32) ** 2  # the last down output is stored as well
        dmacs, dbytes, levels = decoder_work(img)
        r = dict(n_env=n, img=img, launches_per_call=22, decoder_launches=5, decoder_mac_per_env=dmacs,
                 decoder_least_bytes_per_env=dbytes, decoder_levels=[dict(mac_per_env=m, least_bytes_per_env=b) for m, b in levels],
                 mac_per_env=emacs + dmacs, least_bytes_per_env=ebytes + dbytes, gflop_per_call=2 * (emacs + dmacs) * n / 1e9)
        med, ms = bl.timed(lambda: enc.forward_full(obs), args.warmup, args.iters)
        emed, ems = bl.timed(lambda: enc(obs), args.warmup, args.iters)
        r["native_ms"], r["native_ms_all"] = med, ms
        r["encoder_only_ms"], r["encoder_only_ms_all"] = emed, ems
        r["decoder_added_ms"] = med - emed
        r["decoder_least_traffic_ms_at_2TBs"] = dbytes * n / LEVEL0_BW * 1e3
        r["native_frac_f32_peak"] = 2 * (emacs + dmacs) * n / bl.PEAK_F32 / (med * 1e-3)
        r["native_frac_hbm_peak"] = (ebytes + dbytes) * n / bl.PEAK_HBM / (med * 1e-3)
        if not args.native_only:
            with torch.no_grad():
                ref = lambda: full_forward(sd32, obs, "ppo")  # noqa: E731
                tmed, tms = bl.timed(ref, args.warmup, args.iters)
                want, got = ref(), enc.forward_full(obs)
                diff = max(float((want["prob"] - got[1]).abs().max()), float((want["pooled"] - got[0]).abs().max()))
            margin = max(max(ms) - min(ms), max(tms) - min(tms))
            r.update(torch_ms=tmed, torch_ms_all=tms, speedup=tmed / med, margin_ms=margin, not_slower=bool(med <= tmed + margin),
                     max_abs_diff_vs_torch_f32=diff)
        bl.emit(r)
        results.append(r)
    bl.write(dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, iters=args.iters, results=results), args.out)


if __name__ == "__main__":
    main()
