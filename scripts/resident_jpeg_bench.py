"""The JPEG round trip on the device (``devdata.generate_resident(jpeg=95)``: csrc/occ_jpeg.hpp after csrc/occ_datapack.hpp
at the rendering size, before csrc/occ_resize.hpp) against generation without it, in one process at two shapes: 256 envs
rendering and storing 256 x 256, and 64 envs rendering 512 x 512 into a 256 x 256 store.

    python scripts/resident_jpeg_bench.py --out profiles/resident_jpeg_bench.json

Per shape:
  (a) the bare loop the generators share, at the rendering size: ``eng.step`` with its backward and the action draws,
      nothing stored; each sample is ``--calls`` iterations between two device events;
  (b) ``generate_resident`` without ``jpeg``, ``--frames`` frames per run: whole calls on the host clock, ending in a
      device synchronise; ms per engine step and frames / s;
  (c) the same with ``jpeg=95``;
  (d) ``occ_dataset_jpeg`` alone on one step's packed frames through the C ABI (two launches), ``--calls`` calls between
      two device events; next to it the pack alone, pack plus round trip, and (at 512 -> 256) pack, round trip and resize.
      The bytes (d) has to move at the least: 8 B per pixel per launch (a word read and a word written) plus the chroma
      workspace written once and read once, 2 x 2 B per chroma sample.  That figure is an ESTIMATE of the traffic (the
      upsampling pass reads every chroma sample four times, from the caches or not), so the GB/s derived from it is not a
      bandwidth measurement;
  (e) what is replaced: PIL's ``save(format="JPEG", quality=95)`` plus ``open().convert("RGB")`` of one packed frame in
      memory on one CPU, ms per frame.

The bar: everything between the engine's step and the store is at most 25 % of one iteration of (a).  At 256 envs of
256 x 256 that is pack plus round trip.  At 512 x 512 the pack's dither pass alone misses the bar
(profiles/resident_resize_bench.json), so there the round trip's own share is what is reported.
"""
import argparse
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import benchlib as bl  # noqa: E402

BAR = 0.25
QUALITY = 95


def measure(args, N, R, S):
    from bench import build_env
    from PIL import Image

    from occlusionenv_amd import _native as nat
    from occlusionenv_amd import devdata

    F, lr = args.frames, 2.5e-2
    venv, _ = build_env(args.workload, N, R, seed=0)
    eng = venv.engine
    dev = eng.device
    out = dict(envs=N, img=R, size=S, frames=N * F)

    # (a)
    venv.reset()
    venv._drain()
    gen = torch.Generator(device=dev).manual_seed(1)
    bare, state = bl.generation_loop(eng, lr, gen)
    out.update(bl.medians(bl.interleaved(dict(a_bare_iteration=bare), args.warmup, args.iters, args.calls)))
    print("(a)", N, R, out["a_bare_iteration_ms"], flush=True)

    # (d), on the outputs of the last step
    obs, fs = state["obs"].contiguous(), state["fs"].contiguous()
    staged = devdata.DeviceDataset.empty(N, R, dev)
    slots = torch.arange(N, dtype=torch.int64, device=dev)
    ws_bytes = devdata.jpeg_workspace_bytes(R, N, QUALITY)
    ws = torch.empty(ws_bytes // 2, dtype=torch.int16, device=dev)
    lib, st = nat.load(), nat.stream_ptr(dev)

    def pack():
        nat.check(lib.occ_dataset_pack(nat.ptr(obs), nat.ptr(fs, 12), 4, N, R, nat.ptr(slots), nat.ptr(staged.rgbl),
                                       nat.ptr(staged.depth), N, 0, st), "occ_dataset_pack")

    def jpeg():
        nat.check(lib.occ_dataset_jpeg(nat.ptr(staged.rgbl), N, R, nat.ptr(slots), N, QUALITY, nat.ptr(ws), st), "occ_dataset_jpeg")

    def pack_jpeg():
        pack()
        jpeg()

    paths = dict(pack=pack, d_jpeg=jpeg, pack_jpeg=pack_jpeg)
    if R != S:
        ds = devdata.DeviceDataset.empty(N, S, dev)
        rws = torch.empty(devdata.resize_workspace_bytes(R, S, N) // 4, dtype=torch.int32, device=dev)

        def all_three():
            pack_jpeg()
            nat.check(lib.occ_dataset_resize(nat.ptr(staged.rgbl), nat.ptr(staged.depth), N, R, nat.ptr(slots), nat.ptr(ds.rgbl),
                                             nat.ptr(ds.depth), N, S, nat.ptr(rws), st), "occ_dataset_resize")

        paths["pack_jpeg_resize"] = all_three
    pack()
    out.update(bl.medians(bl.interleaved(paths, args.warmup, args.iters, args.calls)))
    a = out["a_bare_iteration_ms"]
    out["pack_share_of_a"], out["d_jpeg_share_of_a"] = out["pack_ms"] / a, out["d_jpeg_ms"] / a
    out["pack_jpeg_share_of_a"] = out["pack_jpeg_ms"] / a
    if R == S:
        out["pack_jpeg_under_bar"] = bool(out["pack_jpeg_share_of_a"] <= BAR)
    else:
        out["pack_jpeg_resize_share_of_a"] = out["pack_jpeg_resize_ms"] / a
    out["d_traffic_estimate_bytes"] = N * R * R * 16 + 2 * ws_bytes
    out["d_traffic_estimate_gb_per_s"] = out["d_traffic_estimate_bytes"] / (out["d_jpeg_ms"] * 1e-3) / 1e9
    print("(d)", out["d_jpeg_ms"], out["d_jpeg_share_of_a"], "pack + jpeg", out["pack_jpeg_ms"], out["pack_jpeg_share_of_a"],
          out["d_traffic_estimate_gb_per_s"], flush=True)

    # (e), one packed frame of the last step
    pack()
    torch.cuda.synchronize()
    rgb = staged.unpack(0)[0]
    v = []
    for it in range(1 + args.iters):
        t = time.perf_counter()
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, format="JPEG", quality=QUALITY)
        back = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
        dt = time.perf_counter() - t
        if it:
            v.append(dt * 1e3)
    jpeg()
    torch.cuda.synchronize()
    assert np.array_equal(staged.unpack(0)[0], back), "the device round trip is not PIL's"
    out["e_pil_ms_per_frame"], out["e_pil_ms_per_frame_all"] = statistics.median(v), v
    out["e_pil_ms_per_step_one_cpu"] = out["e_pil_ms_per_frame"] * N
    print("(e)", out["e_pil_ms_per_frame"], flush=True)
    del staged, ws

    # (b), (c)
    for key, q in (("b_resident", None), ("c_resident_jpeg", QUALITY)):
        def generate(q=q):
            ds = devdata.generate_resident(venv, N, num_frames=F, lr=lr, generator=gen, size=None if R == S else S, jpeg=q)
            assert ds.size == S
            return ds

        out.update(bl.timed_generation(eng, key, generate, args.iters, N * F))
        print(key, out[f"{key}_ms_per_step"], out[f"{key}_frames_per_s"], flush=True)
    out["c_minus_b_ms_per_step"] = out["c_resident_jpeg_ms_per_step"] - out["b_resident_ms_per_step"]
    del venv, eng, bare, state
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20, help="frames per run")
    ap.add_argument("--workload", default="shapenet5k", choices=["shapenet5k", "mixed", "teapot"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="iterations per timed sample of (a) and (d)")
    ap.add_argument("--shapes", default="256:256:256,64:512:256", help="envs:rendering size:stored size, comma separated")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "resident_jpeg_bench needs a GPU"
    out = dict(device=torch.cuda.get_device_name(0), quality=QUALITY, frames_per_run=args.frames, workload=args.workload,
               warmup=args.warmup, iters=args.iters, calls_per_sample=args.calls, bar_share=BAR,
               d_traffic_note="16 B per pixel (a word read and written in each of the two launches) plus the chroma workspace "
                              "written and read once: an estimate of the least traffic, not a bandwidth measurement",
               shapes=[])
    for shape in args.shapes.split(","):
        N, R, S = (int(x) for x in shape.split(":"))
        out["shapes"].append(measure(args, N, R, S))
    for sh in out["shapes"]:
        bl.emit(sh)
    bl.write(out, args.out)


if __name__ == "__main__":
    main()
