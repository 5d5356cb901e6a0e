"""Generating the pretraining dataset at the reference's sizes -- rendered at 512 x 512, stored at 256 x 256 -- into device
memory (``devdata.generate_resident(size=256)``: csrc/occ_datapack.hpp at 512, csrc/occ_resize.hpp into the store) against
through the files (``dataset_io.generate`` at 512 + ``DeviceDataset.from_directory`` at 256), at 64 envs.

    python scripts/resident_resize_bench.py --out profiles/resident_resize_bench.json

  (a) the bare loop both generators share, at the rendering size: ``eng.step`` with its backward and the action draws,
      nothing stored; each sample is ``--calls`` iterations between two device events;
  (b) ``generate_resident(size=--size)``, ``--frames`` frames per run: whole calls on the host clock, ending in a device
      synchronise; ms per engine step and frames / s;
  (c) ``occ_dataset_pack`` (dither) at the rendering size plus ``occ_dataset_resize`` into the store, on one step's
      outputs through the C ABI (four launches); ``--calls`` pairs between two device events;
  (d) ``occ_dataset_resize`` alone (the table launch and the fused pass), and the bytes it has to move at the least:
      6 B x (R^2 + S^2) per frame, every source pixel read once and every destination pixel written once.  That figure is
      an ESTIMATE of the traffic (window overlaps between tiles and the label reads hit the caches or do not), so the
      GB/s derived from it is not a bandwidth measurement;
  (e) the file path for the same frame count, once: ``dataset_io.generate`` at the rendering size into a temporary
      directory, then ``from_directory`` at the store's size; seconds of each and frames / s of both together.

The bar: (c) is at most 25 % of one iteration of (a), so that generation stays bound by rendering.
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import benchlib as bl  # noqa: E402

BAR = 0.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--img", type=int, default=512, help="the size the envs render at")
    ap.add_argument("--size", type=int, default=256, help="the size of the stored frames")
    ap.add_argument("--frames", type=int, default=20, help="frames per run")
    ap.add_argument("--workload", default="shapenet5k", choices=["shapenet5k", "mixed", "teapot"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="iterations per timed sample of (a), (c) and (d)")
    ap.add_argument("--skip-files", action="store_true", help="leave (e) out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "resident_resize_bench needs a GPU"
    from bench import build_env

    from occlusionenv_amd import _native as nat
    from occlusionenv_amd import dataset_io, devdata

    N, R, S, F, lr = args.envs, args.img, args.size, args.frames, 2.5e-2
    venv, _ = build_env(args.workload, N, R, seed=0)
    eng = venv.engine
    dev = eng.device
    out = dict(device=torch.cuda.get_device_name(0), envs=N, img=R, size=S, frames_per_run=F, frames=N * F, workload=args.workload,
               warmup=args.warmup, iters=args.iters, calls_per_sample=args.calls, bar_share=BAR)

    # (a)
    venv.reset()
    venv._drain()
    gen = torch.Generator(device=dev).manual_seed(1)
    bare, state = bl.generation_loop(eng, lr, gen)
    out.update(bl.medians(bl.interleaved(dict(a_bare_iteration=bare), args.warmup, args.iters, args.calls)))
    print("(a)", out["a_bare_iteration_ms"], flush=True)

    # (c), (d), on the outputs of the last step
    obs, fs = state["obs"].contiguous(), state["fs"].contiguous()
    staged, ds = devdata.DeviceDataset.empty(N, R, dev), devdata.DeviceDataset.empty(N, S, dev)
    slots = torch.arange(N, dtype=torch.int64, device=dev)
    ws = torch.empty(devdata.resize_workspace_bytes(R, S, N) // 4, dtype=torch.int32, device=dev)
    lib, st = nat.load(), nat.stream_ptr(dev)

    def pack():
        nat.check(lib.occ_dataset_pack(nat.ptr(obs), nat.ptr(fs, 12), 4, N, R, nat.ptr(slots), nat.ptr(staged.rgbl),
                                       nat.ptr(staged.depth), N, 0, st), "occ_dataset_pack")

    def resize():
        nat.check(lib.occ_dataset_resize(nat.ptr(staged.rgbl), nat.ptr(staged.depth), N, R, nat.ptr(slots), nat.ptr(ds.rgbl),
                                         nat.ptr(ds.depth), N, S, nat.ptr(ws), st), "occ_dataset_resize")

    def both():
        pack()
        resize()

    paths = dict(c_pack_resize=both, d_resize=resize, pack=pack, put_resize=lambda: ds.put(obs, fs, slots, resize=True))
    out.update(bl.medians(bl.interleaved(paths, args.warmup, args.iters, args.calls)))
    out["c_share_of_a"] = out["c_pack_resize_ms"] / out["a_bare_iteration_ms"]
    out["c_under_bar"] = bool(out["c_share_of_a"] <= BAR)
    out["d_traffic_estimate_bytes"] = N * 6 * (R * R + S * S)
    out["d_traffic_estimate_gb_per_s"] = out["d_traffic_estimate_bytes"] / (out["d_resize_ms"] * 1e-3) / 1e9
    out["d_traffic_note"] = "6 B x (R^2 + S^2) per frame: an estimate of the least traffic, not a bandwidth measurement"
    print("(c)", out["c_pack_resize_ms"], out["c_share_of_a"], "(d)", out["d_resize_ms"], out["d_traffic_estimate_gb_per_s"], flush=True)
    del ds, staged

    # (b)
    def generate():
        ds = devdata.generate_resident(venv, N, num_frames=F, lr=lr, generator=gen, size=S)
        assert ds.size == S
        return ds

    out.update(bl.timed_generation(eng, "b_resident", generate, args.iters, N * F))
    print("(b)", out["b_resident_ms_per_step"], out["b_resident_frames_per_s"], flush=True)

    # (e)
    if not args.skip_files:
        root = tempfile.mkdtemp(prefix="resident_resize_bench_")
        try:
            torch.cuda.synchronize()
            t = time.perf_counter()
            dataset_io.generate(venv, os.path.join(root, "train"), num_frames=F, lr=lr, generator=gen)
            out["e_files_generate_s"] = time.perf_counter() - t
            print("(e) written", out["e_files_generate_s"], flush=True)
            t = time.perf_counter()
            ds = devdata.DeviceDataset.from_directory(root, split="train", size=(S, S), device=dev)
            torch.cuda.synchronize()
            out["e_files_load_s"] = time.perf_counter() - t
            assert len(ds) == N * F and ds.size == S
        finally:
            shutil.rmtree(root, ignore_errors=True)
        out["e_files_frames_per_s"] = N * F / (out["e_files_generate_s"] + out["e_files_load_s"])
        out["b_over_e"] = out["b_resident_frames_per_s"] / out["e_files_frames_per_s"]
        print("(e)", out["e_files_load_s"], out["e_files_frames_per_s"], flush=True)
    bl.emit(out)
    bl.write(out, args.out)


if __name__ == "__main__":
    main()
