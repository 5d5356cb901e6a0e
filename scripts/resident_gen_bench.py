"""Generating the pretraining dataset: into device memory (``devdata.generate_resident``, csrc/occ_datapack.hpp) against
through the files (``dataset_io.generate`` + ``DeviceDataset.from_directory``), at 256 envs x 256^2.

    python scripts/resident_gen_bench.py --out profiles/resident_gen_bench.json

  (a) the bare loop both generators share: ``eng.step`` with its backward and the action draws, nothing stored; each
      sample is ``--calls`` iterations between two device events;
  (b) ``generate_resident(label="dither")``, ``--frames`` frames per run: whole calls on the host clock, ending in a device
      synchronise; ms per engine step and frames / s;
  (c) the same with ``label="threshold"`` (no dither pass);
  (d) the file path for the same frame count, once: ``dataset_io.generate`` into a temporary directory, then
      ``from_directory`` at the same size; seconds of each and frames / s of both together;
  (e) ``occ_dataset_pack`` alone on one step's outputs through the C ABI (two launches for dither, one for threshold), and
      through ``DeviceDataset.put``; ``--calls`` calls between two device events.

The bar: (e) with the dither is at most 25 % of one iteration of (a), so that generation stays bound by rendering.
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
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--frames", type=int, default=20, help="frames per run")
    ap.add_argument("--workload", default="shapenet5k", choices=["shapenet5k", "mixed", "teapot"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="iterations per timed sample of (a) and (e)")
    ap.add_argument("--skip-files", action="store_true", help="leave (d) out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "resident_gen_bench needs a GPU"
    from bench import build_env

    from occlusionenv_amd import _native as nat
    from occlusionenv_amd import dataset_io, devdata

    N, S, F, lr = args.envs, args.img, args.frames, 2.5e-2
    venv, _ = build_env(args.workload, N, S, seed=0)
    eng = venv.engine
    dev = eng.device
    out = dict(device=torch.cuda.get_device_name(0), envs=N, img=S, frames_per_run=F, frames=N * F, workload=args.workload,
               warmup=args.warmup, iters=args.iters, calls_per_sample=args.calls, bar_share=BAR)

    # (a)
    venv.reset()
    venv._drain()
    gen = torch.Generator(device=dev).manual_seed(1)
    bare, state = bl.generation_loop(eng, lr, gen)
    out.update(bl.medians(bl.interleaved(dict(a_bare_iteration=bare), args.warmup, args.iters, args.calls)))
    print("(a)", out["a_bare_iteration_ms"], flush=True)

    # (e), on the outputs of the last step
    obs, fs = state["obs"].contiguous(), state["fs"].contiguous()
    ds = devdata.DeviceDataset.empty(N, S, dev)
    slots = torch.arange(N, dtype=torch.int64, device=dev)
    lib, st = nat.load(), nat.stream_ptr(dev)

    def pack(mode):
        nat.check(lib.occ_dataset_pack(nat.ptr(obs), nat.ptr(fs, 12), 4, N, S, nat.ptr(slots), nat.ptr(ds.rgbl), nat.ptr(ds.depth),
                                       N, mode, st), "occ_dataset_pack")

    paths = dict(pack_dither=lambda: pack(0), pack_threshold=lambda: pack(1), put_dither=lambda: ds.put(obs, fs, slots),
                 put_threshold=lambda: ds.put(obs, fs, slots, label="threshold"))
    out.update(bl.medians(bl.interleaved(paths, args.warmup, args.iters, args.calls), "e_"))
    out["e_dither_pass_ms"] = out["e_pack_dither_ms"] - out["e_pack_threshold_ms"]
    out["e_point_pass_bytes"] = N * S * S * (5 * 4 + 6)  # the 16-byte full_state pixel counts as its 4 bytes of alpha
    out["e_share_of_a"] = out["e_pack_dither_ms"] / out["a_bare_iteration_ms"]
    out["e_under_bar"] = bool(out["e_share_of_a"] <= BAR)
    print("(e)", out["e_pack_dither_ms"], out["e_pack_threshold_ms"], out["e_share_of_a"], flush=True)
    del ds

    # (b), (c)
    for key, label in (("b_resident_dither", "dither"), ("c_resident_threshold", "threshold")):
        def generate(label=label):
            return devdata.generate_resident(venv, N, num_frames=F, lr=lr, generator=gen, label=label)

        out.update(bl.timed_generation(eng, key, generate, args.iters, N * F))
        print(f"({key[0]})", out[f"{key}_ms_per_step"], out[f"{key}_frames_per_s"], flush=True)

    # (d)
    if not args.skip_files:
        root = tempfile.mkdtemp(prefix="resident_gen_bench_")
        try:
            torch.cuda.synchronize()
            t = time.perf_counter()
            dataset_io.generate(venv, os.path.join(root, "train"), num_frames=F, lr=lr, generator=gen)
            out["d_files_generate_s"] = time.perf_counter() - t
            print("(d) written", out["d_files_generate_s"], flush=True)
            t = time.perf_counter()
            ds = devdata.DeviceDataset.from_directory(root, split="train", size=(S, S), device=dev)
            torch.cuda.synchronize()
            out["d_files_load_s"] = time.perf_counter() - t
            assert len(ds) == N * F
        finally:
            shutil.rmtree(root, ignore_errors=True)
        out["d_files_frames_per_s"] = N * F / (out["d_files_generate_s"] + out["d_files_load_s"])
        out["b_over_d"] = out["b_resident_dither_frames_per_s"] / out["d_files_frames_per_s"]
        print("(d)", out["d_files_load_s"], out["d_files_frames_per_s"], flush=True)
    bl.emit(out)
    bl.write(out, args.out)


if __name__ == "__main__":
    main()
