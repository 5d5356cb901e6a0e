"""The batched controller evaluation (occlusionenv_amd/episodes.py: ``harness.evaluate_controllers``, episode bookkeeping on
the device) against what a user could write without it, in one process with alternating repeats.

    python scripts/episode_eval_bench.py --out profiles/episode_eval_bench.json

Setup: 256 envs at 256^2, ``max_step = 50``, the four controllers, a random-weight separable dilation-2 FullNetwork
checkpoint (the one the tests build), the same seeded scenes and azimuths in every repeat.

  device  ``evaluate_controllers`` with ``poll_every = 16``: per controller the host clock from the reset render to a
          synchronise after the last step (``seconds`` of its result), over the steps it ran.
  (a)     the batched HOST-SYNCHRONOUS loop: the same engine, the active envs stepped through ``engine.step(env_ids=...)``,
          ``done`` and the NaN test read on the host in every step, the update in torch.  What a user would write today.
          It must give the same iterations as the device loop; the file says whether it did.
  (b)     eight sequential single-env ``harness.gradient_ascent`` episodes (raw gradient only), as ms per env-step times 256:
          an EXTRAPOLATION to the batch, not a measurement of it.

Every pass runs the same scenes: the seeds are set before each, ``venv.reset()``'s acceptance azimuths included
(``environment.seed_reset_rng``, for the duration of the reset: ``same_scenes``); (a) then runs on the scenes its device pass has just drawn, without a reset of its own.
One untimed pass of the device loop and of (a) comes first: it warms every shape, the subset sizes included (the scenes are
the same in every pass, so the subsets are).  Then ``--iters`` timed passes alternate device, (a).  The condition: the device
loop's median is not above (a)'s median by more than the min-max spread of (a)'s repeats.

The cost the bookkeeping adds to a step - one occ_episode_advance launch plus one poll in ``poll_every`` steps - is measured
on its own (HIP events around 200 launches; the host clock around the read of one int from an idle device) and set beside the
bare 256 x 256^2 step of profiles/resident_jpeg_bench.json, row (a).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import benchlib as bl  # noqa: E402
from occlusionenv_amd import _native as nat  # noqa: E402
from occlusionenv_amd import environment, episodes, harness, ppo  # noqa: E402
from occlusionenv_amd.encoder import FrozenEncoder  # noqa: E402


class same_scenes:
    """Seeds everything a ``venv.reset()`` draws from, its acceptance azimuths included, while active."""

    def __enter__(self):
        environment.seed_scene_rng(7)
        environment.seed_reset_rng(7)
        np.random.seed(7)
        torch.manual_seed(7)

    def __exit__(self, *exc):
        environment.seed_reset_rng(None)


def host_loop(eng, ctrl, max_step, az, gen):
    """(a): one controller's episodes with the bookkeeping on the host.  -> (iterations, seconds, steps, row_steps)."""
    N, dev = eng.N, eng.device
    t0 = time.perf_counter()
    eng.reset_render(azimuth=az, elevation=0.0, radius=4.0)
    rule = ctrl.rule
    action = episodes._randn(N, gen, dev) if rule == nat.EPISODE_RANDOM else torch.zeros(N, 2, device=dev)
    active = np.ones(N, dtype=bool)
    iterations = np.zeros(N, dtype=np.int64)
    feats_all = None
    steps = row_steps = 0
    for i in range(max_step):
        ids = np.nonzero(active)[0]
        whole = ids.size == N
        idx = None if whole else torch.as_tensor(ids, device=dev)  # (the engine keeps ``ids`` as its host copy: no read-back)
        a = (action if whole else action[idx]).detach().requires_grad_(rule == nat.EPISODE_GRADIENT)
        obs, reward, done, _fs, _loss = eng.step(a, env_ids=idx, env_ids_host=None if whole else ids)
        ok = None
        if rule == nat.EPISODE_GRADIENT:
            reward.sum().backward()
            ok = ~torch.isnan(a.grad).any(1)
            new = torch.where(ok[:, None], a.detach() + ctrl.lr * a.grad, a.detach())
        elif rule == nat.EPISODE_RANDOM:
            noise = episodes._randn(N, gen, dev)
            new = a + ctrl.lr * (noise if whole else noise[idx])
        else:
            f = (ctrl.enc if rule == nat.EPISODE_MODEL else ctrl.agent.features)(obs)
            if whole:
                feats_all = f
            else:
                feats_all.index_copy_(0, idx, f)
            pred = ctrl.enc.grad_head(feats_all) if rule == nat.EPISODE_MODEL else ctrl.agent.policy_old.act(feats_all, gen)[0]
            pred = pred if whole else pred[idx]
            new = -ctrl.lr * pred if rule == nat.EPISODE_MODEL else pred
        if whole:
            action = new
        else:
            action[idx] = new
        fin = (done if ok is None else done & ok).cpu().numpy()  # the host sync of every step
        steps, row_steps = steps + 1, row_steps + ids.size
        iterations[ids[fin]] = i + 1
        active[ids[fin]] = False
        if not active.any():
            break
    iterations[active] = max_step
    eng.check_status()
    return iterations, time.perf_counter() - t0, steps, row_steps


def single_env_extrapolation(ds, img, max_step, episodes_n):
    """(b): ms per env-step of sequential single-env harness.gradient_ascent episodes."""
    env = environment.OcclusionEnv(ds, img_size=img)
    harness.gradient_ascent(env, steps=3, lr=1.0)  # warm-up
    torch.cuda.synchronize()
    ms, steps = [], 0
    for _ in range(episodes_n):
        t0 = time.perf_counter()
        log, _ = harness.gradient_ascent(env, steps=max_step, lr=1.0)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
        steps += max(len(log), 1)
    return sum(ms) / steps, steps


def added_cost(lib, N, dev, poll_every):
    """us of one occ_episode_advance launch (events around 200 of them) and of one poll (one int read from an idle device)."""
    ep = episodes._Episodes(N, 10 ** 6, dev, torch.zeros(N, 2, device=dev), False)
    done = torch.zeros(N, dtype=torch.uint8, device=dev)
    z, noise = torch.zeros(N, device=dev), torch.randn(N, 2, device=dev)
    for _ in range(20):
        ep.advance(lib, nat.EPISODE_RANDOM, 1.0, 0, done, z, z, None, None, noise)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(200):  # the step index changes with every launch, so this is not benchlib.sample's loop
        ep.advance(lib, nat.EPISODE_RANDOM, 1.0, i, done, z, z, None, None, noise)
    b.record()
    b.synchronize()
    launch_us = 1e3 * a.elapsed_time(b) / 200
    polls = []
    for _ in range(50):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        int(ep.report.item())
        polls.append(1e6 * (time.perf_counter() - t0))
    poll_us = statistics.median(polls)
    return dict(advance_launch_us=launch_us, poll_us=poll_us, poll_every=poll_every,
                added_us_per_step=launch_us + poll_us / poll_every)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_eval_bench.json"))
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--max-step", type=int, default=50)
    ap.add_argument("--poll-every", type=int, default=16)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--single-episodes", type=int, default=8)
    ap.add_argument("--workload", default="shapenet5k", choices=["shapenet5k", "mixed"])
    ap.add_argument("--pool-models", type=int, default=1024)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("episode_eval_bench needs a GPU: nothing is measured without one")

    from bench import build_env
    from tests.encoder_model import golden_state_dict

    N, S = args.envs, args.img
    venv, ds = build_env(args.workload, N, S, seed=0, pool_models=args.pool_models)
    eng, dev = venv.engine, venv.engine.device
    sd = golden_state_dict(np.load(os.path.join(ROOT, "tests", "golden", "encoder_golden.npz")), "ppo")
    enc = FrozenEncoder.from_state_dict(sd, preset="ppo")
    agent = ppo.BatchedPPO.from_fullnetwork(sd, seed=0)
    ctrls = {c.name: c for c in (harness.GradientAscent(), harness.RandomWalk(), harness.PredictedGradient(enc), harness.Agent(agent))}
    az = torch.linspace(-0.5, 0.5, N)

    def device_pass():
        with same_scenes():
            return harness.evaluate_controllers(venv, ctrls, max_step=args.max_step, azimuth=az,
                                                generator=torch.Generator(device=dev).manual_seed(11), poll_every=args.poll_every)

    def host_pass():  # on the scenes the device pass before it has drawn (the loops leave them in the engine)
        gens = harness.controller_generators(torch.Generator(device=dev).manual_seed(11), len(ctrls))
        return {name: host_loop(eng, c, args.max_step, az.to(dev), g) for (name, c), g in zip(ctrls.items(), gens)}

    d0, h0 = device_pass(), host_pass()  # untimed: every shape, the subset sizes included
    match = {k: bool(np.array_equal(d0[k]["iterations"].cpu().numpy(), h0[k][0])) for k in ctrls}
    first_iterations = {k: d0[k]["iterations"].tolist() for k in ctrls}
    print("iterations match the host loop:", match, flush=True)
    dev_ms = {k: [] for k in ctrls}
    host_ms = {k: [] for k in ctrls}
    for _ in range(args.iters):
        d = device_pass()
        h = host_pass()
        for k in ctrls:
            match[k] = match[k] and bool(np.array_equal(d[k]["iterations"].cpu().numpy(), h[k][0]))
            match[k] = match[k] and d[k]["iterations"].tolist() == first_iterations[k]  # the same scenes in every pass
            dev_ms[k].append(1e3 * d[k]["seconds"] / d[k]["steps"])
            host_ms[k].append(1e3 * h[k][1] / h[k][2])
    rows = {}
    for k in ctrls:
        dm, hm = statistics.median(dev_ms[k]), statistics.median(host_ms[k])
        spread = max(host_ms[k]) - min(host_ms[k])
        rows[k] = dict(device_ms_per_step=dm, device_ms_per_step_all=dev_ms[k], a_host_sync_ms_per_step=hm,
                       a_host_sync_ms_per_step_all=host_ms[k], a_spread_ms=spread, not_slower_than_a=bool(dm <= hm + spread),
                       device_steps=d[k]["steps"], a_steps=h[k][2], device_row_steps=d[k]["row_steps"], a_row_steps=h[k][3],
                       frozen_row_step_share=d[k]["frozen_row_steps"] / d[k]["row_steps"], polls=d[k]["polls"],
                       compactions=d[k]["compactions"], iterations_match_a=match[k],
                       finished_share=float(d[k]["finished"].float().mean()), mean_iterations=float(d[k]["iterations"].float().mean()))
        print(k, {x: rows[k][x] for x in ("device_ms_per_step", "a_host_sync_ms_per_step", "a_spread_ms", "not_slower_than_a",
                                         "frozen_row_step_share", "polls", "compactions")}, flush=True)
    b_ms, b_steps = single_env_extrapolation(ds, S, args.max_step, args.single_episodes)
    cost = added_cost(eng.lib, N, dev, args.poll_every)
    bare = None
    try:
        for shp in json.load(open(os.path.join(ROOT, "profiles", "resident_jpeg_bench.json")))["shapes"]:
            if shp["envs"] == 256 and shp["img"] == 256:
                bare = shp["a_bare_iteration_ms"]
    except (OSError, KeyError, ValueError):
        pass
    cost["bare_step_ms_resident_jpeg_bench_row_a"] = bare
    if bare:
        cost["added_share_of_bare_step"] = cost["added_us_per_step"] / (1e3 * bare)
    out = dict(device=torch.cuda.get_device_name(0), envs=N, img=S, max_step=args.max_step, poll_every=args.poll_every,
               workload=args.workload, iters=args.iters, controllers=rows,
               b_single_env=dict(ms_per_env_step=b_ms, env_steps_timed=b_steps, episodes=args.single_episodes,
                                 extrapolated_ms_per_batched_step=b_ms * N,
                                 note="EXTRAPOLATION: sequential single-env harness.gradient_ascent, ms per env-step times the envs"),
               added_cost=cost)
    print(json.dumps(out["b_single_env"]), json.dumps(cost), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    bl.write(out, args.out)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
