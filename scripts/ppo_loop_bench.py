"""The two PPO training loops side by side: ``ppo.train_rollouts`` (acting, records and returns as framework ops) and
``ppo.train_ppo`` (``occ_ppo_act``, ``occ_rollout_advance``, ``occ_ppo_returns``; csrc/occ_rollout.hpp), one update each per
sample.

    python scripts/ppo_loop_bench.py --out profiles/ppo_loop_bench.json

256 envs at 256^2 on the synthetic pool, the agent ``BatchedPPO.from_fullnetwork`` on the randomly initialised separable
dilation-2 checkpoint of scripts/encoder_bench.py, T = 50, K = 80, max_ep_len = 50.  A sample is one call of the loop for one
update, on the host clock between device synchronisations: the rollout part runs from the end of the first vector step (the
hook of both loops) to the start of the update, i.e. T - 1 steps; the update part from there to the loop's return (the new
loop's drain included).  Method of scripts/benchlib.py: ``--warmup`` calls of each loop, then ``--iters`` samples alternating
between the two; medians are compared, the larger min-max spread is the margin.  Loop-owned device launches: the kernel
events (and, apart, copies and memsets) under ``torch.profiler`` of what each loop itself adds to a step around the encoder
and ``venv.step``, and of its update.  Last, ``occ_ppo_act`` and ``occ_rollout_advance`` alone, ``--calls`` launches between
two device events.

``--precision bf16`` adds a third loop to the same interleaved samples: ``ppo.train_ppo`` with the agent of
``BatchedPPO.from_fullnetwork(sd, precision="bf16")`` (the encoder's bf16 inference mode, csrc/occ_encoder_bf16.hpp), and
reports its rollout step and update next to the f32 ``train_ppo`` of the same session under ``rollout_step_bf16`` /
``update_bf16``.  Without the flag the script does what it did.

    python scripts/ppo_loop_bench.py --precision bf16 --out profiles/ppo_loop_bf16_bench.json
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import benchlib as bl  # noqa: E402
from tests.encoder_model import golden_state_dict  # noqa: E402


def make_venv(n, img, models):
    import tempfile

    from occlusionenv_amd.environment import OcclusionEnv, seed_scene_rng
    from occlusionenv_amd.meshes import SyntheticShapeNet
    from occlusionenv_amd.SubProcVecEnv import SimpleVecEnv

    np.random.seed(0)
    seed_scene_rng(0)
    ds = SyntheticShapeNet(n_models=models, seed=1234, cache_dir=tempfile.gettempdir())
    return SimpleVecEnv([(lambda: OcclusionEnv(ds, img_size=img)) for _ in range(n)])


class Split:
    """Host-clock marks of one loop call: after the first step, at the start of the update, at the return."""

    def __init__(self, agent, method):
        self.agent, self.method, self.real = agent, method, getattr(agent, method)
        self.t_first = self.t_update = None
        setattr(agent, method, self.update)

    def hook(self, *_a):
        if self.t_first is None:
            torch.cuda.synchronize()
            self.t_first = time.perf_counter()

    def update(self, *a):
        torch.cuda.synchronize()
        self.t_update = time.perf_counter()
        return self.real(*a)

    def done(self, T):
        torch.cuda.synchronize()
        t_end = time.perf_counter()
        setattr(self.agent, self.method, self.real)
        return (self.t_update - self.t_first) / (T - 1) * 1e3, (t_end - self.t_update) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-env", type=int, default=256)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--models", type=int, default=1024)
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--K", type=int, default=80)
    ap.add_argument("--max-ep-len", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50, help="launches per sample of the two kernels alone")
    ap.add_argument("--precision", choices=("f32", "bf16"), default="f32", help="bf16: also time train_ppo with the bf16 encoder")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ppo_loop_bench needs a GPU"
    from occlusionenv_amd import ppo, rollout
    from occlusionenv_amd.monitor import EpisodeMonitor

    n, T = args.n_env, args.T
    sd = golden_state_dict(np.load(os.path.join(ROOT, "tests", "golden", "encoder_golden.npz")), "ppo")
    venv = make_venv(n, args.img, args.models)
    agents = {k: ppo.BatchedPPO.from_fullnetwork(sd, seed=0, K_epochs=args.K) for k in ("train_rollouts", "train_ppo")}
    if args.precision == "bf16":
        agents["train_ppo_bf16"] = ppo.BatchedPPO.from_fullnetwork(sd, seed=0, K_epochs=args.K, precision="bf16")
    gen = torch.Generator(device="cuda").manual_seed(0)

    def one(name):
        agent = agents[name]
        if name == "train_rollouts":
            sp = Split(agent, "update")
            ppo.train_rollouts(venv, agent, n_updates=1, T=T, generator=gen, on_step=sp.hook, max_ep_len=args.max_ep_len)
        else:
            sp = Split(agent, "update_from")
            ppo.train_ppo(venv, agent, max_training_timesteps=T * n - 1, T=T, max_ep_len=args.max_ep_len, generator=gen,
                          on_step=sp.hook, action_std_decay_freq=10 ** 9, save_model_freq=10 ** 9)
        return sp.done(T)

    step_ms, update_ms = {k: [] for k in agents}, {k: [] for k in agents}
    for it in range(args.warmup + args.iters):
        for name in agents:
            s, u = one(name)
            if it >= args.warmup:
                step_ms[name].append(s)
                update_ms[name].append(u)
    out = dict(device=torch.cuda.get_device_name(0), n_env=n, img=args.img, T=T, K_epochs=args.K, max_ep_len=args.max_ep_len,
               warmup=args.warmup, iters=args.iters,
               what="one update per sample; rollout = ms per vector step over the last T - 1 steps of the rollout (encoder, acting, "
                    "venv.step, bookkeeping), update = ms from the end of the rollout to the loop's return; host clock between "
                    "device synchronisations; interleaved samples, medians, margin = the larger min-max spread")
    out["rollout_step"] = bl.named(bl.compare(step_ms["train_ppo"], step_ms["train_rollouts"]), bl.ONE_RIVAL_NOT_SLOWER,
                                   n="train_ppo", r="train_rollouts")
    out["update"] = bl.named(bl.compare(update_ms["train_ppo"], update_ms["train_rollouts"]), bl.ONE_RIVAL_NOT_SLOWER,
                             n="train_ppo", r="train_rollouts")
    if args.precision == "bf16":  # reported, no bar: the same loop, the encoder's mode apart
        out["rollout_step_bf16"] = bl.named(bl.compare(step_ms["train_ppo_bf16"], step_ms["train_ppo"]), bl.ONE_RIVAL,
                                            n="train_ppo_bf16", r="train_ppo")
        out["update_bf16"] = bl.named(bl.compare(update_ms["train_ppo_bf16"], update_ms["train_ppo"]), bl.ONE_RIVAL_NOT_SLOWER,
                                      n="train_ppo_bf16", r="train_ppo")

    # ---- what each loop itself launches around the encoder and venv.step, on the tensors of a real step ----------------
    old, new = agents["train_rollouts"], agents["train_ppo"]
    obs = venv.reset()[:, 0]
    feats = new.features(obs)
    buf, mon = ppo.RolloutBuffer(T, n, obs.device), EpisodeMonitor(n, obs.device)
    action = new.act_features_into(feats, buf, 0, gen)
    obs, rewards, dones, _infos = venv.step(action)
    codes = venv.episode_end_codes.clone()
    rewards = rewards.detach()
    state = dict(rew_sum=torch.zeros((), device=obs.device))

    def old_step():
        a, lp = old.policy_old.act(feats, gen)
        rollout.pack_records(obs, a, lp, rewards, dones, features=feats)
        state["rew_sum"] = state["rew_sum"] + rewards.mean()

    def new_step():
        new.act_features_into(feats, buf, 0, gen)
        mon.advance(rewards, codes, dones, buffer=buf, t=0)

    rec = rollout.pack_records(obs, action, buf.logprobs[0], rewards, dones, features=feats)

    def old_update():
        old.records = [rec] * T
        old.update()

    def new_update():
        new.update_from(buf)
        mon.drain()

    for t in range(T):  # a full buffer of plausible rows
        new.act_features_into(feats, buf, t, gen)
        mon.advance(rewards, codes, dones, buffer=buf, t=t)
    out.update(bl.launch_counts(dict(train_rollouts=old_step, train_ppo=new_step), prefix="step_"))
    out.update(bl.launch_counts(dict(train_rollouts=old_update, train_ppo=new_update), prefix="update_"))
    ms = bl.interleaved(dict(occ_ppo_act_with_randn=lambda: new.act_features_into(feats, buf, 0, gen),
                             occ_rollout_advance=lambda: mon.advance(rewards, codes, dones, buffer=buf, t=0),
                             torch_act_and_pack=old_step), 2, 10, args.calls)
    out.update(bl.medians(ms, prefix="alone_"))
    bl.emit({k: v for k, v in out.items() if not isinstance(v, dict)})
    bl.emit(out["rollout_step"])
    bl.emit(out["update"])
    if args.precision == "bf16":
        bl.emit(out["rollout_step_bf16"])
    bl.write(out, args.out)


if __name__ == "__main__":
    main()
