"""GPU tests of the training loop ``ppo.train_ppo`` and of ``monitor.EpisodeMonitor`` around a plain step loop: what the
loop's hook sees against the rollout buffer, ``SimpleVecEnv.episode_end_codes`` against ``dones`` and the step's infos, the CSV
against tests/rollout_model.py replayed on the captured rewards and codes, and the decay / checkpoint schedule.

Sizes.  4 envs at 64^2 (the host-driven step path; the monitor alone also runs on 16 envs, the path with a reserve, where the
codes are a view of the device report), T = 6 steps per update, max_ep_len = 4, two updates of two epochs."""
import os

import numpy as np
import pytest
import torch

from tests import rollout_model as rm

pytestmark = pytest.mark.gpu

N, S, T, MAX_EP_LEN = 4, 64, 6, 4
SEED = 5           # a seed with which both a done and a time-limit reset occur in the 12 steps (checked below)
ACTION_STD = 0.6
DECAY_FREQ, SAVE_FREQ, MAX_TIMESTEPS = 30, 26, 30  # timesteps run 4, 8, ... 48: 30 is crossed at 32, 26 at 28; 24 <= 30 < 48


def _same(name, got, want):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, name
    bad = g.view(np.uint8) != w.view(np.uint8)
    assert not bad.any(), f"{name}: {int(bad.sum())} bytes differ, first at {tuple(np.argwhere(bad)[0])}"


@pytest.fixture(scope="module")
def ds():
    from occlusionenv_amd.meshes import SyntheticShapeNet

    return SyntheticShapeNet(n_models=8, seed=1234)


def _venv(ds, n):
    from environment import OcclusionEnv
    from SubProcVecEnv import SimpleVecEnv

    return SimpleVecEnv([lambda: OcclusionEnv(ds, img_size=S) for _ in range(n)])


class _Seeded:
    """Every generator the env draws scenes, reset azimuths and ages from, seeded; the reset generator restored afterwards."""

    def __init__(self, seed):
        self.seed = seed

    def __enter__(self):
        from occlusionenv_amd import environment

        environment.seed_scene_rng(self.seed)
        environment.seed_reset_rng(self.seed)
        np.random.seed(self.seed)
        torch.manual_seed(self.seed)

    def __exit__(self, *exc):
        from occlusionenv_amd import environment

        environment.seed_reset_rng(None)


def _truncated(infos, n):
    return np.array([bool(infos[i].get("TimeLimit.truncated", False)) for i in range(n)])


def run_training(ds, seed, action_std, tmp):
    """Two updates of train_ppo with a hook that captures every step.  -> dict of everything the tests look at."""
    from occlusionenv_amd import ppo

    venv = _venv(ds, N)
    agent = ppo.BatchedPPO(K_epochs=2, device="cuda", seed=0, action_std_init=action_std)
    steps, records, calls = [], [], []
    decay, save = agent.decay_action_std, agent.save
    agent.decay_action_std = lambda *a: (calls.append(("decay", len(steps))), decay(*a))[1]
    agent.save = lambda *a: (calls.append(("save", len(steps))), save(*a))[1]

    def hook(action, rewards, step):
        steps.append(dict(feats=step["feats"].clone(), action=action.detach().clone(), logprob=step["logprob"].clone(),
                          rewards=rewards.detach().clone(), dones=step["dones"].clone(), codes=step["codes"].clone(),
                          truncated=_truncated(step["infos"], N), timestep=step["timestep"], t=step["t"], obs=step["obs"]))
        if step["t"] == T - 1:
            records.append(step["buffer"].records())

    log, ckpt = os.path.join(tmp, "log.csv"), os.path.join(tmp, "ppo.pth")
    with _Seeded(seed):
        stats = ppo.train_ppo(venv, agent, max_training_timesteps=MAX_TIMESTEPS, T=T, max_ep_len=MAX_EP_LEN,
                              action_std_decay_freq=DECAY_FREQ, save_model_freq=SAVE_FREQ, checkpoint_path=ckpt, log_path=log,
                              generator=torch.Generator(device="cuda").manual_seed(5), on_step=hook)
    torch.cuda.synchronize()
    venv.engine.check_status()
    return dict(stats=stats, steps=steps, records=records, calls=calls, log=log, ckpt=ckpt, agent=agent,
                rewards=np.stack([s["rewards"].cpu().numpy() for s in steps]),
                codes=np.stack([s["codes"].cpu().numpy() for s in steps]),
                dones=np.stack([s["dones"].cpu().numpy() for s in steps]))


@pytest.fixture(scope="module")
def trained(ds, tmp_path_factory):
    return run_training(ds, SEED, ACTION_STD, str(tmp_path_factory.mktemp("train_ppo")))


def test_two_updates_of_six_steps(trained):
    assert len(trained["stats"]) == 2 and len(trained["steps"]) == 2 * T
    assert [s["timestep"] for s in trained["steps"]] == [N * (k + 1) for k in range(2 * T)]
    assert [s["t"] for s in trained["steps"]] == list(range(T)) * 2
    for st in trained["stats"]:
        assert st["samples"] == T * N and all(np.isfinite(st[k]) for k in ("loss_first", "loss_last", "value_loss_first", "value_loss_last"))
    agent = trained["agent"]
    for k, v in agent.policy.state_dict().items():
        _same(f"policy_old {k}", agent.policy_old.state_dict()[k].cpu().numpy(), v.cpu().numpy())


def test_buffer_is_what_pack_records_makes_of_the_captured_steps(trained):
    from occlusionenv_amd import rollout

    for u, rec in enumerate(trained["records"]):
        assert rec.shape == (T, N, 261)
        want = torch.stack([rollout.pack_records(s["obs"], s["action"], s["logprob"], s["rewards"], s["dones"], features=s["feats"])
                            for s in trained["steps"][u * T:(u + 1) * T]])
        _same(f"records of update {u}", rec.cpu().numpy(), want.cpu().numpy())


def test_codes_are_dones_and_time_limits(trained):
    codes, dones = trained["codes"], trained["dones"]
    assert codes.dtype == np.int32 and set(np.unique(codes).tolist()) <= {0, 1, 2}
    assert np.array_equal(codes == 1, dones)
    assert np.array_equal(codes == 2, np.stack([s["truncated"] for s in trained["steps"]]))
    print("codes per step", codes.tolist())
    assert (codes == 1).any(), "no env finished: choose another SEED"
    assert (codes == 2).any(), "no env reached the time limit: choose another SEED"


def _csv(path):
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] == "episode,timestep,reward,running_reward,length"
    return lines[1:]


def test_csv_is_the_model_replayed_on_the_captured_stream(trained):
    rows = _csv(trained["log"])
    want, st = rm.replay_log(trained["rewards"], trained["codes"])
    assert rows == want and len(rows) == int((trained["codes"] != 0).sum()) > 0
    assert [int(r.split(",")[0]) for r in rows] == list(range(1, len(rows) + 1))


def test_decay_and_save_ran_once_each_when_their_threshold_was_crossed(trained):
    # the hook runs before the schedule: len(steps) is the number of vector steps taken, the counter is N times that
    want = sorted([("decay", -(-DECAY_FREQ // N)), ("save", -(-SAVE_FREQ // N))], key=lambda c: c[1])
    assert trained["calls"] == want
    assert trained["agent"].action_std == round(ACTION_STD - 0.05, 4)
    assert [st["action_std"] for st in trained["stats"]] == [ACTION_STD, round(ACTION_STD - 0.05, 4)]
    sd = torch.load(trained["ckpt"], map_location="cpu")
    assert set(sd) == set(trained["agent"].policy_old.state_dict())


def test_stats_agree_with_the_csv(trained):
    rows = [r.split(",") for r in _csv(trained["log"])]
    _, st = rm.replay_log(trained["rewards"], trained["codes"])
    seen = 0
    for u, s in enumerate(trained["stats"]):
        mine = [r for r in rows if u * T * N < int(r[1]) <= (u + 1) * T * N]
        assert s["episodes"] == len(mine) and s["lost"] == 0 and s["timestep"] == (u + 1) * T * N
        seen += len(mine)
        if mine:
            assert s["mean_length"] == np.mean([int(r[4]) for r in mine])
            assert abs(s["mean_return"] - np.mean([float(r[2]) for r in mine])) <= 0.5e-4 + 1e-12
            assert round(s["running_reward"], 4) == float(mine[-1][3])
        want_mean = float(trained["rewards"][u * T:(u + 1) * T].astype(np.float64).mean())
        assert abs(s["mean_reward"] - want_mean) <= 1e-5 * max(1.0, abs(want_mean))
    assert seen == len(rows)
    assert np.float32(trained["stats"][-1]["running_reward"]) == st["running"][0]


@pytest.mark.parametrize("n", [4, 16])
def test_monitor_alone_around_a_step_loop(ds, n, tmp_path):
    """EpisodeMonitor around venv.step without train_ppo: 8 steps.  16 envs: the step path with a reserve, where the codes are
    the device report's first words."""
    from occlusionenv_amd.monitor import EpisodeMonitor

    venv = _venv(ds, n)
    assert (venv.engine.R > 0) == (n == 16)
    mon = EpisodeMonitor(n, "cuda", capacity=64)
    gen = torch.Generator(device="cuda").manual_seed(9)
    rewards_l, codes_l, dones_l, trunc_l = [], [], [], []
    with _Seeded(SEED):
        venv.reset()
        mon.reset()
        venv.max_ep_len = MAX_EP_LEN
        venv.stagger_ages()
        for _k in range(8):
            action = torch.randn((n, 2), device="cuda", generator=gen) * ACTION_STD
            _obs, rewards, dones, infos = venv.step(action)
            codes = venv.episode_end_codes
            assert codes.shape == (n,) and codes.dtype == torch.int32 and codes.is_cuda
            mon.advance(rewards, codes, dones)
            rewards_l.append(rewards.detach().cpu().numpy())
            codes_l.append(codes.cpu().numpy())
            dones_l.append(dones.cpu().numpy())
            trunc_l.append(_truncated(infos, n))
    venv._drain()
    venv.engine.check_status()
    rewards, codes, dones = np.stack(rewards_l), np.stack(codes_l), np.stack(dones_l)
    assert np.array_equal(codes == 1, dones) and np.array_equal(codes == 2, np.stack(trunc_l))
    assert (codes == 2).any()
    path = str(tmp_path / "log.csv")
    eps = mon.write_csv(path)
    want, st = rm.replay_log(rewards, codes)
    assert _csv(path) == want and eps["lost"] == 0 and len(eps["ret"]) == len(want) == int((codes != 0).sum())
    tot = mon.totals()
    assert (tot["episodes"], tot["done"], tot["time_limit"]) == (len(want), int((codes == 1).sum()), int((codes == 2).sum()))
    mon.write_csv(path)  # nothing new: no further row, no second header
    assert _csv(path) == want
