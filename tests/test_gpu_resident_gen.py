"""GPU test of ``devdata.generate_resident`` with the engine: every frame of the resident dataset is
tests/datapack_model.py's ``pack_model`` of the engine step that produced it, with that step's camera angles and action
gradient as its labels, in run-major order; more runs than envs go in rounds; the result feeds ``harness.pretrain_epoch``.

2 envs of 32 x 32 (the smallest size the joint network takes) on the teapot pool.  ``eng.step`` is wrapped to keep each
step's outputs on the host; the bookkeeping of ``dataset_io.generate`` (a frame per finite gradient, in step order) is
redone here from what was captured.
"""
import numpy as np
import pytest
import torch

from tests import datapack_model as dm

pytestmark = pytest.mark.gpu

N, S, F = 2, 32, 3


@pytest.fixture(scope="module")
def venv():
    from environment import OcclusionEnv
    from occlusionenv_amd import environment
    from SubProcVecEnv import SimpleVecEnv

    environment.seed_scene_rng(77)
    np.random.seed(77)
    torch.manual_seed(77)
    return SimpleVecEnv([lambda: OcclusionEnv(None, img_size=S) for _ in range(N)])


def capture_steps(venv, monkeypatch):
    """Wraps ``eng.step``: a list of per-step dicts (obs, alpha, elevation, azimuth on the host; the action tensor, whose
    ``.grad`` the caller's backward fills)."""
    eng, steps = venv.engine, []
    real = eng.step

    def step(actions, *args, **kw):
        out = real(actions, *args, **kw)
        if actions.requires_grad:
            steps.append(dict(action=actions, obs=out[0].detach().cpu().numpy().copy(),
                              alpha=out[3][..., 3].detach().cpu().numpy().copy(),
                              el=eng.elevation.detach().cpu().numpy().reshape(N).copy(),
                              az=eng.azimuth.detach().cpu().numpy().reshape(N).copy()))
        return out

    monkeypatch.setattr(eng, "step", step)
    return steps


def expected_store(steps, num_runs, label_mode):
    """The frames in store order from the captured steps, by ``generate``'s rule: an env of a live run writes a frame at
    every step whose gradient is finite until it has F of them; a round ends when no live run lacks a frame."""
    M = num_runs * F
    planes = [np.zeros((M, S, S, 3), np.uint8), np.zeros((M, S, S), np.int16), np.zeros((M, S, S), np.uint8)]
    pos, graw, seen = np.zeros((M, 2), np.float32), np.zeros((M, 2), np.float64), np.zeros(M, bool)
    first, frame = 0, np.zeros(N, np.int64)
    for st in steps:
        live = first + np.arange(N) < num_runs
        if not (live & (frame < F)).any():
            first, frame = first + N, np.zeros(N, np.int64)
            live = first + np.arange(N) < num_runs
        g = st["action"].grad.detach().cpu().numpy()
        model = dm.pack_model(st["obs"], st["alpha"], label_mode)
        for i in range(N):
            if live[i] and frame[i] < F and not np.isnan(g[i]).any():
                slot = (first + i) * F + frame[i]
                for dst, src in zip(planes, model):
                    dst[slot] = src[i]
                pos[slot], graw[slot], seen[slot] = (st["el"][i], st["az"][i]), g[i], True
                frame[i] += 1
    assert seen.all()
    return planes, pos, graw


@pytest.mark.parametrize("num_runs,label", [(2, "dither"), (3, "threshold"), (3, "dither")])
def test_store_holds_the_model_of_every_step(venv, monkeypatch, num_runs, label):
    from occlusionenv_amd import devdata

    steps = capture_steps(venv, monkeypatch)
    ds = devdata.generate_resident(venv, num_runs, num_frames=F, generator=torch.Generator(device="cuda").manual_seed(5), label=label)
    M = num_runs * F
    assert len(ds) == M and ds.size == S and ds.split == "train" and ds.device.type == "cuda"
    assert len(steps) >= F * ((num_runs + N - 1) // N)
    planes, pos, graw = expected_store(steps, num_runs, devdata.LABEL_MODES[label])
    for f in range(M):
        got = ds.unpack(f)
        for name, g, w in zip(("rgb", "depth", "label"), got, planes):
            assert g.dtype == w.dtype and np.array_equal(g, w[f]), (f, name)
    assert planes[2].any() and planes[1].any() and planes[0].any()  # the scenes are there
    assert np.array_equal(ds.pos.cpu().numpy().view(np.uint32), pos.view(np.uint32))
    assert np.array_equal(ds.grad.cpu().numpy().view(np.uint32), devdata.sincos_grad(graw).view(np.uint32))
    assert len({tuple(row) for row in pos.tolist()}) == M  # every frame has a pose of its own


def test_raw_gradients_and_the_step_limit(venv, monkeypatch):
    from occlusionenv_amd import devdata

    steps = capture_steps(venv, monkeypatch)
    ds = devdata.generate_resident(venv, N, num_frames=F, generator=torch.Generator(device="cuda").manual_seed(6), grad_mode="raw", split="val")
    _, _, graw = expected_store(steps, N, dm.LABEL_DITHER)
    assert ds.split == "val" and np.array_equal(ds.grad.cpu().numpy(), graw.astype(np.float32))
    with pytest.raises(RuntimeError, match="stayed NaN"):
        devdata.generate_resident(venv, N, num_frames=F, max_steps=F - 1)
    with pytest.raises(ValueError):
        devdata.generate_resident(venv, N, num_frames=F, label="round")


def test_one_pretrain_epoch_from_the_generated_store(venv):
    from occlusionenv_amd import devdata, harness
    from occlusionenv_amd.encoder import FrozenEncoder
    from tests import train_model as tm

    ds = devdata.generate_resident(venv, N, num_frames=1, generator=torch.Generator(device="cuda").manual_seed(7))
    assert torch.allclose((ds.grad ** 2).sum(1), torch.ones(N, device="cuda"))  # (sin, cos)
    enc = FrozenEncoder.from_state_dict(tm.joint_state_dict("golden"), preset="ppo", dilation=2, residual=True)
    res = harness.pretrain_epoch(enc, ds.loader(batch_size=N, generator=torch.Generator().manual_seed(41)), native_optimizer=True)
    assert res["batches"] == 1 and res["pixels"] == N * S * S and np.isfinite(res["loss"])
