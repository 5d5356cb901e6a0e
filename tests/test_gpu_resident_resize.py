"""GPU test of ``devdata.generate_resident(size=)`` with the engine: the envs render at 64 x 64, the resident dataset holds
32 x 32 frames, and every stored frame is tests/resize_model.py's ``resize_model`` of tests/datapack_model.py's
``pack_model`` of the engine step that produced it -- what the reference's files-and-PIL path gives a frame rendered at
one size and read at another, the JPEG apart -- with that step's camera angles and action gradient as its labels, in
run-major order; the result feeds ``harness.pretrain_epoch``.

2 envs on the teapot pool, 3 frames per run.  ``eng.step`` is wrapped as in tests/test_gpu_resident_gen.py, and the
bookkeeping of ``dataset_io.generate`` is redone here from what was captured.
"""
import numpy as np
import pytest
import torch

from tests import datapack_model as dm
from tests import resize_model as rm
from tests.test_gpu_resident_gen import capture_steps

pytestmark = pytest.mark.gpu

N, R, S, F = 2, 64, 32, 3


@pytest.fixture(scope="module")
def venv():
    from environment import OcclusionEnv
    from occlusionenv_amd import environment
    from SubProcVecEnv import SimpleVecEnv

    environment.seed_scene_rng(78)
    np.random.seed(78)
    torch.manual_seed(78)
    return SimpleVecEnv([lambda: OcclusionEnv(None, img_size=R) for _ in range(N)])


def expected_store(steps, num_runs, label_mode):
    """The S x S frames in store order from the captured R x R steps, by ``generate``'s rule (see
    tests/test_gpu_resident_gen.py ``expected_store``)."""
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
        assert st["obs"].shape[-1] == R
        model = rm.resize_model(*dm.pack_model(st["obs"], st["alpha"], label_mode), S)
        for i in range(N):
            if live[i] and frame[i] < F and not np.isnan(g[i]).any():
                slot = (first + i) * F + frame[i]
                for dst, src in zip(planes, model):
                    dst[slot] = src[i]
                pos[slot], graw[slot], seen[slot] = (st["el"][i], st["az"][i]), g[i], True
                frame[i] += 1
    assert seen.all()
    return planes, pos, graw


@pytest.mark.parametrize("num_runs,label", [(2, "dither"), (3, "threshold")])
def test_store_holds_the_resized_model_of_every_step(venv, monkeypatch, num_runs, label):
    from occlusionenv_amd import devdata

    steps = capture_steps(venv, monkeypatch)
    ds = devdata.generate_resident(venv, num_runs, num_frames=F, generator=torch.Generator(device="cuda").manual_seed(5), label=label,
                                   size=S)
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
    assert list(ds._staging) == [(N, R)]  # one staging store for all the steps


def test_the_env_size_and_none_give_the_plain_pack(venv, monkeypatch):
    from occlusionenv_amd import devdata

    steps = capture_steps(venv, monkeypatch)
    ds = devdata.generate_resident(venv, N, num_frames=1, generator=torch.Generator(device="cuda").manual_seed(6), size=R)
    assert ds.size == R and not ds._staging
    want = dm.pack_model(steps[0]["obs"], steps[0]["alpha"], dm.LABEL_DITHER)
    for name, g, w in zip(("rgb", "depth", "label"), ds.unpack(0), want):
        assert np.array_equal(g, w[0]), name
    assert devdata.generate_resident(venv, N, num_frames=1).size == R
    with pytest.raises(ValueError):
        devdata.generate_resident(venv, N, num_frames=1, size=0)


def test_one_pretrain_epoch_from_the_resized_store(venv):
    from occlusionenv_amd import devdata, harness
    from occlusionenv_amd.encoder import FrozenEncoder
    from tests import train_model as tm

    ds = devdata.generate_resident(venv, N, num_frames=1, generator=torch.Generator(device="cuda").manual_seed(7), size=S)
    assert ds.size == S and torch.allclose((ds.grad ** 2).sum(1), torch.ones(N, device="cuda"))  # (sin, cos)
    enc = FrozenEncoder.from_state_dict(tm.joint_state_dict("golden"), preset="ppo", dilation=2, residual=True)
    res = harness.pretrain_epoch(enc, ds.loader(batch_size=N, generator=torch.Generator().manual_seed(41)), native_optimizer=True)
    assert res["batches"] == 1 and res["pixels"] == N * S * S and np.isfinite(res["loss"])
