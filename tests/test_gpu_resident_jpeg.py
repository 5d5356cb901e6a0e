"""GPU test of ``devdata.generate_resident(jpeg=)`` with the engine, against the files: the captured engine steps are
written through ``dataset_io.RunWriter(jpeg_quality=)``, one run directory per env, and read back with
``devdata.DeviceDataset.from_directory``; every byte of every plane of every frame of the device store, colours included,
and the labels equal what the files give -- at the env's size, and rendered at 32 and stored at 16
(``put(resize=True, jpeg=)``).  ``jpeg=None`` is still tests/test_gpu_resident_gen.py's expectation, and the JPEG store
feeds ``harness.pretrain_epoch``.

2 envs of 32 x 32 on the teapot pool, 3 frames per run.  ``eng.step`` is wrapped as in tests/test_gpu_resident_gen.py.

The scene of the comparison with the files is pinned (``pin_scene``).  ``SimpleVecEnv.reset`` draws its azimuths from a
fresh unseeded generator, as the reference does, so no seed fixes the view, and some views put the far teapot at a view depth
of 5 or more.  There the writer's ``(depth * 51).astype(np.uint8)`` is outside the cast's range: the files hold whatever
numpy's cast leaves (it wraps on x86: 306 becomes 50), the store holds 255 by ``occ_dataset_pack``'s rule
(include/occlusionenv_amd.h), and the depth planes differ at those pixels whatever the JPEG does to the colours.  With the
azimuth at 0 the depth stays near 4; the test asserts that it is inside the cast's range before it compares.
"""
import numpy as np
import pytest
import torch

from tests import datapack_model as dm
from tests.test_gpu_resident_gen import expected_store

pytestmark = pytest.mark.gpu

N, S, F = 2, 32, 3


@pytest.fixture(scope="module")
def venv():
    from environment import OcclusionEnv
    from occlusionenv_amd import environment
    from SubProcVecEnv import SimpleVecEnv

    environment.seed_scene_rng(79)
    np.random.seed(79)
    torch.manual_seed(79)
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


def pin_scene(venv, monkeypatch, seed=79):
    """``venv.reset`` with the azimuths at 0 instead of a draw from an unseeded generator, and the scene draws reseeded:
    every ``generate_resident`` under it renders the same scene from the same view, on every run."""
    from occlusionenv_amd import environment

    def reset():
        np.random.seed(seed)
        environment.seed_scene_rng(seed)
        obs = venv._reset_envs(list(range(N)), [0.0] * N)
        if venv.engine.R:
            venv._warm_reserve()
        return obs

    monkeypatch.setattr(venv, "reset", reset)


def write_files(steps, root, quality):
    """``dataset_io.generate``'s bookkeeping on the captured steps of one round of N runs: a frame per finite gradient, in
    step order, until a run has F of them."""
    from occlusionenv_amd import dataset_io

    writers = [dataset_io.RunWriter(str(root), i, jpeg_quality=quality) for i in range(N)]
    frame = np.zeros(N, np.int64)
    for st in steps:
        g = st["action"].grad.detach().cpu().numpy()
        for i in range(N):
            if frame[i] < F and not np.isnan(g[i]).any():
                writers[i].write_frame(int(frame[i]), st["obs"][i], st["alpha"][i], float(st["el"][i]), float(st["az"][i]), g[i])
                frame[i] += 1
    assert (frame == F).all()
    for w in writers:
        w.close()


@pytest.mark.parametrize("size", [None, 16])
def test_store_equals_the_files_colours_included(venv, monkeypatch, tmp_path, size):
    from occlusionenv_amd import devdata

    pin_scene(venv, monkeypatch)
    steps = capture_steps(venv, monkeypatch)
    ds = devdata.generate_resident(venv, N, num_frames=F, generator=torch.Generator(device="cuda").manual_seed(5), jpeg=75, size=size)
    depth = np.stack([st["obs"][:, 3] for st in steps])
    assert (depth != -1).mean() > 0.1 and float(depth.max()) * 51 < 255, "the pinned view keeps the depth inside the writer's cast"
    T = S if size is None else size
    assert len(ds) == N * F and ds.size == T and ds.device.type == "cuda"
    write_files(steps, tmp_path, 75)
    ref = devdata.DeviceDataset.from_directory(str(tmp_path), "", (T, T), device="cpu")
    assert len(ref) == N * F
    for f in range(N * F):
        for name, g, w in zip(("rgb", "depth", "label"), ds.unpack(f), ref.unpack(f)):
            assert g.dtype == w.dtype and np.array_equal(g, w), (f, name)
    assert torch.equal(ds.rgbl.cpu(), ref.rgbl) and torch.equal(ds.depth.cpu(), ref.depth)
    assert np.array_equal(ds.pos.cpu().numpy().view(np.uint32), ref.pos.numpy().view(np.uint32))
    assert np.array_equal(ds.grad.cpu().numpy().view(np.uint32), ref.grad.numpy().view(np.uint32))
    rgb = np.stack([ds.unpack(f)[0] for f in range(N * F)])
    assert rgb.any() and len(np.unique(rgb)) > 16  # the scenes are there, with the JPEG's ringing around their flat colours
    if size is None:  # and the JPEG is what made the difference
        plain = dm.pack_model(steps[0]["obs"], steps[0]["alpha"], dm.LABEL_DITHER)[0]
        assert not np.array_equal(rgb[0], plain[0]) or not np.array_equal(rgb[F], plain[1])


def test_without_jpeg_nothing_changes(venv, monkeypatch):
    from occlusionenv_amd import devdata

    steps = capture_steps(venv, monkeypatch)
    ds = devdata.generate_resident(venv, N, num_frames=F, generator=torch.Generator(device="cuda").manual_seed(5), jpeg=None)
    planes, pos, graw = expected_store(steps, N, dm.LABEL_DITHER)
    for f in range(N * F):
        for name, g, w in zip(("rgb", "depth", "label"), ds.unpack(f), planes):
            assert g.dtype == w.dtype and np.array_equal(g, w[f]), (f, name)
    assert np.array_equal(ds.pos.cpu().numpy().view(np.uint32), pos.view(np.uint32))
    assert np.array_equal(ds.grad.cpu().numpy().view(np.uint32), devdata.sincos_grad(graw).view(np.uint32))


def test_one_pretrain_epoch_from_the_jpeg_store(venv):
    from occlusionenv_amd import devdata, harness
    from occlusionenv_amd.encoder import FrozenEncoder
    from tests import train_model as tm

    ds = devdata.generate_resident(venv, N, num_frames=1, generator=torch.Generator(device="cuda").manual_seed(7), jpeg=75)
    enc = FrozenEncoder.from_state_dict(tm.joint_state_dict("golden"), preset="ppo", dilation=2, residual=True)
    res = harness.pretrain_epoch(enc, ds.loader(batch_size=N, generator=torch.Generator().manual_seed(41)), native_optimizer=True)
    assert res["batches"] == 1 and res["pixels"] == N * S * S and np.isfinite(res["loss"])
