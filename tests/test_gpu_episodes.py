"""GPU tests of the batched controller evaluation (occlusionenv_amd/episodes.py, csrc/occ_episode.hpp): the kernel against
tests/episode_model.py through the C ABI, bit for bit and between guard words; the loop against host-synchronous oracles
written here, which run the reference's loops (test.py:92-255) one env at a time on a single-env engine with ``.item()`` on
every step; every ``poll_every``; what a frozen env keeps; shared scenes; and the venv afterwards.

Sizes.  The kernel is one block of up to 1024 lanes, a wave is 64: n = 1, 63, 64, 65 and 200 (four waves, the last partial).
The loops run N = 6 envs at 64^2 for at most MAX_STEP = 12 steps."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import episode_model as em

pytestmark = pytest.mark.gpu

GUARD = 256  # bytes on either side of every buffer
N, S, MAX_STEP, SEED = 6, 64, 12, 77
AZ = np.linspace(-0.3, 0.3, N).astype(np.float32)


@pytest.fixture(scope="module")
def lib():
    from occlusionenv_amd import _native as nat

    return nat.load()


# ---- 1. the kernel against the model --------------------------------------------------------------------------------
class Guarded:
    """A device buffer holding ``arr`` (or nothing: a null pointer) between GUARD bytes of seeded random bits."""

    def __init__(self, arr, rng):
        self.arr = None if arr is None else np.ascontiguousarray(arr)
        if arr is None:
            self.ptr = None
            return
        raw = rng.integers(0, 256, 2 * GUARD + self.arr.nbytes, dtype=np.uint8)
        raw[GUARD:GUARD + self.arr.nbytes] = self.arr.view(np.uint8).reshape(-1)
        self.before = raw.copy()
        self.dev = torch.from_numpy(raw).cuda()
        self.ptr = C.c_void_p(self.dev.data_ptr() + GUARD)

    def read(self, name):
        after = self.dev.cpu().numpy()
        nb = self.arr.nbytes
        assert np.array_equal(after[:GUARD], self.before[:GUARD]), f"guard in front of {name} was written"
        assert np.array_equal(after[GUARD + nb:], self.before[GUARD + nb:]), f"guard behind {name} was written"
        return after[GUARD:GUARD + nb].view(self.arr.dtype).reshape(self.arr.shape)


def _same(name, got, want):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, name
    bad = g.view(np.uint8) != w.view(np.uint8)
    assert not bad.any(), f"{name}: {int(bad.sum())} bytes differ, first at {tuple(np.argwhere(bad)[0])}"


def _kernel_case(n, seed):
    """Seeded inputs: a third of the rows frozen (with their inputs NaN), NaN gradients, done flags, a state already in use."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    st = em.new_state(n, MAX_STEP, action=rng.normal(size=(n, 2)))
    frozen = rng.random(n) < 0.35
    frozen[0] = False
    if n > 1:
        frozen[1] = True
    st["active"][frozen], st["skip"][frozen] = 0, 1
    st["iterations"][frozen] = rng.integers(1, MAX_STEP, int(frozen.sum()))
    st["finished"][frozen] = rng.integers(0, 2, int(frozen.sum()))
    st["nan_steps"][:] = rng.integers(0, 3, n)
    st["rewards"][:4] = rng.normal(size=(4, n))
    st["full_rewards"][:4] = rng.normal(size=(4, n))
    inp = dict(done=(rng.random(n) < 0.3).astype(np.uint8), reward=rng.normal(size=n).astype(f32),
               full_reward=rng.random(n).astype(f32), grad=rng.normal(size=(n, 2)).astype(f32),
               pred=rng.normal(size=(n, 2)).astype(f32), noise=rng.normal(size=(n, 2)).astype(f32))
    inp["grad"][rng.random(n) < 0.25, rng.integers(0, 2)] = np.nan
    for k in ("reward", "full_reward", "grad", "pred", "noise"):  # a skipped row's outputs of the step are undefined
        inp[k][frozen] = np.nan
    inp["done"][frozen] = 1
    return st, inp


def _check_kernel(lib, st, inp, rule, lr, step, what):
    """One occ_episode_advance on guarded copies of ``st`` and ``inp`` against the model, which updates ``st``.  -> report[0]."""
    from occlusionenv_amd import _native as nat

    n = st["active"].shape[0]
    rng = np.random.default_rng(5)
    g_in = {k: Guarded(v, rng) for k, v in inp.items()}
    g_st = {k: Guarded(v, rng) for k, v in st.items()}
    g_tr = [g_st.get("rewards", Guarded(None, rng)), g_st.get("full_rewards", Guarded(None, rng))]
    g_rep = Guarded(np.full(1, -7, np.int32), rng)
    nat.check(lib.occ_episode_advance(g_in["done"].ptr, g_in["reward"].ptr, g_in["full_reward"].ptr, g_in["grad"].ptr,
                                      g_in["pred"].ptr, g_in["noise"].ptr, rule, lr, step, MAX_STEP, n,
                                      *(g_st[k].ptr for k in em.FIELDS), g_tr[0].ptr, g_tr[1].ptr, g_rep.ptr,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)), "occ_episode_advance")
    torch.cuda.synchronize()
    left = em.advance(st, rule, lr, step, MAX_STEP, **inp)
    for k, v in st.items():
        _same(f"{k} ({what})", g_st[k].read(k), v)
    for k, v in inp.items():
        _same(f"{k} ({what})", g_in[k].read(k), v)
    assert int(g_rep.read("report")[0]) == left
    return left


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_kernel_against_model(lib, n):
    for rule in (em.GRADIENT, em.RANDOM, em.MODEL, em.AGENT):
        for step in (4, MAX_STEP - 1):
            for traced in (True, False):
                st, inp = _kernel_case(n, 100 * n + 10 * rule + step)
                if not traced:
                    del st["rewards"], st["full_rewards"]
                left = _check_kernel(lib, st, inp, rule, 0.3, step, f"n {n} rule {rule} step {step}")
                assert left == 0 if step == MAX_STEP - 1 else (0 < left < n or n == 1)


def test_kernel_rounds_the_product_then_the_sum(lib):
    """The operands of tests/test_episode_model.py for which a fused multiply-add gives another answer."""
    lr = np.float32(1 + 2.0 ** -12)
    for rule in (em.GRADIENT, em.RANDOM):
        st, inp = _kernel_case(3, 1)
        st["active"][:], st["skip"][:] = 1, 0
        st["action"][:] = -1
        inp["grad"][:] = inp["noise"][:] = lr
        _check_kernel(lib, st, inp, rule, float(lr), 0, f"rule {rule}")
        assert (st["action"] == np.float32(2.0 ** -11)).all()


# ---- the loops ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ds():
    from occlusionenv_amd.meshes import SyntheticShapeNet

    return SyntheticShapeNet(n_models=8, seed=1234)


def _venv(ds, n=N):
    from environment import OcclusionEnv
    from SubProcVecEnv import SimpleVecEnv

    return SimpleVecEnv([lambda: OcclusionEnv(ds, img_size=S) for _ in range(n)])


@pytest.fixture(scope="module")
def venv(ds):
    return _venv(ds)


@pytest.fixture(scope="module")
def nets():
    """A random-weight separable dilation-2 FullNetwork checkpoint, as tests/test_gpu_encoder.py builds it, and the agent on it."""
    import os

    from occlusionenv_amd import ppo
    from occlusionenv_amd.encoder import FrozenEncoder
    from tests.encoder_model import golden_state_dict

    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_golden.npz"))
    sd = golden_state_dict(golden, "ppo")
    enc = FrozenEncoder.from_state_dict(sd, preset="ppo")
    assert enc.separable and enc.dilation == 2
    return enc, ppo.BatchedPPO.from_fullnetwork(sd, seed=0)


def _evaluate(venv, controllers, gen_device="cpu", **kw):
    """evaluate_controllers on the same scene draws every time.  -> (results, the engine's state right afterwards)."""
    from occlusionenv_amd import environment, harness

    environment.seed_scene_rng(SEED)
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    kw.setdefault("azimuth", AZ)
    kw.setdefault("max_step", MAX_STEP)
    # venv.reset() accepts a scene by its loss at an azimuth it draws: seeded too, or two calls would not keep the same scenes
    environment.seed_reset_rng(SEED)
    try:
        res = harness.evaluate_controllers(venv, controllers, generator=torch.Generator(device=gen_device).manual_seed(5), **kw)
    finally:
        environment.seed_reset_rng(None)
    eng = venv.engine
    state = {k: getattr(eng, k).clone() for k in ("elevation", "azimuth", "camera_position", "full_reward", "object_mass")}
    return res, state


def _children(k, gen_device="cpu"):
    from occlusionenv_amd import harness

    return harness.controller_generators(torch.Generator(device=gen_device).manual_seed(5), k)


def _oracle(venv, kind, lr, gen, azimuth=AZ, max_step=MAX_STEP, enc=None, agent=None):
    """The reference's loop, one env at a time on a single-env engine, a host sync on every step.  Noise: the draws of the
    batched loop (one (N,2) draw per step from the controller's generator), of which env e uses row e."""
    from occlusionenv_amd.engine import OcclusionEngine

    big = venv.engine
    n = big.N
    mesh, off = big.scene_mesh.cpu(), big.scene_offset.cpu()
    f32 = np.float32
    first = np.zeros((n, 2), f32)
    draws = []
    if kind == "random":
        first = torch.randn(n, 2, generator=gen).numpy()
        draws = [torch.randn(n, 2, generator=gen).numpy() for _ in range(max_step)]
    elif kind == "rl":
        draws = [torch.randn((n, 2), device="cuda", dtype=torch.float32, generator=gen) for _ in range(max_step)]
    out = dict(iterations=np.zeros(n, np.int64), finished=np.zeros(n, bool), final_action=np.zeros((n, 2), f32),
               nan_steps=np.zeros(n, np.int32), rewards=np.full((max_step, n), np.nan, f32),
               full_rewards=np.full((max_step, n), np.nan, f32), state={})
    for e in range(n):
        eng = OcclusionEngine(big.pool, 1, S)
        eng.set_scene([0], mesh[e:e + 1], off[e:e + 1])
        eng.reset_render(azimuth=float(azimuth[e]), elevation=0.0, radius=4.0)
        action = first[e].copy()
        for i in range(max_step):
            a = torch.from_numpy(action.reshape(1, 2)).cuda().requires_grad_(kind == "raw")
            obs, reward, done, _fs, loss = eng.step(a)
            if kind == "raw":
                reward.sum().backward()
                g = a.grad.cpu().numpy()[0]
                if np.isnan(g).any():
                    out["nan_steps"][e] += 1
                    if i == max_step - 1:
                        out["iterations"][e] = i + 1  # the documented deviation: the cap holds on a NaN step as well
                    continue
                action = action + f32(lr) * g
            elif kind == "random":
                action = action + f32(lr) * draws[i][e]
            elif kind == "model":
                action = f32(-lr) * enc.predict_grad(obs).cpu().numpy()[0]
            else:
                pol = agent.policy_old
                action = (pol.action_head(agent.features(obs)) + draws[i][e:e + 1] * pol.action_var.sqrt()).detach().cpu().numpy()[0]
            out["rewards"][i, e], out["full_rewards"][i, e] = reward.item(), loss.item()
            if done.item():
                out["iterations"][e], out["finished"][e] = i + 1, True
                break
            elif i >= max_step - 1:
                out["iterations"][e] = i + 1
        out["final_action"][e] = action
        out["state"][e] = {k: getattr(eng, k).cpu().numpy()[0] for k in ("elevation", "azimuth", "camera_position", "full_reward", "object_mass")}
        eng.check_status()
    return out


def _against_oracle(name, got, want):
    print(name, "iterations", got["iterations"].tolist(), "finished", got["finished"].tolist(), "nan", got["nan_steps"].tolist(),
          "polls", got["polls"], "compactions", got["compactions"])
    assert got["iterations"].dtype == torch.int64 and got["finished"].dtype == torch.bool
    for k in ("iterations", "finished", "nan_steps", "final_action", "rewards", "full_rewards"):
        _same(f"{name} {k}", got[k].cpu().numpy(), want[k])


@pytest.fixture(scope="module")
def walked(venv):
    """The random walk, then the raw gradient (whose end state the engine is left in), with traces."""
    from occlusionenv_amd import harness

    res, state = _evaluate(venv, [harness.RandomWalk(lr=1.0), harness.GradientAscent(lr=1.0)], trace=True)
    g_random, g_raw = _children(2)
    return res, state, dict(random=_oracle(venv, "random", 1.0, g_random), raw=_oracle(venv, "raw", 1.0, g_raw))


def test_loop_against_host_synchronous_oracle(walked):
    res, _state, want = walked
    assert list(res) == ["random", "raw"]
    for name in res:
        _against_oracle(name, res[name], want[name])
    it = torch.cat([res[k]["iterations"] for k in res])
    fin = torch.cat([res[k]["finished"] for k in res])
    assert bool((fin & (it < MAX_STEP)).any()), "no env finished before the cap"
    assert bool((~fin & (it == MAX_STEP)).any()), "no env reached the cap"
    assert res["raw"]["frozen_row_steps"] == res["raw"]["row_steps"] - int(res["raw"]["iterations"].sum())


def test_frozen_envs_keep_their_state(walked):
    """The engine's state after the run is, row for row, the state of the single-env engine at the end of ITS episode:
    the steps the others took after an env froze changed none of its bits."""
    res, state, want = walked
    early = res["raw"]["iterations"] < MAX_STEP
    assert bool(early.any())
    for k, v in state.items():
        _same(k, v.cpu().numpy(), np.stack([want["raw"]["state"][e][k] for e in range(N)]))


def test_predicted_gradient_and_agent_against_oracle(venv, nets):
    from occlusionenv_amd import harness

    enc, agent = nets
    res, _ = _evaluate(venv, [harness.PredictedGradient(enc, step_lr=0.01), harness.Agent(agent)], gen_device="cuda", trace=True)
    g_model, g_rl = _children(2, "cuda")
    _against_oracle("model", res["model"], _oracle(venv, "model", 0.01, g_model, enc=enc))
    _against_oracle("rl", res["rl"], _oracle(venv, "rl", 0.0, g_rl, agent=agent))


def test_every_poll_interval_gives_the_same_bits(venv, nets):
    from occlusionenv_amd import harness

    enc, agent = nets
    ctrls = [harness.GradientAscent(), harness.RandomWalk(), harness.PredictedGradient(enc), harness.Agent(agent)]
    runs = {p: _evaluate(venv, ctrls, gen_device="cuda", trace=True, poll_every=p)[0] for p in (1, 4, 10 ** 9)}
    for p, res in runs.items():
        print(p, {k: (v["steps"], v["polls"], v["compactions"], v["iterations"].tolist()) for k, v in res.items()})
    base = runs[10 ** 9]
    assert all(v["polls"] == 0 and v["compactions"] == 0 and v["steps"] == MAX_STEP for v in base.values())
    for p in (1, 4):
        for name in base:
            for k in ("iterations", "finished", "nan_steps", "final_action", "rewards", "full_rewards", "initial_loss"):
                _same(f"poll_every {p} {name} {k}", runs[p][name][k].cpu().numpy(), base[name][k].cpu().numpy())
    assert sum(v["compactions"] for v in runs[1].values()) >= 1, "poll_every = 1 never went on with a subset"
    assert all(v["polls"] >= 1 for v in runs[1].values())


def test_same_scenes_and_azimuths(venv, nets):
    from occlusionenv_amd import harness

    enc, agent = nets
    ctrls = [harness.GradientAscent(), harness.RandomWalk(), harness.PredictedGradient(enc), harness.Agent(agent)]
    az = np.array([0.1] * 3 + [-0.2] * 3, np.float32)
    res, _ = _evaluate(venv, ctrls, gen_device="cuda", trace=True, azimuth=az, scene_of=[0] * 3 + [1] * 3)
    # every controller starts from the same render; those that start from a zero action also see the same first step
    for name in ("random", "model", "rl"):
        _same(f"{name} initial loss", res[name]["initial_loss"].cpu().numpy(), res["raw"]["initial_loss"].cpu().numpy())
    for name in ("model", "rl"):
        _same(f"{name} first step", res[name]["full_rewards"][0].cpu().numpy(), res["raw"]["full_rewards"][0].cpu().numpy())
    raw = res["raw"]
    for grp in ([0, 1, 2], [3, 4, 5]):
        for k in ("iterations", "finished", "nan_steps", "final_action", "initial_loss"):
            v = raw[k].cpu().numpy()
            for e in grp[1:]:
                _same(f"{k} of env {e}", v[e], v[grp[0]])
        for k in ("rewards", "full_rewards"):
            v = raw[k].cpu().numpy()
            for e in grp[1:]:
                _same(f"{k} of env {e}", v[:, e], v[:, grp[0]])
    assert not np.array_equal(raw["initial_loss"].cpu().numpy()[0], raw["initial_loss"].cpu().numpy()[3])


def test_default_azimuths_follow_the_scenes(venv):
    """azimuth=None with scene_of: the envs of a group start at the azimuth their scene was drawn with, so they agree."""
    from occlusionenv_amd import harness

    res, _ = _evaluate(venv, [harness.GradientAscent()], azimuth=None, scene_of=[0] * 3 + [1] * 3, max_step=3)
    loss = res["raw"]["initial_loss"].cpu().numpy()
    for grp in ([0, 1, 2], [3, 4, 5]):
        for e in grp[1:]:
            _same(f"initial loss of env {e}", loss[e], loss[grp[0]])


def test_a_subset_step_reads_nothing_back(venv):
    """A step on a compact subset whose indices the caller also holds on the host (what the loop does after a compaction)
    makes no synchronising call; without the host copy the engine copies the indices back, which the same mode catches."""
    eng = venv.engine
    venv.reset()
    venv._drain()
    ids = np.array([1, 3, 4])
    rows = torch.as_tensor(ids, device="cuda")
    skip = torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda")
    a = torch.zeros(3, 2, device="cuda")
    eng.step(a, env_ids=rows, skip=skip, env_ids_host=ids)  # the workspace exists from here on
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eng.step(a, env_ids=rows, skip=skip, env_ids_host=ids)
        with pytest.raises(RuntimeError):
            eng.step(a, env_ids=rows, skip=skip)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    eng.check_status()


def test_venv_steps_again_after_a_reset(ds):
    """16 envs: the venv has a reserve, and a step's report is pending when the evaluation starts."""
    from occlusionenv_amd import harness

    venv = _venv(ds, 16)
    assert venv.engine.R > 0
    venv.reset()
    venv.step(torch.zeros(16, 2, device="cuda"))
    res = harness.evaluate_controllers(venv, [harness.GradientAscent()], max_step=3, poll_every=2)
    assert res["raw"]["iterations"].shape == (16,) and int(res["raw"]["iterations"].max()) <= 3
    obs = venv.reset()
    assert obs.shape == (16, 1, 4, S, S)
    obs, rewards, dones, infos = venv.step(torch.zeros(16, 2, device="cuda"))
    assert obs.shape[0] == 16 and rewards.shape == (16,) and bool(torch.isfinite(rewards).all())
    assert infos[0]["full_state"].shape == (1, S, S, 4)
    venv._drain()
    venv.engine.check_status()
