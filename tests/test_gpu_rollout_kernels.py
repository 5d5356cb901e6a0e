"""GPU tests of csrc/occ_rollout.hpp through the C ABI, against tests/rollout_model.py: ``occ_rollout_advance`` bit for bit
and between guard bytes over 12 consecutive steps on the same state, ``occ_ppo_returns`` (scan and normalisation bit for bit,
statistics to the bound of a reordered f64 sum), ``occ_ppo_act`` (a-priori f32 bounds, the sample bit for bit, row
independence), and ``EpisodeMonitor.drain`` with a ring that wraps.

Sizes.  occ_rollout_advance is one block of 1024 lanes in waves of 64: n = 1, 63, 64, 65 and 1025 (the second round of the
block).  occ_ppo_act takes four envs per block: n = 1, 3, 65.  occ_ppo_returns is one block: (T, n) down to M = 2 and up to
more elements than lanes."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import rollout_model as rm

pytestmark = pytest.mark.gpu

GUARD = 256  # bytes on either side of every buffer
STEPS = 12
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    from occlusionenv_amd import _native as nat

    return nat.load()


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


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- occ_rollout_advance ------------------------------------------------------------------------------------------------
def _codes(rng, n, k):
    """Step 3: nobody finishes.  Step 5: every env finishes, codes 1 and 2 mixed.  Otherwise about a quarter, mixed."""
    if k == 3:
        return np.zeros(n, np.int32)
    if k == 5:
        code = rng.integers(1, 3, n).astype(np.int32)
        if n > 1:
            code[0], code[1] = 1, 2
        return code
    code = np.where(rng.random(n) < 0.25, rng.integers(1, 3, n), 0).astype(np.int32)
    if n == 1:
        code[0] = (0, 2, 0, 0, 1, 0, 0, 2, 1, 0, 0, 0)[k]
    return code


def _step_inputs(rng, n, k):
    code = _codes(rng, n, k)
    done = (code == 1).astype(np.uint8)
    if k % 2:
        done[code == 1] = rng.integers(1, 256, int((code == 1).sum()))  # any nonzero byte is a done
    return dict(reward=(rng.normal(size=n) * 3).astype(f32), done=done, code=code)


@pytest.mark.parametrize("n,cap", [(1, 64), (63, 4096), (64, 4096), (65, 4096), (1025, 4096), (63, 8), (1025, 1000)])
def test_advance_against_model(lib, n, cap):
    from occlusionenv_amd import _native as nat

    rng = np.random.default_rng(1000 * n + cap)
    st = rm.new_state(n, cap, rng)
    bufs = dict(rewards=rng.normal(size=(STEPS, n)).astype(f32), dones=rng.normal(size=(STEPS, n)).astype(f32))
    g_st = {k: Guarded(v, rng) for k, v in st.items()}
    g_buf = {k: Guarded(v, rng) for k, v in bufs.items()}
    cst = nat.OccRolloutState()
    for k in rm.STATE_FIELDS:
        setattr(cst, k, g_st[k].ptr.value)
    completed, seen = 0, set()
    for k in range(STEPS):
        inp = _step_inputs(rng, n, k)
        g_in = {key: Guarded(v, rng) for key, v in inp.items()}
        buffered = k != 7  # one step without the buffer: its row keeps its bits
        nat.check(lib.occ_rollout_advance(g_in["reward"].ptr, g_in["done"].ptr, g_in["code"].ptr, n, k if buffered else 0,
                                          STEPS if buffered else 0, (k + 1) * n, g_buf["rewards"].ptr if buffered else None,
                                          g_buf["dones"].ptr if buffered else None, C.byref(cst), cap, _stream()),
                  "occ_rollout_advance")
        torch.cuda.synchronize()
        ents = rm.advance(st, inp["reward"], inp["done"], inp["code"], (k + 1) * n,
                          bufs["rewards"] if buffered else None, bufs["dones"] if buffered else None, k)
        completed += len(ents)
        seen |= {e[4] for e in ents}
        assert len(ents) == (0 if k == 3 else n if k == 5 else len(ents))
        for key, v in st.items():
            _same(f"{key} after step {k}", g_st[key].read(key), v)
        for key, v in bufs.items():
            _same(f"{key} after step {k}", g_buf[key].read(key), v)
        for key, v in inp.items():
            _same(f"{key} of step {k}", g_in[key].read(key), v)
    assert int(st["n_episodes"][0]) == completed and seen == {1, 2}
    if cap < n:
        assert completed > cap  # the ring wrapped, within one launch too (step 5)


def test_advance_rounds_the_products_then_the_sum(lib):
    """Operands for which 0.95f * running + 0.05f * ret differs between two roundings and a fused multiply-add."""
    from occlusionenv_amd import _native as nat

    rng = np.random.default_rng(3)
    found = None
    for _ in range(10000):
        a, b = f32(rng.normal() * 7), f32(rng.normal() * 7)
        two = f32(f32(0.95) * a) + f32(f32(0.05) * b)
        fused = f32(np.float64(f32(0.95)) * np.float64(a) + np.float64(f32(f32(0.05) * b)))
        fused2 = f32(np.float64(f32(f32(0.95) * a)) + np.float64(f32(0.05)) * np.float64(b))
        if two != fused and two != fused2:
            found = (a, b)
            break
    assert found is not None
    st = rm.new_state(1, 4)
    g_st = {k: Guarded(v, rng) for k, v in st.items()}
    cst = nat.OccRolloutState()
    for k in rm.STATE_FIELDS:
        setattr(cst, k, g_st[k].ptr.value)
    for k, r in enumerate(found):
        inp = dict(reward=np.array([r], f32), done=np.zeros(1, np.uint8), code=np.array([2], np.int32))
        g_in = {key: Guarded(v, rng) for key, v in inp.items()}
        nat.check(lib.occ_rollout_advance(g_in["reward"].ptr, g_in["done"].ptr, g_in["code"].ptr, 1, 0, 0, k + 1, None, None,
                                          C.byref(cst), 4, _stream()), "occ_rollout_advance")
        torch.cuda.synchronize()
        rm.advance(st, inp["reward"], inp["done"], inp["code"], k + 1)
    _same("running", g_st["running"].read("running"), st["running"])
    _same("ring_running", g_st["ring_running"].read("ring_running"), st["ring_running"])


def test_monitor_drain_reports_what_the_ring_lost():
    """EpisodeMonitor with 8 ring entries against the model: more than 8 completions between two drains (and in one step)."""
    from occlusionenv_amd.monitor import EpisodeMonitor

    n, cap = 63, 8
    rng = np.random.default_rng(11)
    mon = EpisodeMonitor(n, "cuda", capacity=cap)
    st = rm.new_state(n, cap)
    ents, drained = [], 0
    for k in range(STEPS):
        inp = _step_inputs(rng, n, k)
        if k in (1, 2):  # a quiet stretch: three completions in all between the first two drains
            inp["code"][:] = 0
            inp["code"][k] = k
        inp["done"] = (inp["code"] == 1).astype(np.uint8)
        mon.advance(torch.from_numpy(inp["reward"]).cuda(), torch.from_numpy(inp["code"]).cuda(),
                    torch.from_numpy(inp["done"]).cuda().bool())
        ents += rm.advance(st, inp["reward"], inp["done"], inp["code"], (k + 1) * n)
        if k in (0, 2, 5, STEPS - 1):
            got = mon.drain()
            new = ents[drained:]
            kept = new[-cap:] if new else []
            print("drain after step", k, "new", len(new), "lost", got["lost"])
            assert got["lost"] == len(new) - len(kept)
            assert (k == 2 and got["lost"] == 0 and len(new) == 2) or k != 2
            assert (k == 5 and got["lost"] > 0) or k != 5
            for j, name in enumerate(("episode", "env", "ret", "length", "code", "timestep", "running")):
                want = np.array([e[j] for e in kept], dtype=got[name].dtype)
                _same(f"{name} at drain {k}", got[name], want)
            drained = len(ents)
            assert got["totals"]["episodes"] == len(ents)
    tot = mon.totals()
    assert tot["episodes"] == len(ents) and tot["done"] == int(st["code_counts"][0]) and tot["time_limit"] == int(st["code_counts"][1])
    assert tot["mean_return"] == float(st["sums"][0]) / len(ents) and tot["mean_length"] == float(st["sums"][1]) / len(ents)
    assert np.float32(mon.running_reward) == st["running"][0]
    assert mon.drain()["ret"].shape == (0,)


# ---- occ_ppo_returns ----------------------------------------------------------------------------------------------------
def _run_returns(lib, rewards, dones, gamma, with_raw=True):
    from occlusionenv_amd import _native as nat

    T, n = rewards.shape
    rng = np.random.default_rng(7)
    g = dict(rewards=Guarded(rewards, rng), dones=Guarded(dones, rng), out=Guarded(rng.normal(size=T * n).astype(f32), rng),
             raw=Guarded(rng.normal(size=T * n).astype(f32) if with_raw else None, rng), stats=Guarded(np.full(2, -7.0), rng))
    nat.check(lib.occ_ppo_returns(g["rewards"].ptr, g["dones"].ptr, T, n, gamma, g["out"].ptr, g["raw"].ptr, g["stats"].ptr,
                                  _stream()), "occ_ppo_returns")
    torch.cuda.synchronize()
    _same("rewards", g["rewards"].read("rewards"), rewards)
    _same("dones", g["dones"].read("dones"), dones)
    return g["out"].read("out"), (g["raw"].read("raw") if with_raw else None), g["stats"].read("stats")


@pytest.mark.parametrize("T,n", [(1, 2), (2, 1), (50, 65), (7, 300)])
def test_returns_against_model(lib, T, n):
    rng = np.random.default_rng(100 * T + n)
    M = T * n
    # positive rewards: the sum of the returns is then the sum of their magnitudes, and the bound of a reordered f64 sum,
    # M 2^-53 sum |x|, is a bound RELATIVE to the mean
    rewards = rng.uniform(0.1, 1.0, size=(T, n)).astype(f32)
    dones = (rng.random((T, n)) < 0.1).astype(f32)
    dones[-1, ::3] = 1
    out, raw, stats = _run_returns(lib, rewards, dones, 0.99)
    want_raw = rm.returns(rewards, dones, 0.99)
    _same("scan", raw.reshape(T, n), want_raw)
    ref = rm.return_stats(want_raw)
    rel = np.abs(stats - ref) / np.abs(ref)
    print(f"T {T} n {n}: mean {stats[0]!r} std {stats[1]!r} relative to numpy {rel[0]:.3e} {rel[1]:.3e} bound {M * 2.0 ** -52:.3e}")
    assert (rel <= M * 2.0 ** -52).all()
    _same("normalised", out, rm.normalise(want_raw, stats).reshape(-1))
    out2, _, stats2 = _run_returns(lib, rewards, dones, 0.99, with_raw=False)
    _same("normalised without the raw output", out2, out)
    _same("stats without the raw output", stats2, stats)


def test_returns_with_signed_rewards(lib):
    """Rewards of both signs and dones everywhere / nowhere per env: the scan and the normalisation bit for bit; the mean to
    the reordering bound in its own terms, M 2^-52 mean |x| (a mean near zero has no relative bound)."""
    rng = np.random.default_rng(5)
    T, n = 50, 65
    rewards = rng.normal(size=(T, n)).astype(f32)
    dones = (rng.random((T, n)) < 0.05).astype(f32)
    dones[:, 0], dones[:, 1] = 1, 0
    out, raw, stats = _run_returns(lib, rewards, dones, 0.5)
    want_raw = rm.returns(rewards, dones, 0.5)
    _same("scan", raw.reshape(T, n), want_raw)
    ref = rm.return_stats(want_raw)
    assert abs(stats[0] - ref[0]) <= T * n * 2.0 ** -52 * np.abs(want_raw.astype(np.float64)).mean()
    assert abs(stats[1] - ref[1]) <= T * n * 2.0 ** -52 * ref[1]
    _same("normalised", out, rm.normalise(want_raw, stats).reshape(-1))


# ---- occ_ppo_act --------------------------------------------------------------------------------------------------------
def _run_act(lib, feats, w, b, noise, std, T=0, t=0, with_mean=True):
    from occlusionenv_amd import _native as nat

    n = feats.shape[0]
    rng = np.random.default_rng(9)
    junk = lambda *shape: rng.normal(size=shape).astype(f32)  # noqa: E731
    g = dict(feats=Guarded(feats, rng), w=Guarded(w, rng), b=Guarded(b, rng), noise=Guarded(noise, rng),
             action=Guarded(junk(n, 2), rng), logprob=Guarded(junk(n), rng), mean=Guarded(junk(n, 2) if with_mean else None, rng),
             feat_buf=Guarded(junk(T, n, 256) if T else None, rng), action_buf=Guarded(junk(T, n, 2) if T else None, rng),
             logprob_buf=Guarded(junk(T, n) if T else None, rng))
    nat.check(lib.occ_ppo_act(g["feats"].ptr, g["w"].ptr, g["b"].ptr, g["noise"].ptr, std, n, g["action"].ptr, g["logprob"].ptr,
                              g["mean"].ptr, g["feat_buf"].ptr, g["action_buf"].ptr, g["logprob_buf"].ptr, t, T, _stream()),
              "occ_ppo_act")
    torch.cuda.synchronize()
    for k, v in (("feats", feats), ("w", w), ("b", b), ("noise", noise)):
        _same(k, g[k].read(k), v)
    return {k: (g[k].read(k), g[k].arr) for k in g if g[k].arr is not None and k not in ("feats", "w", "b", "noise")}


def _act_case(n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.normal(size=(n, 256)) * 2).astype(f32), (rng.normal(size=(2, 256)) * 0.1).astype(f32),
            rng.normal(size=2).astype(f32), rng.normal(size=(n, 2)).astype(f32))


@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("std", [0.6, 0.4])  # at 0.4 the log-probability's constant is nearly zero
def test_act_against_model(lib, n, std):
    feats, w, b, noise = _act_case(n, 10 * n + int(10 * std))
    T, t = 3, 1
    res = _run_act(lib, feats, w, b, noise, std, T=T, t=t)
    mean, action, logprob = res["mean"][0], res["action"][0], res["logprob"][0]
    mean64, mag = rm.act_mean64(feats, w, b)
    err = np.abs(mean.astype(np.float64) - mean64)
    print(f"n {n} std {std}: mean error / bound {float((err / (258 * 2.0 ** -24 * mag)).max()):.3f}")
    assert (err <= 258 * 2.0 ** -24 * mag).all()
    _same("action", action, rm.act_action(mean, noise, std))
    lp64, quad, const = rm.act_logprob64(action, mean, std)
    lp_err = np.abs(logprob.astype(np.float64) - lp64)
    print(f"n {n} std {std}: logprob error / bound {float((lp_err / (8 * 2.0 ** -24 * (quad + abs(const)))).max()):.3f}")
    assert (lp_err <= 8 * 2.0 ** -24 * (quad + abs(const))).all()
    # row t of the buffers: the feature row, the action, the log-probability; the other rows keep their bits
    for key, val in (("feat_buf", feats), ("action_buf", action), ("logprob_buf", logprob)):
        want = res[key][1].copy()
        want[t] = val
        _same(key, res[key][0], want)


def test_act_rows_do_not_depend_on_the_batch(lib):
    feats, w, b, noise = _act_case(65, 77)
    full = _run_act(lib, feats, w, b, noise, 0.6)
    nomean = _run_act(lib, feats, w, b, noise, 0.6, with_mean=False)
    for k in ("action", "logprob"):
        _same(f"{k} without the mean output", nomean[k][0], full[k][0])
    for e in (0, 1, 3, 4, 62, 63, 64):
        one = _run_act(lib, feats[e:e + 1], w, b, noise[e:e + 1], 0.6)
        for k in ("mean", "action", "logprob"):
            _same(f"{k} of row {e}", one[k][0][0], full[k][0][e])
