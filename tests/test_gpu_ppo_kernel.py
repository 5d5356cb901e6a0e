"""``occ_ppo_update`` (csrc/occ_ppo.hpp) through the C ABI against the float64 host model of its epoch
(tests/ppo_model.py), at the sample counts where its grid changes: ceil(M / 128) blocks up to M = 8 192, 64 from there
(the single-GPU learner, 12 800 samples), OCC_PPO_MAX_BLOCKS = 128 from M = 65 536 on (the replicated 8-GPU learner,
102 400).  Every block writes a row of partial sums to the scratch; the last block to bump the counter adds the rows in
block order and takes the Adam step.  A stale, dropped or doubled row shifts a gradient component by about 1 / blocks of
its scale, so the gradient is checked component by component against the model's, relative to the scale
S_k = sum_i |contribution_ik| of its f32 sum (worst case ~200 * 2^-24 at this depth; the bound is 1e-5).

The old log-probabilities are set from the model's log-probabilities so that the ratios fall on chosen targets over
(0.5, 1.6), and every sample keeps a distance of at least MARGIN from the clip bounds at every epoch checked (asserted in
the model): the f32 kernel then cannot legitimately take another branch of the clipped surrogate than the model."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import ppo_model as PM

pytestmark = pytest.mark.gpu

HYPER = dict(action_var=PM.f32(0.6 * 0.6), eps_clip=PM.f32(0.2), lr_actor=PM.f32(3e-4), lr_critic=PM.f32(1e-3),
             beta1=PM.f32(0.9), beta2=PM.f32(0.999), adam_eps=PM.f32(1e-8))  # trainRL.py's, as the kernel reads them
# 20 calls from zeroed moments move every actor parameter by up to 20 lr: a smaller actor rate keeps the ratio targets
# feasible (the gradient check does not depend on it)
HYPER_SLOW = dict(HYPER, lr_actor=PM.f32(1e-5))
LO, HI = 1.0 - HYPER["eps_clip"], 1.0 + HYPER["eps_clip"]
MARGIN = 1e-3    # asserted distance of every ratio from the clip bounds
GRAD_TOL = 1e-5  # |g_k - g64_k| <= GRAD_TOL * S_k
HEADS_GRAD_ERR = 1e-6  # the gradient error the 5-epoch heads check allows for (2.4 x the sweep's worst, 4.2e-7)
SWEEP = [1, 2, 15, 16, 17, 127, 128, 129, 2560, 8064, 8192, 8193, 12800, 65535, 65536, 102400, 131075]
WORST = {}       # worst |err| / S per sample count (printed with -s)


@pytest.fixture(scope="module")
def lib():
    from occlusionenv_amd import _native as nat

    return nat.load()


def grid(lib, M):
    """The block count occ_ppo_update launches for M samples (csrc/occ_kernels.hip)."""
    mb = int(lib.occ_ppo_max_blocks())
    cap = mb if M >= 65536 else min(mb, 64)
    return max(1, min(-(-M // 128), cap))


# ---- data ----------------------------------------------------------------------------------------------------------

def step_bound(t):
    """The largest Adam step of one parameter at step t, in units of lr, whatever the gradients: by Cauchy-Schwarz on
    m_t, |m_t| / sqrt(v_t) <= (1 - b1) / sqrt(1 - b2) * sqrt(sum_{j<t} (b1^2 / b2)^j), and the step is
    lr * sqrt(1 - b2^t) / (1 - b1^t) * m_t / (sqrt(v_t) + ...).  1 at t = 1."""
    b1, b2 = HYPER["beta1"], HYPER["beta2"]
    return (np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * (1 - b1) / np.sqrt(1 - b2)
            * np.sqrt(sum((b1 * b1 / b2) ** j for j in range(t))))


def make_set(M, seed, theta, moved=0.0, feat_scale=1.0, ret_sign=1.0, ret_scale=1.0):
    """One f32 buffer: non-negative features (pooled observations, in [0, feat_scale)), actions drawn around the heads'
    means, returns of the given sign and scale (offset from zero: both signs of the advantage occur), and old
    log-probabilities that put the ratios on targets over (0.5, 1.6).  ``moved`` bounds how far any actor parameter moves
    from ``theta`` over the epochs the set is checked at; the targets are chosen so that every ratio stays 2 * MARGIN
    clear of the clip bounds along ANY such path (so not only along the model's)."""
    rng = np.random.default_rng(seed)
    feats = (feat_scale * rng.random((M, PM.FEAT))).astype(np.float32)
    F = feats.astype(np.float64)
    var = HYPER["action_var"]
    mean = PM.forward(theta, F, np.zeros((M, 2)), np.zeros(M), var)[0]
    actions = (mean + 0.6 * rng.standard_normal((M, 2))).astype(np.float32)
    returns = (ret_sign * ret_scale * (rng.standard_normal(M) + 0.3)).astype(np.float32)
    lp0 = PM.forward(theta, F, actions, np.zeros(M), var)[2]
    # |lp - lp0| <= B: each mean moves by at most dm = moved * (sum_k f_k + 1)
    dm = moved * (F.sum(1) + 1.0)
    B = (np.abs(actions - mean).sum(1) * dm + dm * dm) / var
    cand = rng.uniform(0.5, 1.6, (M, 64))
    lo_r, hi_r = cand * np.exp(-B)[:, None], cand * np.exp(B)[:, None]
    ok = np.ones(cand.shape, bool)
    for b in (LO, HI):
        ok &= (hi_r <= b - 2 * MARGIN) | (lo_r >= b + 2 * MARGIN)
    target = np.where(ok.any(1), cand[np.arange(M), ok.argmax(1)], 0.5 * LO * np.exp(-B))
    old_lp = (lp0 - np.log(target)).astype(np.float32)
    return dict(M=M, feats=feats, F=F, actions=actions, returns=returns, old_lp=old_lp)


def assert_margin(o, M):
    """The model's branch is the one an f32 kernel must take: every ratio MARGIN clear of the bounds; from M = 128 on all
    four ways of leaving the clip range occur (below / above, either sign of the advantage)."""
    assert float(o["margin"].min()) >= MARGIN, float(o["margin"].min())
    if M >= 128:
        r, a = o["ratio"], o["adv"]
        for side in (r < LO, r > HI):
            assert (side & (a > 0)).any() and (side & (a < 0)).any()


# ---- the kernel ----------------------------------------------------------------------------------------------------

class Learner:
    """Device state of one occ_ppo_update caller: the four heads (separate, 16-byte aligned tensors, as BatchedPPO's),
    Adam moments and step, scratch sized by the library's block cap, the arrival counter."""

    def __init__(self, lib):
        from occlusionenv_amd import _native as nat

        self.lib, self.nat = lib, nat
        f32 = dict(dtype=torch.float32, device="cuda")
        self.heads = [torch.zeros(n, **f32) for n in (2 * PM.FEAT, 2, PM.FEAT, 1)]
        self.m, self.v, self.step = torch.zeros(PM.PARAMS, **f32), torch.zeros(PM.PARAMS, **f32), torch.zeros(1, **f32)
        self.scratch = torch.zeros(nat.ppo_scratch_floats(), **f32)
        self.counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.ps = nat.OccPpoState()
        for name, t in zip(("w_a", "b_a", "w_v", "b_v", "adam_m", "adam_v", "adam_step"), self.heads + [self.m, self.v, self.step]):
            setattr(self.ps, name, t.data_ptr())

    def load(self, theta, m=None, v=None, step=0.0):
        t = torch.from_numpy(np.asarray(theta, np.float32))
        off = 0
        for h in self.heads:
            h.copy_(t[off:off + h.numel()])
            off += h.numel()
        self.m.copy_(torch.zeros(PM.PARAMS) if m is None else torch.from_numpy(np.asarray(m, np.float32)))
        self.v.copy_(torch.zeros(PM.PARAMS) if v is None else torch.from_numpy(np.asarray(v, np.float32)))
        self.step.fill_(step)

    def theta(self):
        return torch.cat(self.heads).cpu().numpy()

    def read(self):
        torch.cuda.synchronize()
        return dict(theta=self.theta(), m=self.m.cpu().numpy(), v=self.v.cpu().numpy(), step=float(self.step.cpu()[0]),
                    counter=int(self.counter.cpu()[0]))

    def update(self, d, n_epochs, hyper=HYPER):
        """n_epochs epochs over the device buffer ``d``: the (n_epochs, 2) losses."""
        losses = torch.full((n_epochs, 2), float("nan"), device="cuda")
        H = hyper
        self.nat.check(self.lib.occ_ppo_update(
            C.c_void_p(d["feats"].data_ptr()), C.c_void_p(d["actions"].data_ptr()), C.c_void_p(d["old_lp"].data_ptr()),
            C.c_void_p(d["returns"].data_ptr()), int(d["M"]), H["action_var"], H["eps_clip"], H["lr_actor"], H["lr_critic"],
            H["beta1"], H["beta2"], H["adam_eps"], C.byref(self.ps), int(n_epochs), C.c_void_p(losses.data_ptr()),
            C.c_void_p(self.scratch.data_ptr()), C.c_void_p(self.counter.data_ptr()),
            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "occ_ppo_update")
        torch.cuda.synchronize()
        return losses.cpu().numpy().astype(np.float64)


def to_device(s):
    return dict(M=s["M"], **{k: torch.from_numpy(np.ascontiguousarray(s[k])).cuda() for k in ("feats", "actions", "old_lp", "returns")})


def model_epoch(theta, s, hyper=HYPER, m=None, v=None, step=0.0):
    m = np.zeros(PM.PARAMS) if m is None else m
    v = np.zeros(PM.PARAMS) if v is None else v
    return PM.epoch(theta, m, v, step, s["F"], s["actions"], s["old_lp"], s["returns"], **hyper)


# ---- checks --------------------------------------------------------------------------------------------------------

def grad_err(got_m, o):
    """The kernel's gradient recovered from the first moment of ONE step from zero, m = (1 - b1) g: asserted within
    GRAD_TOL * S_k of the model's, component by component.  Returns (g, worst |g - g64| / S)."""
    g = got_m.astype(np.float64) / (1.0 - HYPER["beta1"])
    err = np.abs(g - o["grad"])
    assert (err <= GRAD_TOL * o["scale"]).all(), _worst_components(err, o)
    return g, float((err / np.where(o["scale"] > 0, o["scale"], np.inf)).max())


def _worst_components(err, o):
    rel = err / np.maximum(o["scale"], 1e-300)
    k = np.argsort(rel)[::-1][:6]
    return f"components {k.tolist()}: |err| / S = {rel[k].tolist()}, g64 = {o['grad'][k].tolist()}"


def check_losses(got, o, label):
    assert abs(got[0] - o["loss"]) <= GRAD_TOL * o["loss_scale"], (label, "loss", got[0], o["loss"])
    assert abs(got[1] - o["vloss"]) <= GRAD_TOL * o["vloss"], (label, "value loss", got[1], o["vloss"])


def record(M, label, w):
    WORST[M] = max(WORST.get(M, 0.0), w)
    print(f"M = {M:6d} ({label}): worst |err| / S {w:.3g}")


def heads0(seed):
    rng = np.random.default_rng(seed)
    return (0.05 * rng.standard_normal(PM.PARAMS)).astype(np.float32).astype(np.float64)


# ---- a. one epoch from zero Adam state over the sample-count sweep ------------------------------------------------

@pytest.mark.parametrize("M", SWEEP)
def test_one_epoch_gradient_over_the_grid_switches(lib, M):
    """One epoch from zero Adam state: the gradient is exactly recoverable, g = m / (1 - beta1).  Every one of the 771
    components within GRAD_TOL of its scale, v = (1 - beta2) g^2, both losses within GRAD_TOL of the scale of their sums,
    every parameter's step as the model's, the step count exactly 1 and the counter back at 0."""
    theta = heads0(1)
    s = make_set(M, 100 + M, theta)
    o = model_epoch(theta, s)
    assert_margin(o, M)
    L = Learner(lib)
    L.load(theta)
    losses = L.update(to_device(s), 1)
    got = L.read()
    g, w = grad_err(got["m"], o)
    record(M, f"{grid(lib, M)} blocks", w)
    assert np.allclose(got["v"], (1.0 - HYPER["beta2"]) * g * g, rtol=1e-5, atol=0.0)
    check_losses(losses[0], o, M)
    # the step lr * g / (|g| + eps): within 1e-3 lr of the model's, plus what the gradient bound moves it by where g ~ eps
    lr = np.where(np.arange(PM.PARAMS) < PM.N_ACTOR, HYPER["lr_actor"], HYPER["lr_critic"])
    eps = HYPER["adam_eps"]
    tol = lr * (1e-3 + eps * GRAD_TOL * o["scale"] / (np.abs(o["grad"]) + eps) ** 2)
    assert (np.abs((got["theta"] - theta) - (o["theta"] - theta)) <= tol).all()
    assert got["step"] == 1.0 and got["counter"] == 0


def test_the_sweep_covers_every_grid(lib):
    """The sweep reaches the capped 64-block grid and the OCC_PPO_MAX_BLOCKS grid, and one block with idle waves."""
    grids = {grid(lib, M) for M in SWEEP}
    assert {1, 2, 63, 64, int(lib.occ_ppo_max_blocks())} <= grids


# ---- b. the hand-off across launches --------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [12800, 102400])
def test_partials_are_not_carried_across_launches(lib, M):
    """20 single-epoch calls on ONE scratch and counter, alternating two buffers whose returns differ in sign and scale
    (a row left over from the previous call would be grossly wrong).  Before each call the moments and the step are
    zeroed and the heads read back as the kernel left them; after it the recovered gradient is checked against the model
    at those heads.  Every call is checked; the failures are reported together."""
    calls, H = 20, HYPER_SLOW
    theta = heads0(2)
    moved = calls * H["lr_actor"] * step_bound(1)
    sets = [make_set(M, 200 + M, theta, moved, 0.1, 1.0, 1.0), make_set(M, 300 + M, theta, moved, 0.1, -1.0, 4.0)]
    dev = [to_device(s) for s in sets]
    L = Learner(lib)
    L.load(theta)
    fails = []
    for c in range(calls):
        i = c % 2
        at = L.theta().astype(np.float64)
        L.load(at)
        losses = L.update(dev[i], 1, H)
        got = L.read()
        o = model_epoch(at, sets[i], H)
        assert_margin(o, M)
        try:
            _, w = grad_err(got["m"], o)
            check_losses(losses[0], o, (M, c))
            assert got["counter"] == 0 and got["step"] == 1.0
            record(M, f"{grid(lib, M)} blocks, call {c}", w)
        except AssertionError as e:
            fails.append(f"call {c}: {e}")
    assert not fails, "\n".join(fails)


# ---- c. epochs inside one call --------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [12800, 102400])
def test_five_epochs_in_one_call_follow_the_model(lib, M):
    """n_epochs = 5 in one call against the model's 5-epoch trajectory (margin asserted at each epoch): heads to 1e-6
    (the bound of test_ppo_golden.py at K <= 5) plus what a per-epoch gradient error of HEADS_GRAD_ERR moves Adam by
    (``adam_spread``; at 102 400 samples one component of 771 sat 2.2e-6 away), m and v to 1e-4 relative (plus what the per-epoch gradient bound lets
    through where a component's sum cancels), all ten loss values."""
    K = 5
    theta = heads0(3)
    s = make_set(M, 400 + M, theta, HYPER["lr_actor"] * sum(step_bound(t) for t in range(1, K + 1)), 0.1)
    traj = PM.run(theta, s["F"], s["actions"], s["old_lp"], s["returns"], K, **HYPER)
    for o in traj:
        assert_margin(o, M)
    L = Learner(lib)
    L.load(theta)
    losses = L.update(to_device(s), K)
    got = L.read()
    last = traj[-1]
    assert (np.abs(got["theta"] - last["theta"]) <= 1e-6 + adam_spread(traj, HEADS_GRAD_ERR)).all()
    assert float(np.abs(last["theta"] - theta).max()) > 1e-3  # the epochs moved the heads
    b1, b2 = HYPER["beta1"], HYPER["beta2"]
    m_tol = sum((1 - b1) * b1 ** (K - 1 - e) * GRAD_TOL * o["scale"] for e, o in enumerate(traj))
    v_tol = sum((1 - b2) * b2 ** (K - 1 - e) * (2 * np.abs(o["grad"]) + GRAD_TOL * o["scale"]) * GRAD_TOL * o["scale"]
                for e, o in enumerate(traj))
    assert (np.abs(got["m"] - last["m"]) <= 1e-4 * np.abs(last["m"]) + m_tol).all()
    assert (np.abs(got["v"] - last["v"]) <= 1e-4 * last["v"] + v_tol).all()
    assert got["step"] == float(K) and got["counter"] == 0
    for e, o in enumerate(traj):
        check_losses(losses[e], o, (M, e))


def adam_spread(traj, rel):
    """How far the Adam steps of ``traj`` end from the model's when every epoch's gradient is off by up to rel * S_k
    (worst sign pattern; Adam is elementwise, the feedback of the heads into later gradients is left out).  Large only
    where a component's gradient sum nearly cancels at some epoch: there m / sqrt(v) turns on rounding."""
    G = np.stack([o["grad"] for o in traj])
    D = np.stack([rel * o["scale"] for o in traj])
    adam = {k: HYPER[k] for k in ("lr_actor", "lr_critic", "beta1", "beta2", "adam_eps")}

    def steps(g):
        x, m, v = np.zeros(PM.PARAMS), np.zeros(PM.PARAMS), np.zeros(PM.PARAMS)
        for e in range(len(g)):
            x, m, v, _ = PM.adam(x, m, v, float(e), g[e], **adam)
        return x

    ref = steps(G)
    return np.max([np.abs(steps(G + np.array(sg)[:, None] * D) - ref)
                   for sg in itertools.product((-1.0, 1.0), repeat=len(traj))], axis=0)


# ---- d. reproducibility -----------------------------------------------------------------------------------------------

def test_update_is_bitwise_reproducible_and_reads_no_unwritten_row(lib):
    """At M = 102 400 (128 blocks): the same three epochs twice from the same state give the same bits (heads, moments,
    step, losses); and again with the scratch filled with NaN before the call: no row that this launch did not write is
    read."""
    M, K = 102400, 3
    theta = heads0(4)
    d = to_device(make_set(M, 500 + M, theta))
    L = Learner(lib)
    runs = []
    for poison in (False, False, True):
        L.load(theta)
        if poison:
            L.scratch.fill_(float("nan"))
        losses = L.update(d, K)
        got = L.read()
        assert got["counter"] == 0 and np.isfinite(losses).all()
        runs.append((got, losses.astype(np.float32)))
    (a, la) = runs[0]
    for b, lb in runs[1:]:
        for k in ("theta", "m", "v"):
            assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
        assert a["step"] == b["step"] == float(K)
        assert np.array_equal(la.view(np.int32), lb.view(np.int32))
