"""The tail of a step - occ_combine_kernel, occ_reduce_kernel, finish_one / occ_finish_kernel (occ_combine.hpp) -
directly against the f64 host model of tests/combine_model.py, on the planes the raster kernel left for that very launch.

(a) the model against the tracked (reserve + output ring), half-tracked (reserve, fresh obs / full_state) and untracked
    engine after every step of a driven sequence, at image sides whose 256-pixel blocks lie differently in the frame;
(b) the three paths against each other, bit for bit, and the background invariant of every tracked buffer;
(c) skipped rows under tracking: a rect carried across two skips still clears what the set held;
(d) the tracked sequence on the build without the background fast path: the same bits.

Every tolerance is a rounding count derived in tests/combine_model.py.  The COVERAGE COUNTERS (conditions computed from
the snapshotted rects with the model's classifiers) are asserted, so a sequence that stops reaching a rule fails."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from tests import combine_model as CM
from tests.parity_utils import ROOT, make_case, tracked_buffers_hold_background

pytestmark = pytest.mark.gpu

N = 6
RESERVE = 2  # reserve rows of the tracked engines; they stay EMPTY and skipped
SEED = 11
SIDES = [8, 24, 40, 64, 72, 256, 264, 512]
KINDS = ("tracked", "half", "plain")
STORED = (64, 72, 264)  # sides whose tracked outputs are kept for the GRAD = false and the no-fast-path comparisons
N_PHASES = 8
LOW_SHIFT = 1.7         # world units: at radius 4 the frame's lower edge lies 4 tan(30 deg) = 2.31 below the centre
KEYS = ("obs", "fs", "alphas", "loss", "reward", "done", "grad", "full_reward")


def n_steps(S):
    return 5 if S >= 264 else 8


def phase_of(env, t):
    return (t + env) % N_PHASES  # every env is somewhere else in the schedule: one launch mixes the states


def phase_state(case, env, phase):
    """Scene offsets (3, 3) and camera radius of ``env`` in a phase of the schedule: 0 the case's view, 1 two objects
    pushed out of the frame, 2 all three out (empty footprint), 3 everything back, the outer two spread vertically (so
    that even a 24-pixel frame's footprint strictly contains the next one), 4 and 5 radius 30 (a tiny rect mid-frame, once
    per ring set), 6 radius 4 again, 7 all three objects lowered so that the rects reach the last rows."""
    off = case["offsets"][env].clone()
    radius = 4.0
    if phase in (1, 2):
        off[1, 0], off[2, 0] = 50.0, -50.0
    if phase == 2:
        off[0, 1] = 60.0
    if phase == 3:
        off[1, 1] += 0.9
        off[2, 1] -= 0.9
    if phase in (4, 5):
        radius = 30.0
    if phase == 7:
        off[:, 1] -= LOW_SHIFT
    return off, radius


def _case(device="cuda"):
    case = make_case(N, SEED, "synthetic", device=device)
    assert case["pool"].atlas_tensors()[0] is None  # flat colour without an atlas: what the model covers
    return case


def _actions(S, t):
    """Random actions for the even envs, zero actions for the odd ones."""
    g = torch.Generator().manual_seed(1000 * S + t)
    a = torch.randn(N, 2, generator=g)
    a[1::2] = 0.0
    return a


def _engine(case, S, kind, pixel_weight=None):
    from occlusionenv_amd.engine import OcclusionEngine

    kw = dict(tracked=dict(reserve=RESERVE, output_ring=2), half=dict(reserve=RESERVE), plain={})[kind]
    if kind == "plain":
        # The wholly untracked engine is launched over N + RESERVE rows too, the extra ones skipped like the EMPTY reserve rows
        # of the other two.  The raster kernel sizes its work items from the row count of the launch (RasterParams.split_log2),
        # and at S = 256 six rows and eight rows get different splits, whose alpha planes differ in the last bits: the three
        # paths can only be compared bit for bit on launches of one shape.
        eng = OcclusionEngine(case["pool"], N + RESERVE, S)
        eng.set_scene(list(range(N, N + RESERVE)), case["mesh_ids"][:RESERVE], case["offsets"][:RESERVE])
        eng.skip_mask = torch.zeros(N + RESERVE, dtype=torch.int32, device=eng.device)
        eng.skip_mask[N:] = 1
    else:
        eng = OcclusionEngine(case["pool"], N, S, **kw)
    eng.set_scene(list(range(N)), case["mesh_ids"], case["offsets"])
    if pixel_weight is not None:
        eng.pixel_weight = pixel_weight
    eng.reset_render(list(range(N)), 4.0, case["az"], 0.0)
    if kind == "plain":  # step() hands the launch's grad_elaz back only with the reserve: keep what _render returns
        inner = eng._render

        def spy(*a, **k):
            eng.last_render = inner(*a, **k)
            return eng.last_render

        eng._render = spy
    return eng


def _set_phase(case, eng, t):
    for e in range(N):
        off, radius = phase_state(case, e, phase_of(e, t))
        eng.scene_offset[e] = off.to(eng.device)
        eng.radius[e] = radius


def _step(eng, kind, a, grad):
    """One step; returns the launch's inputs that the tail reads from outside the workspace and everything it wrote
    (device tensors of the env rows; ring buffers are not cloned: look at them before the set comes round again)."""
    pre = dict(full_reward=eng.full_reward[:N].clone(), object_mass=eng.object_mass[:N].clone())
    act = a.clone().requires_grad_(grad)
    rect = {}
    if kind == "plain":
        obs, reward, done, fs, loss = eng.step(torch.cat([act, act.new_zeros(RESERVE, 2)]), skip=eng.skip_mask)
        out = eng.last_render
    else:
        slot = eng.pick_output_set()[1] if kind == "tracked" else None
        obs, reward, done, fs, loss, out = eng.step(act, with_reserve=True)
        if slot is not None:
            rect.update(rect_prev=slot["rect"][slot["cur"] ^ 1][:N], rect_next=slot["rect"][slot["cur"]][:N])
        rect.update(arect_prev=eng._arect[eng._arect_cur ^ 1][:N], arect_next=eng._arect[eng._arect_cur][:N])
    ga = None
    if grad:
        reward.sum().backward()
        ga = act.grad
    try:
        torch.cuda.synchronize()
    except RuntimeError as ex:  # a device error: nothing more is started on this GPU
        pytest.exit("device error after a step at S = %d (%s): %s" % (eng.S, kind, ex), returncode=3)
    eng.check_status()
    ge = out.get("grad_elaz")
    got = dict(obs=obs[:N], fs=fs[:N], alphas=eng.alphas[:N], loss=loss[:N], reward=reward.detach()[:N], done=done[:N], grad=ga,
               full_reward=eng.full_reward[:N], grad_elaz=None if ge is None else ge[:N], cam=eng.cam[:N], **rect)
    return pre, got


def _inputs(eng):
    """The planes, rects and records the launch left in the workspace, env rows only, on the host."""
    S, t = eng.S, eng._ws_tensors
    px = N * 3 * S * S
    f32 = lambda name, k: t[name].view(torch.float32)[:k]  # noqa: E731
    inp = dict(alpha=f32("obj_alpha", px).view(N, 3, S, S), grad=f32("obj_grad", 2 * px).view(N, 3, S, S, 2),
               hz=f32("obj_hz", px).view(N, 3, S, S), hrec=t["obj_hrec"][:px].view(N, 3, S, S),
               objrect=t["objrect"][: N * 12].view(N, 3, 4), nrec=t["nrec"][: N * 3].view(N, 3),
               partials=f32("partials", N * CM.n_blocks(S) * 4).view(N, CM.n_blocks(S), 4))
    inp = {k: v.cpu().numpy() for k, v in inp.items()}
    off = eng._rec_tensors["rec_off"].cpu().numpy().view(np.int64)[: N * 3 + 1]
    raw = eng._rec_tensors["rec"].view(torch.float32)[: int(off[N * 3]) * CM.REC_STRIDE].cpu().numpy().reshape(-1, CM.REC_STRIDE)
    inp["recs"] = [raw[int(off[eo]): int(off[eo]) + int(inp["nrec"].reshape(-1)[eo])] for eo in range(N * 3)]
    return inp


def _same_inputs(a, b):
    """Bit-equal planes, rects and records (stale plane values included): the model of one launch serves the other."""
    for k in ("alpha", "grad", "hz", "hrec", "objrect", "nrec"):
        if not np.array_equal(a[k].view(np.int32), b[k].view(np.int32)):
            return False
    return all(x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a["recs"], b["recs"]))


def _ratio(err, tol):
    """Largest error-to-bound ratio (0 / 0 counts as 0, anything over a zero bound as inf)."""
    err, tol = np.abs(np.asarray(err, np.float64)), np.asarray(tol, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / tol)
    return float(np.max(r)) if r.size else 0.0


def _check_launch(S, models, inp, pre, got, grad, consts, tag, margins, fails):
    """Everything one launch wrote against the model, env by env.  Failures are collected, not raised: one run reports
    every quantity."""
    host = {k: (None if v is None else v.detach().cpu().numpy()) for k, v in got.items()}
    pre = {k: v.cpu().numpy() for k, v in pre.items()}

    def note(name, r, env, extra=""):
        margins[name] = max(margins.get(name, 0.0), r)
        if not r <= 1.0:
            fails.append("%s env %d: %s %.3g of its bound %s" % (tag, env, name, r, extra))

    def exact(name, ok, env):
        if not ok:
            fails.append("%s env %d: %s differs" % (tag, env, name))

    for e in range(N):
        m = models[e]
        exact("alphas frame", np.array_equal(host["alphas"][e], m["alphas"]), e)
        fs = host["fs"][e]
        exact("full_state[..., :3] == 3", bool((fs[..., :3] == 3.0).all()), e)
        note("I", _ratio(fs[..., 3] - m["I"], m["I_tol"]), e)
        obs = host["obs"][e]
        exact("depth channel", np.array_equal(obs[3], m["depth"]), e)
        exact("background colour", bool((obs[:3][:, ~m["hit"]] == 1.0).all()), e)
        note("flat colour", _ratio((obs[:3] - m["colour"])[:, m["hit"]], np.broadcast_to(m["colour_tol"], (3, S, S))[:, m["hit"]]), e)
        if m["den_min"] <= 100.0 * float(consts["kEpsilon"]):
            fails.append("%s env %d: barycentric denominator %.3g in reach of the kEpsilon clamp" % (tag, e, m["den_min"]))
        b0, b1 = m["fp_blocks"]
        part = inp["partials"][e]
        ncol = 3 if grad else 1
        for b in range(b0, b1 + 1):
            if m["bg_block"][b]:
                exact("partial of background block %d" % b, not part[b].any(), e)
            else:
                note("block partial", _ratio(part[b, :ncol] - m["block_sum"][b, :ncol], m["block_tol"][b, :ncol]), e, "(block %d)" % b)
                exact("unused partial slots of block %d" % b, not part[b, ncol:].any(), e)
        note("loss", _ratio(host["loss"][e] - m["frame_sum"][0], m["frame_tol"][0]), e)
        if grad:
            note("grad_elaz", _ratio(host["grad_elaz"][e] - m["frame_sum"][1:], m["frame_tol"][1:]), e)
        f = CM.finish(host["loss"][e], host["grad_elaz"][e] if grad else None, pre["full_reward"][e], pre["object_mass"][e],
                      host["cam"][e, CM.C_J:CM.C_J + 4], consts)
        exact("done == (loss < 0.1f)", bool(host["done"][e]) == f["done"], e)
        exact("full_reward == loss", host["full_reward"][e].tobytes() == host["loss"][e].tobytes(), e)
        note("reward", _ratio(host["reward"][e] - f["reward"], f["reward_tol"]), e)
        if grad:
            note("action gradient", _ratio(host["grad"][e] - f["grad_action"], f["grad_action_tol"]), e)
        for name in ("rect_next", "arect_next"):
            if host.get(name) is not None:
                exact(name, tuple(int(v) for v in host[name][e]) == m["footprint"], e)
        if CM.is_empty(m["footprint"]):
            exact("loss of an empty footprint is exactly 0", host["loss"][e] == 0.0 and bool(host["done"][e]), e)


_COUNTERS = ("empty_footprint", "strictly_inside_prev", "empty_prev_nonempty_fp", "bg_meets_prev", "tail_visited", "one_row_partial")


def _count(S, models, got, counters):
    """Coverage conditions of a tracked launch, for the output set (ring) and for the alphas state."""
    rp, ap = got["rect_prev"].cpu().numpy(), got["arect_prev"].cpu().numpy()
    for e in range(N):
        m = models[e]
        for name, prev, other in (("set", rp[e], ap[e]), ("alphas", ap[e], rp[e])):
            c = CM.classify(S, m["obj_rects"], m["footprint"], prev, other)
            for k in _COUNTERS:
                counters[name][k] += int(bool(c[k]))


def run_sequence(S, kinds=KINDS, check_model=True, store=False, grad=True, weighted=False):
    """Drive the schedule through one engine per kind, in lockstep.  Returns dict(fails, margins, counters, mismatch,
    outputs): model failures per kind, error-to-bound ratios, coverage counters, (kind, step, key) of every output that
    differs from the first kind's, and - with ``store`` - the first kind's outputs per step on the host."""
    case = _case()
    consts = CM.header_constants()
    pw = None
    if weighted:  # random weights, a quarter of them zero
        g = torch.Generator().manual_seed(5)
        pw = (torch.rand(N, S, S, generator=g) * 2.0 * (torch.rand(N, S, S, generator=g) > 0.25)).cuda().contiguous()
    engs = {k: _engine(case, S, k, pw) for k in kinds}
    res = dict(fails={k: [] for k in kinds}, margins={}, mismatch=[], outputs=[], background=[],
               counters=dict(set={k: 0 for k in _COUNTERS}, alphas={k: 0 for k in _COUNTERS}))
    weights = None if pw is None else pw.cpu().numpy()
    for t in range(n_steps(S)):
        a = _actions(S, t).cuda()
        first = first_inp = models = None
        for kind in kinds:
            eng = engs[kind]
            _set_phase(case, eng, t)
            pre, got = _step(eng, kind, a, grad)
            if check_model:
                inp = _inputs(eng)
                if models is None or not _same_inputs(first_inp, inp):
                    mods = [CM.combine_env(S, inp["alpha"][e], inp["grad"][e], inp["hz"][e], inp["hrec"][e], inp["objrect"][e],
                                           inp["nrec"][e], inp["recs"][3 * e: 3 * e + 3], None if weights is None else weights[e])
                            for e in range(N)]
                    if models is None:
                        models, first_inp = mods, inp
                else:
                    mods = models
                _check_launch(S, mods, inp, pre, got, grad, consts, "S=%d %s step %d" % (S, kind, t), res["margins"], res["fails"][kind])
                if kind == "tracked":
                    _count(S, mods, got, res["counters"])
            if kind == "tracked":
                try:
                    tracked_buffers_hold_background(eng)
                except AssertionError:
                    res["background"].append(t)
            keep = {k: got[k] for k in KEYS if got[k] is not None}
            if first is None:
                first = {k: v.clone() for k, v in keep.items()}
                if store:
                    res["outputs"].append({k: v.cpu() for k, v in first.items()})
            else:
                res["mismatch"] += [(kind, t, k) for k, v in keep.items() if not torch.equal(v, first[k])]
    return res


_RUNS = {}


def _run(S):
    """One lockstep run of the three engines per image side, shared by the tests of this module."""
    if S not in _RUNS:
        _RUNS[S] = run_sequence(S, store=S in STORED)
        print("S=%d margins (largest error / bound): %s" % (S, {k: round(v, 4) for k, v in _RUNS[S]["margins"].items()}))
        print("S=%d counters: %s" % (S, _RUNS[S]["counters"]))
    return _RUNS[S]


def _assert_counters(S, counters):
    """Every rule the sequence is there to reach was reached, wherever the geometry of this side allows it."""
    c = counters["set"]
    assert c["empty_footprint"] >= 1 and c["empty_prev_nonempty_fp"] >= 1, (S, counters)
    assert counters["alphas"]["empty_prev_nonempty_fp"] >= 1, (S, counters)
    if S >= 24:  # (an 8-pixel frame is 2 x 2 rect units and a single tail block: nothing fits strictly inside, no fast path)
        assert c["strictly_inside_prev"] >= 1 and counters["alphas"]["strictly_inside_prev"] >= 1, (S, counters)
        assert c["bg_meets_prev"] >= 1 and counters["alphas"]["bg_meets_prev"] >= 1, (S, counters)
    if (S * S) % CM.PIX_BLOCK:
        assert c["tail_visited"] >= 1, (S, counters)
    if S >= 264:
        assert c["one_row_partial"] >= 1, (S, counters)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", SIDES)
def test_model_against_every_path(S, kind):
    """(a): alphas and depth bit-exact, I, colour, block partials, loss, grad_elaz, reward and action gradient within their
    rounding bounds, background-block partials exactly zero, done on the kernel's own f32 loss, full_reward the loss's
    bits, rect_next / arect_next the model's footprint - after every step, for every env row."""
    run = _run(S)
    assert not run["fails"][kind], run["fails"][kind][:12]
    if kind == "tracked":
        _assert_counters(S, run["counters"])


@pytest.mark.parametrize("S", SIDES)
def test_tracked_half_tracked_and_untracked_agree_bit_for_bit(S):
    """(b): obs, full_state, alphas, loss, reward, done, action gradient and full_reward of the env rows at every step; both
    ring sets and the alphas state are background outside their current rects after every tracked step."""
    run = _run(S)
    assert not run["mismatch"], run["mismatch"][:12]
    assert not run["background"], ("a tracked buffer is not background outside its rect after steps", run["background"])


def test_model_with_pixel_weights_that_contain_zeros():
    run = run_sequence(72, kinds=("tracked",), weighted=True)
    print("weighted margins:", {k: round(v, 4) for k, v in run["margins"].items()})
    assert not run["fails"]["tracked"], run["fails"]["tracked"][:12]
    assert not run["background"]
    _assert_counters(72, run["counters"])


_GRAD_PAIR = {}


def _grad_pair(S=72):
    """Two tracked engines in lockstep through the schedule, one stepped with gradients and one without (the GRAD = false
    instantiations of the setup, raster and combine kernels).  Per (env, step): are the planes the combine kernel reads
    (inside in_rect) and the record slots it reads bit-equal in the two runs, and are the outputs?"""
    if S in _GRAD_PAIR:
        return _GRAD_PAIR[S]
    case, consts = _case(), CM.header_constants()
    engs = {g: _engine(case, S, "tracked") for g in (True, False)}
    res = dict(fails=[], margins={}, same_inputs=0, stage_mismatch=[], strict=[], figures={})
    for t in range(n_steps(S)):
        a = _actions(S, t).cuda()
        got, inp, pre = {}, {}, {}
        for g, eng in engs.items():
            _set_phase(case, eng, t)
            pre[g], got[g] = _step(eng, "tracked", a, g)
            inp[g] = _inputs(eng)
            got[g] = {k: v.detach().cpu().numpy().copy() for k, v in got[g].items() if v is not None}
        models = [CM.combine_env(S, inp[False]["alpha"][e], inp[False]["grad"][e], inp[False]["hz"][e], inp[False]["hrec"][e],
                                 inp[False]["objrect"][e], inp[False]["nrec"][e], inp[False]["recs"][3 * e: 3 * e + 3]) for e in range(N)]
        _check_launch(S, models, inp[False], pre[False], {k: torch.from_numpy(v) for k, v in got[False].items()}, False, consts,
                      "S=%d no gradients, step %d" % (S, t), res["margins"], res["fails"])
        for e in range(N):
            m = models[e]
            same = np.array_equal(inp[True]["objrect"][e], inp[False]["objrect"][e]) and np.array_equal(inp[True]["nrec"][e], inp[False]["nrec"][e])
            for k in ("alpha", "hz", "hrec"):
                x, y = (np.where(m["in_rect"], inp[g][k][e], 0).view(np.int32) for g in (True, False))
                same = same and np.array_equal(x, y)
            for o in range(3):  # the slots the combine kernel reads: positions, id, flags, 1 / area, the shading terms
                x, y = (inp[g]["recs"][3 * e + o] for g in (True, False))
                cols = list(range(13)) + [CM.R_SPEC]
                same = same and x.shape == y.shape and np.array_equal(x[:, cols].view(np.int32), y[:, cols].view(np.int32))
            same_state = bool(pre[True]["full_reward"][e] == pre[False]["full_reward"][e])
            for k in ("obs", "fs", "alphas", "loss", "reward", "done", "full_reward"):
                x, y = got[True][k][e], got[False][k][e]
                if not np.array_equal(x, y):
                    res["strict"].append((t, e, k))
                    d = np.abs(x.astype(np.float64) - y.astype(np.float64))
                    n, worst = res["figures"].get(k, (0, 0.0))
                    res["figures"][k] = (n + int((x != y).sum()), max(worst, float(d.max())))
                    if same and (same_state or k not in ("reward",)):
                        res["stage_mismatch"].append((t, e, k))
            res["same_inputs"] += int(same)
    print("with / without gradients at S=%d: %d of %d (env, step) pairs read equal planes; elements that differ and the largest "
          "difference per output: %s" % (S, res["same_inputs"], N * n_steps(S), res["figures"]))
    _GRAD_PAIR[S] = res
    return res


def test_without_gradients_equal_planes_give_equal_bits():
    """The GRAD = false instantiation of the tail: the model holds (the gradient slots of the partials stay zero), and
    wherever the planes and record slots the combine kernel reads are the same bits in the run with gradients, obs,
    full_state, alphas, loss, done (and reward, given the same full_reward) are the same bits too."""
    run = _grad_pair()
    assert not run["fails"], run["fails"][:12]
    assert run["same_inputs"] >= N, "too few (env, step) pairs with equal planes to say anything"
    assert not run["stage_mismatch"], run["stage_mismatch"][:12]


def test_without_gradients_the_same_bits():
    """A step without gradients returns the obs, full_state, alphas, loss, reward and done of the step with gradients,
    bit for bit, at every step of the schedule.  (This test found that occ_setup_kernel<true> and <false> wrote records
    one ulp apart in the third vertex of about a fifth of the faces - the contraction of the view transform into FMAs
    was left to the compiler; occ_setup.hpp: view_pos now spells the order out.)"""
    run = _grad_pair()
    assert not run["strict"], (run["strict"][:12], run["figures"])


def test_equal_depth_goes_to_the_earlier_object():
    """The one tie of the stage.  Objects 0 and 2 of every env are the same mesh at the same offset, so their records and
    their depth planes are equal bit for bit wherever they are hit; one of the two carries an atlas whose texels are all
    0.25, the other the white vertex texture, so the colour tells which object the kernel let win: it must be object 0,
    in both arrangements, and the model (strict ``<``, objects in order) says so pixel by pixel."""
    from occlusionenv_amd.meshes import MeshPool, SyntheticShapeNet

    S, GREY = 128, 0.25
    ds = SyntheticShapeNet(n_models=2, seed=1234 + SEED)
    pool = MeshPool("cuda")
    (v0, f0), (v1, f1) = ds.models[0], ds.models[1]
    white = pool.add(v0, f0, key="white")
    grey = pool.add(v0, f0, key="grey", atlas=torch.full((f0.shape[0], 2, 2, 3), GREY))
    other = pool.add(v1, f1, key="other")
    mesh_ids = torch.tensor([[white, other, grey], [grey, other, white]] * (N // 2))
    offsets = torch.zeros(N, 3, 3)
    offsets[:, 1, 0], offsets[:, 1, 2] = torch.linspace(0.7, 1.2, N), 1.0  # (to the side: it covers part of the pair at most)
    case = dict(pool=pool, mesh_ids=mesh_ids, offsets=offsets, az=torch.linspace(-0.5, 0.5, N))
    consts = CM.header_constants()
    margins, n_tied = {}, 0
    for kind in ("plain", "tracked"):
        eng = _engine(case, S, kind)
        fails = []
        pre, got = _step(eng, kind, _actions(S, 0).cuda(), True)
        inp = _inputs(eng)
        models = []
        for e in range(N):
            tex = [GREY if int(mesh_ids[e, o]) == grey else None for o in range(3)]
            m = CM.combine_env(S, inp["alpha"][e], inp["grad"][e], inp["hz"][e], inp["hrec"][e], inp["objrect"][e], inp["nrec"][e],
                               inp["recs"][3 * e: 3 * e + 3], tex=tex)
            tie = m["in_rect"][0] & m["in_rect"][2] & (inp["hz"][e][0] == inp["hz"][e][2]) & (inp["hrec"][e][0] >= 0) & m["hit"]
            tie &= m["depth"] == inp["hz"][e][0]
            both = m["in_rect"][0] & m["in_rect"][2] & (inp["hrec"][e][0] >= 0)
            assert int(tie.sum()) > 60, (kind, e, "objects 0 and 2 must tie where they are in front", int(both.sum()),
                                         int((both & (inp["hz"][e][0] == inp["hz"][e][2])).sum()), int(m["hit"].sum()))
            assert (m["win_obj"][tie] == 0).all()
            n_tied += int(tie.sum())
            # the two candidates' colours differ by far more than the bound: the check below can tell them apart
            r = inp["recs"][3 * e][inp["hrec"][e][0][tie]]
            assert (np.abs(r[:, CM.R_AMB]) * (1.0 - GREY) > 1e-2).all()
            models.append(m)
        _check_launch(S, models, inp, pre, got, True, consts, "tie %s" % kind, margins, fails)
        assert not fails, fails[:12]
    print("tie: %d tied pixels; margins %s" % (n_tied, {k: round(v, 4) for k, v in margins.items()}))


# ---- (c) skipped rows under tracking -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 264])
def test_skipped_rows_keep_their_bits_and_their_rect(S):
    """occ_render with an own skip mask, two own output sets used in turn, an own alphas state and own rect arrays.  Row 2
    is rendered large at t0 (set A) and t1 (set B), skipped at t2 and t3, rendered tiny (radius 30) at t4 (A) and t5 (B).
    While skipped the row keeps every bit of the set that is written, rect_next = rect_prev, and its loss, reward, done
    and gradient rows keep the sentinel put there.  At t4 / t5 the row equals an untracked launch's bit for bit: the
    large image that sat in set A since t0 is cleared through a rect that was carried across two skips."""
    from occlusionenv_amd import _native as nat
    from occlusionenv_amd.engine import OcclusionEngine, _p

    ROW, SENT = 2, -77.0
    case = _case()
    eng = OcclusionEngine(case["pool"], N, S)
    eng.set_scene(list(range(N)), case["mesh_ids"], case["offsets"])
    lib, st = eng.lib, eng._stream()
    ws = eng._ensure_workspace()
    f32 = dict(dtype=torch.float32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    empty = torch.tensor(CM.empty_rect(S), **i32)

    def new_set():
        obs, fs = torch.empty(N, 4, S, S, **f32), torch.empty(N, S, S, 4, **f32)
        obs[:, :3], obs[:, 3] = 1.0, -1.0
        fs[..., :3], fs[..., 3] = 3.0, 0.0
        return dict(obs=obs, fs=fs, rect=[empty.repeat(N, 1).contiguous() for _ in range(2)], cur=0)

    sets = [new_set(), new_set()]
    alphas, arect, acur = torch.zeros(N, 3, S, S, **f32), [empty.repeat(N, 1).contiguous() for _ in range(2)], 0
    state = {k: dict(fr=torch.full((N,), 3.0, **f32), om=torch.full((N,), 2.0, **f32)) for k in ("tracked", "fresh")}
    el, cam = torch.zeros(N, **f32), torch.empty(N, nat.CAM_STRIDE, **f32)
    flags = nat.RENDER_SOFT | nat.RENDER_HARD | nat.RENDER_GRAD
    seen_clear = 0
    for t in range(6):
        skipped = t in (2, 3)
        mask = torch.zeros(N, **i32)
        mask[ROW] = int(skipped)
        radius = torch.full((N,), 4.0, **f32)
        radius[ROW] = 30.0 if t >= 4 else 4.0
        radius[4] = 30.0 if t % 2 else 4.0  # (another row keeps changing size, never skipped)
        az = (case["az"] + 0.05 * t).cuda()
        nat.check(lib.occ_camera(nat.CAM_LOOKAT, None, _p(el), _p(az), _p(radius), _p(cam), None, N, st), "occ_camera")
        sc = eng._scene_struct(N, eng.scene_mesh, eng.scene_offset, skip=mask)
        results = {}
        for mode in ("tracked", "fresh"):
            ro, fin = nat.OccRenderOut(), nat.OccStepFinish()
            o = dict(loss=torch.full((N,), SENT, **f32), ge=torch.full((N, 2), SENT, **f32), reward=torch.full((N,), SENT, **f32),
                     done=torch.full((N,), 9, dtype=torch.uint8, device="cuda"), ga=torch.full((N, 2), SENT, **f32))
            if mode == "tracked":
                cur = sets[t % 2]
                rp, rn = cur["rect"][cur["cur"]], cur["rect"][cur["cur"] ^ 1]
                cur["cur"] ^= 1
                ap, an = arect[acur], arect[acur ^ 1]
                acur ^= 1
                before = dict(obs=cur["obs"][ROW].clone(), fs=cur["fs"][ROW].clone(), alphas=alphas[ROW].clone(), rp=rp.clone(), ap=ap.clone())
                o.update(obs=cur["obs"], fs=cur["fs"], alphas=alphas, rn=rn, an=an)
                ro.rect_prev, ro.rect_next, ro.arect_prev, ro.arect_next = rp.data_ptr(), rn.data_ptr(), ap.data_ptr(), an.data_ptr()
            else:
                o.update(obs=torch.empty(N, 4, S, S, **f32), fs=torch.empty(N, S, S, 4, **f32), alphas=torch.empty(N, 3, S, S, **f32))
            ro.obs, ro.full_state, ro.alphas = o["obs"].data_ptr(), o["fs"].data_ptr(), o["alphas"].data_ptr()
            ro.loss, ro.grad_elaz = o["loss"].data_ptr(), o["ge"].data_ptr()
            s = state[mode]
            fin.full_reward, fin.object_mass, fin.reward, fin.done = s["fr"].data_ptr(), s["om"].data_ptr(), o["reward"].data_ptr(), o["done"].data_ptr()
            fin.grad_action, fin.n_step = o["ga"].data_ptr(), N
            ro.finish = C.pointer(fin)
            fr_before = s["fr"].clone()
            nat.check(lib.occ_render(C.byref(sc), _p(cam), C.byref(ws), C.byref(ro), flags, eng.K, st), "occ_render")
            torch.cuda.synchronize()
            o["fr"], o["fr_before"] = s["fr"].clone(), fr_before
            results[mode] = o
        eng.check_status()
        tr, fr = results["tracked"], results["fresh"]
        if skipped:
            assert torch.equal(tr["obs"][ROW], before["obs"]) and torch.equal(tr["fs"][ROW], before["fs"]), t
            assert torch.equal(tr["alphas"][ROW], before["alphas"]), t
            assert torch.equal(tr["rn"][ROW], before["rp"][ROW]) and torch.equal(tr["an"][ROW], before["ap"][ROW]), t
            assert not CM.is_empty(tr["rn"][ROW].tolist()), "the row was rendered before: the carried rect is not empty"
            for o in (tr, fr):
                assert float(o["loss"][ROW]) == SENT and float(o["reward"][ROW]) == SENT and int(o["done"][ROW]) == 9, t
                assert (o["ge"][ROW] == SENT).all() and (o["ga"][ROW] == SENT).all(), t
                assert torch.equal(o["fr"][ROW], o["fr_before"][ROW]), t
        rows = [r for r in range(N) if not (skipped and r == ROW)]
        for k in ("obs", "fs", "alphas", "loss", "ge", "reward", "done", "ga", "fr"):
            assert torch.equal(tr[k][rows], fr[k][rows]), (t, k)
        assert float(tr["loss"][rows].max()) > 0.0
        if t >= 4:  # the tiny footprint lies strictly inside the rect the set carried: there is stale content to clear
            c = CM.classify(S, [tuple(tr["rn"][ROW].tolist())], tuple(tr["rn"][ROW].tolist()), before["rp"][ROW].tolist(),
                            before["ap"][ROW].tolist())
            seen_clear += int(c["strictly_inside_prev"] and c["bg_meets_prev"] > 0)
    assert seen_clear == 2


# ---- (d) the tracked sequence without the background fast path ------------------------------------------------------------------
def tracked_outputs(S):
    """What the child process of test (d) runs: the tracked sequence alone, outputs only."""
    return run_sequence(S, kinds=("tracked",), check_model=False, store=True)["outputs"]


def test_tracked_sequence_without_the_fast_path_gives_the_same_bits():
    lib = os.path.join(ROOT, "occlusionenv_amd", "libocc_hip_nocut.so")
    assert os.path.exists(lib), "run __graft_entry__.build() first"
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "nocut.pt")
        code = ("import sys, torch; sys.path.insert(0, %r); from tests import test_gpu_combine as T\n"
                "torch.save({S: T.tracked_outputs(S) for S in %r}, %r)\n" % (ROOT, STORED, path))
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OCC_HIP_LIB=lib), capture_output=True, text=True,
                             timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        ref = torch.load(path)
    for S in STORED:
        mine = _run(S)["outputs"]
        assert len(mine) == len(ref[S]) == n_steps(S)
        for t, (a, b) in enumerate(zip(mine, ref[S])):
            assert set(a) == set(b) == set(KEYS)
            for k in KEYS:
                assert torch.equal(a[k], b[k]), (S, t, k)
