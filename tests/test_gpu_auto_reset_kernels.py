"""The device auto-reset ABI (occ_step_flags, occ_reset_commit, occ_auto_reset, occ_object_mass, occ_reserve_refill)
against the host model of its contract (tests/reset_model.py), called directly through ctypes: no rendering.  Every
buffer starts with seeded random bits and runs GUARD words past what the ABI names, so rows the call must leave alone
act as canaries; every buffer is compared whole and bit for bit.  At the end, the same path end to end through
SimpleVecEnv at the size where its limits bind (N = 2048, R = 512), and the normWithObjectSize flag set after the
reserve is warm."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import reset_model as M

pytestmark = pytest.mark.gpu

GUARD = 64
F32_01 = np.float32(0.1)
ABOVE = np.nextafter(F32_01, np.float32(1))
BELOW = np.nextafter(F32_01, np.float32(0))
SLOT_LOSSES = np.array([0.0, 0.05, BELOW, F32_01, ABOVE, 0.3, 0.9, 7.5], np.float32)


@pytest.fixture(scope="module")
def lib():
    from occlusionenv_amd import _native as nat

    return nat.load()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sizes(N, R, img):
    NT, S2 = N + R, img * img
    return dict(done=N, loss_all=NT, status=NT, rs_state=R, rs_tries=R, el=NT, az=NT, radius=NT, campos=3 * N,
                cam=M.CAM_STRIDE * NT, alphas=3 * S2 * NT, full_reward=N, object_mass=N, scene_mesh=3 * NT,
                scene_offset=9 * NT, obs_all=4 * S2 * NT, full_state_all=4 * S2 * NT, store_obs=4 * S2 * R,
                store_fs=4 * S2 * R, store_loss=R, skip=NT, term_obs=4 * S2 * R, report=N + 2 * R + 2, pairs=2 + 3 * R,
                age=N, rect=4 * NT, arect=4 * NT, reset_full_state=4 * S2 * R, norm_flags=N, slot_objsum=R)


_INT = ("status", "rs_state", "rs_tries", "scene_mesh", "skip", "report", "pairs", "age", "rect", "arect", "norm_flags")


def _random_buffers(N, R, img, seed):
    """Every buffer of the call (GUARD extra words each) filled with random bits on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = {}
    for k, n in _sizes(N, R, img).items():
        if k == "done":
            out[k] = torch.randint(0, 256, (n + GUARD,), dtype=torch.uint8, device="cuda", generator=g)
            continue
        b = torch.randint(-2 ** 31, 2 ** 31 - 1, (n + GUARD,), dtype=torch.int32, device="cuda", generator=g)
        out[k] = b if k in _INT else b.view(torch.float32)
    return out


def _put(buf, values):
    """Write the ABI part of a flat device buffer from host values (the guard stays as it is)."""
    dt = {torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8}[buf.dtype]
    v = torch.from_numpy(np.ascontiguousarray(np.asarray(values).reshape(-1)).view(dt))
    buf[:v.numel()].copy_(v.to(buf.device))


def _same_bits(name, got, want):
    g, w = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert g.shape == w.shape, name
    gb, wb = g.view(np.uint8 if g.dtype.itemsize == 1 else np.int32), w.view(np.uint8 if w.dtype.itemsize == 1 else np.int32)
    if not np.array_equal(gb, wb):
        bad = np.nonzero(gb != wb)[0]
        raise AssertionError(f"{name}: {bad.size} words differ, first at {bad[:8].tolist()}: got {g[bad[:4]].tolist()} "
                             f"want {w[bad[:4]].tolist()}")


def _controls(kind, N, R, rng):
    """Host-side inputs that make up a scenario: done, slot states / tries / losses, status words, ages."""
    NT = N + R
    c = dict(done=np.zeros(N, np.uint8), status=np.zeros(NT, np.int32), rs_state=rng.integers(0, 3, R).astype(np.int32),
             rs_tries=rng.integers(0, 10, R).astype(np.int32), slot_loss=rng.choice(SLOT_LOSSES, R),
             age=rng.integers(0, 1000, N).astype(np.int32), max_ep_len=0)

    def finish(idx):
        c["done"][idx] = rng.choice(np.array([1, 255], np.uint8), np.size(idx))

    if kind == "no_ready":
        c["rs_state"] = rng.integers(0, 2, R).astype(np.int32)
        c["rs_tries"] = rng.integers(0, 9, R).astype(np.int32)
        c["slot_loss"] = rng.choice(np.array([0.0, 0.05, BELOW, F32_01], np.float32), R)
        finish(np.nonzero(rng.random(N) < 0.3)[0])
        finish([N - 1])
    elif kind == "fin_lt_ready":
        c["rs_state"][rng.random(R) < 0.8] = M.RS_READY
        nfin = max(1, int((c["rs_state"] == M.RS_READY).sum()) // 2)
        finish(rng.choice(N, min(nfin, N), replace=False))
    elif kind == "fin_gt_ready":
        c["rs_state"] = np.where(rng.random(R) < 0.25, M.RS_READY, M.RS_EMPTY).astype(np.int32)
        finish(np.nonzero(rng.random(N) < 0.6)[0])
        finish(rng.choice(N, min(N, R + 1), replace=False))
    elif kind == "over_512":
        c["rs_state"][:] = M.RS_READY
        finish(np.nonzero(rng.random(N) < 0.7)[0])
    elif kind == "all":
        c["rs_state"][:] = M.RS_READY
        finish(np.arange(N))
    elif kind == "time_limit":
        c["max_ep_len"] = 40
        c["age"] = rng.integers(36, 40, N).astype(np.int32)  # 39 + 1 reaches the limit
        finish(np.nonzero(rng.random(N) < 0.2)[0])
        c["age"][N - 1] = 39
        finish([N - 1])  # done and at the limit in the same step
    elif kind == "status_reserve":
        c["status"][N + rng.integers(R)] = int(rng.integers(1, 2 ** 31))
        finish(np.nonzero(rng.random(N) < 0.1)[0])
    elif kind != "none":
        raise ValueError(kind)
    # a NaN loss is a rejection: only on slots whose try is not the 10th (object_mass would carry a NaN bit pattern)
    nan = (c["rs_state"] == M.RS_PENDING) & (c["rs_tries"] < 8) & (rng.random(R) < 0.1)
    c["slot_loss"][nan] = np.nan
    return c


def _call_auto_reset(lib, b, N, R, img, opts_on, max_ep_len, report_host):
    from occlusionenv_amd import _native as nat

    st = nat.OccEnvState()
    for f in ("el", "az", "radius", "campos", "cam", "alphas", "full_reward", "object_mass", "scene_mesh", "scene_offset"):
        setattr(st, f, b[f].data_ptr())
    store = nat.OccReserveStore()
    store.obs, store.full_state, store.loss, store.skip = (b["store_obs"].data_ptr(), b["store_fs"].data_ptr(),
                                                           b["store_loss"].data_ptr(), b["skip"].data_ptr())
    opts = None
    if opts_on:
        opts = nat.OccAutoResetOpts()
        for f in opts_on:
            setattr(opts, f, (report_host if f == "report_host" else b[f]).data_ptr())
        opts.max_ep_len = int(max_ep_len)
    rc = lib.occ_auto_reset(_p(b["done"]), _p(b["loss_all"]), _p(b["status"]), N, R, _p(b["rs_state"]), _p(b["rs_tries"]),
                            C.byref(st), _p(b["obs_all"]), _p(b["full_state_all"]), C.byref(store), _p(b["term_obs"]), img,
                            _p(b["pairs"]), _p(b["report"]), None if opts is None else C.byref(opts), _stream())
    nat.check(rc, "occ_auto_reset")


OPT_SETS = {
    "none": (),
    "all": ("age", "rect", "arect", "reset_full_state", "norm_flags", "slot_objsum", "report_host"),
    "some": ("age", "reset_full_state", "report_host"),
}


def _run_and_compare(lib, b, host, N, R, img, opts_on, max_ep_len):
    """One occ_auto_reset call on the device buffers ``b`` against the model on ``host`` (the same contents); returns
    the model's result (= the device state afterwards)."""
    rh = None
    if "report_host" in opts_on:
        rh = torch.empty(N + 2 * R + 2 + GUARD, dtype=torch.int32).pin_memory()
        rh.copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, rh.shape, dtype=torch.int32))
        rh[:N] = 0  # the contract: zero on entry
        host = dict(host, report_host=rh.numpy().copy())
    _call_auto_reset(lib, b, N, R, img, opts_on, max_ep_len, rh)
    torch.cuda.synchronize()
    model_in = {k: v for k, v in host.items() if k in M.AUTO_RESET_BUFFERS or k in opts_on or k == "pairs"}
    want = M.auto_reset(model_in, N, R, img, max_ep_len=max_ep_len if "age" in opts_on else 0)
    for k, v in b.items():
        if k == "pairs":  # scratch: nothing is promised about its contents, only that the call stays inside it
            _same_bits(k + " past its 2 + 3R words", v.cpu().numpy()[2 + 3 * R:], host[k][2 + 3 * R:])
            continue
        _same_bits(k, v.cpu().numpy(), want[k] if k in want else host[k])
    if rh is not None:
        _same_bits("report_host", rh.numpy(), want["report_host"])
    return want


def _apply_controls(b, host, c, N, R, rng):
    la = host["loss_all"].copy()
    la[N:N + R] = c["slot_loss"]
    new = dict(done=c["done"], status=c["status"], rs_state=c["rs_state"], rs_tries=c["rs_tries"], age=c["age"],
               loss_all=la[:N + R],
               # losses the store and the reset rows may carry: finite, so that loss + 1 is a number
               store_loss=rng.choice(SLOT_LOSSES, R), slot_objsum=rng.uniform(0, 5000, R).astype(np.float32),
               norm_flags=rng.integers(0, 2, N).astype(np.int32))
    for k, v in new.items():
        _put(b[k], v)
        host[k][:np.size(v)] = np.asarray(v).reshape(-1).view(host[k].dtype)


SHAPES = [(1, 1, 8), (16, 4, 64), (1000, 250, 24), (1024, 256, 128), (1025, 512, 8), (3000, 512, 16)]
KINDS = ["none", "no_ready", "fin_lt_ready", "fin_gt_ready", "over_512", "all", "time_limit", "status_reserve"]


@pytest.mark.parametrize("N,R,img", SHAPES, ids=[f"N{n}-R{r}-S{s}" for n, r, s in SHAPES])
def test_auto_reset_matches_the_model(lib, N, R, img):
    base = _random_buffers(N, R, img, seed=N * 7 + R)
    base_host = {k: v.cpu().numpy() for k, v in base.items()}
    rng = np.random.default_rng(N + 1000 * R + img)
    kinds = [k for k in KINDS if k != "over_512" or N >= 1025]
    seen = set()
    for j, kind in enumerate(kinds):
        opts_on = OPT_SETS[("all", "none", "some")[j % 3]]
        if kind == "time_limit" and "age" not in opts_on:
            opts_on = OPT_SETS["some"]
        b = {k: v.clone() for k, v in base.items()}
        host = {k: v.copy() for k, v in base_host.items()}
        c = _controls(kind, N, R, rng)
        _apply_controls(b, host, c, N, R, rng)
        want = _run_and_compare(lib, b, host, N, R, img, opts_on, c["max_ep_len"])
        rep = want["report"]
        nfin, left = int(np.count_nonzero(rep[:N])), int(rep[N + 2 * R + 1])
        seen.add((kind, nfin, nfin - left))
        if kind == "over_512":
            assert nfin > 512 and nfin - left == R == 512
        if kind == "all":
            assert nfin == N and nfin - left == min(N, R)
        if kind == "status_reserve":
            assert rep[N + 2 * R] == 1 and not c["status"][:N].any()
        if kind == "time_limit":
            assert rep[N - 1] == 1 and ((rep[:N] == 2).any() or N == 1)
    print(sorted(seen))


def test_auto_reset_life_cycle_with_refills(lib):
    """Ten calls with the state carried over: fresh renders and losses each step, EMPTY slots refilled in between (from
    device memory and from pinned host rows, plus rows that must change nothing).  Slot 0 keeps failing the acceptance
    test until its 10th try is kept."""
    from occlusionenv_amd import _native as nat

    for N, R, img in ((40, 10, 16), (1500, 512, 8)):
        NT, S2 = N + R, img * img
        rng = np.random.default_rng(N)
        b = _random_buffers(N, R, img, seed=N)
        host = {k: v.cpu().numpy() for k, v in b.items()}
        st = rng.integers(0, 3, R).astype(np.int32)
        tries = rng.integers(0, 9, R).astype(np.int32)
        st[0], tries[0] = M.RS_PENDING, 5
        init = dict(rs_state=st, rs_tries=tries, age=rng.integers(0, 30, N).astype(np.int32),
                    store_loss=rng.choice(SLOT_LOSSES, R), slot_objsum=rng.uniform(0, 100, R).astype(np.float32),
                    norm_flags=rng.integers(0, 2, N).astype(np.int32), status=np.zeros(NT, np.int32))
        for k, v in init.items():
            _put(b[k], v)
            host[k][:np.size(v)] = v.view(host[k].dtype)
        tenth = taken_same_call = taken = 0
        for call in range(10):
            # what the step's render would leave: every row of obs_all / full_state_all / loss_all, alphas of rendered rows
            fresh = dict(obs_all=rng.integers(-2 ** 31, 2 ** 31 - 1, 4 * S2 * NT).astype(np.int32).view(np.float32),
                         full_state_all=rng.integers(-2 ** 31, 2 ** 31 - 1, 4 * S2 * NT).astype(np.int32).view(np.float32),
                         done=(rng.random(N) < 0.15).astype(np.uint8))
            la = rng.uniform(0, 1, NT).astype(np.float32)
            la[N:] = rng.choice(SLOT_LOSSES, R)
            la[N] = 0.05  # slot 0: rejected until its 10th try
            fresh["loss_all"] = la
            al = host["alphas"][:3 * S2 * NT].reshape(NT, 3 * S2).copy()
            rendered = host["skip"][:NT] == 0
            al[rendered] = rng.uniform(0, 1, (int(rendered.sum()), 3 * S2)).astype(np.float32)
            fresh["alphas"] = al
            for k, v in fresh.items():
                _put(b[k], v)
                host[k][:np.size(v)] = np.asarray(v).reshape(-1)
            before = host["rs_state"][:R].copy(), host["rs_tries"][:R].copy()
            want = _run_and_compare(lib, b, host, N, R, img, OPT_SETS["all"], 30)
            host = {k: (want[k] if k in want else host[k]) for k in host}
            assign = want["report"][N + R:N + 2 * R]
            taken += int((assign >= 0).sum())
            taken_same_call += int(((assign >= 0) & (before[0] == M.RS_PENDING)).sum())
            tenth += int(((before[0] == M.RS_PENDING) & (before[1] == 9) & ~(la[N:] > F32_01)).sum())
            # refill the EMPTY slots; rows for slot -1 and slots >= R change nothing
            empty = np.nonzero(host["rs_state"][:R] == M.RS_EMPTY)[0]
            rows = np.zeros((len(empty) + 3, 13), np.int32)
            rows[:len(empty), 0] = empty
            rows[len(empty):, 0] = [-1, R, R + 7]
            rows[:, 1:4] = rng.integers(0, 1000, (len(rows), 3))
            rows[:, 4:] = rng.integers(-2 ** 31, 2 ** 31 - 1, (len(rows), 9))
            rows[0, 4:7] = np.array([0x80000000, 0x7FC12345, 0xFFA00001], np.uint32).view(np.int32)  # -0.0, NaN payloads
            rows = rows[rng.permutation(len(rows))]
            if call % 2:
                packed = torch.from_numpy(rows).pin_memory()
            else:
                packed = torch.from_numpy(rows).cuda()
            nat.check(lib.occ_reserve_refill(_p(packed), len(rows), N, R, _p(b["scene_mesh"]), _p(b["scene_offset"]),
                                             _p(b["rs_state"]), _p(b["skip"]), _stream()), "occ_reserve_refill")
            torch.cuda.synchronize()
            mesh, off, rs, sk = M.reserve_refill(rows, len(rows), N, R, host["scene_mesh"], host["scene_offset"],
                                                 host["rs_state"], host["skip"])
            for k, v in (("scene_mesh", mesh), ("scene_offset", off), ("rs_state", rs), ("skip", sk)):
                _same_bits(f"refill {k}", b[k].cpu().numpy(), v)
                host[k] = v
        assert tenth >= 1 and taken >= 1 and taken_same_call >= 1, (tenth, taken, taken_same_call)


def test_reserve_refill_leaves_rows_outside_the_reserve(lib):
    from occlusionenv_amd import _native as nat

    N, R = 3, 2
    b = _random_buffers(N, R, 8, seed=9)
    host = {k: v.cpu().numpy() for k, v in b.items()}
    rows = np.zeros((3, 13), np.int32)
    rows[:, 0] = [-1, R, 2 ** 30]
    rows[:, 1:] = 5
    packed = torch.from_numpy(rows).cuda()
    nat.check(lib.occ_reserve_refill(_p(packed), 3, N, R, _p(b["scene_mesh"]), _p(b["scene_offset"]), _p(b["rs_state"]),
                                     _p(b["skip"]), _stream()), "occ_reserve_refill")
    assert lib.occ_reserve_refill(None, 0, N, R, None, None, None, None, _stream()) == 0
    torch.cuda.synchronize()
    for k in ("scene_mesh", "scene_offset", "rs_state", "skip"):
        _same_bits(k, b[k].cpu().numpy(), host[k])


@pytest.mark.parametrize("N,R", [(1, 0), (200, 55), (256, 0), (1, 256), (1024, 256), (3000, 512)])
def test_step_flags_match_the_model(lib, N, R):
    NT = N + R
    rng = np.random.default_rng(NT)
    done = torch.from_numpy((rng.random(N + GUARD) < 0.3).astype(np.uint8)).cuda()
    la = rng.choice(np.array([0.0, 0.05, BELOW, F32_01, ABOVE, 0.5, np.nan], np.float32), NT + GUARD)
    la[N:N + min(R, 3)] = [F32_01, ABOVE, BELOW][:min(R, 3)]
    loss = torch.from_numpy(la).cuda()
    from occlusionenv_amd import _native as nat

    for status_case in ("zero", "last", "guard_only"):
        st = np.zeros(NT + GUARD, np.int32)
        if status_case == "last":
            st[NT - 1] = 1 << 30
        elif status_case == "guard_only":
            st[NT:] = 3  # past the n_env + n_reserve words: not the call's
        status = torch.from_numpy(st).cuda()
        for with_loss in ((False, True) if R == 0 else (True,)):
            flags = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31 - 1, NT + 1 + GUARD).astype(np.int32)).cuda()
            before = flags.cpu().numpy()
            nat.check(lib.occ_step_flags(_p(done), _p(loss) if with_loss else None, _p(status), N, R, _p(flags), _stream()),
                      "occ_step_flags")
            torch.cuda.synchronize()
            want = before.copy()
            want[:NT + 1] = M.step_flags(done.cpu().numpy(), la, st, N, R)
            assert want[NT] == (1 if status_case == "last" else 0)
            _same_bits(f"flags {status_case}", flags.cpu().numpy(), want)


def test_reset_commit_matches_the_model(lib):
    from occlusionenv_amd import _native as nat

    N, R, img = 300, 100, 24
    NT, S2 = N + R, img * img
    b = _random_buffers(N, R, img, seed=31)
    b["obs"] = _random_buffers(N, 0, img, seed=32)["obs_all"]  # (N rows): the commit's destination
    g = torch.Generator(device="cuda").manual_seed(33)
    b["loss_all"][:NT] = torch.rand(NT, device="cuda", generator=g)
    rng = np.random.default_rng(34)
    n = 80
    pairs = np.stack([rng.choice(N, n, replace=False), rng.integers(N, NT, n)], 1).astype(np.int32).reshape(-1)
    pairs_d = torch.from_numpy(np.concatenate([pairs, np.full(GUARD, -1, np.int32)])).cuda()
    host = {k: v.cpu().numpy() for k, v in b.items()}
    names = ("el", "az", "radius", "campos", "cam", "alphas", "full_reward", "object_mass", "scene_mesh", "scene_offset",
             "obs")
    rc = lib.occ_reset_commit(_p(pairs_d), n, *[_p(b[k]) for k in names], _p(b["obs_all"]), _p(b["loss_all"]), img, _stream())
    nat.check(rc, "occ_reset_commit")
    torch.cuda.synchronize()
    want = M.reset_commit(pairs, n, *[host[k] for k in names], host["obs_all"], host["loss_all"], img)
    for k in b:
        _same_bits(k, b[k].cpu().numpy(), want[k] if k in want else host[k])
    assert lib.occ_reset_commit(None, 0, *([None] * 13), img, _stream()) == 0


@pytest.mark.parametrize("img", [8, 24, 64, 72, 128, 512])
def test_object_mass_against_a_float64_sum(lib, img):
    from occlusionenv_amd import _native as nat

    S2 = img * img
    n = min(3000, max(16, 2 ** 24 // (3 * S2)))
    g = torch.Generator(device="cuda").manual_seed(img)
    al = torch.rand(n, 3, img, img, device="cuda", generator=g)
    al[0] = 0.0
    al[1] = 1.0
    out = torch.empty(n + GUARD, device="cuda")
    out2 = torch.empty(n + GUARD, device="cuda")
    out[n:] = out2[n:] = -3.0
    for o in (out, out2):
        nat.check(lib.occ_object_mass(_p(al), n, img, None, 0, _p(o), _stream()), "occ_object_mass")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    _same_bits("two calls", got, out2.cpu().numpy())
    assert (got[n:] == -3.0).all()
    ref = M.object_mass(al.cpu().numpy(), n, img)
    assert got[0] == 0.0 and got[1] == 9.0 * S2
    err = np.abs(got[:n].astype(np.float64) - ref)
    bound = M.object_mass_bound(ref, img)
    ratio = float(np.max(err[2:] / bound[2:]))
    print(f"img {img}, {n} rows: worst |got - ref| / bound = {ratio:.4f}")
    assert (err <= bound).all(), np.nonzero(err > bound)[0][:8]
    # gated rows keep what out holds, bit for bit; the others get the ungated value
    rng = np.random.default_rng(img)
    gate = torch.from_numpy(rng.integers(0, 3, n).astype(np.int32)).cuda()
    prev = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31 - 1, n + GUARD).astype(np.int32)).cuda().view(torch.float32)
    before = prev.cpu().numpy()
    nat.check(lib.occ_object_mass(_p(al), n, img, _p(gate), 1, _p(prev), _stream()), "occ_object_mass")
    torch.cuda.synchronize()
    want = before.copy()
    on = gate.cpu().numpy() == 1
    want[:n][on] = got[:n][on]
    _same_bits("gated", prev.cpu().numpy(), want)


# ---- end to end: SimpleVecEnv ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ds():
    from occlusionenv_amd.meshes import SyntheticShapeNet

    return SyntheticShapeNet(n_models=8, seed=1234)


def _push_apart(eng, envs):
    idx = torch.as_tensor(list(envs), dtype=torch.long, device=eng.device)
    off = eng.scene_offset[idx].clone()
    off[:, 1, 0], off[:, 2, 0] = 50.0, -50.0  # no occlusion left: these envs finish in the next step
    eng.scene_offset[idx] = off


def test_auto_reset_at_the_reserve_cap(ds):
    """N = 2048 -> R = 512: more than 512 envs finish in one step.  The first 512 (index order) take slots 0..511 in order
    on the device, the rest go through the synchronous fallback; every reset env holds exactly its new scene's render."""
    from occlusionenv_amd import environment
    from environment import OcclusionEnv
    from SubProcVecEnv import SimpleVecEnv

    environment.seed_scene_rng(2048)
    np.random.seed(2048)
    N, S = 2048, 64
    try:
        venv = SimpleVecEnv([lambda: OcclusionEnv(ds, img_size=S) for _ in range(N)])
        eng = venv.engine
        assert eng.R == 512
        az0 = (torch.rand(N, generator=torch.Generator().manual_seed(3)) * 2 - 1) * 0.6
        venv._reset_envs(list(range(N)), az0)
        venv._warm_reserve()
        # one step in which (almost) nothing finishes: the slots that stay READY are skipped by its render
        venv.step(torch.zeros(N, 2, device="cuda"))
        venv._drain()
        ready_before = (eng.rs_state == 2).cpu().numpy()
        venv._warm_reserve()  # every slot READY again
        assert eng.rs_state.tolist() == [2] * 512
        slot_scene = list(venv._rs_scene)
        push = sorted(np.random.default_rng(5).choice(N, 600, replace=False).tolist())
        _push_apart(eng, push)
        pre_cam = (eng.azimuth.clone(), eng.elevation.clone(), eng.radius.clone())
        pushed_off = eng.scene_offset.cpu().numpy()
        pushed_ids = [venv.envs[i]._scene[0] for i in range(N)]
        obs, rewards, dones, infos = venv.step(torch.zeros(N, 2, device="cuda"))
        fin = torch.nonzero(dones).reshape(-1).tolist()
        assert set(push) <= set(fin) and len(fin) > 512
        assert eng.rs_state.tolist() == [0] * 512  # every slot taken, none refilled yet
        term = {i: infos[i]["terminal_observation"] for i in fin}  # reading infos runs the host's share (fallback, refill)
        assert eng.rs_state.tolist() == [1] * 512
        slot_envs, rest = fin[:512], fin[512:]
        for k, i in enumerate(slot_envs):
            assert venv.envs[i]._scene is slot_scene[k], (k, i)
        for i in rest:
            assert venv.envs[i]._scene is not slot_scene[0] and all(venv.envs[i]._scene is not s for s in slot_scene)
        # every reset env against a batched render of its new scene with the reset() camera
        ids = [venv.envs[i]._scene[0] for i in fin]
        offs = np.stack([np.asarray(venv.envs[i]._scene[1], np.float32) for i in fin])
        ref = eng.evaluate_scenes(ids, offs, 4.0, 0.0, 0.0)
        fi = torch.as_tensor(fin, device="cuda")
        assert torch.equal(obs[fi], ref["obs"])
        assert torch.equal(eng.full_reward[fi], ref["loss"])
        assert torch.equal(eng.object_mass[fi], ref["loss"] + 1.0)
        assert torch.equal(eng.alphas[fi], ref["alphas"])
        assert torch.equal(eng.azimuth[fi], torch.zeros(len(fin), device="cuda"))
        assert float(eng.camera_position[fi].abs().sum()) == 0.0
        assert any(ready_before[k] for k in range(512)), "no slot stayed READY through a step"
        # the terminal observation: the step's render of the pushed scene from the env's camera (zero action, el = 0: the
        # step's camera is the reset() camera of the same angles)
        tref = eng.evaluate_scenes([pushed_ids[i] for i in fin], pushed_off[fin], pre_cam[2][fi], pre_cam[0][fi], pre_cam[1][fi])
        got = torch.cat([term[i] for i in fin])
        assert torch.allclose(got, tref["obs"], atol=1e-4, rtol=0), float((got - tref["obs"]).abs().max())
        eng.check_status()
    finally:
        environment.seed_scene_rng(None)


def test_norm_with_object_size_set_after_the_reserve_is_warm(ds):
    """normWithObjectSize switched on after reset(): the READY slots were stored while no env had the flag, so their
    silhouette mass must be computed when the flag goes on (an env taking such a slot got object_mass = 0 + 1)."""
    from occlusionenv_amd import environment
    from environment import OcclusionEnv
    from SubProcVecEnv import SimpleVecEnv

    environment.seed_scene_rng(16)
    np.random.seed(16)
    N, S = 16, 64
    try:
        venv = SimpleVecEnv([lambda: OcclusionEnv(ds, img_size=S) for _ in range(N)])
        eng = venv.engine
        venv._reset_envs(list(range(N)), torch.zeros(N))
        venv._warm_reserve()
        def settle():  # step until every slot is READY again (taken slots are refilled and tested on the device)
            for _ in range(12):
                venv.step(torch.zeros(N, 2, device="cuda"))
                venv._drain()
                if eng.rs_state.tolist() == [2] * eng.R:
                    return
            raise AssertionError(f"reserve not READY: {eng.rs_state.tolist()}")

        def mass(i):
            return float((eng.alphas[i].sum(0) ** 2).sum()) + 1.0

        def finish(i):
            slot_scene = list(venv._rs_scene)
            _push_apart(eng, [i])
            _, _, dones, _ = venv.step(torch.zeros(N, 2, device="cuda"))
            venv._drain()
            assert bool(dones[i]) and any(venv.envs[i]._scene is s for s in slot_scene), "not reset from the reserve"

        # one slot is taken and comes back to READY through the device path, every flag still off
        finish(0)
        settle()
        venv.set_attr("normWithObjectSize", True, indices=[3])
        finish(3)
        assert float(eng.object_mass[3]) != 1.0
        assert float(eng.object_mass[3]) == pytest.approx(mass(3), rel=1e-5)
        # off again: slots refilled meanwhile become READY while no env has the flag
        venv.set_attr("normWithObjectSize", False, indices=[3])
        settle()
        for on in (True, False, True):
            venv.set_attr("normWithObjectSize", on, indices=[5])
        finish(5)
        assert float(eng.object_mass[5]) != 1.0
        assert float(eng.object_mass[5]) == pytest.approx(mass(5), rel=1e-5)
        finish(7)  # flag off: loss + 1
        assert float(eng.object_mass[7]) == float(eng.full_reward[7]) + 1.0
        eng.check_status()
    finally:
        environment.seed_scene_rng(None)
