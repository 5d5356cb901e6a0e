"""The intermediates of the step's forward-mode action gradient, directly against the f64 host model of
tests/setup_model.py: every used slot of the camera buffer (occ_camera.hpp: R, T, C, their tangents along el and az,
the action Jacobian, the f32 state update) in all three modes and from occ_step's prologue, and every slot of the face
records the setup kernel writes (occ_setup.hpp): positions in the oracle's vertex order, flags, the twelve tangents,
1 / area, the three 1 / |edge|^2 with their -1 sentinel, the two flat-shading terms, the unused slots.

Tolerances.  Camera: the kernel is f64 rounded once, so one f32 ulp of the f64 model (setup_model.camera_bound).
Tangents: not fixed in advance - the oracle's own chain under forward AD in FLOAT32 (the reference's precision) is run
beside the f64 one, and the engine may be at most GRAD_ORC32_FACTOR = 2 times as far from f64 as that, never held below
8 eps.  Derived slots: forward error bounds of their f32 formulas (see each check).  eps = 2^-24 throughout."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import p3d_restate as O
from tests import dense_meshes as D
from tests import setup_model as M
from tests.parity_utils import GRAD_ORC32_FACTOR, TVIEW, face_noise_bounds, make_case, run_engine

pytestmark = pytest.mark.gpu

EPS = M.EPS32
N_ROWS = 16


# ---- camera buffer --------------------------------------------------------------------------------------------------
def camera_rows():
    """16 rows: azimuths in all four quadrants, |el| up to 1.4, radii 0.8 / 2.5 / 4 / 30; actions: zero, axis-aligned,
    magnitudes 1e-3 and 1e3, the rest drawn."""
    rng = np.random.default_rng(45)
    n = N_ROWS
    az = np.array([0.3, 1.2, 2.0, 2.9, -0.4, -1.3, -2.2, -3.0, 0.9, 2.4, -0.8, -2.6, 1.5, -1.6, 3.1, 0.05], np.float32)
    el = np.array([0.0, 1.4, -1.4, 0.7, -0.7, 1.1, -1.1, 0.2, -0.3, 1.39, -1.39, 0.5, 0.9, -0.9, 0.0, 1.0], np.float32)
    radius = np.tile(np.array([0.8, 2.5, 4.0, 30.0], np.float32), n // 4)
    action = rng.normal(size=(n, 2)).astype(np.float32)
    action[0] = (0.0, 0.0)
    action[1], action[2], action[3], action[4] = (1.0, 0.0), (-1.0, 0.0), (0.0, 2.0), (0.0, -0.5)
    action[5] *= np.float32(1e-3) / np.linalg.norm(action[5])
    action[6] *= np.float32(1e3) / np.linalg.norm(action[6])
    action[7], action[8] = (1e-3, 0.0), (0.0, -1e3)
    return action, el, az, radius


def check_camera(mode, cam, el_out, az_out, pos_out, action, el, az, radius, label):
    """One camera buffer (n, 48) and its outputs against the model.  Returns the number of state rows (el AND az) that are
    bit-equal to the float32 two-step model; the others equal its contracted form (HIP contracts el + n0 * step into an
    FMA: DESIGN section 7)."""
    cam = np.asarray(cam, dtype=np.float32)
    n = cam.shape[0]
    own = M.camera(mode, action, el, az, radius)
    equal = n
    if mode == M.CAM_POSITION:
        assert not cam[:, M.C_EL:M.C_AZ + 1].any(), label
        want = own["cam"]
    else:
        # The state update: the float32 model rounds n0 * step and the sum (two roundings, like the reference's tensors); the
        # ENGINE IS FUSED - the gfx950 build contracts el + n0 * step (and a0 a0 + a1 a1) into FMAs, one rounding each.  A
        # row must be bit-equal to the two-step or to the contracted form, and within one ulp of the float32 model.  The
        # issue's "one f32 ulp" cannot be an ulp of the SUM for a fused engine: where the sum cancels, half an ulp of the
        # product is more than that (camera_rows' last row: az = 0.05 - 0.0398, the engine 2 ulps of the sum from the
        # two-step model).  The ulp is therefore taken where the two roundings differ, at the larger of |n0 * step| and
        # |el_new|; wherever the sum does not cancel that IS an ulp of the sum.
        fe, fa, nrm = M.state_update_fused32(action, el, az) if mode == M.CAM_STEP else (own["el_new"], own["az_new"], None)
        for got, mod, fus, k, name in ((el_out, own["el_new"], fe, 0, "el"), (az_out, own["az_new"], fa, 1, "az")):
            got = np.asarray(got, dtype=np.float32)
            assert ((got == mod) | (got == fus)).all(), (label, name, "neither the two-step nor the fused f32 update", got, mod, fus)
            prod = np.zeros(n, np.float32) if nrm is None else np.abs(nrm[:, k] * M.STEP32)
            ulp = np.spacing(np.maximum(np.abs(mod), prod).astype(np.float32)).astype(np.float64)
            dev = np.abs(got.astype(np.float64) - mod.astype(np.float64))
            assert (dev <= ulp).all(), (label, name, "state update more than one f32 ulp from the float32 model", got, mod)
        equal = int(((np.asarray(el_out, np.float32) == own["el_new"]) & (np.asarray(az_out, np.float32) == own["az_new"])).sum())
        print("%s: %d of %d state rows bit-equal to the contracted f32 model" % (
            label, int(((np.asarray(el_out, np.float32) == fe) & (np.asarray(az_out, np.float32) == fa)).sum()), n))
        if mode == M.CAM_LOOKAT:
            assert equal == n, (label, "a look-at camera does not move the state")
        assert np.array_equal(cam[:, M.C_EL], el_out) and np.array_equal(cam[:, M.C_AZ], az_out), label
        # every other slot at the ENGINE's updated angles: the ulp above does not propagate
        want = M.camera(mode, action, el, az, radius, at=(el_out, az_out))["cam"]
    assert M.off_pole(want).min() >= 1e-2, (label, "rows stay off the pole (it has tests of its own)")
    bound = M.camera_bound(want)
    err = np.abs(cam.astype(np.float64) - want)
    bad = err > bound
    assert not bad.any(), (label, [(int(r), int(s), float(cam[r, s]), float(want[r, s])) for r, s in np.argwhere(bad)[:8]])
    assert not cam[:, 45:].any(), label
    if mode != M.CAM_STEP:
        assert not cam[:, M.C_DR_EL:M.C_J + 4].any(), (label, "tangents and J of a camera that no action moves")
    if pos_out is not None:
        assert np.array_equal(np.asarray(pos_out, np.float32), cam[:, M.C_C:M.C_C + 3]), (label, "cam_pos_out is C")
    return equal


@pytest.mark.parametrize("mode", [M.CAM_STEP, M.CAM_LOOKAT, M.CAM_POSITION])
def test_camera_buffer_against_the_f64_model(mode):
    from occlusionenv_amd import _native as nat

    assert (nat.CAM_STEP, nat.CAM_LOOKAT, nat.CAM_POSITION, nat.CAM_STRIDE) == (M.CAM_STEP, M.CAM_LOOKAT, M.CAM_POSITION, M.CAM_STRIDE)
    assert (nat.C_R, nat.C_T, nat.C_C, nat.C_J, nat.C_EL, nat.C_AZ) == (M.C_R, M.C_T, M.C_C, M.C_J, M.C_EL, M.C_AZ)
    lib = nat.load()
    action, el, az, radius = camera_rows()
    n = N_ROWS
    if mode == M.CAM_POSITION:  # the centres of the look-at rows, and a few plain ones
        action = M.camera(M.CAM_LOOKAT, None, el, az, radius)["cam"][:, M.C_C:M.C_C + 3].astype(np.float32)
        action[:3] = [[1.0, 2.0, 3.0], [0.0, 0.0, 4.0], [-2.0, 0.5, -1.0]]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d_act, d_el, d_az, d_rad = dev(action), dev(el), dev(az), dev(radius)
    cam = torch.full((n, nat.CAM_STRIDE), 7.0, device="cuda")
    pos = torch.full((n, 3), 7.0, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if mode == M.CAM_POSITION:
        nat.check(lib.occ_camera(mode, p(d_act), None, None, None, p(cam), p(pos), n, st), "occ_camera")
    else:
        nat.check(lib.occ_camera(mode, p(d_act) if mode == M.CAM_STEP else None, p(d_el), p(d_az), p(d_rad), p(cam), p(pos), n, st),
                  "occ_camera")
    torch.cuda.synchronize()
    equal = check_camera(mode, cam.cpu().numpy(), d_el.cpu().numpy(), d_az.cpu().numpy(), pos.cpu().numpy(), action, el, az,
                         radius, "occ_camera mode %d" % mode)
    print("camera mode %d: %d of %d state rows bit-equal to the float32 model" % (mode, equal, n))


# ---- face records ---------------------------------------------------------------------------------------------------
def _set_elevation(eng):
    eng.elevation.copy_(torch.tensor([0.9, -0.9, 0.9][: eng.N], device=eng.elevation.device))


CASES = {
    "teapot_r4": dict(n_env=2, seed=0, mesh="teapot", radius=4.0, az_range=0.6),
    # (seed: of 40 tried on the host, the one that keeps the most z-clipped pieces visible)
    "teapot_r1.2_clipped": dict(n_env=2, seed=27, mesh="teapot", radius=1.2, az_range=0.3),
    "mixed_el0.9": dict(n_env=3, seed=6, mesh="mixed", radius=4.0, az_range=0.6, before_step=_set_elevation),
    "sheet4096_sorted": dict(n_env=D.SHEET_ENVS, seed=D.SHEET_SEED, mesh="sheet4096", radius=4.0, az_range=D.SHEET_AZ_RANGE),
}
_RUNS = {}


def _run(name):
    """One engine run per case (reset render + one step), shared by the tests of this module."""
    if name not in _RUNS:
        c = CASES[name]
        case = make_case(c["n_env"], c["seed"], c["mesh"], c["az_range"])
        el0 = torch.zeros(c["n_env"])
        if c.get("before_step"):
            el0 = torch.tensor([0.9, -0.9, 0.9][: c["n_env"]])
        got = run_engine(case, 64, radius=c["radius"], before_step=c.get("before_step"))
        _RUNS[name] = dict(case=case, got=got, cam=got["engine"].cam.cpu().numpy().copy(), el0=el0.numpy().astype(np.float32),
                           el=got["engine"].elevation.cpu().numpy().copy(), az=got["engine"].azimuth.cpu().numpy().copy(),
                           pos=got["engine"].camera_position.cpu().numpy().copy(), radius=c["radius"])
    return _RUNS[name]


def _world(case, i, o):
    mid = int(case["mesh_ids"][i, o])
    v, f = case["pool"].get(mid)
    return v.cpu() + case["offsets"][i, o], f.cpu()


def _model_cameras(run, phase):
    """f64 camera rows of every env: the step camera at the ENGINE's updated angles, or the reset (look-at) camera."""
    case, n = run["case"], run["cam"].shape[0]
    rad = np.full(n, run["radius"], np.float32)
    az0 = case["az"][:n].numpy().astype(np.float32)
    if phase == "step":
        return M.camera(M.CAM_STEP, case["actions"][:n].numpy(), run["el0"], az0, rad, at=(run["cam"][:, M.C_EL], run["cam"][:, M.C_AZ]))["cam"]
    return M.camera(M.CAM_LOOKAT, None, np.zeros(n, np.float32), az0, rad)["cam"]


def _model_records(run, cam64, i, o, dtype=torch.float64):
    c = cam64[i]
    w, f = _world(run["case"], i, o)
    R, T = torch.tensor(c[M.C_R:M.C_R + 9].reshape(3, 3)), torch.tensor(c[M.C_T:M.C_T + 3])
    dR = np.stack([c[M.C_DR_EL:M.C_DR_EL + 9].reshape(3, 3), c[M.C_DR_AZ:M.C_DR_AZ + 9].reshape(3, 3)])
    dT = np.stack([c[M.C_DT_EL:M.C_DT_EL + 3], c[M.C_DT_AZ:M.C_DT_AZ + 3]])
    m = M.records(w, f, R, T, dR, dT, c[M.C_C:M.C_C + 3], dtype=dtype)
    if dtype == torch.float64:
        m["bounds"] = face_noise_bounds(O.world_to_ndc(w.double(), R, T)[f])
    return m


def match_in_order(rec, model):
    """Model piece of every engine record (by id and half), positions compared vertex by vertex IN ORDER: the setup
    kernel claims the oracle's (p4, p5, p1), (p4, p2, p5), (p5, p2, p3), and the closest-edge tie order hangs on it.
    Bound per vertex: the view-space noise bound of the record's original face (face_noise_bounds), 2 TVIEW in depth."""
    piece, either = M.match_records(rec["ids"], rec["flags"], model)
    ev = rec["fv"].double().numpy()
    for j, cs in either.items():  # a half whose partner the engine culled: whichever piece it is
        piece[j] = min(cs, key=lambda c: float(np.abs(ev[j] - model["fv"][c]).max()))
    assert len(set(piece.tolist())) == piece.shape[0], "two records claim one oracle piece"
    mv = model["fv"][piece]
    b = model["bounds"][rec["ids"]]
    dxy = np.abs(ev[..., :2] - mv[..., :2]).reshape(len(piece), -1).max(1) if len(piece) else np.zeros(0)
    dz = np.abs(ev[..., 2] - mv[..., 2]).max(1) if len(piece) else np.zeros(0)
    bad = (dxy > b) | (dz > 2.0 * TVIEW)
    assert not bad.any(), ("record positions differ from the oracle's piece, vertex by vertex in order",
                           [(int(j), int(rec["ids"][j]), int(rec["flags"][j]), float(dxy[j] / b[j])) for j in np.nonzero(bad)[0][:6]])
    fl = rec["flags"]
    assert np.array_equal((fl & M.FLAG_CLIPPED) != 0, model["clipped"][piece]), "FLAG_CLIPPED"
    paired = (fl & 3) != 0
    assert np.array_equal((fl & 3)[paired], model["half"][piece][paired]), "pair flags"
    return piece


@pytest.mark.parametrize("name", list(CASES))
def test_step_prologue_camera_equals_the_model(name):
    """The same camera contract when the camera runs in occ_step's prologue: eng.cam after a step."""
    run = _run(name)
    case, n = run["case"], run["cam"].shape[0]
    equal = check_camera(M.CAM_STEP, run["cam"], run["el"], run["az"], run["pos"], case["actions"][:n].numpy(), run["el0"],
                         case["az"][:n].numpy(), np.full(n, run["radius"], np.float32), name)
    print("%s: %d of %d state rows bit-equal to the float32 model" % (name, equal, n))


@pytest.mark.parametrize("name", list(CASES))
def test_record_tangents_against_forward_ad_of_the_oracle(name):
    run = _run(name)
    n = run["cam"].shape[0]
    cam64 = _model_cameras(run, "step")
    e_eng = e_o32 = 0.0
    n_rec = n_clip = n_pair = 0
    for i in range(n):
        for o in range(3):
            rec = run["got"]["records"][3 * i + o]
            if name == "sheet4096_sorted":
                assert rec["ids"].shape[0] == 4096  # the sorted path (kSortMin <= nrec <= kSortCap): records are unaffected
            m64 = _model_records(run, cam64, i, o)
            m32 = _model_records(run, cam64, i, o, dtype=torch.float32)
            assert np.array_equal(m32["ids"], m64["ids"]) and np.array_equal(m32["half"], m64["half"])
            piece = match_in_order(rec, m64)
            if piece.shape[0] == 0:
                continue
            T = float(np.abs(m64["tan"]).max())
            e_eng = max(e_eng, float(M.tangent_distance(rec["tan"], m64["tan"][piece], T).max()))
            e_o32 = max(e_o32, float(M.tangent_distance(m32["tan"][piece], m64["tan"][piece], T).max()))
            n_rec += piece.shape[0]
            n_clip += int(((rec["flags"] & M.FLAG_CLIPPED) != 0).sum())
            n_pair += int(((rec["flags"] & 3) != 0).sum())
    bound = max(GRAD_ORC32_FACTOR * e_o32, 8 * EPS)
    print("%s: %d records (%d z-clipped, %d pair members): tangent distance from f64: engine %.3e, f32 oracle %.3e, bound %.3e"
          % (name, n_rec, n_clip, n_pair, e_eng, e_o32, bound))
    assert n_rec > 500
    if "clipped" in name:
        # (most of what the clip plane cuts at this camera is culled or off screen: a handful of records, of both kinds)
        assert n_pair >= 2 and n_clip > n_pair, "pair flags and FLAG_CLIPPED without a pair flag must both occur"
    else:
        assert n_clip == 0
    assert e_eng <= bound, (name, e_eng, e_o32)


@pytest.mark.parametrize("name", list(CASES))
def test_derived_record_slots(name):
    """1 / area, 1 / |edge|^2 and the sentinel from the record's OWN f32 positions; the flat-shading terms from the
    world-space face; the unused slots - on the records of the reset render and of the step."""
    run = _run(name)
    n = run["cam"].shape[0]
    worst = dict(area=0.0, il=0.0, amb=0.0, spec=0.0)
    n_vis = n_skip = n_sent = 0
    for phase, key in (("reset", "records0"), ("step", "records")):
        cam64 = _model_cameras(run, phase)
        if phase == "step":  # the engine shades with the f32 camera centre it stored
            cam64 = cam64.copy()
            cam64[:, M.C_C:M.C_C + 3] = run["cam"][:, M.C_C:M.C_C + 3].astype(np.float64)
        for i in range(n):
            for o in range(3):
                rec = run["got"][key][3 * i + o]
                raw = rec["raw"]
                if raw.shape[0] == 0:
                    continue
                d = M.derived(rec["fv"].numpy())
                # forward error bound of a 2x2 determinant of differences (4 eps on the products' magnitudes) plus the
                # addition of kEpsilon and the division (2 eps on the result)
                got_area = 1.0 / raw[:, M.R_INV_AREA].astype(np.float64)
                err = np.abs(got_area - d["area"])
                lim = 4 * EPS * d["det_mag"] + 2 * EPS * np.abs(d["area"])
                assert (err <= lim).all(), (name, phase, i, o, "1 / R_INV_AREA", float((err / lim).max()))
                worst["area"] = max(worst["area"], float((err / lim).max()))
                il = raw[:, [M.R_IL01, M.R_IL02, M.R_IL12]].astype(np.float64)
                l2 = d["l2"]
                must = l2 <= M.KEPS * (1 - 8 * EPS)
                must_not = l2 >= M.KEPS * (1 + 8 * EPS)
                assert (il[must] == -1.0).all() and (il[must_not] != -1.0).all(), (name, phase, i, o, "sentinel")
                reg = il != -1.0
                rel = np.abs(il[reg] * l2[reg] - 1.0)
                assert (rel <= 8 * EPS).all(), (name, phase, i, o, "R_IL", float(rel.max()))
                worst["il"] = max(worst["il"], float(rel.max()) if rel.size else 0.0)
                n_sent += int((~reg).sum())
                assert not raw[:, 13:16].any(), (name, phase, i, o, "slots 13..15")
                # the shading terms of the ORIGINAL face
                w, f = _world(run["case"], i, o)
                amb, spec, cosang = M.flat_terms(w, f, cam64[i, M.C_C:M.C_C + 3])
                ids = rec["ids"]
                keep = np.abs(cosang[ids]) >= 1e-6  # the specular gate (n.l > 0) can flip there
                n_vis += ids.shape[0]
                n_skip += int((~keep).sum())
                ea = np.abs(raw[:, M.R_AMB].astype(np.float64) - amb[ids])[keep]
                es = np.abs(raw[:, M.R_SPEC].astype(np.float64) - spec[ids])[keep]
                worst["amb"] = max(worst["amb"], float(ea.max()) if ea.size else 0.0)
                worst["spec"] = max(worst["spec"], float(es.max()) if es.size else 0.0)
                assert (ea <= 1e-5).all() and (es <= 1e-5).all(), (name, phase, i, o, "R_AMB / R_SPEC", worst)
    print("%s: %d records, %d sentinel edges, %d skipped at the specular gate; worst: 1/area %.3f of its bound, "
          "1/|edge|^2 %.2f eps, amb+diff %.2e, spec %.2e" % (name, n_vis, n_sent, n_skip, worst["area"], worst["il"] / EPS,
                                                              worst["amb"], worst["spec"]))
    assert n_vis > 1000 and n_skip <= 1e-3 * n_vis
