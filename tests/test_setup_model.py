"""Host tests of tests/setup_model.py, the f64 model the GPU tests of tests/test_gpu_setup_records.py hold the camera
and setup kernels to: closed-form cameras, finite differences where they are valid (unclipped faces), hand-worked
z-clipped pieces with the detached cut weight, the action Jacobian, a hand-computed shaded face."""
import math

import numpy as np
import pytest
import torch

from oracle import p3d_restate as O
from tests import setup_model as M


def _cam(mode, action, el, az, radius, **kw):
    return M.camera(mode, np.asarray(action, np.float32), np.asarray(el, np.float32), np.asarray(az, np.float32),
                    np.asarray(radius, np.float32), **kw)


def test_slot_maps_are_those_of_occ_constants_h():
    import os
    import re

    from tests.parity_utils import ROOT

    text = open(os.path.join(ROOT, "occlusionenv_amd", "csrc", "occ_constants.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"\b((?:C|R|FLAG)_[A-Z0-9_]+) = (\d+)", text)}
    for name in ("C_R", "C_T", "C_C", "C_DR_EL", "C_DT_EL", "C_DR_AZ", "C_DT_AZ", "C_J", "C_EL", "C_AZ", "R_INV_AREA", "R_AMB",
                 "R_IL01", "R_IL02", "R_IL12", "R_SPEC", "R_TAN", "FLAG_PAIR_FIRST", "FLAG_PAIR_SECOND", "FLAG_CLIPPED"):
        assert consts[name] == getattr(M, name), name
    assert sorted(M.CAM_GROUPS.values()) == [(0, 9), (9, 12), (12, 15), (15, 24), (24, 27), (27, 36), (36, 39), (39, 43)]
    assert re.search(r"kEpsilon = 1e-8f", text) and re.search(r"kStepSize = 0.05f", text)


def test_closed_form_cameras():
    half_pi = np.float32(math.pi / 2)
    # step()'s convention, no action: az = pi/2, el = 0 puts C on +X; az = 0 on +Z whatever el is
    c = _cam(M.CAM_STEP, [[0, 0], [0, 0]], [0.0, 0.7], [half_pi, 0.0], [2.5, 4.0])["cam"]
    assert np.allclose(c[0, M.C_C:M.C_C + 3], [2.5, 0, 0], atol=2.5e-7)  # (f32 pi/2)
    assert np.allclose(c[1, M.C_C:M.C_C + 3], [0, 0, 4.0], atol=1e-15)
    # C = (0, 0, r) => x = (-1, 0, 0), y = (0, 1, 0), z = (0, 0, -1), T = (0, 0, r)
    assert np.allclose(c[1, M.C_R:M.C_R + 9].reshape(3, 3), np.diag([-1.0, 1.0, -1.0]), atol=1e-15)
    assert np.allclose(c[1, M.C_T:M.C_T + 3], [0, 0, 4.0], atol=1e-15)
    # C on +X: z = (-1, 0, 0), x = cross(up, z) = (0, 0, 1), y = (0, 1, 0); columns of R
    want = np.array([[0.0, 0, -1], [0, 1, 0], [1, 0, 0]])
    assert np.allclose(c[0, M.C_R:M.C_R + 9].reshape(3, 3), want, atol=1e-7)
    # T = -R^T C = (0, 0, |C|) for every look-at camera: its tangents vanish
    assert np.abs(c[:, M.C_DT_EL:M.C_DT_EL + 3]).max() < 1e-14 and np.abs(c[:, M.C_DT_AZ:M.C_DT_AZ + 3]).max() < 1e-14
    # look_at_view_transform's convention: el lifts C towards +Y
    lk = _cam(M.CAM_LOOKAT, None, [half_pi / 2, 0.0], [0.0, half_pi], [2.0, 3.0])
    s = math.sqrt(0.5) * 2.0
    assert np.allclose(lk["cam"][0, M.C_C:M.C_C + 3], [0, s, s], atol=1e-7)
    assert np.allclose(lk["cam"][1, M.C_C:M.C_C + 3], [3.0, 0, 0], atol=3e-7)
    assert not lk["cam"][:, M.C_DR_EL:M.C_J + 4].any()  # zero tangents, zero J
    assert np.array_equal(lk["cam"][:, M.C_EL], [float(half_pi / 2), 0.0]) and np.array_equal(lk["el_new"], [half_pi / 2, 0])
    assert not lk["cam"][:, 45:].any()
    # OCC_CAM_POSITION equals the look-at camera at the same centre
    ps = _cam(M.CAM_POSITION, lk["cam"][:, M.C_C:M.C_C + 3], None, None, None)["cam"]
    assert np.allclose(ps[:, :12], lk["cam"][:, :12], atol=1e-6) and not ps[:, M.C_DR_EL:].any()


def test_state_update_is_float32_and_the_chain_sits_at_the_updated_angles():
    a = np.array([[3.0, 4.0], [0.0, 0.0], [0.0, -2.0]], np.float32)
    el, az = np.array([0.1, 0.2, 0.3], np.float32), np.array([1.0, -2.0, 0.5], np.float32)
    c = _cam(M.CAM_STEP, a, el, az, [4.0, 4.0, 4.0])
    f = np.float32
    assert c["el_new"].dtype == np.float32
    assert c["el_new"][0] == f(0.1) + f(f(0.6) * f(0.05)) and c["az_new"][0] == f(1.0) + f(f(0.8) * f(0.05))
    assert c["el_new"][1] == f(0.2) and c["az_new"][1] == f(-2.0)  # the zero action is not divided: no NaN, no move
    assert c["az_new"][2] == f(0.5) + f(f(-1.0) * f(0.05)) and c["el_new"][2] == f(0.3)
    e, z = float(c["el_new"][0]), float(c["az_new"][0])
    assert np.allclose(c["cam"][0, M.C_C:M.C_C + 3], [4 * math.sin(z) * math.cos(e), 4 * math.sin(z) * math.sin(e), 4 * math.cos(z)], atol=1e-14)
    # the fused form (one rounding) differs only where the sum cancels, and then by more than an ulp of the SUM
    a2, e2, z2 = np.array([[1.0, -1.0], [-0.6, -0.8]], np.float32), np.array([1.0, 0.3], f), np.array([0.5, 0.05], f)
    two, fus = M.state_update32(a2, e2, z2), M.state_update_fused32(a2, e2, z2)
    assert np.array_equal(two[0], fus[0]) and two[1][0] == fus[1][0] and np.array_equal(two[2], fus[2])
    d = abs(float(fus[1][1]) - float(two[1][1]))
    assert np.spacing(two[1][1]) < d <= np.spacing(f(0.04))
    # `at`: the chain at the angles handed in, the f32 state still the model's own
    c2 = _cam(M.CAM_STEP, a, el, az, [4.0, 4.0, 4.0], at=(np.nextafter(c["el_new"], f(9)), c["az_new"]))
    assert np.array_equal(c2["el_new"], c["el_new"]) and c2["cam"][0, M.C_EL] == float(np.nextafter(c["el_new"][0], f(9)))
    assert 0 < abs(c2["cam"][0, M.C_C] - c["cam"][0, M.C_C]) < 1e-6


def test_action_jacobian():
    J = M.action_jacobian(np.array([[0.0, 0.0], [3.0, 4.0], [2.0, 0.0]], np.float32))
    s = float(np.float32(0.05))
    assert np.array_equal(J[0], s * np.eye(2))  # the zero action: angles += a * step
    assert np.allclose(J[1], s * np.array([[0.64, -0.48], [-0.48, 0.36]]) / 5.0, rtol=1e-15)
    assert np.allclose(J[2], s * np.array([[0.0, 0.0], [0.0, 0.5]]), atol=1e-18)  # axis-aligned: only the other axis turns
    # against finite differences of a -> a / |a| * step
    a, h = np.array([0.3, -1.1]), 1e-6
    fd = np.stack([(s * (a + h * e) / np.linalg.norm(a + h * e) - s * (a - h * e) / np.linalg.norm(a - h * e)) / (2 * h)
                   for e in np.eye(2)], 1)
    assert np.allclose(M.action_jacobian(a.astype(np.float32)[None])[0], fd, atol=1e-8)
    # the slots: C_J + 2 i + j = d angle_i / d a_j
    c = _cam(M.CAM_STEP, [[3.0, 4.0]], [0.0], [1.0], [4.0])["cam"][0]
    assert np.array_equal(c[M.C_J:M.C_J + 4], J[1].reshape(4))


def _teapot_world():
    from occlusionenv_amd.meshes import load_obj
    from tests.parity_utils import TEAPOT

    v, f = load_obj(TEAPOT)
    return v + torch.tensor([0.3, 0.0, 1.0]), f


def _records_at(w, f, action, el, az, radius, **kw):
    c = _cam(M.CAM_STEP, action, el, az, radius)
    cam = c["cam"][0]
    R, T = torch.tensor(cam[M.C_R:M.C_R + 9].reshape(3, 3)), torch.tensor(cam[M.C_T:M.C_T + 3])
    dR = np.stack([cam[M.C_DR_EL:M.C_DR_EL + 9].reshape(3, 3), cam[M.C_DR_AZ:M.C_DR_AZ + 9].reshape(3, 3)])
    dT = np.stack([cam[M.C_DT_EL:M.C_DT_EL + 3], cam[M.C_DT_AZ:M.C_DT_AZ + 3]])
    return c, M.records(w, f, R, T, dR, dT, cam[M.C_C:M.C_C + 3], **kw)


def _fd_pieces(w, f, radius, e0, a0, h=1e-6):
    def at(e, a):
        C = M.step_centre(torch.tensor([float(np.float32(radius))], dtype=torch.float64), torch.tensor([e], dtype=torch.float64),
                          torch.tensor([a], dtype=torch.float64))
        R = O.look_at_rotation(C)
        return O.clip_faces(O.world_to_ndc(w.double(), R[0], O.translation_from(R, C)[0])[f])[0]

    de = (at(e0 + h, a0) - at(e0 - h, a0)) / (2 * h)
    da = (at(e0, a0 + h) - at(e0, a0 - h)) / (2 * h)
    return torch.stack([de[..., 0], de[..., 1], da[..., 0], da[..., 1]], -1).numpy()


def test_tangents_against_finite_differences_on_unclipped_faces_only():
    """Finite differences of the oracle's f64 chain agree with the model's forward-AD tangents to 1e-8 on unclipped
    faces; on z-clipped pieces they do NOT (the cut weight is detached: the tangent is not the derivative)."""
    w, f = _teapot_world()
    for radius, el, az, clipped in ((4.0, 0.4, 0.3, False), (1.2, 0.0, -0.17, True)):
        c, m = _records_at(w, f, [[0.7, -0.4]], [el], [az], [radius])
        fd = _fd_pieces(w, f, radius, float(c["el_new"][0]), float(c["az_new"][0]))
        d = np.abs(fd - m["tan"]).reshape(len(fd), -1).max(1)
        T = np.abs(m["tan"]).max()
        assert m["clipped"].any() == clipped
        assert d[~m["clipped"]].max() <= 1e-8 * T, (radius, d[~m["clipped"]].max(), T)
        if clipped:
            assert (m["half"] > 0).sum() >= 50 and (m["clipped"] & (m["half"] == 0)).any()  # case 4 and case 3 both occur
            assert d[m["clipped"]].max() > 1e-2 * T
        # the float32 run of the same chain: the reference's own precision, a few f32 roundings away
        m32 = _records_at(w, f, [[0.7, -0.4]], [el], [az], [radius], dtype=torch.float32)[1]
        e = M.tangent_distance(m32["tan"], m["tan"]).max()
        assert 1e-8 < e < 1e-5, e


def _hand_pieces(view, tT):
    """records() of ONE face given directly in view space (R = I, T = 0), tangents along pure translations tT (2, 3)."""
    verts = torch.tensor(view, dtype=torch.float64)
    return M.records(verts, torch.tensor([[0, 1, 2]]), torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64),
                     np.zeros((2, 3, 3)), np.asarray(tT, dtype=np.float64), (0.0, 0.0, -3.0))


def test_hand_worked_cut_pieces_carry_the_detached_weight():
    s = float(O.proj_scale(torch.float64))
    # directions: "el" moves every view-space vertex along +x, "az" along +z
    tT = [[1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]

    def proj(p):  # NDC position and its tangents (dx/del, dy/del, dx/daz, dy/daz) of an unclipped vertex
        x, y, z = p
        return [s * x / z, s * y / z, z], [s / z, 0.0, -s * x / z ** 2, -s * y / z ** 2]

    def cut(a, b):  # cut vertex of edge a -> b: w = (za - 0.5) / (za - zb) held constant; xy = s (a (1 - w) + b w) / 0.5
        w = (a[2] - 0.5) / (a[2] - b[2])
        x, y = a[0] * (1 - w) + b[0] * w, a[1] * (1 - w) + b[1] * w
        # along +x both ends move alike: d = s / 0.5; along +z the xy of the cut does not move AT ALL (detached weight)
        return [s * x / 0.5, s * y / 0.5, 0.5], [s / 0.5, 0.0, 0.0, 0.0]

    # case 3: v1 alone in front (z = 1.5), v0 and v2 behind -> one piece (p4, p5, p1): cut(v1 -> v2), cut(v1 -> v0), v1
    v = [[0.2, 0.1, 0.25], [-0.3, 0.4, 1.5], [0.5, -0.2, 0.125]]
    m = _hand_pieces(v, tT)
    want = [cut(v[1], v[2]), cut(v[1], v[0]), proj(v[1])]
    assert m["fv"].shape == (1, 3, 3) and m["clipped"].all() and m["half"].tolist() == [0] and m["ids"].tolist() == [0]
    assert np.allclose(m["fv"][0], [p for p, _ in want], atol=1e-14)
    assert np.allclose(m["tan"][0], [t for _, t in want], atol=1e-14)
    # differentiating the weight would NOT give zero along +z: the cut slides along its edge
    assert abs((v[2][0] - v[1][0]) / (v[1][2] - v[2][2])) > 0.1
    # case 4: v2 alone behind -> (p4, p2, p5), (p5, p2, p3) with p1 = v2, p2 = v0, p3 = v1: a pair
    v = [[0.2, 0.1, 0.75], [-0.3, 0.4, 1.5], [0.5, -0.2, 0.25]]
    m = _hand_pieces(v, tT)
    p4, p5 = cut(v[2], v[0]), cut(v[2], v[1])
    want = [[p4, proj(v[0]), p5], [p5, proj(v[0]), proj(v[1])]]
    assert m["half"].tolist() == [1, 2] and m["clipped"].all() and m["ids"].tolist() == [0, 0]
    for k in range(2):
        assert np.allclose(m["fv"][k], [p for p, _ in want[k]], atol=1e-14)
        assert np.allclose(m["tan"][k], [t for _, t in want[k]], atol=1e-14)
    # nothing behind: the face itself, unclipped
    m = _hand_pieces([[0.2, 0.1, 0.75], [-0.3, 0.4, 1.5], [0.5, -0.2, 0.6]], tT)
    assert m["half"].tolist() == [0] and not m["clipped"].any()
    assert np.allclose(m["tan"][0, 2], proj([0.5, -0.2, 0.6])[1], atol=1e-14)


def test_match_records_by_id_and_half():
    model = dict(ids=np.array([0, 2, 2, 3, 5, 5]))
    piece, either = M.match_records(np.array([5, 0, 2, 2, 5, 3]), np.array([6, 0, 5, 6, 4, 4]), model)
    assert piece.tolist() == [5, 0, 1, 2, -1, 3] and either == {4: [4, 5]}
    with pytest.raises(AssertionError):
        M.match_records(np.array([1]), np.array([0]), model)


def test_hand_computed_shaded_face():
    # a face in the plane z = 0 around the origin, normal +z... seen from the light's side: the normal must face (2, 2, -2)
    v = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [-1.0, -1.0, 0]])
    f = torch.tensor([[0, 2, 1], [0, 1, 2]])  # normal -z (towards the light) and +z (away from it)
    amb, spec, cosang = M.flat_terms(v, f, (0.0, 0.0, -3.0))
    # centre = origin; l = (1, 1, -1) / sqrt 3; n = (0, 0, -1): cos = 1 / sqrt 3
    c = 1.0 / math.sqrt(3.0)
    assert np.allclose(cosang, [c, -c], atol=1e-15)
    assert np.allclose(amb, [0.5 + 0.3 * c, 0.5], atol=1e-15)
    # r = -l + 2 c n = (-1, -1, 1) / sqrt 3 + (0, 0, -2 / 3) sqrt 3 ... = (-c, -c, c - 2 c) = (-c, -c, -c); view = (0, 0, -1)
    assert np.allclose(spec, [0.2 * c ** 64, 0.0], atol=1e-30) and spec[0] > 0
    # the camera on the mirror direction sees the full highlight
    _, spec, _ = M.flat_terms(v, f[:1], (-3.0, -3.0, -3.0))
    assert np.allclose(spec, [0.2], atol=1e-14)
    # a degenerate face (zero normal): eps 1e-6 keeps it finite, no light reaches it
    amb, spec, cosang = M.flat_terms(torch.tensor([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]]), torch.tensor([[0, 1, 2]]), (0, 0, -3.0))
    assert amb.tolist() == [0.5] and spec.tolist() == [0.0] and cosang.tolist() == [0.0]
    # the double normalisation shows on a tiny face: |cross| = 1e-14 -> / eps = 1e-8 -> / eps again = 1e-2: the cosine is
    # a hundredth of the unit normal's (a single normalisation would leave a ten-thousandth of that)
    t = torch.tensor([[0.0, 0, 0], [0, 1e-7, 0], [1e-7, 0, 0]], dtype=torch.float64)
    _, _, cs = M.flat_terms(t, torch.tensor([[0, 1, 2]]), (0, 0, -3.0))
    lt = np.array([2.0, 2.0, -2.0]) - np.array([1e-7 / 3, 1e-7 / 3, 0.0])
    assert np.allclose(cs, [1e-2 * (-lt[2]) / np.linalg.norm(lt)], rtol=1e-9)


def test_derived_slots():
    fv = np.array([[[0.0, 0.0, 1.0], [0.0, 0.5, 1.0], [-0.25, 0.0, 1.0]],
                   [[0.1, 0.1, 2.0], [0.1 + 5e-5, 0.1, 2.0], [0.1, 0.4, 2.0]],
                   [[0.1, 0.1, 2.0], [0.1 + 2e-4, 0.1, 2.0], [0.1, 0.4, 2.0]]], dtype=np.float32)
    d = M.derived(fv)
    v = fv.astype(np.float64)
    assert d["area"][0] == (-0.25) * 0.5 - 0.0 + M.KEPS  # back-facing in the engine's sign convention: E(v2; v0, v1)
    assert np.array_equal(d["l2"][0], [0.25, 0.0625, 0.0625 + 0.25])
    assert d["sentinel"].tolist() == [[False] * 3, [True, False, False], [False] * 3]
    assert d["l2"][1, 0] == (v[1, 1, 0] - v[1, 0, 0]) ** 2 and d["l2"][1, 0] < 1e-8 < d["l2"][2, 0]
    assert d["det_mag"][0] == 0.125


def test_needle_kinds_are_wired_into_the_dense_cases():
    from tests import dense_meshes as D
    from tests.parity_utils import make_case

    for kind in D.NEEDLE_KINDS:
        assert kind in D.DENSE_KINDS
        case = make_case(2, 3, kind, device="cpu")
        v, f = case["pool"].get(int(case["mesh_ids"][0, 0]))
        assert 200 <= f.shape[0] <= 600 and case["mesh_ids"].shape == (2, 3)
