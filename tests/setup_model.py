"""f64 host model of what the camera and setup stages hand on (tests/test_setup_model.py pins it on the host,
tests/test_gpu_setup_records.py holds the kernels to it).  Plain torch / numpy on the CPU, no GPU import.

Written from the header comments of occ_camera.hpp / occ_setup.hpp, SURVEY.md A.1 - A.3 and A.7 and the slot maps of
occ_constants.h - not from the kernels' arithmetic.  The derivative part is NOT restated at all: R, T, the NDC
vertices and the z-clipped pieces are the oracle's own functions (oracle/p3d_restate.py: look_at_rotation,
translation_from, world_to_ndc, clip_faces) evaluated in float64 under forward-mode AD
(torch.autograd.forward_ad), one sweep per direction (d / d el, d / d az).  Finite differences are no reference for
the z-clipped pieces: PyTorch3D, the oracle and the engine all DETACH the cut weight, so the tangent of a cut vertex
is not the derivative of its position (they differ by O(1)); forward AD of the oracle's chain carries the detach.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

from oracle import p3d_restate as O

# occ_constants.h / include/occlusionenv_amd.h
CAM_STEP, CAM_LOOKAT, CAM_POSITION = 0, 1, 2
CAM_STRIDE, CAM_USED = 48, 45
C_R, C_T, C_C, C_DR_EL, C_DT_EL, C_DR_AZ, C_DT_AZ, C_J, C_EL, C_AZ = 0, 9, 12, 15, 24, 27, 36, 39, 43, 44
# slot groups of the camera buffer: a slot's absolute error term scales with the largest magnitude of ITS group
CAM_GROUPS = {"R": (0, 9), "T": (9, 12), "C": (12, 15), "DR_EL": (15, 24), "DT_EL": (24, 27), "DR_AZ": (27, 36),
              "DT_AZ": (36, 39), "J": (39, 43)}
R_INV_AREA, R_AMB, R_IL01, R_IL02, R_IL12, R_SPEC, R_TAN = 11, 12, 16, 17, 18, 19, 20
FLAG_PAIR_FIRST, FLAG_PAIR_SECOND, FLAG_CLIPPED = 1, 2, 4
STEP32 = np.float32(0.05)       # kStepSize
KEPS = float(np.float32(1e-8))  # kEpsilon as the kernels hold it
EPS32 = 2.0 ** -24              # unit roundoff of f32 (tests/parity_utils.py: "eps = 2^-24")


# ---- camera ---------------------------------------------------------------------------------------------------------
def state_update32(action, el, az):
    """environment.py:356-365 in float32 steps: norm, divide, el + n0 * float32(0.05).  A zero action is not divided.
    Returns (el_new, az_new, n) as float32 arrays."""
    a = np.asarray(action, dtype=np.float32).reshape(-1, 2)
    el = np.asarray(el, dtype=np.float32).reshape(-1)
    az = np.asarray(az, dtype=np.float32).reshape(-1)
    nrm = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]).astype(np.float32)).astype(np.float32)
    safe = np.where(nrm != 0, nrm, np.float32(1.0)).astype(np.float32)
    n = np.where((nrm != 0)[:, None], (a / safe[:, None]).astype(np.float32), a).astype(np.float32)
    el_new = (el + (n[:, 0] * STEP32).astype(np.float32)).astype(np.float32)
    az_new = (az + (n[:, 1] * STEP32).astype(np.float32)).astype(np.float32)
    return el_new, az_new, n


def state_update_fused32(action, el, az):
    """The same update as the compiler CONTRACTS it (what the gfx950 build of occ_camera.hpp holds: two v_fmac_f32):
    |a|^2 = fma(a0, a0, fl(a1 * a1)) and el_new = fma(n0, step, el), each rounded once; square root and division
    correctly rounded as in state_update32.  The product of two f32 is exact in f64, so one f64 addition and one
    rounding to f32 model an f32 FMA.  The sum differs from state_update32's by at most half an ulp of the PRODUCT -
    more than an ulp of the sum where the two cancel (az = 0.05, n1 * step = -0.04: two ulps) - and the norm by an ulp,
    which n0 and the sum may or may not inherit."""
    a = np.asarray(action, dtype=np.float32).reshape(-1, 2)
    a0, a1 = a[:, 0].astype(np.float64), a[:, 1].astype(np.float64)
    nrm2 = (a0 * a0 + (a[:, 1] * a[:, 1]).astype(np.float32).astype(np.float64)).astype(np.float32)
    nrm = np.sqrt(nrm2).astype(np.float32)
    safe = np.where(nrm != 0, nrm, np.float32(1.0)).astype(np.float32)
    n = np.where((nrm != 0)[:, None], (a / safe[:, None]).astype(np.float32), a).astype(np.float32)
    el = np.asarray(el, dtype=np.float32).reshape(-1).astype(np.float64)
    az = np.asarray(az, dtype=np.float32).reshape(-1).astype(np.float64)
    st = float(STEP32)
    return (el + n[:, 0].astype(np.float64) * st).astype(np.float32), (az + n[:, 1].astype(np.float64) * st).astype(np.float32), n


def action_jacobian(action):
    """d (el, az) / d action = float32(0.05) (I - n n^T) / |a| in f64 from the f32 action; float32(0.05) I for a zero
    action (the reference does not divide then).  (n, 2, 2): [i, j] = d angle_i / d a_j."""
    a = np.asarray(action, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    nrm = np.sqrt((a * a).sum(1))
    J = np.zeros((a.shape[0], 2, 2))
    for k in range(a.shape[0]):
        if nrm[k] == 0.0:
            J[k] = np.eye(2)
        else:
            n = a[k] / nrm[k]
            J[k] = (np.eye(2) - np.outer(n, n)) / nrm[k]
    return float(STEP32) * J


def step_centre(r, el, az):
    """step()'s convention (environment.py:363-365): C = (r sin az cos el, r sin az sin el, r cos az)."""
    return torch.stack([r * torch.sin(az) * torch.cos(el), r * torch.sin(az) * torch.sin(el), r * torch.cos(az)], dim=1)


def lookat_centre(r, el, az):
    """look_at_view_transform's convention: C = r (cos el sin az, sin el, cos el cos az)."""
    return torch.stack([r * torch.cos(el) * torch.sin(az), r * torch.sin(el), r * torch.cos(el) * torch.cos(az)], dim=1)


def _rt_tangents(centre_fn, r, el, az):
    """R, T, C of every row and their tangents along el and az: forward AD of the oracle's functions.  Every row depends
    on its own angles only, so one sweep with a tangent of ones gives every row's derivative."""
    out = {}
    for name, te, ta in (("el", 1.0, 0.0), ("az", 0.0, 1.0)):
        with fwAD.dual_level():
            C = centre_fn(r, fwAD.make_dual(el, torch.full_like(el, te)), fwAD.make_dual(az, torch.full_like(az, ta)))
            R = O.look_at_rotation(C)
            T = O.translation_from(R, C)
            (Rp, Rt), (Tp, Tt), (Cp, _) = fwAD.unpack_dual(R), fwAD.unpack_dual(T), fwAD.unpack_dual(C)
            out[name] = (Rp.clone(), Rt.clone(), Tp.clone(), Tt.clone(), Cp.clone())
    return out


def camera(mode, action, el, az, radius, at=None):
    """All 45 used slots of the camera buffer per env, as an (n, 48) float64 array (slots 45..47 zero), plus the f32
    state.  Returns dict(cam, el_new, az_new) - el_new / az_new float32 arrays.

    OCC_CAM_STEP: the state update in float32 steps (state_update32); the chain in float64 AT the updated f32 angles -
    or at ``at = (el_new, az_new)`` when given (the engine's own updated angles, so that an ulp of the f32 update does
    not travel into the other slots).  OCC_CAM_LOOKAT: look_at_view_transform's convention at (el, az), zero tangents,
    zero J.  OCC_CAM_POSITION: ``action`` holds C (n, 3); angles, tangents and J zero."""
    if mode == CAM_POSITION:
        Cn = np.asarray(action, dtype=np.float32).reshape(-1, 3)
        n = Cn.shape[0]
        C = torch.from_numpy(Cn.astype(np.float64))
        R = O.look_at_rotation(C)
        T = O.translation_from(R, C)
        cam = np.zeros((n, CAM_STRIDE))
        cam[:, C_R:C_R + 9], cam[:, C_T:C_T + 3], cam[:, C_C:C_C + 3] = R.reshape(n, 9).numpy(), T.numpy(), C.numpy()
        z = np.zeros(n, dtype=np.float32)
        return dict(cam=cam, el_new=z, az_new=z.copy())
    el32 = np.asarray(el, dtype=np.float32).reshape(-1)
    az32 = np.asarray(az, dtype=np.float32).reshape(-1)
    n = el32.shape[0]
    r = torch.from_numpy(np.asarray(radius, dtype=np.float32).reshape(-1).astype(np.float64))
    cam = np.zeros((n, CAM_STRIDE))
    if mode == CAM_STEP:
        el_new, az_new, _ = state_update32(action, el32, az32)
        e_at, a_at = (el_new, az_new) if at is None else (np.asarray(at[0], np.float32), np.asarray(at[1], np.float32))
        d = _rt_tangents(step_centre, r, torch.from_numpy(e_at.astype(np.float64)), torch.from_numpy(a_at.astype(np.float64)))
        Rp, Rte, Tp, Tte, Cp = d["el"]
        _, Rta, _, Tta, _ = d["az"]
        cam[:, C_DR_EL:C_DR_EL + 9], cam[:, C_DT_EL:C_DT_EL + 3] = Rte.reshape(n, 9).numpy(), Tte.numpy()
        cam[:, C_DR_AZ:C_DR_AZ + 9], cam[:, C_DT_AZ:C_DT_AZ + 3] = Rta.reshape(n, 9).numpy(), Tta.numpy()
        cam[:, C_J:C_J + 4] = action_jacobian(action).reshape(n, 4)
        cam[:, C_EL], cam[:, C_AZ] = e_at.astype(np.float64), a_at.astype(np.float64)
    elif mode == CAM_LOOKAT:
        el_new, az_new = el32.copy(), az32.copy()
        Cp = lookat_centre(r, torch.from_numpy(el32.astype(np.float64)), torch.from_numpy(az32.astype(np.float64)))
        Rp = O.look_at_rotation(Cp)
        Tp = O.translation_from(Rp, Cp)
        cam[:, C_EL], cam[:, C_AZ] = el32.astype(np.float64), az32.astype(np.float64)
    else:
        raise ValueError(mode)
    cam[:, C_R:C_R + 9], cam[:, C_T:C_T + 3], cam[:, C_C:C_C + 3] = Rp.reshape(n, 9).numpy(), Tp.numpy(), Cp.numpy()
    return dict(cam=cam, el_new=el_new, az_new=az_new)


def camera_bound(want):
    """|got - want| <= 2^-23 |want| + 2^-40 g per slot, g = the largest magnitude of the slot's group in that row: the
    kernel is f64 rounded once, so one ulp is the contract; the absolute term covers the f64 cancellation residue of
    entries that are zero in exact arithmetic.  One group is zero in exact arithmetic AS A WHOLE: T = -R^T C is
    (0, 0, |C|) for every look-at camera, so its tangents -(dR^T C + R^T dC) vanish and what either side holds there is
    the residue (1e-16) of terms of size |dR| |C| and |dC| <= |C|; for DT_EL / DT_AZ g is therefore the size of those
    terms, max|dR| |C| + |C|, where that is larger than the group's own magnitude.
    (n, 48) array; slots outside the groups get 0 (compared exactly)."""
    b = np.zeros_like(want)
    normC = np.sqrt((want[:, C_C:C_C + 3] ** 2).sum(1, keepdims=True))
    for name, (lo, hi) in CAM_GROUPS.items():
        g = np.abs(want[:, lo:hi]).max(1, keepdims=True)
        if name.startswith("DT_"):
            dlo, dhi = CAM_GROUPS["DR_" + name[3:]]
            g = np.maximum(g, np.abs(want[:, dlo:dhi]).max(1, keepdims=True) * normC + normC)
        b[:, lo:hi] = 2.0 ** -23 * np.abs(want[:, lo:hi]) + 2.0 ** -40 * g
    return b


def off_pole(cam64):
    """|cross(up, z)| of every row: z = the third column of R is -C / |C|, up = +Y."""
    Rm = cam64[:, C_R:C_R + 9].reshape(-1, 3, 3)
    z = Rm[:, :, 2]
    return np.hypot(z[:, 0], z[:, 2])


# ---- face records ---------------------------------------------------------------------------------------------------
def flat_terms(world_verts, faces, campos):
    """The two flat-shading terms of every ORIGINAL face, f64: face normal of cross(v1 - v0, v2 - v0)
    normalised twice (once for the face normal, once more inside the lighting functions), eps 1e-6 everywhere; face
    centre = mean of the corners; light at (2, 2, -2); diffuse 0.3 relu(n.l), ambient 0.5; specular
    0.2 (relu(v.r) [n.l > 0])^64.  Returns (amb_diff (F,), spec (F,), cosang (F,))."""
    v = torch.as_tensor(world_verts).double()
    fv = v[faces.long()]
    C = torch.as_tensor(np.asarray(campos, dtype=np.float64))

    def normalise(x):
        return x / x.norm(dim=1, keepdim=True).clamp(min=1e-6)

    n = normalise(normalise(torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1)))
    centre = fv.mean(dim=1)
    l = normalise(torch.tensor(O.LIGHT_LOCATION, dtype=torch.float64) - centre)
    cosang = (n * l).sum(1)
    view = normalise(C[None, :] - centre)
    refl = -l + 2.0 * cosang[:, None] * n
    alpha = (view * refl).sum(1).clamp(min=0.0) * (cosang > 0).double()
    return (O.AMBIENT + O.DIFFUSE * cosang.clamp(min=0.0)).numpy(), (O.SPECULAR * alpha ** 64).numpy(), cosang.numpy()


def _pieces(world_verts, faces, R, T, tR=None, tT=None, dtype=torch.float64):
    """clip_faces(world_to_ndc(...)) of the oracle, with the tangent along (tR, tT) when given."""
    v = torch.as_tensor(world_verts).to(dtype)
    f = faces.long()
    R, T = R.to(dtype), T.to(dtype)
    if tR is None:
        return O.clip_faces(O.world_to_ndc(v, R, T)[f], O.Z_CLIP, True)
    with fwAD.dual_level():
        ndc = O.world_to_ndc(v, fwAD.make_dual(R, tR.to(dtype)), fwAD.make_dual(T, tT.to(dtype)))
        out = O.clip_faces(ndc[f], O.Z_CLIP, True)
        p, t = fwAD.unpack_dual(out[0])
        t = torch.zeros_like(p) if t is None else t
        return (p.clone(), t.clone()) + tuple(out[1:])


def records(world_verts, faces, R64, T64, dR, dT, campos, dtype=torch.float64):
    """One row per oracle piece, in the oracle's piece order (clip_faces): dict of
      fv (P,3,3)   NDC vertices (x_ndc, y_ndc, z_view), vertex order as the oracle lists them
      tan (P,3,4)  per vertex d x/d el, d y/d el, d x/d az, d y/d az: forward-AD tangents of
                   clip_faces(world_to_ndc(...))[0], xy only, along (dR[0], dT[0]) and (dR[1], dT[1])
      ids (P,)     original face;  half (P,) 0 = no partner, 1 / 2 = first / second of a case-4 pair
      clipped (P,) bool: the piece is a z-clipped part of its face
      amb, spec, cosang (P,)  flat-shading terms of the ORIGINAL face (flat_terms).
    ``dtype`` float32 runs the same chain in float32 (the reference's own precision, for the tolerance)."""
    dR, dT = torch.as_tensor(dR), torch.as_tensor(dT)
    pe, te, c2u, nb, _, _ = _pieces(world_verts, faces, R64, T64, dR[0], dT[0], dtype)
    pa, ta, _, _, _, _ = _pieces(world_verts, faces, R64, T64, dR[1], dT[1], dtype)
    assert torch.equal(pe, pa)
    P = pe.shape[0]
    ids = np.arange(P) if c2u is None else c2u.numpy()
    half = np.zeros(P, dtype=np.int64)
    clipped = np.zeros(P, dtype=bool)
    if nb is not None:
        nbn = nb.numpy()
        half[(nbn >= 0) & (nbn > np.arange(P))] = 1
        half[(nbn >= 0) & (nbn < np.arange(P))] = 2
        ndc = O.world_to_ndc(torch.as_tensor(world_verts).to(dtype), R64.to(dtype), T64.to(dtype))
        behind = (ndc[faces.long()][..., 2] < O.Z_CLIP).any(1).numpy()
        clipped = behind[ids]
    tan = torch.stack([te[..., 0], te[..., 1], ta[..., 0], ta[..., 1]], dim=-1)
    amb, spec, cosang = flat_terms(world_verts, faces, campos)
    return dict(fv=pe.double().numpy(), tan=tan.double().numpy(), ids=ids, half=half, clipped=clipped, amb=amb[ids],
                spec=spec[ids], cosang=cosang[ids])


def match_records(rec_ids, rec_flags, model):
    """Model piece of every engine record, by original face id and half as tests/parity_utils.upstream_check does: a
    record with a pair flag is the first / second piece of its face; one without takes the face's only piece - or, for
    a half whose partner the engine found invisible, -1 in ``piece`` and both candidates in ``either``."""
    by_id = {}
    for p, k in enumerate(model["ids"].tolist()):
        by_id.setdefault(int(k), []).append(p)
    piece = np.full(len(rec_ids), -1, dtype=np.int64)
    either = {}
    for j, (k, fl) in enumerate(zip(rec_ids.tolist(), rec_flags.tolist())):
        cs = by_id.get(int(k), [])
        if len(cs) == 2 and fl & 3:
            piece[j] = cs[1] if fl & 2 else cs[0]
        elif len(cs) == 1:
            piece[j] = cs[0]
        elif len(cs) == 2:
            either[j] = cs
        else:
            raise AssertionError("engine record %d of face %d has no oracle piece" % (j, k))
    return piece, either


def tangent_distance(tan_got, tan64, scale_T=None):
    """e_r = max|tan_got - tan64| / max(max|tan64 of r|, 1e-3 T) per record r; T = the object's largest |tangent|."""
    tan_got, tan64 = np.asarray(tan_got, dtype=np.float64), np.asarray(tan64, dtype=np.float64)
    n = tan64.shape[0]
    if n == 0:
        return np.zeros(0)
    T = float(np.abs(tan64).max()) if scale_T is None else scale_T
    den = np.maximum(np.abs(tan64).reshape(n, -1).max(1), 1e-3 * T)
    return np.abs(tan_got - tan64).reshape(n, -1).max(1) / den


# ---- derived slots --------------------------------------------------------------------------------------------------
def derived(fv32):
    """From a record's OWN f32 positions, evaluated in f64: area = E(v2; v0, v1) + kEpsilon, the three |edge|^2
    (order e01, e02, e12), which edges take the -1 sentinel (|edge|^2 <= kEpsilon), and the magnitude
    |dx20 dy10| + |dy20 dx10| the determinant's forward error bound scales with."""
    v = np.asarray(fv32, dtype=np.float32).astype(np.float64)
    x, y = v[:, :, 0], v[:, :, 1]
    dx20, dy10, dy20, dx10 = x[:, 2] - x[:, 0], y[:, 1] - y[:, 0], y[:, 2] - y[:, 0], x[:, 1] - x[:, 0]
    area = dx20 * dy10 - dy20 * dx10 + KEPS
    l2 = np.stack([(x[:, 1] - x[:, 0]) ** 2 + (y[:, 1] - y[:, 0]) ** 2, (x[:, 2] - x[:, 0]) ** 2 + (y[:, 2] - y[:, 0]) ** 2,
                   (x[:, 2] - x[:, 1]) ** 2 + (y[:, 2] - y[:, 1]) ** 2], 1)
    return dict(area=area, l2=l2, sentinel=l2 <= KEPS, det_mag=np.abs(dx20 * dy10) + np.abs(dy20 * dx10))
