"""The setup kernel's store path: a record is a function of (face, camera) only - not of the lane, wave or round its
face runs in, of how many faces of its wave survive culling (the wave's staged copy-out takes 1 ... 5 and 1 ... 3 trips),
of how its vertices reached the block (LDS copy in 1 ... 8 loads per thread, or gathered) or of whether its wave stores
through the LDS staging or directly.

Everything is engine against engine, bitwise on the raw words: records through parity_utils.snapshot_records, scan rows
and chunk boxes the way tests/test_gpu_dense_meshes.py reads them.  Every case runs the reset render (no gradient:
occ_setup_kernel<false>) and one step with an action gradient (occ_setup_kernel<true>).  What the host must know about
a scene (which faces are culled, which are z-clipped) is checked first on the CPU against the oracle's projection, with
margins far from both thresholds.

All meshes derive from one camera-facing sheet (tests/dense_meshes.py) at 64 x 64: every case of a group is one env
of ONE launch, rendered once and shared by the group's tests."""
import functools

import numpy as np
import pytest
import torch

from tests import dense_meshes as D
from tests.test_gpu_dense_meshes import _chunk_boxes, _engine, _fill_sentinel, _structures, SENTINEL

pytestmark = pytest.mark.gpu

S = 64
AZ = 0.1
ACTION = (0.3, -0.8)
K_EPS = 1e-8      # occ_constants.h kEpsilon: a face is visible if its NDC edge function exceeds it
M_FACES = 700     # the base mesh M: 700 front-facing faces, 11 chunks of 64, two rounds of 512
ROUND = 512       # faces per round of the setup kernel (kSetupTB)
# object offsets: the sheet cases' (tests/dense_meshes.py dense_layout), and - for the camera at radius 1.2 - away from it
OFFSETS_R4 = ((0.0, 0.0, 0.0), (0.05, 0.05, 1.0), (-0.05, -0.05, 2.0))
OFFSETS_NEAR = ((0.0, 0.0, 0.0), (0.05, 0.05, -0.5), (-0.05, -0.05, -1.0))


# ---- scenes ---------------------------------------------------------------------------------------------------------
def _case(meshes, offsets, az=AZ):
    """One env per mesh (the same mesh in its three object slots), every env with the same camera and action."""
    from occlusionenv_amd.meshes import MeshPool

    pool = MeshPool("cuda")
    ids = [pool.add(v, f) for v, f in meshes]
    n = len(ids)
    return dict(pool=pool, mesh_ids=torch.tensor(ids)[:, None].repeat(1, 3), offsets=torch.tensor(offsets).repeat(n, 1, 1),
                az=torch.full((n,), az), actions=torch.tensor([ACTION]).repeat(n, 1))


def _render(case, radius):
    """{phase: [per (env, object): dict(n, scan, cbox, rec, rect)]} of the reset render and of one step with gradient."""
    eng = _engine(case, S)
    rb = _fill_sentinel(eng)

    def snap():
        st = _structures(eng, rb)
        rect = eng._ws_tensors["objrect"].cpu().numpy()[: eng.N * 12].reshape(-1, 4).copy()
        for eo, s in enumerate(st):
            s["rect"] = rect[eo]
        return st

    eng.reset_render(None, radius, case["az"], 0.0)
    out = {"reset": snap()}
    rb.fill_(SENTINEL)
    eng.step(case["actions"].to(eng.device).requires_grad_(True))
    eng.check_status()
    out["step"] = snap()
    return out


def _ndc(case, env, radius):
    """[(phase, object, NDC corners (F, 3, 3) in f64, z-clipped mask (F,))] of one env by the oracle's projection."""
    from oracle import p3d_restate as O

    out = []
    for i, phase, R, T in D.sheet_cameras(case, radius):
        if i != env:
            continue
        for o in range(3):
            v, f = case["pool"].get(int(case["mesh_ids"][env, o]))
            fv = O.world_to_ndc(v.double() + case["offsets"][env, o].double(), R, T)[f]
            z = fv[..., 2].numpy()
            # (clip_faces cases: a face with a vertex behind z = Z_CLIP is cut or dropped)
            out.append((phase, o, fv.numpy(), (z < O.Z_CLIP).any(1)))
    return out


def _visible(fv, label, skip=None):
    """Visibility of every face as finish_tri decides it (edge function > kEpsilon), asserted to be FAR from every
    threshold: |edge function| > 100 kEpsilon, no vertex within 0.05 of the clip plane, every vertex on screen."""
    x, y, z = fv[..., 0], fv[..., 1], fv[..., 2]
    area = (x[:, 0] - x[:, 1]) * (y[:, 2] - y[:, 1]) - (y[:, 0] - y[:, 1]) * (x[:, 2] - x[:, 1])
    keep = np.ones(fv.shape[0], dtype=bool) if skip is None else ~skip
    assert (np.abs(area[keep]) > 100 * K_EPS).all(), (label, "a face on the cull boundary")
    assert (z[keep] > 0.5 + 0.05).all(), (label, "a face at the clip plane")
    assert (np.abs(x[keep]) < 0.95).all() and (np.abs(y[keep]) < 0.95).all(), (label, "a face off screen")
    return area > K_EPS


def _remap(raw, orig):
    """Record rows with the face id (slot 9) mapped through ``orig``."""
    out = raw.copy()
    ids = out[:, 9].view(np.int32)
    assert (orig[ids] >= 0).all(), "a record of a face that is not of the base mesh"
    out[:, 9] = orig[ids].astype(np.int32).view(np.float32)
    return out


def _same_words(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _check_against(base, got, orig, label, keep=None):
    """Object ``got`` (faces renumbered by ``orig``; ``keep``: mask of its records to compare) against ``base``: records in
    order, scan rows except .w (= the row's position), nrec, objrect; the chunk boxes against the host recomputation."""
    raw, scan = got["rec"]["raw"], got["scan"]
    assert np.array_equal(scan[:, 3], np.arange(got["n"], dtype=np.uint32)), (label, "scan .w")
    assert np.array_equal(got["cbox"], _chunk_boxes(scan)), (label, "chunk boxes")
    if keep is not None:
        raw, scan = raw[keep], scan[keep]
    else:
        assert got["n"] == base["n"], (label, "nrec", got["n"], base["n"])
        assert np.array_equal(got["rect"], base["rect"]), (label, "objrect", got["rect"], base["rect"])
    assert _same_words(_remap(raw, orig), base["rec"]["raw"]), (label, "records")
    assert np.array_equal(scan[:, :3], base["scan"][:, :3]), (label, "scan rows")


def _base_mesh():
    v, f = D.sheet(M_FACES)
    return v.clone(), f.clone()


# ---- padding with culled faces --------------------------------------------------------------------------------------
N_PAD = (1, 63, 64, 65, 449, 511, 512, 513)
# survivors of the LEADING 64-face chunks of M' (the rest of the padding is spread at seeded positions over the rest of
# the mesh): the staged copy-out moves 5 n and 3 n 16-byte parts of a wave's n records, 64 per trip - 12 | 13, 25 | 26,
# 38 | 39 and 21 | 22 are where it takes a trip more; 0: nothing to copy; 64 (every chunk without padding): all trips full
LEAD = {1: (63,), 63: (1,), 64: (0,), 65: (12,), 449: (0, 13, 21, 22, 25, 26, 38), 511: (0,) * 7, 512: (0,) * 8, 513: (0,) * 8}
SURVIVORS_REQUIRED = (0, 1, 12, 13, 21, 22, 64)


def padded_mesh(n_pad):
    """M with n_pad reversed-winding copies of its own faces inserted: (verts, faces, orig) with orig[k] = the face of M
    that face k is, or -1 for a padded face."""
    v, f = _base_mesh()
    f = f.numpy()
    F = f.shape[0]
    rng = np.random.default_rng(7000 + n_pad)
    chunks = []
    for s in LEAD[n_pad]:
        c = np.ones(64, dtype=bool)
        c[rng.choice(64, s, replace=False)] = False
        chunks.append(c)
    lead = np.concatenate(chunks)
    rest_pad, rest_real = n_pad - int(lead.sum()), F - int((~lead).sum())
    assert rest_pad >= 0 and rest_real >= 0
    rest = np.zeros(rest_pad + rest_real, dtype=bool)
    rest[rng.choice(rest.size, rest_pad, replace=False)] = True
    is_pad = np.concatenate([lead, rest])
    orig = np.full(F + n_pad, -1, dtype=np.int64)
    orig[~is_pad] = np.arange(F)
    out = np.empty((F + n_pad, 3), dtype=np.int64)
    out[~is_pad] = f
    out[is_pad] = f[rng.integers(0, F, n_pad)][:, [0, 2, 1]]
    return v, torch.from_numpy(out), orig


@functools.lru_cache(maxsize=None)
def _padding_run():
    meshes = [_base_mesh()] + [padded_mesh(n)[:2] for n in N_PAD]
    case = _case(meshes, OFFSETS_R4)
    # on the CPU first: the oracle's projection culls every padded face and keeps every other, far from the thresholds
    for env, n_pad in enumerate((0,) + N_PAD):
        orig = np.arange(M_FACES) if env == 0 else padded_mesh(n_pad)[2]
        for phase, o, fv, clipped in _ndc(case, env, 4.0):
            assert not clipped.any(), (n_pad, phase, o)
            assert np.array_equal(_visible(fv, (n_pad, phase, o)), orig >= 0), (n_pad, phase, o)
    return _render(case, 4.0)


@pytest.mark.parametrize("phase", ["reset", "step"])  # occ_setup_kernel<false> / <true>
@pytest.mark.parametrize("n_pad", N_PAD)
def test_culled_padding_moves_no_record(n_pad, phase):
    sts = _padding_run()[phase]
    env = 1 + N_PAD.index(n_pad)
    orig = padded_mesh(n_pad)[2]
    for o in range(3):
        assert sts[o]["n"] == M_FACES
        _check_against(sts[o], sts[env * 3 + o], orig, (n_pad, phase, o))


@pytest.mark.parametrize("phase", ["reset", "step"])
def test_culled_padding_reaches_every_copy_out_edge(phase):
    """From the record ids: the padded meshes gave some wave 0, 1, 12, 13, 21, 22 and 64 survivors."""
    sts = _padding_run()[phase]
    seen = set()
    for k, n_pad in enumerate(N_PAD):
        ids = sts[(1 + k) * 3]["rec"]["ids"]
        seen.update(np.bincount(ids // 64, minlength=(M_FACES + n_pad + 63) // 64).tolist())
    assert set(SURVIVORS_REQUIRED) <= seen, sorted(seen)


# ---- face counts around the round size ------------------------------------------------------------------------------
N_FACES = (1, 64, 511, 512, 513, 1023, 1024, 1025)


def _prefix_meshes():
    """Prefixes of one 1 025-face sheet of which a seeded third of the faces is turned away from the camera."""
    v, f = D.sheet(max(N_FACES))
    f = f.clone()
    back = torch.from_numpy(np.random.default_rng(7100).random(f.shape[0]) < 0.33)
    f[back] = f[back][:, [0, 2, 1]]
    return [(v.clone(), f[:n].clone()) for n in N_FACES], ~back.numpy()


@functools.lru_cache(maxsize=None)
def _prefix_run():
    meshes, front = _prefix_meshes()
    case = _case(meshes, OFFSETS_R4)
    for phase, o, fv, clipped in _ndc(case, len(N_FACES) - 1, 4.0):
        assert not clipped.any() and np.array_equal(_visible(fv, (phase, o)), front), (phase, o)
    return _render(case, 4.0), front


@pytest.mark.parametrize("phase", ["reset", "step"])
@pytest.mark.parametrize("nF", N_FACES[:-1])
def test_prefix_records_are_the_first_records_of_the_longer_mesh(nF, phase):
    run, front = _prefix_run()
    sts = run[phase]
    env, last = N_FACES.index(nF), len(N_FACES) - 1
    n = int(front[:nF].sum())
    for o in range(3):
        full, got = sts[last * 3 + o], sts[env * 3 + o]
        assert full["n"] == int(front.sum()) and got["n"] == n, (nF, phase, o, got["n"], n)
        assert np.array_equal(got["rec"]["ids"], np.nonzero(front[:nF])[0]), (nF, phase, o)
        assert _same_words(got["rec"]["raw"], full["rec"]["raw"][:n]), (nF, phase, o, "records")
        assert np.array_equal(got["scan"], full["scan"][:n]), (nF, phase, o, "scan rows")
        assert np.array_equal(got["cbox"], _chunk_boxes(got["scan"])), (nF, phase, o, "chunk boxes")


# ---- vertex counts around the trips of the LDS copy -----------------------------------------------------------------
N_VERTS = (511, 512, 513, 1024, 1025, 4095, 4096, 4097)  # (4 097: more than the kernel stages, the faces gather)


@functools.lru_cache(maxsize=None)
def _vertex_run():
    v, f = _base_mesh()
    assert v.shape[0] < min(N_VERTS)
    extra = torch.from_numpy(np.random.default_rng(7200).uniform(-1.0, 1.0, (max(N_VERTS), 3))).float()
    meshes = [(torch.cat([v, extra[: n - v.shape[0]]]), f) for n in N_VERTS]
    assert [m[0].shape[0] for m in meshes] == list(N_VERTS)
    return _render(_case(meshes, OFFSETS_R4), 4.0)


@pytest.mark.parametrize("phase", ["reset", "step"])
@pytest.mark.parametrize("nV", N_VERTS[1:])
def test_unused_vertices_change_no_record(nV, phase):
    sts = _vertex_run()[phase]
    env = N_VERTS.index(nV)
    same = np.arange(M_FACES)
    for o in range(3):
        assert sts[o]["n"] == M_FACES
        _check_against(sts[o], sts[env * 3 + o], same, (nV, phase, o))


# ---- staged against direct stores -----------------------------------------------------------------------------------
CLIP_AT = 5  # index of the extra face: in the first wave's face range


def _clip_meshes():
    """M, and M with one small face across the clip plane of the radius-1.2 camera (view depth 1.2 - z: 0.6 and 0.4 at
    z = 0.6 and 0.8) inserted as face CLIP_AT."""
    v, f = _base_mesh()
    nv = v.shape[0]
    v2 = torch.cat([v, torch.tensor([[0.02, 0.0, 0.6], [0.06, 0.0, 0.8], [0.02, 0.04, 0.6]])])
    f2 = torch.cat([f[:CLIP_AT], torch.tensor([[nv, nv + 1, nv + 2]]), f[CLIP_AT:]])
    orig = np.concatenate([np.arange(CLIP_AT), [-1], np.arange(CLIP_AT, M_FACES)])
    return [(v, f), (v2, f2)], orig


@functools.lru_cache(maxsize=None)
def _clip_run():
    meshes, orig = _clip_meshes()
    case = _case(meshes, OFFSETS_NEAR, az=0.0)
    n_clipped = 0
    for env in range(2):
        for phase, o, fv, clipped in _ndc(case, env, 1.2):
            extra = orig < 0 if env == 1 else np.zeros(M_FACES, dtype=bool)
            # the oracle clips only the extra face (object 0, the nearest; the objects farther away see it whole)
            assert not clipped[~extra].any(), (env, phase, o)
            assert _visible(fv, (env, phase, o), skip=extra)[~extra].all(), (env, phase, o)
            n_clipped += int(clipped.sum())
    assert n_clipped >= 2, "the extra face is z-clipped in the reset render and in the step"
    return _render(case, 1.2), orig


@pytest.mark.parametrize("phase", ["reset", "step"])
def test_a_clipped_face_in_the_first_wave_changes_no_other_record(phase):
    run, orig = _clip_run()
    sts = run[phase]
    for o in range(3):
        base, got = sts[o], sts[3 + o]
        assert base["n"] == M_FACES
        keep = got["rec"]["ids"] != CLIP_AT
        assert int(keep.sum()) == M_FACES, (phase, o)
        _check_against(base, got, orig, (phase, o), keep=keep)
    # the wave of the extra face did store directly: object 0 holds it as z-clipped records
    got = sts[3]
    assert ((got["rec"]["ids"] == CLIP_AT) & (got["rec"]["flags"] != 0)).any(), (phase, "no z-clipped record of the extra face")
