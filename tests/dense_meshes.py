"""Deterministic dense test meshes (tests/test_gpu_dense_meshes.py, tests/test_dense_mesh_builders.py): nothing is
stored, every mesh is built in code from fixed parameters and seeds.

* ``dense_icosphere``: subdiv-6 icosphere with smooth radial noise, like ``meshes.synthetic_mesh`` (81 920 faces).
* ``dense_torus``: ``torus(384, 320)``, 245 760 faces, just under the reference's MAX_MESH_FACES = 250 000.
* ``sheet(F)``: a camera-facing height field with exactly F faces, every one of them front-facing, on screen and
  unclipped at the sheet cameras (``SHEET_AZ_RANGE``): the setup kernel writes exactly F records per object.  The
  counts straddle the front-to-back sort's thresholds (occ_setup.hpp: kSortMin = 4 096 <= nrec <= kSortCap = 8 192).
* ``vertex_sheet(nV)``: a sheet with exactly nV vertices (4 096 / 4 097: either side of the setup kernel's LDS vertex cap).
* ``reorder``: the same mesh with its faces reversed (roughly back to front) or in a seeded random order.
* ``needles(kind)``: visible needle triangles with one edge far below kEpsilon in NDC (the -1 sentinel of a record's
  1 / |edge|^2 slots), the degenerate edge in each of the three slots in turn.
"""
from __future__ import annotations

import numpy as np
import torch

MAX_MESH_FACES = 250_000  # the reference's limit on a mesh (environment.py)
SHEET_COUNTS = (4095, 4096, 8192, 8193)
VERTEX_COUNTS = (4096, 4097)
SHEET_AZ_RANGE = 0.25  # azimuth range of the sheet cases (make_case(..., az_range=SHEET_AZ_RANGE))
SHEET_WIDTH = 0.6      # world units: at distance 2 ... 4 from the camera the sheet spans 0.26 ... 0.52 NDC
ORDERS = ("native", "reversed", "shuffled")
_CACHE = {}


def _height(x, y):
    """Smooth, non-planar relief of the sheets (slopes < 0.3): no two faces share a plane, none folds over another."""
    return 0.03 * np.sin(7.0 * x + 1.0) * np.cos(5.0 * y - 0.5) + 0.05 * x * y + 0.02 * np.sin(11.0 * y + 3.0 * x)


def _grid_sheet(nx, ny, quads, extra_tri):
    """(nx + 1) x (ny + 1) grid of vertices in the plane z ~ 0, facing +z (the camera at azimuth 0); the first ``quads``
    quads in row-major order as two triangles each, plus one triangle of the next quad if ``extra_tri``; unused
    vertices dropped."""
    d = SHEET_WIDTH / nx
    xs = (np.arange(nx + 1) - nx / 2.0) * d
    ys = (np.arange(ny + 1) - ny / 2.0) * d
    X, Y = np.meshgrid(xs, ys, indexing="xy")  # (ny+1, nx+1): vertex (row j, column i) = j * (nx + 1) + i
    verts = np.stack([X, Y, _height(X, Y)], -1).reshape(-1, 3)
    faces = []
    for q in range(quads + (1 if extra_tri else 0)):
        j, i = divmod(q, nx)
        a, b = j * (nx + 1) + i, j * (nx + 1) + i + 1
        c, e = a + nx + 1, b + nx + 1
        faces.append([a, b, e])  # counter-clockwise seen from +z: front-facing
        if q < quads:
            faces.append([a, e, c])
    faces = np.array(faces, dtype=np.int64)
    used = np.unique(faces)
    remap = np.full(verts.shape[0], -1, dtype=np.int64)
    remap[used] = np.arange(used.size)
    return verts[used], remap[faces]


def sheet(F: int):
    """Height-field sheet with exactly F faces (64 quads a row)."""
    key = ("sheet", F)
    if key not in _CACHE:
        nx = 64
        quads, odd = divmod(F, 2)
        ny = -(-(quads + odd) // nx)
        v, f = _grid_sheet(nx, ny, quads, odd)
        assert f.shape[0] == F
        _CACHE[key] = (torch.tensor(v, dtype=torch.float32), torch.tensor(f, dtype=torch.int64))
    return _CACHE[key]


def vertex_sheet(nV: int):
    """Sheet with exactly nV vertices: a 64 x 64 vertex grid (4 096), plus one vertex beyond its top edge joined to the
    grid's last two vertices by one more triangle (4 097: the highest vertex index is the one past the LDS cap)."""
    key = ("vsheet", nV)
    if key not in _CACHE:
        assert nV in VERTEX_COUNTS
        v, f = _grid_sheet(63, 63, 63 * 63, False)
        if nV == 4097:
            last, prev = 4095, 4094  # top-right and its left neighbour
            d = SHEET_WIDTH / 63
            p = np.array([v[prev, 0] + 0.5 * d, v[last, 1] + d, 0.0])
            p[2] = _height(p[0], p[1])
            v = np.concatenate([v, p[None]])
            f = np.concatenate([f, np.array([[prev, last, 4096]], dtype=np.int64)])
        assert v.shape[0] == nV
        _CACHE[key] = (torch.tensor(v, dtype=torch.float32), torch.tensor(f, dtype=torch.int64))
    return _CACHE[key]


def dense_icosphere(seed: int = 6):
    """Subdiv-6 icosphere (40 962 vertices, 81 920 faces) with the smooth radial noise, anisotropic scale and rotation
    of ``meshes.synthetic_mesh``, normalised to unit bounding-box diagonal."""
    key = ("ico", seed)
    if key not in _CACHE:
        from occlusionenv_amd.meshes import _normalise, _orient_outward, icosphere

        rng = np.random.default_rng(seed)
        v, f = icosphere(6)
        k = rng.normal(size=(4, 3))
        amp = 0.1 * rng.normal(size=4)
        v = v * (1.0 + sum(a * np.sin(2.0 * v @ kk) for a, kk in zip(amp, k)))[:, None]
        v = v * rng.uniform(0.4, 1.0, size=3)[None, :]
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                       [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                       [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        v = _normalise(v @ Rm.T)
        _CACHE[key] = (torch.tensor(v, dtype=torch.float32), torch.tensor(_orient_outward(v, f), dtype=torch.int64))
    return _CACHE[key]


def dense_torus():
    """torus(384, 320): 122 880 vertices, 245 760 faces, normalised to unit bounding-box diagonal."""
    if "torus" not in _CACHE:
        from occlusionenv_amd.meshes import _normalise, _orient_outward, torus

        v, f = torus(384, 320, 1.0, 0.4)
        v = _normalise(v)
        _CACHE["torus"] = (torch.tensor(v, dtype=torch.float32), torch.tensor(_orient_outward(v, f), dtype=torch.int64))
    return _CACHE["torus"]


NEEDLE_KINDS = ("needles01", "needles02", "needles12")
NEEDLE_COUNT = 320
NEEDLE_SHORT = 2e-5          # world distance of the two close corners: ~1e-5 NDC at radius 4, |edge|^2 ~ 1e-10 << kEpsilon
NEEDLE_LENGTH = (0.3, 0.6)   # world distance of the third corner: area (edge function) ~ 3e-6 NDC >> kEpsilon, visible


def needles(kind: str):
    """NEEDLE_COUNT front-facing needle triangles, each with its own three vertices: corners a, b NEEDLE_SHORT apart, the
    tip c 0.3 ... 0.6 away at right angles to (a, b); centres in a patch half a unit wide, directions all round the
    clock (pixel centres then fall beyond both ends and beside the flanks of some needle), every needle in a plane
    z = const of its own (all face +z, no two share a depth).  The kinds are the three rotations of the vertex order -
    (a, b, c), (b, c, a), (c, a, b) - so that the degenerate edge is (v0, v1), (v0, v2) or (v1, v2): the closest-edge tie
    order e01, e02, e12 decides which edge the gradient flows through at the tip."""
    key = ("needles", kind)
    if key not in _CACHE:
        rot = {"needles01": (0, 1, 2), "needles02": (1, 2, 0), "needles12": (2, 0, 1)}[kind]
        rng = np.random.default_rng(1201)  # the same needles for the three kinds
        n = NEEDLE_COUNT
        p = rng.uniform(-0.25, 0.25, size=(n, 2))
        th = (np.arange(n) + rng.uniform(0.0, 1.0, size=n)) * (2.0 * np.pi / n)
        rng.shuffle(th)
        L = rng.uniform(*NEEDLE_LENGTH, size=n)
        z = rng.permutation(n) * (0.1 / n) - 0.05
        u = np.stack([np.cos(th), np.sin(th)], 1)
        nrm = np.stack([-u[:, 1], u[:, 0]], 1)  # u turned by +90 degrees
        m, c = p - 0.5 * L[:, None] * u, p + 0.5 * L[:, None] * u
        # (a, b, c) counter-clockwise seen from +z (front-facing like the sheets): (b - a) x (c - a) = -nrm x u > 0 for a = m + h nrm
        a, b = m + 0.5 * NEEDLE_SHORT * nrm, m - 0.5 * NEEDLE_SHORT * nrm
        tri = np.stack([a, b, c], 1)  # (n, 3, 2)
        verts = np.concatenate([tri, np.repeat(z[:, None, None], 3, 1)], -1)[:, rot, :].reshape(-1, 3)
        faces = np.arange(3 * n, dtype=np.int64).reshape(n, 3)
        _CACHE[key] = (torch.tensor(verts, dtype=torch.float32), torch.tensor(faces, dtype=torch.int64))
    return _CACHE[key]


def needle_short_slot(kind: str) -> int:
    """Which of a record's three 1 / |edge|^2 slots (R_IL01, R_IL02, R_IL12) holds the degenerate edge of the kind."""
    return NEEDLE_KINDS.index(kind)


def face_order(n_faces: int, order: str) -> np.ndarray:
    """Permutation p of the faces: face k of the reordered mesh is face p[k] of the native one."""
    if order == "native":
        return np.arange(n_faces)
    if order == "reversed":
        return np.arange(n_faces)[::-1].copy()
    if order == "shuffled":
        return np.random.default_rng(2024).permutation(n_faces)
    raise ValueError(order)


def reorder(verts, faces, order: str):
    p = face_order(faces.shape[0], order)
    return verts, faces[torch.from_numpy(p)].contiguous()


# make_case mesh kinds built here: kind -> list of (verts, faces) of the case's pool, in pool order
def _kinds():
    k = {"sheet%d" % F: (lambda F=F: [sheet(F)]) for F in SHEET_COUNTS}
    k.update({"ico81k": lambda: [dense_icosphere()], "torus245k": lambda: [dense_torus()],
              "ico81k_reversed": lambda: [reorder(*dense_icosphere(), "reversed")],
              "ico81k_shuffled": lambda: [reorder(*dense_icosphere(), "shuffled")],
              # the variable record layout with a 100x spread of span sizes: torus + teapot-size objects
              "torus_teapots": None,
              # the setup kernel's vertex staging: meshes of 4 096, 4 097 and 122 880 vertices in one pool
              "vstage": lambda: [vertex_sheet(4096), vertex_sheet(4097), dense_torus()]})
    k.update({kind: (lambda kind=kind: [needles(kind)]) for kind in NEEDLE_KINDS})
    return k


DENSE_KINDS = tuple(_kinds())


def dense_pool_meshes(kind: str):
    if kind == "torus_teapots":
        from occlusionenv_amd.meshes import load_obj
        from tests.parity_utils import TEAPOT

        return [dense_torus(), load_obj(TEAPOT)]
    return _kinds()[kind]()


def dense_layout(kind, n_env, x2):
    """Mesh slot of every object (indices into ``dense_pool_meshes(kind)``) and the object offsets of a dense case.
    Sheets and needle patches sit at depths 0 / 1 / 2 in front of the origin, shifted sideways by a tenth of the case's x2 draw (the
    random offsets of the other kinds would push them off screen); the other kinds use make_case's usual offsets."""
    slots = torch.zeros(n_env, 3, dtype=torch.int64)
    if kind == "torus_teapots":  # the torus in one slot of every env, teapots in the others
        slots[:] = 1
        slots[torch.arange(n_env), torch.arange(n_env) % 3] = 0
    elif kind == "vstage":  # every env holds all three meshes, in a rotating order
        slots = (torch.arange(n_env)[:, None] + torch.arange(3)[None, :]) % 3
    offsets = torch.zeros(n_env, 3, 3)
    if kind.startswith("sheet") or kind == "vstage" or kind in NEEDLE_KINDS:
        s = 0.1 * x2.clamp(-2.0, 2.0)
        offsets[:, 1, 0], offsets[:, 1, 1], offsets[:, 1, 2] = s, 0.05, 1.0
        offsets[:, 2, 0], offsets[:, 2, 1], offsets[:, 2, 2] = -s, -0.05, 2.0
    else:
        offsets[:, 1, 0], offsets[:, 1, 2] = x2, 1.0
        offsets[:, 2, 0], offsets[:, 2, 2] = -x2, 2.0
    return slots, offsets


# the sheet cases of the GPU tests: make_case(SHEET_ENVS, SHEET_SEED, "sheet<F>", az_range=SHEET_AZ_RANGE), radius 4
SHEET_SEED = 4095
SHEET_ENVS = 2


def sheet_cameras(case, radius=4.0):
    """(R, T) in f64 of every env of a case, at reset (radius, az, elevation 0) and after its one step (the oracle's
    OracleEnv.reset / step camera, environment.py): [(env, phase, R (3,3), T (3,))]."""
    from oracle import p3d_restate as O

    out = []
    for i in range(case["az"].shape[0]):
        az = torch.tensor([float(case["az"][i])], dtype=torch.float64)
        r = torch.tensor([radius], dtype=torch.float64)
        R, T = O.look_at_view_transform(r, torch.zeros(1, dtype=torch.float64), az)
        out.append((i, "reset", R[0], T[0]))
        a = case["actions"][i].double()
        na = a / a.norm()
        el, az1 = na[0] * O.STEP_SIZE, az[0] + na[1] * O.STEP_SIZE
        C = torch.stack([r[0] * torch.sin(az1) * torch.cos(el), r[0] * torch.sin(az1) * torch.sin(el),
                         r[0] * torch.cos(az1)])[None]
        R = O.look_at_rotation(C)
        out.append((i, "step", R[0], O.translation_from(R, C)[0]))
    return out
