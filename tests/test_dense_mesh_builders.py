"""The dense test meshes (tests/dense_meshes.py) are what the GPU tests of tests/test_gpu_dense_meshes.py take them
for: exact face and vertex counts, within the reference's mesh limit, and sheets whose every face the setup kernel
must turn into exactly one record at the cameras those tests use (checked with the oracle's own f64 projection)."""
import numpy as np
import pytest
import torch

from tests import dense_meshes as D


def test_dense_mesh_counts_and_limit():
    v, f = D.dense_icosphere()
    assert (v.shape[0], f.shape[0]) == (40962, 81920)
    v, f = D.dense_torus()
    assert (v.shape[0], f.shape[0]) == (122880, 245760)
    assert f.shape[0] <= D.MAX_MESH_FACES
    for F in D.SHEET_COUNTS:
        assert D.sheet(F)[1].shape[0] == F
    for nV in D.VERTEX_COUNTS:
        assert D.vertex_sheet(nV)[0].shape[0] == nV
    for kind in D.DENSE_KINDS:
        for v, f in D.dense_pool_meshes(kind):
            assert f.shape[0] <= D.MAX_MESH_FACES
            assert int(f.min()) >= 0 and int(f.max()) < v.shape[0]
            assert torch.unique(f).numel() == v.shape[0], (kind, "every vertex is used")


def test_face_order_variants_are_permutations_of_the_same_faces():
    v, f = D.dense_icosphere()
    for order in D.ORDERS:
        v2, f2 = D.reorder(v, f, order)
        p = D.face_order(f.shape[0], order)
        assert torch.equal(v2, v)
        assert torch.equal(f2, f[torch.from_numpy(p)])
        assert np.array_equal(np.sort(p), np.arange(f.shape[0]))
    assert not np.array_equal(D.face_order(100, "shuffled"), np.arange(100))


@pytest.mark.parametrize("kind", ["sheet%d" % F for F in D.SHEET_COUNTS] + ["vstage"])
def test_sheet_faces_all_front_facing_on_screen_unclipped(kind):
    """At the reset and step cameras of the GPU sheet cases, every face of every sheet object is front-facing with an
    NDC area far above kEpsilon, inside the image and far in front of the clip plane (f64 projection of the oracle)."""
    from oracle import p3d_restate as O
    from tests.parity_utils import make_case

    case = make_case(D.SHEET_ENVS, D.SHEET_SEED, kind, az_range=D.SHEET_AZ_RANGE, device="cpu")
    for i, phase, R, T in D.sheet_cameras(case):
        for o in range(3):
            v, f = case["pool"].get(int(case["mesh_ids"][i, o]))
            if f.shape[0] > 10000:  # (vstage: the torus is no sheet)
                continue
            ndc = O.world_to_ndc(v.double() + case["offsets"][i, o].double(), R, T)
            fv = ndc[f]
            x, y = fv[..., 0], fv[..., 1]
            area = (x[:, 0] - x[:, 1]) * (y[:, 2] - y[:, 1]) - (y[:, 0] - y[:, 1]) * (x[:, 2] - x[:, 1])
            assert float(area.min()) > 1e-6, (kind, i, phase, o, float(area.min()))
            assert float(fv[..., :2].abs().max()) < 0.9, (kind, i, phase, o)
            assert float(fv[..., 2].min()) > 1.5, (kind, i, phase, o)


@pytest.mark.parametrize("kind", D.NEEDLE_KINDS)
def test_needles_have_one_degenerate_edge_in_the_promised_slot_and_a_visible_area(kind):
    """In f64 at radius 4, az 0, for the three objects of the needle layout: every face is front-facing with exactly ONE
    edge of |edge|^2 <= kEpsilon / 4 - the one the kind names - and an area (edge function) of at least 16 kEpsilon; the
    margins are wide enough that the f32 projection noise TVERT per vertex decides neither.  The three kinds are the
    same needles with the vertex order rotated."""
    from oracle import p3d_restate as O
    from tests.parity_utils import TVERT, make_case

    case = make_case(1, 0, kind, az_range=0.0, device="cpu")
    assert float(case["az"][0]) == 0.0
    R, T = O.look_at_view_transform(torch.tensor([4.0], dtype=torch.float64), torch.zeros(1, dtype=torch.float64),
                                    torch.zeros(1, dtype=torch.float64))
    slot = D.needle_short_slot(kind)
    assert (("needles01", "needles02", "needles12")[slot], slot) == (kind, D.NEEDLE_KINDS.index(kind))
    for o in range(3):
        v, f = case["pool"].get(int(case["mesh_ids"][0, o]))
        assert f.shape[0] == D.NEEDLE_COUNT and 200 <= f.shape[0] <= 600
        fv = O.world_to_ndc(v.double() + case["offsets"][0, o].double(), R[0], T[0])[f].numpy()
        x, y = fv[..., 0], fv[..., 1]
        l2 = np.stack([(x[:, b] - x[:, a]) ** 2 + (y[:, b] - y[:, a]) ** 2 for a, b in ((0, 1), (0, 2), (1, 2))], 1)
        short = l2 <= 1e-8 / 4
        assert (short.sum(1) == 1).all() and short[:, slot].all(), (kind, o)
        area = (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0]) - (y[:, 2] - y[:, 0]) * (x[:, 1] - x[:, 0])  # E(v2; v0, v1) > 0: front
        assert float(area.min()) >= 16 * 1e-8, (kind, o, float(area.min()))
        # noise: each end of an edge moves by at most TVERT in x and in y -> its length by 2 sqrt 2 TVERT; the area by
        # TVERT x perimeter (tests/parity_utils.py, TAREA)
        per = np.sqrt(l2).sum(1)
        assert ((np.sqrt(l2[:, slot]) + 2 * np.sqrt(2) * TVERT) ** 2 < 1e-8 * 0.5).all()
        others = np.delete(l2, slot, axis=1)
        assert ((np.sqrt(others) - 2 * np.sqrt(2) * TVERT) ** 2 > 1e-8 * 1e4).all()
        assert (area - TVERT * per > 2 * 1e-8).all()
        assert float(np.abs(fv[..., :2]).max()) < 0.9 and float(fv[..., 2].min()) > 1.5  # on screen, far from the clip plane
    v0, f0 = D.needles("needles01")
    v1, _ = D.needles(kind)
    r = {"needles01": (0, 1, 2), "needles02": (1, 2, 0), "needles12": (2, 0, 1)}[kind]
    assert torch.equal(v1[f0], v0[f0][:, r, :])
    # directions all round the clock: every octant holds needles
    d = (v0[f0][:, 2, :2] - v0[f0][:, 0, :2]).numpy()
    assert np.bincount((np.floor(np.arctan2(d[:, 1], d[:, 0]) / (np.pi / 4)).astype(int) + 4) % 8, minlength=8).min() >= 20
