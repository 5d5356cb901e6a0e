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
