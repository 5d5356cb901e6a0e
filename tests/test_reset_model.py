"""Hand-worked cases that pin the host model of the auto-reset contract (tests/reset_model.py), which the GPU tests of
tests/test_gpu_auto_reset_kernels.py hold the kernels to.  Every row of an image-sized buffer holds one constant, so an
expected buffer is written out literally as its row constants."""
import numpy as np
import pytest

from tests import reset_model as M

S = 8
S2 = S * S
F32_01 = np.float32(0.1)
ABOVE = np.nextafter(F32_01, np.float32(1))
BELOW = np.nextafter(F32_01, np.float32(0))


def _rows(base, n, width):
    return np.repeat(np.float32(base) + np.arange(n, dtype=np.float32), width)


def _state(N, R, **over):
    """Buffers of occ_auto_reset with a distinct constant per row: what moved where is readable from the values."""
    NT = N + R
    a = dict(done=np.zeros(N, np.uint8), loss_all=np.full(NT, 0.9, np.float32), status=np.zeros(NT, np.int32),
             rs_state=np.zeros(R, np.int32), rs_tries=np.zeros(R, np.int32),
             el=_rows(1000, NT, 1), az=_rows(2000, NT, 1), radius=_rows(3000, NT, 1), campos=np.full(3 * N, 7, np.float32),
             cam=_rows(4000, NT, M.CAM_STRIDE), alphas=_rows(5000, NT, 3 * S2), full_reward=np.full(N, -1, np.float32),
             object_mass=np.full(N, -2, np.float32), scene_mesh=np.repeat(6000 + np.arange(NT, dtype=np.int32), 3),
             scene_offset=_rows(7000, NT, 9), obs_all=_rows(100, NT, 4 * S2), full_state_all=_rows(200, NT, 4 * S2),
             store_obs=_rows(300, R, 4 * S2), store_fs=_rows(400, R, 4 * S2), store_loss=np.zeros(R, np.float32),
             skip=np.full(NT, 9, np.int32), term_obs=np.full(R * 4 * S2, -5, np.float32),
             report=np.full(N + 2 * R + 2, -7, np.int32))
    for k, v in over.items():
        a[k] = np.asarray(v, dtype=a[k].dtype if k in a else None)
    return a


def _rowvals(buf, width):
    """The constant of every row of ``buf`` (asserting that each row is one)."""
    r = np.asarray(buf).reshape(-1, width)
    assert (r == r[:, :1]).all() | (np.isnan(r) & np.isnan(r[:, :1])).all()
    return r[:, 0].tolist()


def _f32(v):
    return np.asarray(v, dtype=np.float32).tolist()


def _unchanged(a, o, *names):
    for k in names:
        assert np.array_equal(np.asarray(a[k]).reshape(-1).view(np.uint8), o[k].view(np.uint8)), k


def test_tenth_try_is_kept_whatever_its_loss():
    a = _state(1, 3, rs_state=[1, 1, 1], rs_tries=[8, 9, 0], loss_all=[0.9, 0.05, 0.05, 0.05])
    o = M.auto_reset(a, 1, 3, S)
    assert o["rs_state"].tolist() == [0, 2, 0]   # 9th try rejected, 10th kept, 1st rejected
    assert o["rs_tries"].tolist() == [9, 10, 1]  # a rejected slot keeps its count
    assert o["skip"].tolist() == [9, 1, 1, 1]    # rows < n_env are not the call's
    assert o["report"].tolist() == [0, 0, 2, 0, -1, -1, -1, 0, 0]
    # all three were rendered now and nobody takes them: the store holds this step's rows, whatever the new state
    assert _rowvals(o["store_obs"], 4 * S2) == [101, 102, 103]
    assert _rowvals(o["store_fs"], 4 * S2) == [201, 202, 203]
    assert o["store_loss"].tolist() == _f32([0.05, 0.05, 0.05])
    _unchanged(a, o, "obs_all", "term_obs", "el", "alphas", "full_reward", "object_mass", "campos", "status", "done")


def test_acceptance_is_strictly_above_float32_point_one():
    loss = np.array([0.9, F32_01, ABOVE, BELOW, np.nan], np.float32)
    a = _state(1, 4, rs_state=[1, 1, 1, 1], loss_all=loss)
    o = M.auto_reset(a, 1, 4, S)
    assert o["rs_state"].tolist() == [0, 2, 0, 0]  # 0.1 exactly: rejected; one ulp above: kept; NaN: rejected
    assert o["rs_tries"].tolist() == [1, 1, 1, 1]
    assert o["report"].tolist() == [0, 0, 2, 0, 0, -1, -1, -1, -1, 0, 0]
    assert M.step_flags(np.array([1], np.uint8), loss, np.zeros(5, np.int32), 1, 4).tolist() == [1, 0, 1, 0, 0, 0]
    assert M.step_flags(np.array([0], np.uint8), None, np.array([0, 3], np.int32), 1, 0).tolist() == [0, 0]
    assert M.step_flags(np.array([0], np.uint8), loss, np.array([0, 0, 0, 0, 3], np.int32), 1, 4).tolist() == [0, 0, 1, 0, 0, 1]


def test_done_wins_over_the_time_limit_and_finished_envs_outnumber_ready_slots():
    a = _state(4, 2, rs_state=[2, 2], store_loss=[0.25, 0.75], loss_all=[0.01] * 4 + [0.9, 0.9], done=[0, 1, 0, 1])
    a.update(age=np.array([4, 9, 9, 0], np.int32), rect=np.full(6 * 4, 55, np.int32), arect=np.full(6 * 4, 56, np.int32),
             reset_full_state=np.full(2 * 4 * S2, -6, np.float32),
             report_host=np.array([0, 0, 0, 0] + [-3] * 6, np.int32))
    o = M.auto_reset(a, 4, 2, S, max_ep_len=10)
    # env 0 ages to 5; env 1 is done and at the limit: done wins (1); env 2 reaches the limit (2); env 3 is done
    assert o["report"].tolist() == [0, 1, 2, 1, 0, 0, 1, 2, 0, 1]  # three finished, two slots: one left without
    assert o["report_host"].tolist() == [0, 1, 2, 1, 0, 0, 1, 2, 0, 1]
    assert o["age"].tolist() == [5, 0, 0, 1]
    assert o["rs_state"].tolist() == [0, 0] and o["rs_tries"].tolist() == [0, 0]
    assert o["skip"].tolist() == [9, 9, 9, 9, 1, 1]
    assert o["el"].tolist() == [1000, 1004, 1005, 1003, 1004, 1005]
    assert o["radius"].tolist() == [3000, 3004, 3005, 3003, 3004, 3005]
    assert _rowvals(o["cam"], M.CAM_STRIDE) == [4000, 4004, 4005, 4003, 4004, 4005]
    assert _rowvals(o["alphas"], 3 * S2) == [5000, 5004, 5005, 5003, 5004, 5005]
    assert o["scene_mesh"].reshape(-1, 3)[:, 0].tolist() == [6000, 6004, 6005, 6003, 6004, 6005]
    assert _rowvals(o["scene_offset"], 9) == [7000, 7004, 7005, 7003, 7004, 7005]
    assert _rowvals(o["campos"], 3) == [7, 0, 0, 7]
    assert o["full_reward"].tolist() == [-1, 0.25, 0.75, -1]  # READY slots: the stored loss
    assert o["object_mass"].tolist() == [-2, 1.25, 1.75, -2]
    assert _rowvals(o["obs_all"], 4 * S2) == [100, 300, 301, 103, 104, 105]  # from the store
    assert _rowvals(o["term_obs"], 4 * S2) == [101, 102]
    assert _rowvals(o["reset_full_state"], 4 * S2) == [400, 401]
    assert o["rect"].reshape(-1, 4).tolist() == [[55] * 4, [0, 0, 7, 7], [0, 0, 7, 7], [55] * 4, [55] * 4, [55] * 4]
    assert o["arect"].reshape(-1, 4).tolist() == [[56] * 4, [0, 0, 7, 7], [0, 0, 7, 7], [56] * 4, [56] * 4, [56] * 4]
    _unchanged(a, o, "store_obs", "store_fs", "store_loss", "full_state_all", "loss_all")


def test_a_slot_taken_in_the_call_that_made_it_ready_and_more_ready_slots_than_finished_envs():
    a = _state(3, 4, rs_state=[0, 1, 2, 2], rs_tries=[5, 3, 0, 0], done=[1, 255, 0],
               loss_all=[0.01, 0.01, 0.01, 0.9, 0.5, 0.9, 0.9], store_loss=[0.0, 0.0, 0.75, 0.125])
    a.update(norm_flags=np.array([1, 0, 1], np.int32), slot_objsum=np.array([10, 20, 30, 40], np.float32),
             reset_full_state=np.full(4 * 4 * S2, -6, np.float32))
    o = M.auto_reset(a, 3, 4, S)
    # slot 1 passes now and goes to env 0 at once; env 1 takes slot 2; slot 3 stays READY; EMPTY slot 0 is left alone
    assert o["rs_state"].tolist() == [0, 0, 0, 2] and o["rs_tries"].tolist() == [5, 0, 0, 0]
    assert o["report"].tolist() == [1, 1, 0, 0, 0, 0, 2, -1, 0, 1, -1, 0, 0]
    assert o["skip"].tolist() == [9, 9, 9, 1, 1, 1, 1]
    assert o["full_reward"].tolist() == [0.5, 0.75, -1]
    assert o["object_mass"].tolist() == [21, 1.75, -2]  # env 0: the slot's silhouette mass + 1; env 1: its loss + 1
    assert _rowvals(o["obs_all"], 4 * S2) == [104, 302, 102, 103, 104, 105, 106]  # this step's row / the store
    assert _rowvals(o["reset_full_state"], 4 * S2) == [-6, 204, 402, -6]
    assert _rowvals(o["term_obs"], 4 * S2) == [-5, 100, 101, -5]
    assert o["az"].tolist() == [2004, 2005, 2002, 2003, 2004, 2005, 2006]
    _unchanged(a, o, "store_obs", "store_fs", "store_loss")  # a slot that is taken is not stashed


def test_no_ready_slot_and_a_status_word_in_a_reserve_row():
    a = _state(2, 2, rs_state=[0, 1], rs_tries=[2, 4], done=[1, 1], loss_all=[0.01, 0.01, 0.9, 0.02],
               status=[0, 0, 0, 4])
    o = M.auto_reset(a, 2, 2, S)
    assert o["rs_state"].tolist() == [0, 0] and o["rs_tries"].tolist() == [2, 5]
    assert o["report"].tolist() == [1, 1, 0, 0, -1, -1, 1, 2]
    assert o["skip"].tolist() == [9, 9, 1, 1]
    assert o["store_loss"].tolist() == _f32([0, 0.02])
    _unchanged(a, o, "obs_all", "el", "full_reward", "object_mass", "term_obs", "alphas")


def test_nobody_finished_leaves_every_env_row_alone():
    a = _state(2, 3, rs_state=[2, 1, 0], rs_tries=[0, 0, 1], loss_all=[0.01, 0.01, 0.9, 0.9, 0.9])
    a.update(age=np.array([3, 3], np.int32))
    o = M.auto_reset(a, 2, 3, S, max_ep_len=5)
    assert o["report"].tolist() == [0, 0, 2, 2, 0, -1, -1, -1, 0, 0] and o["age"].tolist() == [4, 4]
    assert o["skip"].tolist() == [9, 9, 1, 1, 1]  # the PENDING slot is READY now: not rendered again
    _unchanged(a, o, "obs_all", "el", "cam", "alphas", "full_reward", "object_mass", "campos", "term_obs")


def test_reserve_refill_ignores_rows_outside_the_reserve_and_keeps_offset_bits():
    N, R = 2, 2
    bits = np.array([0x80000000, 0x7FC12345, 0x3FC00000, 0xFF800001, 1, 0, 0x40490FDB, 0xBF800000, 0x00000001],
                    np.uint32).view(np.int32)
    packed = np.array([[1, 7, 8, 9, *bits], [-1, 1, 1, 1, *bits], [2, 1, 1, 1, *bits]], np.int32)
    mesh, off, st, sk = M.reserve_refill(packed, 3, N, R, np.full(12, -1, np.int32), np.full(36, 5, np.float32),
                                         np.array([0, 2], np.int32), np.full(4, 1, np.int32))
    assert mesh.tolist() == [-1] * 9 + [7, 8, 9]
    assert off.view(np.int32)[27:].tolist() == bits.tolist() and off[:27].tolist() == [5] * 27
    assert st.tolist() == [0, 1] and sk.tolist() == [1, 1, 1, 0]


def test_reset_commit_copies_the_rows_and_sets_reward_and_mass():
    N, R = 3, 2
    NT = N + R
    pairs = np.array([2, 4, 0, 3], np.int32)
    o = M.reset_commit(pairs, 2, _rows(1000, NT, 1), _rows(2000, NT, 1), _rows(3000, NT, 1), np.full(3 * N, 7, np.float32),
                       _rows(4000, NT, M.CAM_STRIDE), _rows(5000, NT, 3 * S2), np.full(N, -1, np.float32),
                       np.full(N, -2, np.float32), np.repeat(np.arange(NT, dtype=np.int32), 3), _rows(7000, NT, 9),
                       np.full(N * 4 * S2, -3, np.float32), _rows(100, NT, 4 * S2),
                       np.array([0, 0, 0, 0.25, 0.5], np.float32), S)
    assert o["el"].tolist() == [1003, 1001, 1004, 1003, 1004]
    assert o["full_reward"].tolist() == [0.25, -1, 0.5] and o["object_mass"].tolist() == [1.25, -2, 1.5]
    assert _rowvals(o["obs"], 4 * S2) == [103, -3, 104]
    assert _rowvals(o["campos"], 3) == [0, 7, 0]
    assert _rowvals(o["alphas"], 3 * S2) == [5003, 5001, 5004, 5003, 5004]
    assert o["scene_mesh"].reshape(-1, 3)[:, 0].tolist() == [3, 1, 4, 3, 4]


def test_object_mass_of_a_hand_worked_row():
    al = np.zeros((2, 3, 2, 2), np.float32)
    al[0, 0, 0, 0], al[0, 1, 0, 0], al[0, 2, 1, 1] = 1.0, 0.5, 2.0  # (1 + 0.5)^2 + 2^2
    al[1] = 1.0                                                       # 4 pixels of (1 + 1 + 1)^2
    assert M.object_mass(al, 2, 2).tolist() == [6.25, 36.0]
    assert M.object_mass_bound([1.0], 16).tolist() == [13 * 2.0 ** -24]


@pytest.mark.parametrize("nfin,nready", [(5, 2), (2, 5), (0, 3), (3, 0)])
def test_pairing_is_in_index_order(nfin, nready):
    fin = np.zeros(9, np.int32)
    fin[np.arange(nfin) * 2] = 1
    st = np.zeros(6, np.int32)
    st[5 - np.arange(nready)] = M.RS_READY
    pairs, n = M.pair(fin, st, 6)
    assert n == nfin and len(pairs) == min(nfin, nready)
    assert pairs == list(zip((np.arange(nfin) * 2).tolist(), sorted((5 - np.arange(nready)).tolist())))[:len(pairs)]
