"""Host tests of tests/combine_model.py, the f64 model tests/test_gpu_combine.py holds the combine, reduce and finish
kernels to: the block geometry against brute force, a hand-computed 8 x 8 frame, the strict depth tie, the region-tracking
rule set by induction on the write-set simulator, and the constants against occ_constants.h."""
import numpy as np
import pytest

from tests import combine_model as CM

SIDES = list(range(8, 81, 8)) + [256, 264, 512]


def _random_rect(rng, S, aligned=False):
    """An inclusive pixel rect; one in eight is empty, one in eight the whole frame."""
    k = rng.integers(8)
    if k == 0:
        return CM.empty_rect(S)
    if k == 1:
        return (0, 0, S - 1, S - 1)
    x = np.sort(rng.integers(0, S, 2))
    y = np.sort(rng.integers(0, S, 2))
    if k == 2:  # a single row or column, or a rect that hugs an edge
        y[1] = y[0]
    if k == 3:
        x[0], x[1] = (0, x[0]) if rng.integers(2) else (x[1], S - 1)
    if k == 4:  # inside the first or the last eight columns: what a one-row block of a 264-pixel row can miss
        x = np.sort(rng.integers(0, 8, 2)) + (0 if rng.integers(2) else S - 8)
    r = [int(x[0]), int(y[0]), int(x[1]), int(y[1])]
    if aligned:
        r = [r[0] // 4 * 4, r[1] // 4 * 4, r[2] // 4 * 4 + 3, r[3] // 4 * 4 + 3]
    return tuple(r)


def _block_pixels(blk, S):
    p = np.arange(blk * CM.PIX_BLOCK, min((blk + 1) * CM.PIX_BLOCK, S * S))
    return p // S, p % S


def _some_pixel_in(blk, S, r):
    y, x = _block_pixels(blk, S)
    return bool(((x >= r[0]) & (x <= r[2]) & (y >= r[1]) & (y <= r[3])).any())


@pytest.mark.parametrize("S", SIDES)
def test_block_geometry_against_brute_force(S):
    rng = np.random.default_rng(1000 + S)
    bpe = CM.n_blocks(S)
    assert bpe == -(-S * S // 256)
    tails = [b for b in range(bpe) if CM.block_span(b, S)["tail"]]
    assert tails == ([bpe - 1] if (S * S) % 256 else [])
    one_row = [b for b in range(bpe) if CM.block_span(b, S)["r0"] == CM.block_span(b, S)["r1"]]
    assert bool(one_row) == (S >= 256)
    n_bg = n_col = 0
    for _ in range(300):
        r = _random_rect(rng, S)
        # the block range of a row range: every block that holds a pixel of the rows, and no other
        if CM.is_empty(r):
            assert CM.rows_to_blocks(r[1], r[3], S) == (1, 0)
        else:
            p = np.arange(r[1] * S, (r[3] + 1) * S) // CM.PIX_BLOCK
            assert CM.rows_to_blocks(r[1], r[3], S) == (int(p.min()), int(p.max())), r
        rects = [r, _random_rect(rng, S, aligned=True)]
        blocks = range(bpe) if bpe <= 48 else sorted({0, bpe - 1, bpe - 2, *rng.integers(0, bpe, 40).tolist(), *rng.permutation(one_row)[:12].tolist()})
        for b in blocks:
            hit = [_some_pixel_in(b, S, q) for q in rects]
            for q, h in zip(rects, hit):
                assert CM.meets(b, S, q) or not h, (b, q)  # meets() is a superset of "some pixel of the block lies in the rect"
            if CM.is_background_block(b, S, rects):
                n_bg += 1
                assert not any(hit), (b, rects)  # background implies: no pixel of the block in any rect
                assert not CM.block_span(b, S)["tail"]
                sp = CM.block_span(b, S)
                if sp["r0"] == sp["r1"] and any(sp["r0"] >= q[1] and sp["r0"] <= q[3] for q in rects if not CM.is_empty(q)):
                    n_col += 1  # decided by the column arm
    assert n_bg > 0 or S == 8   # at S = 8 the only block is a tail block
    if S > 256:
        assert n_col > 0


def _planes(S, nan=True):
    fill = np.nan if nan else 0.0
    return (np.full((3, S, S), fill, np.float32), np.full((3, S, S, 2), fill, np.float32), np.full((3, S, S), fill, np.float32),
            np.full((3, S, S), 7, np.int32))


def test_hand_computed_frame():
    """S = 8: object 0 covers columns 0..3 with alpha 1/2, object 1 rows 0..3 with alpha 1/4, object 2 has no records and
    planes full of NaN.  They overlap in 16 pixels: I = 1/8 there, loss = 16 / 64, the el term 2 I (a1 d0 + a0 d1) =
    1/4 (1/4 2 + 1/2 4) = 5/8 per pixel, the az term 1/4 (1/4 (-1) + 1/2 (3/2)) = 1/8 per pixel."""
    S = 8
    alpha, grad, hz, hrec = _planes(S)
    objrect = np.array([[0, 0, 0, 1], [0, 0, 1, 0], [0, 0, 1, 1]], np.int32)
    nrec = np.array([3, 2, 0])
    alpha[0], alpha[1] = 0.5, 0.25
    grad[0], grad[1] = (2.0, -1.0), (4.0, 1.5)
    hz[0], hz[1] = 3.0, 2.0
    hrec[0], hrec[1] = 1, 0
    recs = [np.zeros((3, 32), np.float32), np.zeros((2, 32), np.float32), np.zeros((0, 32), np.float32)]
    m = CM.combine_env(S, alpha, grad, hz, hrec, objrect, nrec, recs, flat=False)
    ys, xs = np.mgrid[0:S, 0:S]
    both = (xs < 4) & (ys < 4)
    assert np.array_equal(m["in_rect"][0], xs < 4) and np.array_equal(m["in_rect"][1], ys < 4) and not m["in_rect"][2].any()
    assert np.array_equal(m["I"], np.where(both, 0.125, 0.0))
    assert np.array_equal(m["alphas"], np.stack([np.where(xs < 4, 0.5, 0), np.where(ys < 4, 0.25, 0), np.zeros((S, S))]).astype(np.float32))
    assert m["frame_sum"].tolist() == [0.25, 10.0, 2.0] and m["block_sum"].tolist() == [[0.25, 10.0, 2.0]]
    assert m["frame_l1"][0] == 0.25 and m["frame_l1"][1] == 10.0 and m["frame_l1"][2] == 16 * 0.25 * (0.25 + 0.75)
    assert m["footprint"] == (0, 0, 7, 7) and m["fp_blocks"] == (0, 0) and not m["bg_block"].any()
    # the nearer object 1 wins where both are, object 0 elsewhere in its rect, background in the last quadrant
    assert np.array_equal(m["depth"], np.where(ys < 4, 2.0, np.where(xs < 4, 3.0, -1.0)).astype(np.float32))
    assert np.array_equal(m["win_obj"][m["hit"]], np.where(ys < 4, 1, 0)[m["hit"]])
    assert np.array_equal(CM.expected_full_state(m)[..., :3], np.full((S, S, 3), 3.0))
    # a weight with zeros takes pixels out of every sum
    wgt = np.where(xs < 2, 0.0, 2.0).astype(np.float32)
    mw = CM.combine_env(S, alpha, grad, hz, hrec, objrect, nrec, recs, pix_weight=wgt, flat=False)
    assert mw["frame_sum"].tolist() == [0.25, 10.0, 2.0]  # half the pixels, twice the weight
    assert np.array_equal(mw["I"], m["I"])
    # reward rule and action Jacobian
    k = CM.header_constants()
    f = CM.finish(np.float32(0.25), np.float32([10.0, 2.0]), np.float32(1.25), np.float32(2.0), np.float32([0.05, 0, 0, 0.05]), k)
    assert not f["done"] and abs(f["reward"] - (0.5 - float(k["kStepPenalty"]))) < 1e-15 and f["full_reward"] == np.float32(0.25)
    assert np.allclose(f["grad_action"], [-10 * float(np.float32(0.05)) / 2, -2 * float(np.float32(0.05)) / 2], rtol=1e-15)
    assert 0 < f["reward_tol"] < 1e-6 and (f["grad_action_tol"] > 0).all()
    # an env with an empty footprint: loss 0, done, reward full_reward / mass + bonus
    e = CM.combine_env(S, alpha, grad, hz, hrec, objrect, np.zeros(3, int), recs, flat=False)
    assert e["footprint"] == CM.empty_rect(S) and e["fp_blocks"] == (1, 0) and not e["frame_sum"].any() and not e["alphas"].any()
    assert (e["depth"] == -1).all() and not e["hit"].any()
    f0 = CM.finish(np.float32(0.0), None, np.float32(1.25), np.float32(2.0), None, k)
    assert f0["done"] and f0["reward"] == 1.25 / 2.0 + float(k["kDoneBonus"]) and "grad_action" not in f0
    assert CM.finish(np.float32(0.1), None, 1.0, 1.0, None, k)["done"] is False  # strict: 0.1f is not below 0.1f
    assert CM.finish(np.nextafter(np.float32(0.1), np.float32(0)), None, 1.0, 1.0, None, k)["done"] is True


def test_flat_colour_of_a_hand_made_record():
    """One record whose three depths are equal: q are the plain barycentrics, they add up to 1 - 1e-8 / area, and the
    colour is R_AMB (q0 + q1 + q2) + R_SPEC."""
    S = 8
    alpha, grad, hz, hrec = _planes(S, nan=False)
    objrect = np.array([[0, 0, 1, 1]] * 3, np.int32)
    rec = np.zeros((1, 32), np.float32)
    rec[0, :9] = [-2, -2, 2.0, 2, -2, 2.0, 0, 2, 2.0]
    area = (0 - -2) * (-2 - -2) - (2 - -2) * (2 - -2)  # edge function of v2 against (v0, v1)
    rec[0, CM.R_INV_AREA], rec[0, CM.R_AMB], rec[0, CM.R_SPEC] = 1.0 / area, 0.75, 0.125
    hz[0], hrec[0] = 2.0, 0
    hrec[0, 0, 0] = -1
    m = CM.combine_env(S, alpha, grad, hz, hrec, objrect, np.array([1, 0, 0]), [rec, rec[:0], rec[:0]], k_epsilon=np.float32(1e-8))
    assert np.allclose(m["colour"][:, 1:, :], 0.875, atol=1e-6) and (m["colour"][:, 0, 0] == 1.0).all() and m["depth"][0, 0] == -1.0
    assert abs(m["den_min"] - 4.0) < 1e-5 and (m["colour_tol"][m["hit"]] > 27 * CM.U * 0.875).all() and m["colour_tol"][0, 0] == 0


def test_strict_depth_tie():
    S = 8
    alpha, grad, hz, hrec = _planes(S, nan=False)
    objrect = np.array([[0, 0, 1, 1]] * 3, np.int32)
    nrec = np.array([1, 1, 1])
    hz[0], hz[1], hz[2] = 2.0, 2.5, 2.0
    hrec[0], hrec[1], hrec[2] = 4, 5, 6
    recs = [np.zeros((8, 32), np.float32)] * 3
    m = CM.combine_env(S, alpha, grad, hz, hrec, objrect, nrec, recs, flat=False)
    assert (m["win_obj"] == 0).all() and (m["win_rec"] == 4).all() and (m["depth"] == 2.0).all()  # equal depth: the earlier object
    hz[2] = np.nextafter(np.float32(2.0), np.float32(0))
    m = CM.combine_env(S, alpha, grad, hz, hrec, objrect, nrec, recs, flat=False)
    assert (m["win_obj"] == 2).all() and (m["win_rec"] == 6).all()
    hz[1], hrec[1] = 1.0, -1  # the nearest object reports no face: background, whatever lies behind
    m = CM.combine_env(S, alpha, grad, hz, hrec, objrect, nrec, recs, flat=False)
    assert not m["hit"].any() and (m["depth"] == -1.0).all()


def _scene_rects(rng, S):
    """0..3 object rects in pixels (4-pixel aligned), with the special cases mixed in: none, the whole frame, single 4 x 4 blocks
    in the corners, objects with an empty rect."""
    nb = S // 4
    k = rng.integers(10)
    if k == 0:
        return []
    if k == 1:
        return [(0, 0, S - 1, S - 1)]
    if k == 2:  # single 4 x 4 blocks in the corners
        corners = [(0, 0), (nb - 1, 0), (0, nb - 1), (nb - 1, nb - 1)]
        pick = rng.permutation(4)[: rng.integers(1, 4)]
        return [(4 * corners[i][0], 4 * corners[i][1], 4 * corners[i][0] + 3, 4 * corners[i][1] + 3) for i in pick]
    out = []
    for _ in range(rng.integers(1, 4)):
        r = _random_rect(rng, S, aligned=True)
        out.append(r)  # (an empty one stays: an object with records and an empty rect)
    return out


@pytest.mark.parametrize("ring", [1, 2, 3])
@pytest.mark.parametrize("S", SIDES)
def test_region_tracking_invariant_by_induction(S, ring):
    """A buffer that is background outside rect_prev equals the full expected frame after the simulated write and is
    background outside rect_next - for ``ring`` output sets used in turn (rect_prev = the footprint of ``ring`` steps
    ago) together with a one-set alphas state, whose previous rect widens the visited range like the kernel's."""
    rng = np.random.default_rng(7 * S + ring)
    bg_o, bg_a = np.array([-1.0]), np.array([0.0])
    sets = [dict(buf=np.full((S * S, 1), -1.0), rect=CM.empty_rect(S)) for _ in range(ring)]
    state = dict(buf=np.zeros((S * S, 1)), rect=CM.empty_rect(S))
    steps = 14 if S <= 80 else 8
    for t in range(steps):
        rects = _scene_rects(rng, S)
        skip = t > 0 and rng.integers(9) == 0
        touched = np.zeros((S, S), bool)
        for r in rects:
            touched |= CM.in_rect_px(S, r)
        vals = rng.integers(-1, 3, (S, S)).astype(np.float64)  # (some pixels inside a rect hold the background value too)
        exp_o = np.where(touched, vals, -1.0).reshape(-1, 1)
        exp_a = np.where(touched, np.maximum(vals, 0.0), 0.0).reshape(-1, 1)
        cur = sets[t % ring]
        before_o, before_a = cur["buf"].copy(), state["buf"].copy()
        new_o, rect_o = CM.simulate_tracked_write(cur["buf"], cur["rect"], exp_o, bg_o, rects, S, other_prev=state["rect"], skip=skip)
        new_a, rect_a = CM.simulate_tracked_write(state["buf"], state["rect"], exp_a, bg_a, rects, S, other_prev=cur["rect"], skip=skip)
        if skip:
            assert np.array_equal(new_o, before_o) and np.array_equal(new_a, before_a)
            assert rect_o == tuple(cur["rect"]) and rect_a == tuple(state["rect"])
        else:
            assert np.array_equal(new_o, exp_o), (S, ring, t, rects, cur["rect"])
            assert np.array_equal(new_a, exp_a), (S, ring, t, rects, state["rect"])
            assert rect_o == rect_a
        for buf, rect, bg in ((new_o, rect_o, -1.0), (new_a, rect_a, 0.0)):
            assert (buf.reshape(S, S)[~CM.in_rect_px(S, rect)] == bg).all()
        cur["buf"], cur["rect"] = new_o, rect_o
        state["buf"], state["rect"] = new_a, rect_a


def test_the_simulator_needs_each_of_its_rules():
    """The induction above is not vacuous: without the previous rect in the visited range, or without the clear of a
    background block that meets it, stale content survives."""
    S = 64
    big, small = (8, 8, 55, 55), (24, 24, 31, 31)
    frame = np.where(CM.in_rect_px(S, big), 2.0, -1.0).reshape(-1, 1)
    buf, rect = CM.simulate_tracked_write(np.full((S * S, 1), -1.0), CM.empty_rect(S), frame, np.array([-1.0]), [big], S)
    assert np.array_equal(buf, frame) and rect == big
    frame2 = np.where(CM.in_rect_px(S, small), 5.0, -1.0).reshape(-1, 1)
    ok, _ = CM.simulate_tracked_write(buf, rect, frame2, np.array([-1.0]), [small], S)
    assert np.array_equal(ok, frame2)
    stale, _ = CM.simulate_tracked_write(buf, CM.empty_rect(S), frame2, np.array([-1.0]), [small], S)  # the rect forgotten
    assert not np.array_equal(stale, frame2)
    c = CM.classify(S, [small], small, big)
    assert c["strictly_inside_prev"] and c["bg_meets_prev"] > 0 and not c["empty_footprint"] and not c["tail_visited"]
    assert CM.classify(72, [], CM.empty_rect(72), (0, 60, 71, 71))["tail_visited"]
    assert CM.classify(264, [], CM.empty_rect(264), (40, 40, 200, 200))["one_row_partial"] > 0


def test_constants_and_slots_are_those_of_the_sources():
    from occlusionenv_amd import _native as nat
    from tests import setup_model as M

    k = CM.header_constants()
    assert (k["kDoneThreshold"], k["kDoneBonus"], k["kStepPenalty"]) == (np.float32(0.1), np.float32(5.0), np.float32(0.2))
    assert k["kEpsilon"] == np.float32(1e-8)
    for i, name in enumerate(("R_X0", "R_Y0", "R_Z0", "R_X1", "R_Y1", "R_Z1", "R_X2", "R_Y2", "R_Z2")):
        assert k[name] == i == getattr(CM, name)
    assert (k["R_INV_AREA"], k["R_AMB"], k["R_SPEC"], k["C_J"]) == (CM.R_INV_AREA, CM.R_AMB, CM.R_SPEC, CM.C_J)
    assert (M.R_INV_AREA, M.R_AMB, M.R_SPEC, M.C_J) == (CM.R_INV_AREA, CM.R_AMB, CM.R_SPEC, CM.C_J)
    assert (nat.C_J, nat.CAM_STRIDE, nat.REC_STRIDE) == (CM.C_J, CM.CAM_STRIDE, CM.REC_STRIDE)
    assert nat.TILE == 2 * CM.OCC_BLOCK
    import os
    import re

    from tests.parity_utils import ROOT

    text = open(os.path.join(ROOT, "include", "occlusionenv_amd.h")).read()
    assert int(re.search(r"#define OCC_BLOCK (\d+)", text).group(1)) == CM.OCC_BLOCK
    assert int(re.search(r"#define OCC_REC_STRIDE (\d+)", text).group(1)) == CM.REC_STRIDE
