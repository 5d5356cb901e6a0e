"""A float64 host model of the tail of a step (occ_combine.hpp: occ_combine_kernel, occ_reduce_kernel, finish_one /
occ_finish_kernel), in numpy.  It needs no GPU and no oracle: the tail is a pure function of planes the raster kernel
leaves in the workspace (obj_alpha, obj_grad, obj_hz, obj_hrec, objrect, nrec), of the face records, the camera buffer,
the optional pixel weights and the reward state, and tests/test_gpu_combine.py hands it snapshots of those.

The model restates the kernel's RULES from their comments and from DESIGN 4.3; it shares no code with the kernel.

    in_rect[o]   nrec[o] > 0 and the pixel's 4 x 4 block lies inside objrect[o] (4-pixel units, inclusive).  A plane value
                 outside in_rect is stale and is never read: alpha, gradient are 0 there, depth is +inf, record -1.
    I            a0 a1 + a1 a2 + a0 a2
    loss term    w I^2;   gradient terms  w 2 I (g0 d0 + g1 d1 + g2 d2),  g_o = sum of the two other alphas
    winner       objects in order 0, 1, 2; a STRICTLY smaller depth wins; record < 0: background, depth -1
    flat colour  R_AMB (q0 + q1 + q2) + R_SPEC of the winning record, q = perspective-correct barycentrics
    footprint    union of the non-empty object rects with nrec > 0, in pixels; empty = (S, S, -1, -1)
    blocks       256 consecutive pixels of the row-major frame; the last one is a TAIL block when S S is no multiple of 256
    finish       reward = (full_reward - loss) / object_mass, + kDoneBonus when loss < kDoneThreshold else - kStepPenalty

REGION TRACKING (``simulate_tracked_write``): a persistent buffer holds background outside the rect it recorded last.
The kernel visits the blocks that meet the pixel rows of the footprint or of one of the previous rects.  A visited block
none of whose pixels can lie in an object rect (the BACKGROUND rule: a block that stays inside one pixel row is tested
against rows and columns, a block that spans rows against rows only) writes constants, and only if it ``meets`` the
buffer's previous rect by the same test.  Every other block, and always the tail block, goes pixel by pixel: a pixel is
written if it lies in an object rect of this step or inside the previous rect.

TOLERANCES.  u = 2^-24, gamma(n) = n u / (1 - n u): n roundings on non-negative data.  Every bound below is a count of
the roundings in the kernel's expression (a contraction into an FMA only removes one); none is fitted to an output.
    I            3 products, 2 additions, every term non-negative: a term passes <= 3 roundings; handed out as 4 u I.
    loss term    w (I I): I carries 3, the square doubles them and adds 1, the weight adds 1: C_LOSS = 8.
    grad term    g_o 1, g_o d_o 1 more, two additions of signed terms: 4 on sum |g_o d_o|; 2 I exact x 3; the product with
                 it 1; the weight 1: C_GRAD = 9, relative to the L1 form w 2 I sum |g_o d_o|.
    block sum    6 DPP levels + 3 serial additions of the four wave sums (0 + x is exact): DEPTH_BLOCK = 9.
    reduce       a lane adds ceil(blocks in range / 64) partials one after the other, then 6 DPP levels.
    finish       subtraction, division, addition: 3 on |full_reward - loss| / mass + |constant|; the action gradient:
                 two products, an addition, a division: 4 on (|ge J| + |ga J|) / mass.
    flat colour  the pixel centre 2 (division, addition); a difference of it 1 more: 3; the other difference 1; their
                 product 1: 5; the subtraction of the two products 1; times 1 / area 1: b carries 7; w = b z z 2 more: 9;
                 the sum of the three w 2: 11; the division (2.5 ulp at worst) 3: q carries 9 + 11 + 3 = 23; q0 + q1 + q2
                 2; R_AMB x + R_SPEC 2: C_FLAT = 27 on |R_AMB| max(1, sum |q_i|) + |R_SPEC|.
"""
from __future__ import annotations

import math
import os
import re

import numpy as np

U = 2.0 ** -24
OCC_BLOCK = 4      # include/occlusionenv_amd.h: unit of objrect
PIX_BLOCK = 256    # pixels per block of the combine kernel
REC_STRIDE, CAM_STRIDE = 32, 48
R_X0, R_Y0, R_Z0, R_X1, R_Y1, R_Z1, R_X2, R_Y2, R_Z2 = range(9)
R_INV_AREA, R_AMB, R_SPEC = 11, 12, 19
C_J = 39
C_LOSS, C_GRAD, C_FLAT, DEPTH_BLOCK, DPP_LEVELS = 8, 9, 27, 9, 6
HZ_NONE = np.float32(3.0e38)  # the kernel's start value of the nearest depth
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "occlusionenv_amd", "csrc", "occ_constants.h")


def gamma(n):
    return n * U / (1.0 - n * U)


def header_constants(path=HEADER):
    """kDoneThreshold, kDoneBonus, kStepPenalty, kEpsilon as float32, and the integer slot maps, read from occ_constants.h."""
    text = open(path).read()
    out = {}
    for name in ("kDoneThreshold", "kDoneBonus", "kStepPenalty", "kEpsilon"):
        m = re.search(r"\b%s = ([0-9.eE+-]+)f\b" % name, text)
        assert m, name
        out[name] = np.float32(float(m.group(1)))
    out.update({k: int(v) for k, v in re.findall(r"\b((?:C|R)_[A-Z0-9_]+) = (\d+)", text)})
    return out


# ---- block geometry ---------------------------------------------------------------------------------------------------
def n_blocks(S):
    return (S * S + PIX_BLOCK - 1) // PIX_BLOCK


def empty_rect(S):
    return (S, S, -1, -1)


def is_empty(r):
    return r[2] < r[0] or r[3] < r[1]


def rows_to_blocks(y0, y1, S):
    """First and last block that hold a pixel of rows y0..y1 (inclusive); (1, 0) for no rows."""
    if y1 < y0:
        return 1, 0
    return max((y0 * S) // PIX_BLOCK, 0), min(((y1 + 1) * S - 1) // PIX_BLOCK, n_blocks(S) - 1)


def block_span(blk, S):
    """p0, p1 (first and last pixel index, p1 may lie beyond the frame), r0, r1 (rows of those), c0, c1 (column of p0 and
    c0 + 255: a column span only when r0 == r1) and whether the block is the partly live TAIL block."""
    p0 = blk * PIX_BLOCK
    p1 = p0 + PIX_BLOCK - 1
    r0, r1 = p0 // S, p1 // S
    c0 = p0 - r0 * S
    return dict(p0=p0, p1=p1, r0=r0, r1=r1, c0=c0, c1=c0 + PIX_BLOCK - 1, tail=p1 >= S * S)


def meets(blk, S, rect):
    """The kernel's conservative test "this block may hold a pixel of rect (x0, y0, x1, y1)": rows always; columns only
    for a block that stays inside one row."""
    b = block_span(blk, S)
    x0, y0, x1, y1 = (int(v) for v in rect)
    return b["r1"] >= y0 and b["r0"] <= y1 and (b["r0"] != b["r1"] or (b["c1"] >= x0 and b["c0"] <= x1))


def rect_pixels(objrect_row):
    """An object rect in 4-pixel units -> pixels."""
    x0, y0, x1, y1 = (int(v) for v in objrect_row)
    return (x0 * OCC_BLOCK, y0 * OCC_BLOCK, x1 * OCC_BLOCK + OCC_BLOCK - 1, y1 * OCC_BLOCK + OCC_BLOCK - 1)


def live_object_rects(objrect, nrec):
    """Pixel rects of the objects the kernel's rules look at: nrec > 0 (an empty rect stays in the list: the block tests
    apply their formula to it as it is, the footprint leaves it out)."""
    return [rect_pixels(objrect[o]) for o in range(3) if int(nrec[o]) > 0]


def footprint(objrect, nrec, S):
    u = list(empty_rect(S))
    for r in live_object_rects(objrect, nrec):
        if not is_empty(r):
            u = [min(u[0], r[0]), min(u[1], r[1]), max(u[2], r[2]), max(u[3], r[3])]
    return tuple(u)


def is_background_block(blk, S, obj_rects):
    """The fast path's rule: a whole block (never the tail) that meets no object rect."""
    return not block_span(blk, S)["tail"] and not any(meets(blk, S, r) for r in obj_rects)


def visited_range(S, fp, prev_rects):
    """Blocks a fully tracked launch visits: the rows of the footprint and of every non-empty previous rect."""
    y0, y1 = fp[1], fp[3]
    for r in prev_rects:
        if r is not None and not is_empty(r):
            y0, y1 = min(y0, int(r[1])), max(y1, int(r[3]))
    return rows_to_blocks(y0, y1, S)


def in_rect_px(S, rect):
    """(S, S) bool: pixels inside the inclusive pixel rect."""
    ys, xs = np.mgrid[0:S, 0:S]
    return (xs >= rect[0]) & (xs <= rect[2]) & (ys >= rect[1]) & (ys <= rect[3])


def classify(S, obj_rects, fp, rect_prev, other_prev=None, tracked=True):
    """Coverage conditions of one (env, launch), from its rects alone.  ``rect_prev``: the previous rect of the buffer
    looked at, ``other_prev``: that of the other tracked buffer (both widen the visited range)."""
    b0, b1 = visited_range(S, fp, [rect_prev, other_prev]) if tracked else (0, n_blocks(S) - 1)
    c = dict(empty_footprint=is_empty(fp), empty_prev_nonempty_fp=False, strictly_inside_prev=False, bg_meets_prev=0,
             bg_blocks=0, tail_visited=False, one_row_partial=0, visited=(b0, b1))
    if rect_prev is None:
        return c
    rp = tuple(int(v) for v in rect_prev)
    c["empty_prev_nonempty_fp"] = is_empty(rp) and not is_empty(fp)
    c["strictly_inside_prev"] = (not is_empty(fp) and not is_empty(rp) and fp[0] > rp[0] and fp[1] > rp[1] and fp[2] < rp[2]
                                 and fp[3] < rp[3])
    for blk in range(b0, b1 + 1):
        b = block_span(blk, S)
        if b["tail"]:
            c["tail_visited"] = True
        if is_background_block(blk, S, obj_rects):
            c["bg_blocks"] += 1
            if meets(blk, S, rp):
                c["bg_meets_prev"] += 1
                if b["r0"] == b["r1"] and not (rp[0] <= b["c0"] and min(b["c1"], S - 1) <= rp[2]):
                    c["one_row_partial"] += 1
    return c


# ---- the frames ---------------------------------------------------------------------------------------------------------
def combine_env(S, alpha, grad, hz, hrec, objrect, nrec, recs, pix_weight=None, flat=True, k_epsilon=None, tex=None):
    """One env of one launch.  alpha, hz (3, S, S) f32, grad (3, S, S, 2) f32, hrec (3, S, S) i32, objrect (3, 4) i32,
    nrec (3,), recs: three (n_o, 32) f32 record arrays, pix_weight (S, S) f32 or None.  ``tex``: per object None (white
    vertex texture: the texel is q0 + q1 + q2) or the one grey level of an atlas whose texels are all equal (the texel
    is that level whatever the barycentrics: it tells which OBJECT won without modelling the atlas lookup).  Returns the
    expected frames, the per-block and whole-frame sums with their L1 forms, the footprint and the block classes."""
    bpe = n_blocks(S)
    ys, xs = np.mgrid[0:S, 0:S]
    tx, ty = xs // OCC_BLOCK, ys // OCC_BLOCK
    in_rect = np.zeros((3, S, S), bool)
    for o in range(3):
        r = objrect[o]
        in_rect[o] = (int(nrec[o]) > 0) & (tx >= r[0]) & (ty >= r[1]) & (tx <= r[2]) & (ty <= r[3])
    a32 = np.where(in_rect, alpha, np.float32(0)).astype(np.float32)
    a = a32.astype(np.float64)
    d = np.where(in_rect[..., None], grad, np.float32(0)).astype(np.float64)
    I = a[0] * a[1] + a[1] * a[2] + a[0] * a[2]
    w = np.ones((S, S)) if pix_weight is None else pix_weight.astype(np.float64)
    g = np.stack([a[1] + a[2], a[0] + a[2], a[0] + a[1]])
    terms = np.stack([w * I * I, w * 2.0 * I * (g * d[..., 0]).sum(0), w * 2.0 * I * (g * d[..., 1]).sum(0)])
    l1 = np.stack([np.abs(w) * I * I, np.abs(w) * 2.0 * I * np.abs(g * d[..., 0]).sum(0), np.abs(w) * 2.0 * I * np.abs(g * d[..., 1]).sum(0)])

    def per_block(t):
        flat_ = np.zeros((3, bpe * PIX_BLOCK))
        flat_[:, : S * S] = t.reshape(3, -1)
        return flat_.reshape(3, bpe, PIX_BLOCK).sum(-1).T  # (bpe, 3)

    # the winner: objects in order, strictly smaller depth wins
    best = np.full((S, S), HZ_NONE, np.float32)
    wrec = np.full((S, S), -1, np.int64)
    wobj = np.zeros((S, S), np.int64)
    for o in range(3):
        take = in_rect[o] & (hz[o] < best)
        best = np.where(take, hz[o], best)
        wrec = np.where(take, hrec[o], wrec)
        wobj = np.where(take, o, wobj)
    hit = wrec >= 0
    depth = np.where(hit, best, np.float32(-1)).astype(np.float32)
    out = dict(in_rect=in_rect, alphas=a32, I=I, I_tol=4.0 * U * I, depth=depth, hit=hit, win_obj=wobj, win_rec=wrec,
               block_sum=per_block(terms), block_l1=per_block(l1), frame_sum=terms.reshape(3, -1).sum(1),
               frame_l1=l1.reshape(3, -1).sum(1))
    fp = footprint(objrect, nrec, S)
    obj_rects = live_object_rects(objrect, nrec)
    out["footprint"] = fp
    out["obj_rects"] = obj_rects
    out["fp_blocks"] = rows_to_blocks(fp[1], fp[3], S)
    out["bg_block"] = np.array([is_background_block(b, S, obj_rects) for b in range(bpe)])
    c_terms = np.array([C_LOSS, C_GRAD, C_GRAD])
    out["block_tol"] = gamma(c_terms + DEPTH_BLOCK)[None, :] * out["block_l1"]
    nb = max(out["fp_blocks"][1] - out["fp_blocks"][0] + 1, 0)
    out["reduce_chain"] = int(math.ceil(nb / 64.0)) + DPP_LEVELS
    out["frame_tol"] = gamma(c_terms + DEPTH_BLOCK + out["reduce_chain"]) * out["frame_l1"]
    if flat:
        colour = np.ones((3, S, S))
        ctol = np.zeros((S, S))
        den_min = np.inf
        yy, xx = np.nonzero(hit)
        if yy.size:
            r = np.zeros((yy.size, REC_STRIDE))
            for o in range(3):
                m = wobj[yy, xx] == o
                if m.any():
                    r[m] = recs[o][wrec[yy, xx][m]].astype(np.float64)
            xf = -1.0 + (2.0 * (S - 1 - xx) + 1.0) / S
            yf = -1.0 + (2.0 * (S - 1 - yy) + 1.0) / S
            x0, y0, z0, x1, y1, z1, x2, y2, z2 = (r[:, k] for k in range(9))
            ia = r[:, R_INV_AREA]
            b0 = ((xf - x1) * (y2 - y1) - (yf - y1) * (x2 - x1)) * ia
            b1 = ((yf - y2) * (x2 - x0) - (xf - x2) * (y2 - y0)) * ia
            b2 = ((xf - x0) * (y1 - y0) - (yf - y0) * (x1 - x0)) * ia
            w0, w1, w2 = b0 * z1 * z2, z0 * b1 * z2, z0 * z1 * b2
            den = w0 + w1 + w2
            den_min = float(den.min())
            if k_epsilon is not None:  # the kernel clamps den at kEpsilon; the model only covers launches where it cannot
                assert den_min > 100.0 * float(k_epsilon), ("the kEpsilon clamp of the barycentric denominator is in reach", den_min)
            q = np.stack([w0, w1, w2]) / den
            c = r[:, R_AMB] * q.sum(0) + r[:, R_SPEC]
            tol = gamma(C_FLAT) * (np.abs(r[:, R_AMB]) * np.maximum(1.0, np.abs(q).sum(0)) + np.abs(r[:, R_SPEC]))
            for o in range(3):
                if tex is not None and tex[o] is not None:  # a constant texel: one product, one addition
                    m = wobj[yy, xx] == o
                    c[m] = r[m, R_AMB] * float(tex[o]) + r[m, R_SPEC]
                    tol[m] = gamma(2) * (np.abs(r[m, R_AMB] * float(tex[o])) + np.abs(r[m, R_SPEC]))
            colour[:, yy, xx] = c
            ctol[yy, xx] = tol
        out.update(colour=colour, colour_tol=ctol, den_min=den_min)
    return out


def expected_full_state(m):
    S = m["I"].shape[0]
    fs = np.full((S, S, 4), 3.0)
    fs[..., 3] = m["I"]
    return fs


# ---- reward rule and action Jacobian --------------------------------------------------------------------------------------
def finish(loss32, grad_elaz32, full_reward32, object_mass32, J32, consts):
    """finish_one for one env, in f64 on the f32 operands: reward, done, the new full_reward, the action gradient (None
    without grad_elaz) and their rounding bounds."""
    l, fr, om = float(np.float32(loss32)), float(np.float32(full_reward32)), float(np.float32(object_mass32))
    done = bool(np.float32(loss32) < consts["kDoneThreshold"])
    k = float(consts["kDoneBonus"]) if done else -float(consts["kStepPenalty"])
    reward = (fr - l) / om + k
    out = dict(reward=reward, reward_tol=gamma(3) * (abs(fr - l) / om + abs(k)), done=done, full_reward=np.float32(loss32))
    if grad_elaz32 is not None:
        ge, ga = (float(v) for v in np.asarray(grad_elaz32, np.float32))
        J = np.asarray(J32, np.float32).astype(np.float64).reshape(4)
        out["grad_action"] = np.array([-(ge * J[0] + ga * J[2]) / om, -(ge * J[1] + ga * J[3]) / om])
        out["grad_action_tol"] = gamma(4) * np.array([(abs(ge * J[0]) + abs(ga * J[2])) / om, (abs(ge * J[1]) + abs(ga * J[3])) / om])
    return out


# ---- region tracking: the write set ----------------------------------------------------------------------------------------
def simulate_tracked_write(prev_buffer, rect_prev, expected_frame, background, obj_rects, S, other_prev=None, skip=False):
    """What a tracked launch leaves in a persistent buffer.  ``prev_buffer``, ``expected_frame``: (S S, C) arrays, pixel
    major; ``background``: (C,); ``obj_rects``: pixel rects of the objects with nrec > 0; ``rect_prev``: what the buffer
    recorded last; ``other_prev``: the previous rect of the other tracked buffer of the launch (obs / full_state and the
    alphas state are tracked separately, the visited range is shared).  Returns (buffer, rect_next)."""
    buf = np.array(prev_buffer, copy=True)
    if skip:  # a skipped row keeps its content and its rect
        return buf, tuple(int(v) for v in rect_prev)
    fp = list(empty_rect(S))
    for r in obj_rects:
        if not is_empty(r):
            fp = [min(fp[0], r[0]), min(fp[1], r[1]), max(fp[2], r[2]), max(fp[3], r[3])]
    fp = tuple(fp)
    b0, b1 = visited_range(S, fp, [rect_prev, other_prev])
    touched = np.zeros((S, S), bool)
    for r in obj_rects:
        touched |= in_rect_px(S, r)
    write_px = (touched | in_rect_px(S, rect_prev)).reshape(-1)
    for blk in range(b0, b1 + 1):
        b = block_span(blk, S)
        if is_background_block(blk, S, obj_rects):
            if meets(blk, S, rect_prev):
                buf[b["p0"]: b["p1"] + 1] = background
            continue
        hi = min(b["p1"] + 1, S * S)
        sel = np.nonzero(write_px[b["p0"]: hi])[0] + b["p0"]
        buf[sel] = expected_frame[sel]
    return buf, fp
