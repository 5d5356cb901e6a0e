"""Host model of the device auto-reset contract (include/occlusionenv_amd.h: occ_step_flags, occ_reset_commit,
occ_auto_reset, occ_object_mass, occ_reserve_refill), written from the header comments and the reference lines they
cite (SubProcVecEnv.py:209-218, environment.py:288-327, trainRL.py:191-229), not from the kernels.

Pure numpy: every function takes arrays and returns new ones; its inputs are never written.  Rows are addressed with
explicit n_env / n_reserve / img, so a buffer may be longer than the ABI needs: whatever lies past the rows the contract
names is returned unchanged (the GPU tests put canaries there).
"""
from __future__ import annotations

import numpy as np

RS_EMPTY, RS_PENDING, RS_READY = 0, 1, 2
CAM_STRIDE = 48
# reset()'s acceptance test `loss > 0.1` (environment.py:327) on float32 losses: the threshold is float32(0.1)
DONE_THRESHOLD = np.float32(0.1)
MAX_TRIES = 10  # environment.py:288: the 10th try is kept whatever its loss


def _accepted(loss) -> bool:
    # NaN > 0.1 is False: a NaN loss is a rejection, as in the reference
    return bool(np.float32(loss) > DONE_THRESHOLD)


def step_flags(done, loss_all, status, n_env, n_reserve):
    """flags (n_env + n_reserve + 1) int32: done | reserve scene accepted (loss > 0.1) | some status word non-zero."""
    N, R = n_env, n_reserve
    flags = np.zeros(N + R + 1, dtype=np.int32)
    flags[:N] = np.asarray(done).reshape(-1)[:N].astype(np.int32)
    if R:
        la = np.asarray(loss_all).reshape(-1)
        flags[N:N + R] = [1 if _accepted(la[N + r]) else 0 for r in range(R)]
    flags[N + R] = 1 if np.any(np.asarray(status).reshape(-1)[:N + R] != 0) else 0
    return flags


def reset_commit(pairs, n, el, az, radius, campos, cam, alphas, full_reward, object_mass, scene_mesh, scene_offset,
                 obs, obs_all, loss_all, img):
    """occ_reset_commit: env row pairs[2k] takes over row pairs[2k+1] for k < n.  Returns a dict of the written arrays
    (el, az, radius, campos, cam, alphas, full_reward, object_mass, scene_mesh, scene_offset, obs), all flat."""
    o = dict(el=el, az=az, radius=radius, campos=campos, cam=cam, alphas=alphas, full_reward=full_reward,
             object_mass=object_mass, scene_mesh=scene_mesh, scene_offset=scene_offset, obs=obs)
    o = {k: np.array(v).reshape(-1) for k, v in o.items()}
    src_obs, src_loss = np.asarray(obs_all).reshape(-1), np.asarray(loss_all).reshape(-1)
    p = np.asarray(pairs).reshape(-1)
    S2 = img * img

    def rows(name, i, width):
        return o[name][i * width:(i + 1) * width]

    for k in range(n):
        dst, src = int(p[2 * k]), int(p[2 * k + 1])
        for name in ("el", "az", "radius"):
            rows(name, dst, 1)[:] = rows(name, src, 1)  # (slices: copies bit for bit, NaN payloads included)
        l = np.float32(src_loss[src])
        o["full_reward"][dst] = l
        o["object_mass"][dst] = l + np.float32(1.0)  # environment.py:324, in float32
        rows("campos", dst, 3)[:] = 0.0
        rows("scene_mesh", dst, 3)[:] = rows("scene_mesh", src, 3)
        rows("scene_offset", dst, 9)[:] = rows("scene_offset", src, 9)
        rows("cam", dst, CAM_STRIDE)[:] = rows("cam", src, CAM_STRIDE)
        rows("alphas", dst, 3 * S2)[:] = rows("alphas", src, 3 * S2)
        rows("obs", dst, 4 * S2)[:] = src_obs[src * 4 * S2:(src + 1) * 4 * S2]
    return o


def age_slots(rs_state, rs_tries, loss_all, n_env, n_reserve):
    """Step (1) of occ_auto_reset: every PENDING slot was rendered by this step.  Its try count goes up by one; it is
    READY if the render passes reset()'s test or this was its 10th try, else EMPTY (try count kept).  Returns
    (state, tries, was_pending) for the n_reserve slots."""
    R = n_reserve
    state = np.array(np.asarray(rs_state).reshape(-1)[:R], dtype=np.int32)
    tries = np.array(np.asarray(rs_tries).reshape(-1)[:R], dtype=np.int32)
    la = np.asarray(loss_all).reshape(-1)
    was_pending = state == RS_PENDING
    for r in np.nonzero(was_pending)[0]:
        t = int(tries[r]) + 1
        tries[r] = t
        state[r] = RS_READY if (_accepted(la[n_env + r]) or t >= MAX_TRIES) else RS_EMPTY
    return state, tries, was_pending


def finished_envs(done, n_env, age=None, max_ep_len=0):
    """Finished envs of this step: done != 0, or (the time limit, trainRL.py:191-229) age + 1 >= max_ep_len > 0.
    Returns (report words (n_env): 1 = done, else 2 = time limit, else 0; the new ages or None)."""
    N = n_env
    d = np.asarray(done).reshape(-1)[:N] != 0
    rep = np.where(d, 1, 0).astype(np.int32)
    new_age = None
    if age is not None:
        new_age = np.asarray(age).reshape(-1)[:N].astype(np.int32) + 1  # every env ages by one step
        if max_ep_len > 0:
            rep[(new_age >= max_ep_len) & ~d] = 2
    return rep, new_age


def pair(fin_report, slot_state, n_reserve):
    """The k-th finished env (index order) with the k-th READY slot (index order), min(nfin, nready, R) pairs.
    Returns ([(env, slot)], nfin)."""
    fin = np.nonzero(np.asarray(fin_report) != 0)[0]
    ready = np.nonzero(np.asarray(slot_state) == RS_READY)[0]
    npair = min(len(fin), len(ready), n_reserve)
    return [(int(fin[k]), int(ready[k])) for k in range(npair)], len(fin)


AUTO_RESET_BUFFERS = ("done", "loss_all", "status", "rs_state", "rs_tries", "el", "az", "radius", "campos", "cam",
                      "alphas", "full_reward", "object_mass", "scene_mesh", "scene_offset", "obs_all", "full_state_all",
                      "store_obs", "store_fs", "store_loss", "skip", "term_obs", "report")
AUTO_RESET_OPTIONAL = ("age", "rect", "arect", "reset_full_state", "norm_flags", "slot_objsum", "report_host")


def auto_reset(a: dict, n_env: int, n_reserve: int, img: int, max_ep_len: int = 0) -> dict:
    """occ_auto_reset.  ``a`` maps the names of AUTO_RESET_BUFFERS (and of AUTO_RESET_OPTIONAL that are given; None or
    missing = not given) to arrays of any shape; a buffer may be longer than the ABI needs.  Returns a dict with a
    flat copy of every buffer as the call leaves it (inputs included, unchanged)."""
    N, R, S2 = n_env, n_reserve, img * img
    o = {k: np.array(v).reshape(-1) for k, v in a.items() if v is not None}

    def rows(name, i, width):
        return o[name][i * width:(i + 1) * width]

    # (1) age the PENDING slots
    state, tries, was_pending = age_slots(o["rs_state"], o["rs_tries"], o["loss_all"], N, R)
    # (2) finished envs and their report words
    fin, new_age = finished_envs(o["done"], N, o.get("age"), max_ep_len)
    if new_age is not None:
        o["age"][:N] = new_age
    # (3) pairs; a taken slot goes back to EMPTY with a fresh try count; only PENDING slots are rendered next step
    pairs, nfin = pair(fin, state, R)
    slot_env = np.full(R, -1, dtype=np.int32)
    for i, r in pairs:
        slot_env[r] = i
        state[r] = RS_EMPTY
        tries[r] = 0
    o["rs_state"][:R] = state
    o["rs_tries"][:R] = tries
    o["skip"][N:N + R] = (state != RS_PENDING).astype(np.int32)
    any_status = 1 if np.any(o["status"][:N + R] != 0) else 0
    rep = np.concatenate([fin, state, slot_env, [any_status, nfin - len(pairs)]]).astype(np.int32)
    o["report"][:N + 2 * R + 2] = rep
    if "report_host" in o:
        f = np.nonzero(fin)[0]
        o["report_host"][f] = fin[f]  # only the envs that are reset: the rest of the first section stays as it was (zero)
        o["report_host"][N:N + 2 * R + 2] = rep[N:]
    # (4) stash: a slot rendered now (it was PENDING) that nobody takes keeps this step's render in the store
    for r in range(R):
        if was_pending[r] and slot_env[r] < 0:
            src = N + r
            rows("store_obs", r, 4 * S2)[:] = rows("obs_all", src, 4 * S2)
            rows("store_fs", r, 4 * S2)[:] = rows("full_state_all", src, 4 * S2)
            rows("store_loss", r, 1)[:] = rows("loss_all", src, 1)
    # (5) commit: the slot's last render (this step's rows if it was PENDING, else the store) and state become the env's
    norm = "norm_flags" in o
    for i, r in pairs:
        dst, src, pend = i, N + r, bool(was_pending[r])
        l = np.float32(o["loss_all"][src] if pend else o["store_loss"][r])
        for name in ("el", "az", "radius"):
            rows(name, dst, 1)[:] = rows(name, src, 1)  # (slices: copies bit for bit, NaN payloads included)
        rows("cam", dst, CAM_STRIDE)[:] = rows("cam", src, CAM_STRIDE)
        rows("scene_mesh", dst, 3)[:] = rows("scene_mesh", src, 3)
        rows("scene_offset", dst, 9)[:] = rows("scene_offset", src, 9)
        rows("alphas", dst, 3 * S2)[:] = rows("alphas", src, 3 * S2)
        rows("campos", dst, 3)[:] = 0.0
        o["full_reward"][dst] = l
        base = np.float32(o["slot_objsum"][r]) if (norm and o["norm_flags"][dst] != 0) else l
        o["object_mass"][dst] = base + np.float32(1.0)  # environment.py:324, in float32
        rows("term_obs", r, 4 * S2)[:] = rows("obs_all", dst, 4 * S2)  # the final observation, before it is overwritten
        if pend:
            rows("obs_all", dst, 4 * S2)[:] = rows("obs_all", src, 4 * S2)
            fs = rows("full_state_all", src, 4 * S2)
        else:
            rows("obs_all", dst, 4 * S2)[:] = rows("store_obs", r, 4 * S2)
            fs = rows("store_fs", r, 4 * S2)
        if "reset_full_state" in o:
            rows("reset_full_state", r, 4 * S2)[:] = fs
        if new_age is not None:
            o["age"][dst] = 0
        for name in ("rect", "arect"):
            if name in o:
                rows(name, dst, 4)[:] = [0, 0, img - 1, img - 1]  # the row holds a whole frame now
    return o


def object_mass(alphas, n_rows, img):
    """sum over the pixels of (a1 + a2 + a3)^2 per row of alphas (n_rows,3,S,S), in float64."""
    a = np.asarray(alphas).reshape(-1)[:n_rows * 3 * img * img].reshape(n_rows, 3, img * img).astype(np.float64)
    return (a.sum(axis=1) ** 2).sum(axis=1)


def object_mass_bound(ref, img):
    """|got - ref| allowed for the float32 kernel: each thread adds ceil(S^2/256) non-negative terms in order, then come
    the wave and block levels; every level costs at most one rounding of 2^-24 relative."""
    return (-(-img * img // 256) + 12) * 2.0 ** -24 * np.asarray(ref, dtype=np.float64)


def reserve_refill(packed, n, n_env, n_reserve, scene_mesh, scene_offset, rs_state, skip):
    """occ_reserve_refill: n rows of 13 int32 (slot, mesh id x3, offset x9 as float bits); a row whose slot lies outside
    [0, n_reserve) changes nothing.  Returns flat (scene_mesh, scene_offset, rs_state, skip)."""
    p = np.asarray(packed, dtype=np.int32).reshape(-1)[:13 * n].reshape(n, 13)
    mesh, off = np.array(scene_mesh).reshape(-1), np.array(scene_offset).reshape(-1)
    st, sk = np.array(rs_state).reshape(-1), np.array(skip).reshape(-1)
    off_bits = off.view(np.int32)
    for row in p:
        slot = int(row[0])
        if not 0 <= slot < n_reserve:
            continue
        e = n_env + slot
        mesh[e * 3:e * 3 + 3] = row[1:4]
        off_bits[e * 9:e * 9 + 9] = row[4:13]  # bit for bit: the offsets travel as float bits
        st[slot] = RS_PENDING
        sk[e] = 0  # rendered from the next launch on
    return mesh, off, st, sk
