"""The rule of occ_episode_advance (include/occlusionenv_amd.h, csrc/occ_episode.hpp) in numpy: what the reference's
evaluation loops do on the host after every env.step (test.py:92-255, iterator.py:104-204), for a batch of envs.

State: a dict of arrays ``action`` (n,2) f32, ``active`` (n) i32, ``skip`` (n) i32, ``iterations`` (n) i32, ``finished`` (n) u8,
``nan_steps`` (n) i32 and optionally ``rewards`` / ``full_rewards`` (max_step, n) f32.  ``advance`` updates it in place and
returns report[0], the number of envs still active."""
import numpy as np

GRADIENT, RANDOM, MODEL, AGENT = 0, 1, 2, 3
FIELDS = ("action", "active", "skip", "iterations", "finished", "nan_steps")
f32 = np.float32


def new_state(n, max_step=None, action=None):
    st = dict(action=np.zeros((n, 2), f32) if action is None else np.array(action, f32).reshape(n, 2),
              active=np.ones(n, np.int32), skip=np.zeros(n, np.int32), iterations=np.zeros(n, np.int32),
              finished=np.zeros(n, np.uint8), nan_steps=np.zeros(n, np.int32))
    if max_step is not None:
        st["rewards"] = np.full((max_step, n), np.nan, f32)
        st["full_rewards"] = np.full((max_step, n), np.nan, f32)
    return st


def advance(st, rule, lr, step, max_step, done, reward=None, full_reward=None, grad=None, pred=None, noise=None):
    n = st["active"].shape[0]
    lr = f32(lr)
    for e in range(n):
        if st["active"][e] == 0:
            continue  # frozen: nothing read, nothing written
        nan_step = False
        if rule == GRADIENT:
            nan_step = bool(np.isnan(grad[e]).any())
            if not nan_step:
                st["action"][e] = st["action"][e] + lr * grad[e].astype(f32)  # f32 product, then f32 sum: two roundings
        elif rule == RANDOM:
            st["action"][e] = st["action"][e] + lr * noise[e].astype(f32)
        elif rule == MODEL:
            st["action"][e] = f32(-lr) * pred[e].astype(f32)
        else:
            st["action"][e] = pred[e]
        freeze = False
        if nan_step:
            st["nan_steps"][e] += 1
        else:
            if "rewards" in st:
                st["rewards"][step, e] = reward[e]
                st["full_rewards"][step, e] = full_reward[e]
            if done[e]:
                st["finished"][e] = 1
                freeze = True
        if step == max_step - 1:
            freeze = True  # the cap, on a NaN step as well
        if freeze:
            st["iterations"][e] = step + 1
            st["active"][e] = 0
            st["skip"][e] = 1
    return int(np.count_nonzero(st["active"]))
