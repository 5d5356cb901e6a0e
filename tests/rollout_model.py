"""The three rules of csrc/occ_rollout.hpp in numpy (include/occlusionenv_amd.h states them): the episode bookkeeping of
``occ_rollout_advance``, the returns of ``occ_ppo_returns`` and the acting formulas of ``occ_ppo_act``.  Every f32
operation is a numpy f32 operation, i.e. rounded once; the statistics are f64."""
import numpy as np

f32 = np.float32
LOG_2PI = np.log(2.0 * np.pi)

#: the fields of OccRolloutState, in the struct's order
STATE_FIELDS = ("ep_return", "ep_len", "ring_env", "ring_return", "ring_length", "ring_code", "ring_timestep", "ring_running",
                "n_episodes", "code_counts", "sums", "running")


def new_state(n, cap, rng=None):
    """A fresh state; with ``rng`` the ring holds seeded junk (what is not written must keep its bits)."""
    st = dict(ep_return=np.zeros(n, f32), ep_len=np.zeros(n, np.int32), ring_env=np.zeros(cap, np.int32),
              ring_return=np.zeros(cap, f32), ring_length=np.zeros(cap, np.int32), ring_code=np.zeros(cap, np.int32),
              ring_timestep=np.zeros(cap, np.int64), ring_running=np.zeros(cap, f32), n_episodes=np.zeros(1, np.int64),
              code_counts=np.zeros(2, np.int64), sums=np.zeros(2, np.float64), running=np.zeros(1, f32))
    if rng is not None:
        for k in ("ring_env", "ring_length", "ring_code"):
            st[k][:] = rng.integers(-9, 9, cap)
        st["ring_timestep"][:] = rng.integers(-9, 9, cap)
        st["ring_return"][:] = rng.normal(size=cap)
        st["ring_running"][:] = rng.normal(size=cap)
    return st


def advance(st, reward, done, code, timestep, rewards=None, dones=None, t=0):
    """One occ_rollout_advance on ``st`` (in place).  -> the entries completed in this step, in order, as tuples
    (episode number from 1, env, return, length, code, timestep, running reward)."""
    n = st["ep_return"].shape[0]
    cap = st["ring_env"].shape[0]
    reward = np.asarray(reward, f32)
    st["ep_return"][:] = st["ep_return"] + reward  # f32 + f32, rounded once
    st["ep_len"] += 1
    if rewards is not None:
        rewards[t] = reward
        dones[t] = np.where(np.asarray(done) != 0, f32(1), f32(0))
    out = []
    for e in range(n):
        if code[e] == 0:
            continue
        k = int(st["n_episodes"][0])
        ret, length = st["ep_return"][e], st["ep_len"][e]
        if k == 0:
            st["running"][0] = ret
        else:
            st["running"][0] = f32(f32(0.95) * st["running"][0]) + f32(f32(0.05) * ret)
        s = k % cap
        st["ring_env"][s], st["ring_return"][s], st["ring_length"][s] = e, ret, length
        st["ring_code"][s], st["ring_timestep"][s], st["ring_running"][s] = code[e], timestep, st["running"][0]
        st["n_episodes"][0] = k + 1
        st["code_counts"][int(code[e]) - 1] += 1
        st["sums"][0] += np.float64(ret)
        st["sums"][1] += np.float64(length)
        out.append((k + 1, e, ret, int(length), int(code[e]), int(timestep), st["running"][0].copy()))
        st["ep_return"][e], st["ep_len"][e] = 0, 0
    return out


def csv_row(entry):
    """trainRL.py:235-239: the row of one completed episode."""
    ep, _env, ret, length, _code, ts, running = entry
    return "{},{},{},{},{}".format(ep, ts, round(float(ret), 4), round(float(running), 4), length)


def replay_log(rewards, codes, timestep_of=None):
    """The CSV rows (without the header) of a (K,n) stream of step rewards and end codes, from a fresh state."""
    K, n = rewards.shape
    st = new_state(n, 1)
    rows = []
    for k in range(K):
        ts = (k + 1) * n if timestep_of is None else timestep_of(k)
        rows += [csv_row(en) for en in advance(st, rewards[k], np.zeros(n, np.uint8), codes[k], ts)]
    return rows, st


def returns(rewards, dones, gamma):
    """PPO.py:178-185 per env as ppo.mc_returns states it: running = r + (gamma * running) * not_done, three rounded f32
    operations.  rewards, dones (T,n) f32 -> (T,n) f32."""
    rewards, dones = np.asarray(rewards, f32), np.asarray(dones, f32)
    out = np.empty_like(rewards)
    running = np.zeros_like(rewards[0])
    g = f32(gamma)
    for t in range(rewards.shape[0] - 1, -1, -1):
        not_done = f32(1) - dones[t]
        running = rewards[t] + (g * running) * not_done
        out[t] = running
    return out


def return_stats(raw):
    """f64 mean and unbiased standard deviation of the f32 returns."""
    x = np.asarray(raw, np.float64).reshape(-1)
    return np.array([x.mean(), x.std(ddof=1)])


def normalise(raw, stats):
    """(ret - (float)mean) / ((float)std + 1e-7f), every operation in f32."""
    return (np.asarray(raw, f32) - f32(stats[0])) / (f32(stats[1]) + f32(1e-7))


def act_mean64(feats, w_a, b_a):
    """The action head in f64, and per component the magnitude sum_i |w_i f_i| + |b| that bounds an f32 dot product's error."""
    f, w, b = (np.asarray(x, np.float64) for x in (feats, w_a, b_a))
    return f @ w.T + b, (np.abs(f)[:, None, :] * np.abs(w)[None]).sum(-1) + np.abs(b)


def act_action(mean, noise, std):
    """action = mean + noise * std in f32: the product is rounded, then the sum."""
    return np.asarray(mean, f32) + np.asarray(noise, f32) * f32(std)


def act_logprob64(action, mean, std):
    """log N(action; mean, var I) with var = the f32 square of the f32 std, in f64.  -> (logprob, quadratic term, constant)."""
    var = np.float64(f32(std) * f32(std))
    e = np.asarray(action, np.float64) - np.asarray(mean, np.float64)
    quad = 0.5 * (e * e).sum(-1) / var
    const = -0.5 * (2.0 * LOG_2PI + 2.0 * np.log(var))
    return -quad + const, quad, const
