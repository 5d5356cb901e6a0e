"""Host model of one epoch of ``occ_ppo_update`` (csrc/occ_ppo.hpp), restated in float64 numpy from the formulas of that
header's comment (PPO.py:62-104 and :196-217, torch.optim.Adam), not from the kernel: no autograd.

Every input is what the kernel reads, widened: f32 features, actions, old log-probabilities and returns, and the
f32-rounded action variance, clip, learning rates, betas and eps (``f32`` below).  So a comparison with the kernel
measures the kernel, not the rounding of its constants.

The 771 parameters and the Adam moments use the layout of OccPpoState (include/occlusionenv_amd.h): W_a (2,256) row-major
| b_a (2) | W_v (256) | b_v (1).  Besides the update, ``epoch`` returns per component the scale S_k = sum_i |c_ik| of the
per-sample gradient contributions c_ik (the yardstick of an f32 sum of them) and per sample the distance of the ratio
from the clip bounds 1 -/+ eps_clip (where the kernel's branch may legitimately differ from the model's).
"""
from __future__ import annotations

import math

import numpy as np

FEAT = 256
PARAMS = 3 * FEAT + 3
N_ACTOR = 2 * FEAT + 2  # W_a | b_a take lr_actor; W_v | b_v lr_critic
LOG_2PI = math.log(2.0 * math.pi)


def f32(x) -> float:
    """A python float as the kernel sees it."""
    return float(np.float32(x))


def pack(w_a, b_a, w_v, b_v) -> np.ndarray:
    """The four heads -> the flat (771,) float64 parameter vector."""
    return np.concatenate([np.asarray(t, np.float64).reshape(-1) for t in (w_a, b_a, w_v, b_v)])


def unpack(theta):
    """The flat parameter vector -> (w_a (2,256), b_a (2), w_v (1,256), b_v (1))."""
    t = np.asarray(theta)
    return (t[:2 * FEAT].reshape(2, FEAT), t[2 * FEAT:N_ACTOR], t[N_ACTOR:N_ACTOR + FEAT].reshape(1, FEAT), t[-1:])


def forward(theta, feats, actions, old_lp, action_var):
    """The heads on M samples: (mean (M,2), value (M), lp (M), ratio (M))."""
    w_a, b_a, w_v, b_v = unpack(theta)
    F = np.asarray(feats, np.float64)
    mean = F @ w_a.T + b_a
    value = F @ w_v[0] + b_v[0]
    var = float(action_var)
    e = np.asarray(actions, np.float64) - mean
    lp = -0.5 * (e * e).sum(1) / var - 0.5 * (2.0 * LOG_2PI + 2.0 * math.log(var))
    return mean, value, lp, np.exp(lp - np.asarray(old_lp, np.float64))


def epoch(theta, m, v, step, feats, actions, old_lp, returns, *, action_var, eps_clip, lr_actor, lr_critic, beta1, beta2,
          adam_eps) -> dict:
    """One epoch: forward, clipped surrogate, its gradient and the Adam step.  ``theta``, ``m``, ``v``: (771,) arrays,
    ``step``: the float step count before this epoch.  Returns a dict of new arrays (the inputs are not written):
    theta, m, v, step; grad and scale (771,); loss, vloss (as the kernel writes them) and loss_scale; ratio, margin,
    through, adv (M,)."""
    F = np.asarray(feats, np.float64)
    M = F.shape[0]
    ret = np.asarray(returns, np.float64)
    mean, value, lp, ratio = forward(theta, F, actions, old_lp, action_var)
    var = float(action_var)
    e = np.asarray(actions, np.float64) - mean
    adv = ret - value
    lo, hi = 1.0 - eps_clip, 1.0 + eps_clip
    s1, s2 = ratio * adv, np.clip(ratio, lo, hi) * adv
    # d min(s1, s2) / d ratio: 1 inside the clip range (s1 == s2 there, torch.min splits a tie between equal derivatives)
    # or where the unclipped branch is the smaller one, else 0
    through = ((ratio >= lo) & (ratio <= hi)) | (s1 < s2)
    dlp = np.where(through, -adv * ratio / M, 0.0)  # d loss / d lp
    gm = dlp[:, None] * e / var                      # d loss / d mean_j  (d lp / d mean_j = e_j / var)
    gval = (value - ret) / M                         # d loss / d value (0.5 * mean((value - ret)^2))
    absF = np.abs(F)
    grad = np.concatenate([gm[:, 0] @ F, gm[:, 1] @ F, gm.sum(0), gval @ F, [gval.sum()]])
    scale = np.concatenate([np.abs(gm[:, 0]) @ absF, np.abs(gm[:, 1]) @ absF, np.abs(gm).sum(0), np.abs(gval) @ absF,
                            [np.abs(gval).sum()]])
    surr = -np.minimum(s1, s2)
    vloss = float(((value - ret) ** 2).sum() / M)
    ent = 0.5 * (2.0 * (1.0 + LOG_2PI) + 2.0 * math.log(var))  # constant: no gradient
    loss = float(surr.sum() / M + 0.5 * vloss - 0.01 * ent)
    theta2, m2, v2, t = adam(theta, m, v, step, grad, lr_actor=lr_actor, lr_critic=lr_critic, beta1=beta1, beta2=beta2,
                             adam_eps=adam_eps)
    return dict(theta=theta2, m=m2, v=v2, step=t, grad=grad, scale=scale, loss=loss, vloss=vloss,
                loss_scale=float(np.abs(surr).sum() / M + 0.5 * vloss + 0.01 * abs(ent)), ratio=ratio,
                margin=np.minimum(np.abs(ratio - lo), np.abs(ratio - hi)), through=through, adv=adv)


def adam(theta, m, v, step, grad, *, lr_actor, lr_critic, beta1, beta2, adam_eps):
    """torch.optim.Adam (no weight decay, no amsgrad) with bias corrections from the float step count:
    (theta, m, v, step) after the step."""
    t = float(step) + 1.0
    m2 = beta1 * np.asarray(m, np.float64) + (1.0 - beta1) * grad
    v2 = beta2 * np.asarray(v, np.float64) + (1.0 - beta2) * grad * grad
    lr = np.where(np.arange(PARAMS) < N_ACTOR, lr_actor, lr_critic)
    bc1, bc2s = 1.0 - beta1 ** t, math.sqrt(1.0 - beta2 ** t)
    return np.asarray(theta, np.float64) - (lr / bc1) * m2 / (np.sqrt(v2) / bc2s + adam_eps), m2, v2, t


def run(theta, feats, actions, old_lp, returns, n_epochs, m=None, v=None, step=0.0, **hyper) -> list:
    """``n_epochs`` epochs from (theta, m, v, step) (zero moments by default): the list of the per-epoch dicts."""
    m = np.zeros(PARAMS) if m is None else m
    v = np.zeros(PARAMS) if v is None else v
    out = []
    for _ in range(n_epochs):
        out.append(epoch(theta, m, v, step, feats, actions, old_lp, returns, **hyper))
        theta, m, v, step = out[-1]["theta"], out[-1]["m"], out[-1]["v"], out[-1]["step"]
    return out
