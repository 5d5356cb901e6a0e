"""The float64 host model of one ``occ_ppo_update`` epoch (tests/ppo_model.py) on the CPU: against torch autograd and
torch.optim.Adam on float64 heads (``BatchedPPO(fused=False)`` after ``.double()``), and against the reference's own float64
run of PPO.py's update (the ``final64`` fixtures of tests/golden/ppo_golden.npz).  This pins the yardstick of the GPU
tests of the kernel (tests/test_gpu_ppo_kernel.py) to the reference, independently of any GPU."""
import ast
import os

import numpy as np
import pytest
import torch

from occlusionenv_amd import ppo
from tests import ppo_model as PM

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_golden.npz"))
HYPER = ast.literal_eval(str(GOLD["hyper"]))
HEADS = ("w_a", "b_a", "w_v", "b_v")


def _theta(policy):
    return PM.pack(*(p.detach().numpy() for p in (policy.action_head.weight, policy.action_head.bias,
                                                  policy.value_head.weight, policy.value_head.bias)))


def test_model_equals_autograd_and_adam():
    """Six epochs of ``BatchedPPO.update`` (autograd of the loss of PPO.py:199-212, torch.optim.Adam with its two learning
    rates) on float64 heads and a float64 buffer, against the model from the same start.  The old log-probabilities put
    the first epoch's ratios on targets over (0.5, 1.6): every epoch has samples clipped below and above the range with
    either sign of the advantage.  Heads and the four loss values to 1e-12."""
    T, N, K = 16, 40, 6
    g = torch.Generator().manual_seed(23)
    agent = ppo.BatchedPPO(K_epochs=K, graph_epochs=False, fused=False, device="cpu", seed=4)
    agent.policy.double()
    theta0 = _theta(agent.policy)
    var = float(agent.policy.action_var[0])
    feats = torch.rand(T, N, 256, generator=g, dtype=torch.float64)
    with torch.no_grad():
        mean = agent.policy.action_head(feats)
    actions = mean + 0.6 * torch.randn(T, N, 2, generator=g, dtype=torch.float64)
    F, A = feats.reshape(-1, 256).numpy(), actions.reshape(-1, 2).numpy()
    lp0 = PM.forward(theta0, F, A, np.zeros(T * N), var)[2]
    target = torch.empty(T * N, dtype=torch.float64).uniform_(0.5, 1.6, generator=g).numpy()
    old_lp = lp0 - np.log(target)
    rewards = -0.2 + 0.5 * torch.randn(T, N, generator=g, dtype=torch.float64)
    dones = (torch.rand(T, N, generator=g) < 0.1).double()
    rec = torch.cat([feats, actions, torch.from_numpy(old_lp).reshape(T, N, 1), rewards[..., None], dones[..., None]], -1)
    for t in range(T):
        agent.store(rec[t])
    st = agent.update()
    returns = ppo.mc_returns(rewards, dones, agent.gamma)
    returns = ((returns - returns.mean()) / (returns.std() + 1e-7)).reshape(-1).numpy()
    (g_a, g_v) = agent.optimizer.param_groups
    out = PM.run(theta0, F, A, old_lp, returns, K, action_var=var, eps_clip=agent.eps_clip, lr_actor=g_a["lr"],
                 lr_critic=g_v["lr"], beta1=g_a["betas"][0], beta2=g_a["betas"][1], adam_eps=g_a["eps"])
    lo, hi = 1 - agent.eps_clip, 1 + agent.eps_clip
    for o in out:
        r, a = o["ratio"], o["adv"]
        for side in (r < lo, r > hi):
            assert int((side & (a > 0)).sum()) >= 10 and int((side & (a < 0)).sum()) >= 10
    assert float(np.abs(out[-1]["theta"] - theta0).max()) > 1e-3  # the update moved the heads
    assert float(np.abs(_theta(agent.policy) - out[-1]["theta"]).max()) <= 1e-12
    for key, want in (("loss_first", out[0]["loss"]), ("loss_last", out[-1]["loss"]),
                      ("value_loss_first", out[0]["vloss"]), ("value_loss_last", out[-1]["vloss"])):
        assert abs(st[key] - want) <= 1e-12 * max(1.0, abs(want)), (key, st[key], want)


@pytest.mark.parametrize("scen", ["enc", "dir"])
def test_model_reproduces_the_references_float64_update(scen):
    """The reference's update() over 80 epochs on float64 heads (tests/golden/make_ppo_golden.py: the f32 buffer, rewards and
    action variance widened, eps_clip and the Adam constants as python floats) against the model from the same inputs:
    every head parameter to 1e-9 (measured: enc 7.9e-16, dir 4.9e-17).  The returns are that run's own: PPO.py:178-188
    sums the widened rewards in float64, then rounds them to f32 and normalises in f32 - up to 4.8e-7 away from the f32
    run's ``returns_norm_K80``, which would move the heads by 1e-8."""
    def gold(name):
        return np.asarray(GOLD[f"{scen}_{name}"])

    rewards = torch.from_numpy(gold("rewards")).double()[:, None]
    returns = ppo.mc_returns(rewards, torch.from_numpy(gold("terminals"))[:, None], HYPER["gamma"])[:, 0].float()
    returns = (returns - returns.mean()) / (returns.std() + 1e-7)
    assert float((returns - torch.from_numpy(gold("returns_norm_K80"))).abs().max()) <= 1e-6
    theta0 = PM.pack(*(gold(f"init_{k}") for k in HEADS))
    var = float(np.float32(HYPER["action_std"] ** 2))  # the f32 action_var, .double()'d
    out = PM.run(theta0, gold("features"), gold("actions"), gold("logprobs"), returns.numpy(), 80,
                 action_var=var, eps_clip=HYPER["eps_clip"], lr_actor=HYPER["lr_actor"], lr_critic=HYPER["lr_critic"],
                 beta1=0.9, beta2=0.999, adam_eps=1e-8)
    ref = PM.pack(*(gold(f"final64_{k}_K80") for k in HEADS))
    assert float(np.abs(ref - theta0).max()) > 1e-4  # the reference moved the heads
    assert float(np.abs(out[-1]["theta"] - ref).max()) <= 1e-9
