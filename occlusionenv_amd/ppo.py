"""Batched counterpart of the reference's PPO learner for the vectorised env.

The reference (/root/reference/PPO.py) drives ONE env: ``select_action`` stores the frozen encoder's 256-d pooled
feature, the action and its log-probability per step (PPO.py:152-164); ``update`` turns the reward list into
Monte-Carlo returns that restart at terminals (PPO.py:178-188), normalises them, and runs K epochs of the clipped
surrogate over the ACTION and VALUE heads only (optimizer over ``action_head`` / ``value_head``, PPO.py:113-116;
``FullNetwork.act`` detaches the features, model.py:168-171).

Here the buffer is the (T, N, 261) rollout-record tensor of ``rollout.pack_records`` (features | action | logprob |
reward | done), every env is its own trajectory, and the update is one batched pass over T*N samples.  With several
GPUs every rank all-gathers the records (``rollout.all_gather_records``) and runs the SAME update on the same
data with the same seed: the learner is replicated, no gradient collective is needed (the heads are 771 floats).
The features come from ``encoder``: ``BatchedPPO.from_fullnetwork`` runs the reference's frozen FullNetwork encoder
natively (``encoder.FrozenEncoder``) and starts the heads from the checkpoint's; without an encoder
``rollout.pooled_features`` (8x8 average pooling) stands in for it.

On the GPU the K epochs of an update run in the library (``occ_ppo_update``, csrc/occ_ppo.hpp): one launch per epoch
does forward, loss, backward and the Adam step over the 771 parameters (80 epochs over 12 800 samples: 1.3 ms instead
of 35 ms of framework launches).  ``fused=False`` keeps the torch implementation (the reference for the tests, and the
CPU path of the gloo rehearsals).

``train_ppo`` is the reference's whole training loop (trainRL.py:165-250: rollouts, updates, action-std decay,
checkpoints and the episode log) on one rank: acting is one launch that also fills the step's row of a ``RolloutBuffer``
(``act_into``, ``occ_ppo_act``), the episode bookkeeping another (``monitor.EpisodeMonitor``, ``occ_rollout_advance``), and
``update_from`` runs ``occ_ppo_returns`` and ``occ_ppo_update`` on the buffer's own tensors (csrc/occ_rollout.hpp).
``train_rollouts`` stays the loop of the multi-rank rollout and of the torch path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch
import torch.nn as nn

from . import _native as nat
from . import rollout

LOG_2PI = math.log(2.0 * math.pi)


def mc_returns(rewards: torch.Tensor, dones: torch.Tensor, gamma: float) -> torch.Tensor:
    """Monte-Carlo returns per env, restarting at terminals (PPO.py:178-185, one reversed scan per env).
    rewards, dones: (T, N) -> (T, N)."""
    T = rewards.shape[0]
    out = torch.empty_like(rewards)
    running = torch.zeros_like(rewards[0])
    not_done = 1.0 - dones.to(rewards.dtype)
    for t in range(T - 1, -1, -1):
        running = rewards[t] + gamma * running * not_done[t]
        out[t] = running
    return out


class ActorCriticHeads(nn.Module):
    """``FullNetwork.action_head`` / ``value_head`` (model.py:153-154,168-171) on 256-d features, with the fixed
    diagonal Gaussian of ``ActorCritic`` (PPO.py:43-45,62-80,82-104)."""

    def __init__(self, feat_dim: int = 256, action_dim: int = 2, action_std_init: float = 0.6):
        super().__init__()
        self.action_dim = action_dim
        self.action_head = nn.Linear(feat_dim, action_dim)
        self.value_head = nn.Linear(feat_dim, 1)
        self.register_buffer("action_var", torch.full((action_dim,), action_std_init * action_std_init))

    def set_action_std(self, new_action_std: float) -> None:
        self.action_var.fill_(new_action_std * new_action_std)

    def _logprob_entropy(self, mean, action):
        # MultivariateNormal(mean, diag(var)): log N and entropy in closed form
        var = self.action_var
        logdet = torch.log(var).sum()
        lp = -0.5 * (((action - mean) ** 2) / var).sum(-1) - 0.5 * (self.action_dim * LOG_2PI + logdet)
        ent = 0.5 * (self.action_dim * (1.0 + LOG_2PI) + logdet)
        return lp, ent.expand(mean.shape[:-1])

    @torch.no_grad()
    def act(self, features: torch.Tensor, generator: Optional[torch.Generator] = None):
        mean = self.action_head(features)
        eps = torch.randn(mean.shape, device=mean.device, dtype=mean.dtype, generator=generator)
        action = mean + eps * self.action_var.sqrt()
        lp, _ = self._logprob_entropy(mean, action)
        return action, lp

    def evaluate(self, features: torch.Tensor, action: torch.Tensor):
        feats = features.detach()
        mean = self.action_head(feats)
        value = self.value_head(feats).squeeze(-1)
        lp, ent = self._logprob_entropy(mean, action)
        return lp, value, ent


class RolloutBuffer:
    """The rollout of T vector steps of n envs as five contiguous tensors (PPO.py:13-33's lists): ``feats`` (T,n,256),
    ``actions`` (T,n,2), ``logprobs`` (T,n), ``rewards`` (T,n), ``dones`` (T,n) as 0.0 / 1.0.  ``BatchedPPO.act_into``
    writes the first three of a step, ``monitor.EpisodeMonitor.advance`` the other two; ``BatchedPPO.update_from`` hands
    them to the library as they are."""

    def __init__(self, T: int, n: int, device):
        if T <= 0 or n <= 0:
            raise ValueError("RolloutBuffer needs T >= 1 and n >= 1")
        self.T, self.n = int(T), int(n)
        f32 = dict(dtype=torch.float32, device=device)
        self.feats = torch.zeros(self.T, self.n, 256, **f32)
        self.actions = torch.zeros(self.T, self.n, 2, **f32)
        self.logprobs = torch.zeros(self.T, self.n, **f32)
        self.rewards = torch.zeros(self.T, self.n, **f32)
        self.dones = torch.zeros(self.T, self.n, **f32)

    def records(self) -> torch.Tensor:
        """The (T,n,261) record layout of ``rollout.pack_records`` (a copy; for callers of the older interface)."""
        return torch.cat([self.feats, self.actions, self.logprobs.unsqueeze(-1), self.rewards.unsqueeze(-1),
                          self.dones.unsqueeze(-1)], dim=-1)


class BatchedPPO:
    """PPO (PPO.py:107-223) over batched rollouts.  Hyper-parameters default to trainRL.py:42-56.
    ``fused`` (default on the GPU): the epochs of ``update`` run in the library (``occ_ppo_update``); the Adam moments and
    step count then live in ``_fused_state`` (``optimizer`` only supplies the learning rates, betas and eps)."""

    def __init__(self, lr_actor: float = 3e-4, lr_critic: float = 1e-3, gamma: float = 0.99, K_epochs: int = 80,
                 eps_clip: float = 0.2, action_std_init: float = 0.6, device=None, seed: Optional[int] = None,
                 graph_epochs: bool = True, fused: Optional[bool] = None, encoder=None):
        """``encoder``: any callable obs (N,4,S,S) -> features (N,256), run under no_grad - the socket for the frozen
        encoder whose pooled features the reference stores (PPO.py:47,155-157: ``FullNetwork.forward``'s first output,
        model.py:157-166), e.g. ``encoder.FrozenEncoder`` (``from_fullnetwork``).  Default: ``rollout.pooled_features``
        (8x8 average pooling).  An encoder that can leave rows alone itself says so with an attribute ``takes_skip_mask =
        True`` and is then called as ``encoder(obs, skip=, out=)`` (``FrozenEncoder`` does); any other callable is only
        ever called as ``encoder(obs)`` (``features``)."""
        self.encoder = encoder
        self.gamma, self.eps_clip, self.K_epochs = gamma, eps_clip, K_epochs
        self.action_std = action_std_init
        if seed is not None:
            torch.manual_seed(seed)
        self.policy = ActorCriticHeads(action_std_init=action_std_init).to(device)
        self.policy_old = ActorCriticHeads(action_std_init=action_std_init).to(device)
        self.policy_old.load_state_dict(self.policy.state_dict())
        on_gpu = next(self.policy.parameters()).is_cuda
        # capturable: the optimizer keeps its step count on the device, so that an epoch can be captured in a HIP graph
        self.optimizer = torch.optim.Adam([
            {"params": self.policy.action_head.parameters(), "lr": lr_actor},
            {"params": self.policy.value_head.parameters(), "lr": lr_critic},
        ], capturable=on_gpu)
        # The K epochs of an update are one fixed launch sequence (~35 small kernels) over fixed-size tensors: on the GPU
        # epochs 4..K are replays of ONE captured HIP graph (the first three run eagerly, as the capture's warm-up).
        self.graph_epochs = bool(graph_epochs) and on_gpu
        self._graph = None  # (key, graph, static inputs, static loss outputs)
        # On the GPU the epochs run in the HIP library by default (no silent fallback: a missing library raises here).
        self.fused = on_gpu if fused is None else bool(fused)
        self._fused_state = None
        if self.fused:
            if not on_gpu:
                raise nat.NativeError("the fused PPO update needs CUDA/ROCm tensors; there is no CPU fallback (fused=False: torch)")
            nat.load()
            dev = next(self.policy.parameters()).device
            f32 = dict(dtype=torch.float32, device=dev)
            self._fused_state = dict(m=torch.zeros(nat.PPO_PARAMS, **f32), v=torch.zeros(nat.PPO_PARAMS, **f32),
                                     step=torch.zeros(1, **f32), scratch=torch.empty(nat.ppo_scratch_floats(), **f32),
                                     counter=torch.zeros(1, dtype=torch.int32, device=dev))
        self.records = []  # list of (N_total, 261) tensors, one per step

    @classmethod
    def from_fullnetwork(cls, sd_or_module, dilation: Optional[int] = None, residual: Optional[bool] = None,
                         max_chunk: int = 256, precision: str = "f32", **kw) -> "BatchedPPO":
        """The reference's agent (PPO.py:47-48): a FullNetwork checkpoint (state dict, or the module itself) gives the
        frozen encoder (``encoder.FrozenEncoder``, preset "ppo") and the initial action / value heads of ``policy`` and
        ``policy_old`` (model.py:153-154,168-171).  ``precision``: "f32", or "bf16" for the encoder's reduced-precision
        inference mode (``encoder.FrozenEncoder``); the heads stay f32.  ``kw``: the other BatchedPPO arguments (device default "cuda")."""
        from .encoder import FrozenEncoder

        kw.setdefault("device", "cuda")
        if isinstance(sd_or_module, nn.Module):
            enc = FrozenEncoder.from_module(sd_or_module, device=kw["device"], max_chunk=max_chunk, precision=precision)
        else:
            enc = FrozenEncoder.from_state_dict(sd_or_module, "ppo", dilation, residual, device=kw["device"], max_chunk=max_chunk,
                                                precision=precision)
        if set(enc.heads) != {"action_head", "value_head"}:
            raise ValueError("the checkpoint has no action_head / value_head")
        agent = cls(encoder=enc, **kw)
        with torch.no_grad():
            for pol in (agent.policy, agent.policy_old):
                for name, (w, b) in enc.heads.items():
                    head = getattr(pol, name)
                    head.weight.copy_(w.to(torch.float32))
                    head.bias.copy_(b.to(torch.float32))
        return agent

    # ---- acting (PPO.py:152-164) ------------------------------------------------------------
    def features(self, obs: torch.Tensor, skip=None, out=None) -> torch.Tensor:
        """obs (N,4,S,S) -> the (N,256) features the heads act on.  ``skip``: an (N,) int32 or bool mask of rows to leave
        alone, ``out``: the (N,256) f32 contiguous tensor to write into, both as in ``encoder.FrozenEncoder.__call__``: a
        skipped row keeps the bits of ``out`` or, without ``out``, is zero.  An encoder with ``takes_skip_mask`` (a
        ``FrozenEncoder``) gets both and skips the work of such a row; any other encoder, and the pooled path without one, is
        called as before, on every row, and the contract is honoured afterwards."""
        if skip is None and out is None:
            return self._all_rows(obs)
        if self.encoder is not None and getattr(self.encoder, "takes_skip_mask", False):
            with torch.no_grad():
                return self._checked(self.encoder(obs, skip=skip, out=out), obs)
        from .encoder import FrozenEncoder

        if skip is not None:
            skip = FrozenEncoder._check_skip(skip, obs)
        if out is not None:
            FrozenEncoder._check_out("features", out, (int(obs.shape[0]), 256), obs.device)
        feats = self._all_rows(obs)
        if skip is not None:
            keep = (skip != 0).unsqueeze(1)
            feats = torch.where(keep, torch.zeros_like(feats) if out is None else out, feats)
        return feats if out is None else out.copy_(feats)

    def _all_rows(self, obs: torch.Tensor) -> torch.Tensor:
        """The features of every row: the encoder called as ``encoder(obs)``, or the 8x8 pooling."""
        if self.encoder is None:
            return rollout.pooled_features(obs)
        with torch.no_grad():  # PPO.py:154: the encoder is frozen
            return self._checked(self.encoder(obs), obs)

    @staticmethod
    def _checked(feats: torch.Tensor, obs: torch.Tensor) -> torch.Tensor:
        if feats.shape != (obs.shape[0], 256):
            raise ValueError(f"the encoder must map (N,4,S,S) to (N,256) features, got {tuple(feats.shape)}")
        return feats.detach().to(torch.float32).contiguous()

    def select_action(self, obs: torch.Tensor, generator: Optional[torch.Generator] = None, skip=None):
        """obs (N,4,S,S) -> (features, action, logprob) from the OLD policy.  ``skip`` as in ``features``: the features of
        a skipped row are zero; the noise is drawn for all N rows, so what the other rows get does not depend on the mask."""
        feats = self.features(obs, skip=skip)
        action, logprob = self.policy_old.act(feats, generator)
        return feats, action, logprob

    def _need_fused(self, what: str) -> None:
        if not self.fused:
            raise nat.NativeError(f"{what} runs in the HIP library on CUDA/ROCm tensors only (fused=True); the torch path is "
                                  "select_action / update")

    def act_into(self, obs: torch.Tensor, buf: "RolloutBuffer", t: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """``select_action`` with the heads, the sample and the log-probability in ONE launch (``occ_ppo_act``,
        csrc/occ_rollout.hpp), which also writes the acting state's features, the action and the log-probability into row
        ``t`` of ``buf``.  The features are computed as in ``select_action`` and the noise is the same ``torch.randn`` draw
        from ``generator``; the arithmetic of mean and log-probability is the update kernel's, not torch's, so the two
        ways of acting agree to rounding, not in every bit.  Returns the (N,2) action."""
        self._need_fused("act_into")
        return self.act_features_into(self.features(obs), buf, t, generator)

    def act_features_into(self, feats: torch.Tensor, buf: "RolloutBuffer", t: int,
                          generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """``act_into`` for a caller that already holds the (N,256) f32 contiguous features of the acting state."""
        self._need_fused("act_into")
        n = int(feats.shape[0])
        if feats.shape != (n, nat.PPO_FEATURES) or feats.dtype != torch.float32 or not feats.is_contiguous():
            raise ValueError("act_features_into: the features must be a contiguous (N,256) float32 tensor")
        if not 0 <= t < buf.T or buf.n != n or buf.feats.device != feats.device:
            raise ValueError(f"act_into: step {t} of a ({buf.T}, {buf.n}) buffer on {buf.feats.device} for {n} envs on {feats.device}")
        head = self.policy_old.action_head
        if head.weight.shape != (2, nat.PPO_FEATURES):
            raise nat.NativeError("occ_ppo_act is built for 256 features and 2 action components (PPO.py / model.py)")
        noise = torch.randn((n, 2), device=feats.device, dtype=torch.float32, generator=generator)
        action = torch.empty(n, 2, dtype=torch.float32, device=feats.device)
        logprob = torch.empty(n, dtype=torch.float32, device=feats.device)
        with torch.no_grad():
            nat.check(nat.load().occ_ppo_act(nat.ptr(feats), nat.ptr(head.weight), nat.ptr(head.bias), nat.ptr(noise),
                                             float(self.action_std), n, nat.ptr(action), nat.ptr(logprob), None,
                                             nat.ptr(buf.feats), nat.ptr(buf.actions), nat.ptr(buf.logprobs), int(t), buf.T,
                                             nat.stream_ptr(feats.device)), "occ_ppo_act")
        return action

    def update_from(self, buf: "RolloutBuffer") -> dict:
        """``update`` on a full ``RolloutBuffer``: ``occ_ppo_returns`` (one launch: the Monte-Carlo returns of
        PPO.py:178-185 and their normalisation, statistics in f64) and then ``occ_ppo_update`` on the buffer's own
        tensors - no stack, no slice, no copy.  Ends as ``update`` ends: ``policy_old`` synchronised, the same stats dict."""
        self._need_fused("update_from")
        import numpy as np

        M = buf.T * buf.n
        dev = buf.feats.device
        returns = torch.empty(M, dtype=torch.float32, device=dev)
        self._return_stats = torch.empty(2, dtype=torch.float64, device=dev)  # (mean, std) of the raw returns, on the device
        nat.check(nat.load().occ_ppo_returns(nat.ptr(buf.rewards), nat.ptr(buf.dones), buf.T, buf.n, float(self.gamma),
                                             nat.ptr(returns), None, nat.ptr(self._return_stats), nat.stream_ptr(dev)),
                  "occ_ppo_returns")
        std32 = np.float32(self.action_std)
        losses, vlosses = self._fused_epochs(buf.feats.view(M, 256), buf.actions.view(M, 2), buf.logprobs.view(M), returns,
                                             action_var=float(std32 * std32))
        return self._finish_update(losses, vlosses, M)

    def store(self, record: torch.Tensor) -> None:
        self.records.append(record)

    def set_action_std(self, new_action_std: float) -> None:
        self.action_std = new_action_std
        self.policy.set_action_std(new_action_std)
        self.policy_old.set_action_std(new_action_std)

    def decay_action_std(self, rate: float, min_std: float) -> None:
        self.set_action_std(max(round(self.action_std - rate, 4), min_std))  # PPO.py:136-149

    # ---- learning (PPO.py:176-217) ----------------------------------------------------------
    def _epoch_graph(self, epoch, feats, actions, old_lp, returns):
        """The captured epoch for inputs of this shape: static copies of the four inputs, the graph, its two loss outputs.
        Built after three eager epochs of the first update (optimizer state and library workspaces exist by then);
        later updates of the same size copy their data into the static inputs and replay."""
        key = (tuple(feats.shape), feats.device)
        if self._graph is None or self._graph[0] != key:
            static = [t.clone() for t in (feats, actions, old_lp, returns)]
            side = torch.cuda.Stream(device=feats.device)
            side.wait_stream(torch.cuda.current_stream(feats.device))
            g = torch.cuda.CUDAGraph()
            self.optimizer.zero_grad(set_to_none=True)
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):
                    out = epoch(*static)
            torch.cuda.current_stream(feats.device).wait_stream(side)
            self._graph = (key, g, static, out)
        else:
            for dst, src in zip(self._graph[2], (feats, actions, old_lp, returns)):
                dst.copy_(src)
        return self._graph

    def update(self) -> dict:
        rec = torch.stack(self.records)  # (T, N, 261)
        feats, actions = rec[..., :256], rec[..., 256:258]
        old_lp, rewards, dones = rec[..., 258], rec[..., 259], rec[..., 260]
        returns = mc_returns(rewards, dones, self.gamma)
        returns = (returns - returns.mean()) / (returns.std() + 1e-7)
        feats, actions = feats.reshape(-1, 256), actions.reshape(-1, 2)
        old_lp, returns = old_lp.reshape(-1), returns.reshape(-1)
        if self.fused:
            return self._finish_update(*self._fused_epochs(feats, actions, old_lp, returns), int(feats.shape[0]))
        losses, vlosses = [], []

        def epoch(feats, actions, old_lp, returns):
            lp, value, ent = self.policy.evaluate(feats, actions)
            ratios = torch.exp(lp - old_lp)
            adv = returns - value.detach()
            surr1 = ratios * adv
            surr2 = torch.clamp(ratios, 1 - self.eps_clip, 1 + self.eps_clip) * adv
            vloss = torch.mean((value - returns) ** 2)
            loss = (-torch.min(surr1, surr2) + 0.5 * vloss - 0.01 * ent).mean()
            self.optimizer.zero_grad(set_to_none=True)
            loss.backward()
            self.optimizer.step()
            return loss.detach(), vloss.detach()

        n_eager = self.K_epochs
        if self.graph_epochs and self.K_epochs > 4:
            n_eager = 3
        for _ in range(n_eager):
            l, v = epoch(feats, actions, old_lp, returns)
            losses.append(l)
            vlosses.append(v)
        if n_eager < self.K_epochs:
            try:
                g = self._epoch_graph(epoch, feats, actions, old_lp, returns)
                for _ in range(self.K_epochs - n_eager):
                    g[1].replay()
                    losses.append(g[3][0].clone())
                    vlosses.append(g[3][1].clone())
            except Exception as e:  # noqa: BLE001 - capture unsupported here: the same epochs, launched one by one
                import warnings

                warnings.warn(f"HIP-graph capture of the PPO epoch failed ({e!r}); running the epochs eagerly")
                self.graph_epochs, self._graph = False, None
                for _ in range(self.K_epochs - len(losses)):
                    l, v = epoch(feats, actions, old_lp, returns)
                    losses.append(l)
                    vlosses.append(v)
        return self._finish_update(torch.stack(losses), torch.stack(vlosses), int(feats.shape[0]))

    def _fused_epochs(self, feats, actions, old_lp, returns, action_var: Optional[float] = None):
        """The K epochs in the library (csrc/occ_ppo.hpp): parameters and Adam state are updated in place.
        ``action_var``: the variance to pass instead of ``action_std ** 2`` (``update_from``: the f32 square that
        ``occ_ppo_act`` used)."""
        pol, st = self.policy, self._fused_state
        if feats.shape[1] != nat.PPO_FEATURES or pol.action_dim != 2:
            raise nat.NativeError("occ_ppo_update is built for 256 features and 2 action components (PPO.py / model.py)")
        feats, actions = feats.contiguous().float(), actions.contiguous().float()
        old_lp, returns = old_lp.contiguous().float(), returns.contiguous().float()
        ps = nat.OccPpoState()
        for name, t in (("w_a", pol.action_head.weight), ("b_a", pol.action_head.bias), ("w_v", pol.value_head.weight),
                        ("b_v", pol.value_head.bias), ("adam_m", st["m"]), ("adam_v", st["v"]), ("adam_step", st["step"])):
            assert t.is_contiguous() and t.dtype == torch.float32
            setattr(ps, name, t.data_ptr())
        losses = torch.empty(self.K_epochs, 2, dtype=torch.float32, device=feats.device)
        g_a, g_v = self.optimizer.param_groups
        b1, b2 = g_a["betas"]
        stream = nat.stream_ptr(feats.device)
        with torch.no_grad():
            nat.check(nat.load().occ_ppo_update(
                nat.ptr(feats), nat.ptr(actions), nat.ptr(old_lp), nat.ptr(returns), int(feats.shape[0]),
                float(self.action_std) ** 2 if action_var is None else float(action_var), float(self.eps_clip), float(g_a["lr"]), float(g_v["lr"]), float(b1), float(b2),
                float(g_a["eps"]), C.byref(ps), int(self.K_epochs), nat.ptr(losses), nat.ptr(st["scratch"]),
                nat.ptr(st["counter"]), stream), "occ_ppo_update")
        self._keep = (feats, actions, old_lp, returns)  # alive until the stream has run the launches
        return losses[:, 0], losses[:, 1]

    def _finish_update(self, losses, vlosses, samples: int) -> dict:
        # one host sync for the whole update (the reference syncs nowhere inside its epoch loop either, PPO.py:196-217)
        losses, vlosses = losses.cpu(), vlosses.cpu()
        self.policy_old.load_state_dict(self.policy.state_dict())
        self.records = []
        # NB the total is not monotone: the advantages (returns - value) are re-evaluated with the improving critic
        return dict(loss_first=float(losses[0]), loss_last=float(losses[-1]), value_loss_first=float(vlosses[0]),
                    value_loss_last=float(vlosses[-1]), samples=samples)


    # ---- checkpoints (PPO.py:225-230: the old policy's weights, loaded into both) -------------
    def save(self, checkpoint_path) -> None:
        torch.save(self.policy_old.state_dict(), checkpoint_path)

    def load(self, checkpoint_path) -> None:
        dev = next(self.policy.parameters()).device
        sd = torch.load(checkpoint_path, map_location=dev)
        self.policy_old.load_state_dict(sd)
        self.policy.load_state_dict(sd)
        self.action_std = float(self.policy.action_var[0].sqrt())


def train_rollouts(venv, agent: BatchedPPO, n_updates: int = 1, T: int = 50, with_action_grad: bool = False,
                   generator: Optional[torch.Generator] = None, on_step=None, max_ep_len: Optional[int] = None,
                   stagger: bool = True) -> list:
    """trainRL.py:189-229, batched: T vectorised steps (auto-reset inside the env) -> one PPO update; repeated.
    Returns the per-update stats (mean reward, loss before/after).  ``on_step(action, rewards)`` is called after every
    step (and its backward): the hook of callers that consume ``action.grad`` (train_predict.py:52-58).

    ``max_ep_len`` (trainRL.py:22: 50): the reference ends every episode in ``env.reset()`` after max_ep_len steps,
    done or not, and records ``is_terminal = done`` - False for such a reset, so the Monte-Carlo return of PPO.py:178-185
    runs on across it.  Here the env counts every env's steps since its reset on the device and resets the expired ones
    from its reserve (``SimpleVecEnv.max_ep_len``); ``stagger`` spreads the initial ages so that the envs, which all
    start together, do not all expire in the same step (``SimpleVecEnv.stagger_ages``).

    The per-step record exchange runs on a side stream (``rollout.RecordExchange``): the record of step t is stored
    while step t + 1 renders."""
    obs = venv.reset()[:, 0]
    if max_ep_len is not None:
        venv.max_ep_len = int(max_ep_len)
        if stagger:
            venv.stagger_ages()
    import torch.distributed as dist

    world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
    xch = rollout.RecordExchange(obs.shape[0], obs.device, world, keep=True)
    stats = []
    for _ in range(n_updates):
        rew_sum = torch.zeros((), device=obs.device)
        pending = False
        for _t in range(T):
            feats, action, logprob = agent.select_action(obs, generator)
            action = action.detach().requires_grad_(with_action_grad)
            obs, rewards, dones, _infos = venv.step(action)
            if with_action_grad:
                rewards.sum().backward()
            if on_step is not None:
                on_step(action, rewards)
            if pending:
                agent.store(xch.wait())  # the previous step's gathered records
            xch.submit(obs, action, logprob, rewards, dones, features=feats)  # PPO.py:158: the acting state's features
            venv.obs_consumer_event = xch.ready
            pending = True
            rew_sum = rew_sum + rewards.detach().mean()
        agent.store(xch.wait())
        st = agent.update()
        st["mean_reward"] = float(rew_sum) / T
        stats.append(st)
    return stats


def train_ppo(venv, agent: BatchedPPO, max_training_timesteps: int = int(2e4), T: int = 50, max_ep_len: Optional[int] = 50,
              action_std_decay_rate: float = 0.05, min_action_std: float = 0.1, action_std_decay_freq: int = int(1.5e4),
              save_model_freq: int = int(5e3), checkpoint_path=None, log_path=None,
              generator: Optional[torch.Generator] = None, on_step=None, with_action_grad: bool = False,
              stagger: bool = True, monitor=None) -> list:
    """``trainRL.train()`` (trainRL.py:165-250) on the batched env, with its training log: roll out, update every T
    vector steps, decay the action std, save checkpoints, and append ``episode,timestep,reward,running_reward,length``
    to ``log_path``.  The defaults are the script's, scaled to a short run (trainRL.py:22-56).

    ``venv.reset()``; then per vector step ``agent.act_into`` (features, then one launch), ``venv.step``,
    ``monitor.advance`` (one launch: returns, lengths, the episode ring, the buffer's rewards and dones) and the hook;
    after every T steps ``agent.update_from`` and one ``monitor.drain()``, whose rows go to the CSV.  The loop itself
    waits for the device once per update, in the drain (``update_from`` reads its losses back as ``update`` does, and
    ``venv.step`` keeps its own one sync per step).

    A timestep is one env step, so a vector step advances the counter by N.  ``decay_action_std``
    and ``agent.save(checkpoint_path)`` (skipped without a path) run once for each multiple of their frequency that the
    counter crosses in a vector step - the reference tests ``time_step % freq == 0``, which a counter moving N at a time
    may step over.  The loop stops after the update during which the counter passes ``max_training_timesteps``
    (``while time_step <= max_training_timesteps``, trainRL.py:189).

    ``on_step(action, rewards, step)`` is called after every step and its ``monitor.advance``; ``step`` is a dict with
    ``t``, ``timestep``, ``feats`` and ``logprob`` (row t of the buffer), ``dones``, ``codes``, ``infos``, ``obs`` (the next
    observation) and ``buffer`` (the ``RolloutBuffer``, rows 0..t of this update filled).  ``with_action_grad``: as in ``train_rollouts``.  ``monitor``: an ``EpisodeMonitor`` to continue; by
    default a new one whose ring holds N T entries, so that no episode of an update is lost.

    Returns the per-update stats of ``update_from`` plus ``mean_reward`` (mean step reward), ``episodes`` (completed in
    the update's T steps), ``mean_return`` and ``mean_length`` over them (NaN without one), ``lost`` and
    ``running_reward``, ``timestep`` and ``action_std``.

    One rank only: with an initialised process group of more than one rank this raises.  The multi-rank rollout stays
    with ``train_rollouts`` and ``rollout.RecordExchange``.  From the same seed the two loops do not give the same bits:
    the acting arithmetic differs in rounding (``act_into``)."""
    import torch.distributed as dist

    from .monitor import EpisodeMonitor

    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise RuntimeError("train_ppo runs on one rank; the multi-rank rollout is train_rollouts with rollout.RecordExchange")
    obs = venv.reset()[:, 0]
    if max_ep_len is not None:
        venv.max_ep_len = int(max_ep_len)
        if stagger:
            venv.stagger_ages()
    n, dev = int(obs.shape[0]), obs.device
    if monitor is None:
        monitor = EpisodeMonitor(n, dev, capacity=n * T)  # an env ends at most T episodes between two drains: none is lost
    monitor.reset()
    buf = RolloutBuffer(T, n, dev)
    mean_host = torch.empty((), dtype=torch.float32).pin_memory()
    time_step, stats = 0, []
    while time_step <= max_training_timesteps:
        for t in range(T):
            action = agent.act_into(obs, buf, t, generator).requires_grad_(with_action_grad)
            obs, rewards, dones, infos = venv.step(action)
            if with_action_grad:
                rewards.sum().backward()
            codes = venv.episode_end_codes
            before, time_step = time_step, time_step + n
            monitor.advance(rewards, codes, dones, buffer=buf, t=t, timestep=time_step)
            if on_step is not None:
                on_step(action, rewards, dict(t=t, timestep=time_step, feats=buf.feats[t], logprob=buf.logprobs[t], dones=dones,
                                              codes=codes, infos=infos, obs=obs, buffer=buf))
            for _ in range(time_step // action_std_decay_freq - before // action_std_decay_freq):
                agent.decay_action_std(action_std_decay_rate, min_action_std)  # trainRL.py:214-215
            for _ in range(time_step // save_model_freq - before // save_model_freq):
                if checkpoint_path is not None:
                    agent.save(checkpoint_path)  # trainRL.py:218-225
        # the mean step reward travels to pinned memory behind the rollout; the update's read-back of its losses is later
        # on the same stream, so the value has arrived by then without a wait of its own
        mean_host.copy_(buf.rewards.mean(), non_blocking=True)
        st = agent.update_from(buf)
        eps = monitor.drain()
        if log_path is not None:
            monitor.write_csv(log_path, eps)
        k = len(eps["ret"])
        st.update(mean_reward=float(mean_host), episodes=k + eps["lost"], lost=eps["lost"],
                  mean_return=float(eps["ret"].astype("float64").mean()) if k else float("nan"),
                  mean_length=float(eps["length"].mean()) if k else float("nan"),
                  running_reward=float(eps["running"][-1]) if k else eps["totals"]["running_reward"],
                  timestep=time_step, action_std=agent.action_std)
        stats.append(st)
    return stats
