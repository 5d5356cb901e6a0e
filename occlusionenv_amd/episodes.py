"""The experiment the reference exists to report, batched: how many steps a controller needs until ``step()`` says
``finished``, for several controllers on the same scenes (test.py:92-255, iterator.py:104-204).

  * ``GradientAscent``     ascent on the action with the environment's own gradient (iterator.py:104-138, test.py:92-124)
  * ``RandomWalk``         a random walk of the action (test.py:130-151)
  * ``PredictedGradient``  ``action = -step_lr * grad_pred`` from the pretrained network (iterator.py:169-204, test.py:182-217)
  * ``Agent``              the PPO agent's sampled action (test.py:222-255)

``evaluate_controllers`` runs every controller over all envs of a ``SimpleVecEnv`` at once.  An env that is through must
stop (``SimpleVecEnv.step`` would reset it), so the loop drives the engine itself: per step one ``engine.step(action,
skip=skip)``, the controller's network if it has one, and one ``occ_episode_advance`` launch (csrc/occ_episode.hpp) that does
on the device what the reference's loops do on the host - the update of the action, the NaN test of the raw gradient, the
traces, the ``finished`` / step-cap test - and freezes the envs that are through: their row of ``skip`` is set, and the next
step's launch leaves them alone.  The network takes the same mask (``enc(obs, skip=, out=)``): a frozen env's blocks return at
once and its features keep their bits.  Nothing on the host reads a device value inside a step.

``write_iterations`` writes the counts as the reference's ``iterations_{raw,random,model,rl}_3.txt``, which its
``BayesianTTest.py``, ``plotter.py`` and ``iterator_diagram.py`` read; ``summarise_iterations`` gives the plain statistics.
"""
from __future__ import annotations

import itertools
import time
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np
import torch

from . import _native as nat
from ._native import ptr as _p


@dataclass(frozen=True)
class GradientAscent:
    """``action += lr * action.grad`` from zeros; a step whose gradient has a NaN is left out (iterator.py:118-120)."""
    lr: float = 1.0
    name = "raw"
    rule = nat.EPISODE_GRADIENT


@dataclass(frozen=True)
class RandomWalk:
    """``action += lr * randn(2)`` from ``randn(2)`` (test.py:130,140)."""
    lr: float = 1.0
    name = "random"
    rule = nat.EPISODE_RANDOM


@dataclass(frozen=True)
class PredictedGradient:
    """``action = -step_lr * enc.predict_grad(obs)`` from zeros; ``enc``: a ``FrozenEncoder`` with a grad head."""
    enc: Any
    step_lr: float = 0.01
    name = "model"
    rule = nat.EPISODE_MODEL

    @property
    def lr(self) -> float:
        return self.step_lr


@dataclass(frozen=True)
class Agent:
    """The action a ``ppo.BatchedPPO`` samples from its old policy (``select_action``), from zeros."""
    agent: Any
    name = "rl"
    rule = nat.EPISODE_AGENT
    lr = 0.0


def controller_generators(generator: Optional[torch.Generator], k: int) -> list:
    """One generator per controller, seeded by ``k`` draws from ``generator`` (None: torch's global one), on its device.
    A controller that ends early draws less noise; with its own generator that changes nothing for the next one."""
    dev = generator.device if generator is not None else torch.device("cpu")
    seeds = torch.randint(0, 2 ** 62, (k,), generator=generator, device=dev).tolist()
    return [torch.Generator(device=dev).manual_seed(int(s)) for s in seeds]


def _randn(n: int, gen: torch.Generator, device) -> torch.Tensor:
    """One (n,2) standard normal draw for the whole batch, whoever is still active."""
    return torch.randn(n, 2, generator=gen, device=gen.device).to(device)


class _Episodes:
    """Device state of one controller's episodes over a working set of rows (all envs, or a compact subset of them)."""

    FIELDS = ("action", "active", "skip", "iterations", "finished", "nan_steps")

    def __init__(self, n: int, max_step: int, device, action: torch.Tensor, trace: bool):
        i32 = dict(dtype=torch.int32, device=device)
        self.n, self.max_step, self.device = n, max_step, device
        self.rows = None  # the working set: None = all n envs, or their indices (device, int64)
        self.rows_host = None  # ... and the same indices on the host: the engine sizes its record arrays from them
        self.action = action.to(device, torch.float32).contiguous()
        self.active, self.skip = torch.ones(n, **i32), torch.zeros(n, **i32)
        self.iterations, self.nan_steps = torch.zeros(n, **i32), torch.zeros(n, **i32)
        self.finished = torch.zeros(n, dtype=torch.uint8, device=device)
        self.report = torch.zeros(1, **i32)
        self.traces = [torch.full((max_step, n), float("nan"), device=device) for _ in range(2)] if trace else [None, None]
        # what the envs that left the working set ended with (whole-batch arrays; written at compactions and at the end)
        self.result = None

    def advance(self, lib, rule, lr, step, done, reward, loss, grad, pred, noise) -> None:
        w = int(self.action.shape[0])
        nat.check(lib.occ_episode_advance(_p(done), _p(reward), _p(loss), _p(grad), _p(pred), _p(noise), int(rule), float(lr),
                                          int(step), self.max_step, w, _p(self.action), _p(self.active), _p(self.skip),
                                          _p(self.iterations), _p(self.finished), _p(self.nan_steps), _p(self.traces[0]),
                                          _p(self.traces[1]), _p(self.report), nat.stream_ptr(self.device)), "occ_episode_advance")

    def write_back(self) -> dict:
        """The working set's state into the whole-batch result."""
        if self.rows is None:
            self.result = {k: getattr(self, k) for k in self.FIELDS}
            self.result["traces"] = self.traces
            return self.result
        for k in self.FIELDS:
            self.result[k][self.rows] = getattr(self, k)
        for full, part in zip(self.result["traces"], self.traces):
            if full is not None:
                full[:, self.rows] = part
        return self.result

    def compact(self, keep: torch.Tensor) -> None:
        """Continue on rows ``keep`` (indices into the working set) alone."""
        self.write_back()  # (the first time the whole-batch arrays become the result; the working set gets copies)
        keep_host = keep.cpu().numpy()  # the caller has just synchronised for ``keep``: this read costs nothing more
        self.rows = keep if self.rows is None else self.rows[keep]
        self.rows_host = keep_host if self.rows_host is None else self.rows_host[keep_host]
        for k in self.FIELDS:
            setattr(self, k, getattr(self, k)[keep].contiguous())
        self.traces = [None if t is None else t[:, keep].contiguous() for t in self.traces]


def _run(eng, ctrl, max_step: int, az, gen, poll_every: int, trace: bool) -> dict:
    lib, N, dev = eng.lib, eng.N, eng.device
    t0 = time.perf_counter()
    # every controller starts from the same scenes and cameras: reset(new_scene=False, azimuth=...) (test.py:127,154)
    _obs, loss0, _fs = eng.reset_render(azimuth=az, elevation=0.0, radius=4.0)
    first = _randn(N, gen, dev) if ctrl.rule == nat.EPISODE_RANDOM else torch.zeros(N, 2, device=dev)
    ep = _Episodes(N, max_step, dev, first, trace)
    want_grad = ctrl.rule == nat.EPISODE_GRADIENT
    ones = {}
    feats_all = feats_work = None
    steps = polls = compactions = row_steps = 0
    for i in range(max_step):
        rows, w = ep.rows, int(ep.action.shape[0])
        a = ep.action.detach().requires_grad_(want_grad)
        with torch.set_grad_enabled(want_grad):
            obs, reward, done, _full_state, loss = eng.step(a, env_ids=rows, skip=ep.skip, env_ids_host=ep.rows_host)
        grad = pred = noise = None
        if want_grad:  # the launch has computed d reward / d action; this only hands it over (times one)
            if w not in ones:
                ones[w] = torch.ones(w, device=dev)
            (grad,) = torch.autograd.grad(reward, a, ones[w])
            reward = reward.detach()
        elif ctrl.rule == nat.EPISODE_RANDOM:
            noise = _randn(N, gen, dev)
            noise = noise if rows is None else noise[rows]
        else:
            # The network runs on the working set under the mask the engine step of this iteration took (ep.skip before
            # advance changes it): the blocks of a frozen env return at once, and its row of features keeps the bits it
            # held, in a buffer of the working set's rows (gathered from feats_all after every compaction).
            # The heads always run on all N rows of features, frozen ones kept from before, and the agent's noise is drawn
            # for all N: what a row gets then does not depend on who else is still in the working set.
            with torch.no_grad():
                net = ctrl.enc if ctrl.rule == nat.EPISODE_MODEL else ctrl.agent.features
                if feats_all is None:
                    feats_all = net(obs, skip=ep.skip)  # (the first step: nobody is frozen yet)
                elif rows is None:
                    net(obs, skip=ep.skip, out=feats_all)
                else:
                    if feats_work is None:
                        feats_work = feats_all[rows]
                    net(obs, skip=ep.skip, out=feats_work)
                    feats_all.index_copy_(0, rows, feats_work)
                if ctrl.rule == nat.EPISODE_MODEL:
                    pred = ctrl.enc.grad_head(feats_all)
                else:
                    pred = ctrl.agent.policy_old.act(feats_all, gen)[0]
                pred = (pred if rows is None else pred[rows]).contiguous()
        ep.advance(lib, ctrl.rule, ctrl.lr, i, done, reward, loss, grad, pred, noise)
        steps, row_steps = steps + 1, row_steps + w
        if (i + 1) % poll_every == 0 and i + 1 < max_step:
            polls += 1
            left = int(ep.report.item())  # the one value the host reads, every poll_every steps
            if left == 0:
                break
            if 2 * left < w:  # a long tail of unfinished envs does not pay for the whole batch
                ep.compact(torch.nonzero(ep.active).reshape(-1))
                compactions += 1
                feats_work = None  # (the working set has changed: its feature rows are gathered anew)
    res = ep.write_back()
    eng.check_status()  # (a host sync: the clock below has seen the last launch finish)
    seconds = time.perf_counter() - t0
    it = res["iterations"].to(torch.int64)
    out = dict(iterations=it, finished=res["finished"].to(torch.bool), final_action=res["action"], nan_steps=res["nan_steps"],
               initial_loss=loss0, seconds=seconds, steps=steps, polls=polls, compactions=compactions, row_steps=row_steps,
               frozen_row_steps=row_steps - int(it.sum()))
    if trace:
        out["rewards"], out["full_rewards"] = res["traces"]
    return out


def evaluate_controllers(venv, controllers, max_step: int = 50, azimuth=None, scene_of=None,
                         generator: Optional[torch.Generator] = None, poll_every: int = 16, trace: bool = False) -> dict:
    """Iterations to clear the occlusion, per controller and env, on the same scenes.

    ``controllers``: a dict name -> controller, or a sequence of controllers (named ``raw``, ``random``, ``model``, ``rl``
    after the reference's files).  Scenes are drawn once through ``venv.reset()``, with its acceptance rule; every
    controller then starts from the same scenes through ``engine.reset_render(azimuth=..., elevation=0, radius=4)``.
    ``azimuth``: a scalar or an (N,) array, default what ``venv.reset()`` drew for the scene an env runs.  ``scene_of``: an (N,) index, env ``i`` runs
    the scene drawn for env ``scene_of[i]`` - with ``azimuth`` this is iterator.py's sweep of one scene over
    ``range(-310, 311, 100) / 3200``.  Initial actions are the reference's: zeros, and ``randn`` for the random walk.

    Noise comes from one generator per controller (``controller_generators(generator, len(controllers))``), as one
    ``randn(N, 2)`` per step for the whole batch whoever is still active; the agent's sampling draws for all N envs as well
    (for an ``Agent``, ``generator`` must live on the agent's device, as for ``select_action``).  Every ``poll_every`` steps the
    host reads one int, the number of envs still active: at zero the loop ends, and when fewer than half of the rows it
    works on are active it goes on with those alone (``engine.step(env_ids=...)``, the network on that subset; between polls
    the network skips the frozen rows of the working set through its ``skip`` mask).  The results
    are the same, bit for bit, for every ``poll_every``.

    Per controller a dict: ``iterations`` (N,) int64, the reference's ``i + 1`` at ``finished`` or at the cap ``max_step``;
    ``finished`` (N,) bool; ``final_action`` (N,2); ``nan_steps`` (N,) int32; ``initial_loss`` (N,), the loss of the reset
    render; with ``trace`` ``rewards`` and ``full_rewards`` (max_step, N), NaN where an env logged nothing; and the loop's
    counters ``steps``, ``polls``, ``compactions``, ``row_steps`` (rows stepped, summed over the steps),
    ``frozen_row_steps`` (those spent on rows that were through already) and ``seconds`` (host clock from the reset render
    to a synchronise after the last step).
    Deviation from the reference: an env whose LAST allowed step has a NaN gradient still gets its ``iterations = max_step``
    (the reference's ``continue`` would leave no entry for it).

    The loop drives ``venv.engine`` directly and leaves the envs wherever their episodes ended, with the scenes of
    ``scene_of``: the caller must ``venv.reset()`` before stepping ``venv`` again."""
    eng = venv.engine
    N, dev = eng.N, eng.device
    max_step, poll_every = int(max_step), int(poll_every)
    if max_step < 1 or poll_every < 1:
        raise ValueError("max_step and poll_every must be >= 1")
    if not isinstance(controllers, dict):
        controllers = {c.name: c for c in controllers}
    venv.reset()
    venv._drain()  # no report of a step may be pending while the engine is driven directly
    drawn = eng.azimuth.clone()
    if scene_of is not None:
        so = np.asarray(scene_of, dtype=np.int64).reshape(-1)
        if so.shape != (N,) or so.min() < 0 or so.max() >= N:
            raise ValueError(f"scene_of must hold {N} env indices")
        eng.set_scene(np.arange(N), eng.scene_mesh.cpu()[so], eng.scene_offset.cpu()[so])
        drawn = drawn[torch.as_tensor(so, device=dev)]  # a scene keeps the azimuth it was accepted at
    if azimuth is None:
        az = drawn
    else:
        az = torch.as_tensor(azimuth, dtype=torch.float32).to(dev).expand(N).contiguous()
    gens = controller_generators(generator, len(controllers))
    return {name: _run(eng, c, max_step, az, g, poll_every, trace) for (name, c), g in zip(controllers.items(), gens)}


def write_iterations(path, iterations, keys=None) -> dict:
    """The reference's ``iterations_*.txt``: ``repr`` of a dict key -> count, which ``ast.literal_eval(...).values()`` reads
    back (BayesianTTest.py:60-72, plotter.py:22-31).  ``keys``: default 0, 1, ... (test.py's scene number); iterator.py uses
    the azimuth.  Returns the dict."""
    counts = [int(v) for v in (iterations.tolist() if hasattr(iterations, "tolist") else iterations)]
    keys = list(range(len(counts))) if keys is None else [k.item() if hasattr(k, "item") else k for k in keys]
    if len(keys) != len(counts) or len(set(keys)) != len(keys):
        raise ValueError("write_iterations: one distinct key per count")
    d = dict(zip(keys, counts))
    with open(path, "w") as f:
        f.write(repr(d))
    return d


def summarise_iterations(results: dict) -> dict:
    """``results``: name -> the dict of ``evaluate_controllers`` (or anything with ``iterations`` and ``finished``).  Per
    controller the ``mean`` and ``median`` of the iterations and the ``finished`` share; per pair ``(a, b)`` in the given order
    the ``mean`` and ``std`` (sample, ddof = 1; 0 for a single scene) of the paired difference ``a - b`` and ``faster``, the
    share of scenes on which ``a`` needed fewer steps."""
    its = {k: np.asarray(torch.as_tensor(v["iterations"]).cpu(), dtype=np.float64) for k, v in results.items()}
    fin = {k: np.asarray(torch.as_tensor(v["finished"]).cpu(), dtype=bool) for k, v in results.items()}
    out = dict(controllers={k: dict(mean=float(x.mean()), median=float(np.median(x)), finished=float(fin[k].mean()))
                            for k, x in its.items()}, pairs={})
    for a, b in itertools.combinations(its, 2):
        d = its[a] - its[b]
        out["pairs"][(a, b)] = dict(mean=float(d.mean()), std=float(d.std(ddof=1)) if d.size > 1 else 0.0,
                                    faster=float((d < 0).mean()))
    return out
