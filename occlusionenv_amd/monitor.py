"""The training log of the reference's main script on the batched env: episode returns, lengths and the running reward.

trainRL.py:176-178,189-247 keeps ``current_ep_reward`` and the loop index ``t`` on the host and, at the end of every
episode, writes ``episode,timestep,reward,running_reward,length`` to a CSV.  On the vectorised env an episode's end is
not in what ``step`` returns: a time-limit reset leaves ``dones`` False (the reference's ``is_terminal``), the boundary is
only in the auto-reset report on the device (``SimpleVecEnv.episode_end_codes``).  ``EpisodeMonitor`` keeps the
per-env accumulators, a ring of completed episodes and the totals on the device: one launch per step
(``occ_rollout_advance``, csrc/occ_rollout.hpp; tests/rollout_model.py is the rule in numpy) and one small copy to the
host whenever the caller wants the log (``drain``).

    mon = EpisodeMonitor(venv.num_envs, "cuda")
    venv.reset(); mon.reset()
    for ...:
        obs, rewards, dones, infos = venv.step(actions)
        mon.advance(rewards, venv.episode_end_codes, dones)
    mon.write_csv("log.csv")

Deviations of the batched log from the reference's: a vector step advances the timestep by N, and
the episodes that end in the same vector step are logged in env-index order.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np
import torch

from . import _native as nat

CSV_HEADER = "episode,timestep,reward,running_reward,length"
_HEADER_BYTES = 48  # n_episodes i64 | code_counts 2 x i64 | sums 2 x f64 | running f32 | pad
# the ring's arrays in the order they follow the header: 8-byte entries first, so that every array stays aligned
_RING = (("timestep", np.int64, torch.int64), ("env", np.int32, torch.int32), ("ret", np.float32, torch.float32),
         ("length", np.int32, torch.int32), ("code", np.int32, torch.int32), ("running", np.float32, torch.float32))


class EpisodeMonitor:
    """Episode bookkeeping of ``n_envs`` envs on ``device``; ``capacity``: the ring's entries, i.e. how many episodes may
    complete between two drains before the oldest are lost (counted, never silently)."""

    def __init__(self, n_envs: int, device, capacity: int = 4096):
        if n_envs <= 0 or capacity <= 0:
            raise ValueError("EpisodeMonitor needs n_envs >= 1 and capacity >= 1")
        self.n, self.cap = int(n_envs), int(capacity)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise nat.NativeError("EpisodeMonitor keeps its state on the GPU; there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = nat.load()
        self.ep_return = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        self.ep_len = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        # header and ring in ONE allocation: a drain is one copy
        self._blob = torch.zeros(_HEADER_BYTES + sum(np.dtype(d).itemsize for _, d, _ in _RING) * self.cap, dtype=torch.uint8,
                                 device=self.device)
        st, base = nat.OccRolloutState(), self._blob.data_ptr()
        st.ep_return, st.ep_len = self.ep_return.data_ptr(), self.ep_len.data_ptr()
        st.n_episodes, st.code_counts, st.sums, st.running = base, base + 8, base + 24, base + 40
        self._off, off = {}, _HEADER_BYTES
        for name, npdt, _ in _RING:
            self._off[name] = off
            off += np.dtype(npdt).itemsize * self.cap
        st.ring_timestep, st.ring_env, st.ring_return = base + self._off["timestep"], base + self._off["env"], base + self._off["ret"]
        st.ring_length, st.ring_code, st.ring_running = base + self._off["length"], base + self._off["code"], base + self._off["running"]
        self._state = st
        self.steps = 0      # vector steps seen by advance()
        self._drained = 0   # episodes handed out (or lost) so far
        self._header = self._parse_header(np.zeros(_HEADER_BYTES, np.uint8))

    # ---- device side ------------------------------------------------------------------------------------------------
    def reset(self) -> None:
        """After ``venv.reset()``: every env starts a new episode (the ring, the totals and the step count stay)."""
        self.ep_return.zero_()
        self.ep_len.zero_()

    def advance(self, rewards: torch.Tensor, codes: torch.Tensor, dones: torch.Tensor, buffer=None, t: Optional[int] = None,
                timestep: Optional[int] = None) -> None:
        """One launch after ``venv.step``: ``rewards`` (N) f32, ``codes`` (N) int32 (``venv.episode_end_codes``), ``dones``
        (N) bool or uint8.  ``buffer`` (a ``ppo.RolloutBuffer``) and ``t``: row t of its ``rewards`` / ``dones`` is written
        by the same launch.  ``timestep``: what the entries of this step carry; default (vector steps so far, this one
        included) * N, the reference's ``time_step`` after its increment (trainRL.py:206,239)."""
        n = self.n
        rewards = rewards.detach()
        if dones.dtype == torch.bool:
            dones = dones.view(torch.uint8)
        for name, x, dt in (("rewards", rewards, torch.float32), ("codes", codes, torch.int32), ("dones", dones, torch.uint8)):
            if x.shape != (n,) or x.dtype != dt or x.device != self.device or not x.is_contiguous():
                raise ValueError(f"{name} must be a contiguous ({n},) {dt} tensor on {self.device}")
        self.steps += 1
        if timestep is None:
            timestep = self.steps * n
        T, rew_buf, done_buf = 0, None, None
        if buffer is not None:
            if t is None or buffer.n != n or buffer.rewards.device != self.device:
                raise ValueError("advance(buffer=) needs the step index t and a buffer of this monitor's envs and device")
            T, rew_buf, done_buf = buffer.T, buffer.rewards, buffer.dones
        nat.check(self.lib.occ_rollout_advance(nat.ptr(rewards), nat.ptr(dones), nat.ptr(codes), n, int(t or 0), int(T),
                                               int(timestep), nat.ptr(rew_buf), nat.ptr(done_buf), C.byref(self._state),
                                               self.cap, nat.stream_ptr(self.device)), "occ_rollout_advance")

    # ---- host side --------------------------------------------------------------------------------------------------
    @staticmethod
    def _parse_header(raw: np.ndarray) -> dict:
        n_ep = int(raw[0:8].view(np.int64)[0])
        counts = raw[8:24].view(np.int64)
        sums = raw[24:40].view(np.float64)
        return dict(episodes=n_ep, done=int(counts[0]), time_limit=int(counts[1]),
                    mean_return=float(sums[0]) / n_ep if n_ep else float("nan"),
                    mean_length=float(sums[1]) / n_ep if n_ep else float("nan"),
                    running_reward=float(raw[40:44].view(np.float32)[0]))

    def drain(self) -> dict:
        """The episodes completed since the last drain, oldest first: arrays ``episode`` (1-based number, the log's first
        column), ``env``, ``ret`` (f32), ``length``, ``code`` (1 = done, 2 = time limit), ``timestep``, ``running`` (the
        running reward after the episode, f32), and ``lost``: how many more completed but were overwritten in the ring
        before this drain (they are in the totals, their rows are gone); ``totals``: what ``totals()`` gives.  One copy of the ring to the host: the one
        host sync."""
        raw = self._blob.cpu().numpy()
        self._header = self._parse_header(raw)
        total = self._header["episodes"]
        new = total - self._drained
        kept = min(new, self.cap)
        ordinal = np.arange(total - kept, total, dtype=np.int64)
        slot = ordinal % self.cap
        out = dict(episode=ordinal + 1, lost=int(new - kept), totals=dict(self._header))
        for name, npdt, _ in _RING:
            lo = self._off[name]
            out[name] = raw[lo:lo + np.dtype(npdt).itemsize * self.cap].view(npdt)[slot].copy()
        self._drained = total
        return out

    def totals(self) -> dict:
        """Counts and means over every episode completed so far (lost ones included): ``episodes``, ``done``,
        ``time_limit``, ``mean_return``, ``mean_length``, ``running_reward``.  Reads the header from the device (a sync)."""
        self._header = self._parse_header(self._blob[:_HEADER_BYTES].cpu().numpy())
        return dict(self._header)

    @property
    def running_reward(self) -> float:
        """trainRL.py:236's running reward after the last completed episode (read from the device: a sync)."""
        return self.totals()["running_reward"]

    @staticmethod
    def csv_rows(episodes: dict) -> list:
        """The reference's rows (trainRL.py:235-239: reward and running reward rounded to 4 places) of a ``drain()`` result."""
        return ["{},{},{},{},{}".format(int(ep), int(ts), round(float(r), 4), round(float(rr), 4), int(ln))
                for ep, ts, r, rr, ln in zip(episodes["episode"], episodes["timestep"], episodes["ret"], episodes["running"],
                                             episodes["length"])]

    def write_csv(self, path, episodes: Optional[dict] = None) -> dict:
        """Append the rows of ``episodes`` (default: ``self.drain()``) to ``path``; a new or empty file gets the header
        first (trainRL.py:178).  Returns the episodes."""
        if episodes is None:
            episodes = self.drain()
        fresh = not os.path.exists(path) or os.path.getsize(path) == 0
        with open(path, "a") as f:
            if fresh:
                f.write(CSV_HEADER + "\n")
            for row in self.csv_rows(episodes):
                f.write(row + "\n")
        return episodes
