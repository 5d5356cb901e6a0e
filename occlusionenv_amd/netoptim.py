"""``PackedAdamW``: ``torch.optim.AdamW`` (pretrainer.py:91) for a joint network (``fullnet.JointNet``, dense or separable,
either BatchNorm mode) on the library's packed layout, one native launch per step (csrc/occ_adamw.hpp, ``occ_net_adamw_*``).

Why.  The native train forward reads, and the native backward writes, one packed f32 buffer per part (encoder; decoder with
the classifier).  With the parameters under the checkpoint's ~110 keys a step folds 21 BatchNorm layers and ``cat``s the
buffers before the forward, slices the packed gradient into ~110 clones after the backward, and ``torch.optim.AdamW`` then
walks the same tensors: several hundred small launches around the backward.  Every packed slot is a permutation of a
checkpoint tensor or half of a BatchNorm (scale, shift) pair, and AdamW is elementwise, so it can run in packed order.

``PackedAdamW(net)`` makes ``net`` packed-resident (``net._resident``, a ``PackedState``):

  * per part one master tensor in packed order whose BatchNorm slots hold raw gamma and beta, built once from the current
    parameters with the part's own ``netlayout.Part.pack``; a flat tensor (weight | bias) for the grad head.  These are the trainable
    leaves: plain attributes, not registered parameters, so the state-dict keys stay the checkpoint's;
  * per part the packed buffer the forward reads, written by the optimizer's kernel: a copy of the master with, under running
    statistics, every (gamma, beta) folded to (scale, shift) in f64 as ``netlayout.fold_bn_vectors`` folds them, to the bit;
  * ``net(obs)`` runs ``nettrain._PackedStep``: the native forward on those buffers, the packed gradients returned unchanged
    as the masters' ``.grad`` (autograd adds the gradients of several backward calls); the head's ``linear`` reads views of
    the flat tensor;
  * ``opt.step()`` is one launch: the chain rule (d scale, d shift) -> (d gamma, d beta) under running statistics, torch's
    AdamW rule in f32 on every slot (the decay on gamma, beta and the biases too: the reference's single parameter group;
    the roundings are those of torch's foreach implementation on the device, so that training with either optimizer
    leaves the same bits), and the next forward's packed buffers.  ``param_groups[0]["lr"]`` is read at every step, so the
    lr schedulers drive it; ``state_dict()`` / ``load_state_dict()`` are ``torch.optim.Optimizer``'s and carry ``exp_avg``,
    ``exp_avg_sq`` and ``step`` per leaf, in packed order;
  * ``net.sync_parameters()`` writes the masters back to the per-key parameters (``Part.unpack``); ``net.state_dict()`` does it
    first, so ``enc.with_state(net.state_dict())`` and ``BatchedPPO.from_fullnetwork(net.state_dict())`` see the trained
    values; ``net.load_state_dict`` re-packs.  Between syncs ``net.parameters()`` are stale;
  * when the BatchNorm mode of a step differs from the previous one's (``net.train()`` / ``net.eval()`` with
    ``batch_stats=True``) the packed buffers are re-derived from the masters, with the running statistics of that moment, by
    the kernel's own fold; the moments are kept.  Running statistics that are changed by hand under running-statistics mode
    need ``net._resident.invalidate()``.

A leaf without a gradient is left out of a step as ``torch.optim`` leaves it out (in practice the head, when a loss does not
use it); the step count is one for all leaves.  A net without ``PackedAdamW`` is untouched by all of this.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native as nat

HEAD_FLOATS = 2 * 256 + 2  # gradPredictor: weight (2,256) | bias (2,)


class PackedState:
    """The packed-resident tensors of a ``JointNet``: ``theta`` (the masters, leaves), ``out`` (what the forward reads),
    ``head`` (flat leaf or None), ``stats`` (the running statistics, mean[c] | var[c] per layer in packed order)."""

    def __init__(self, net):
        self.net = net
        dev = net.enc.device
        sizes = [C.c_int64(), C.c_int64(), C.c_int64()]
        nat.check(nat.load().occ_net_adamw_query(C.byref(net._cfg(64)), *[C.byref(s) for s in sizes]), "occ_net_adamw_query")
        enc_floats, dec_floats, stat_floats = (int(s.value) for s in sizes)
        if [enc_floats, dec_floats] != [part.floats for part in net.parts]:
            raise nat.NativeError("the library's packed sizes do not match the network's parts")
        self.theta = [torch.empty(part.floats, dtype=torch.float32, device=dev).requires_grad_() for part in net.parts]
        self.out = [torch.empty(part.floats, dtype=torch.float32, device=dev) for part in net.parts]
        self.head = torch.empty(HEAD_FLOATS, dtype=torch.float32, device=dev).requires_grad_() if net.has_grad_head else None
        self.stats = torch.empty(stat_floats, dtype=torch.float32, device=dev)
        self.mode: Optional[bool] = None  # the BatchNorm mode ``out`` was derived for; None: to be derived
        self.repack()

    def leaves(self):
        return self.theta + ([self.head] if self.head is not None else [])

    def _head_keys(self):
        return self.net.grad_prefix + "weight", self.net.grad_prefix + "bias"

    @torch.no_grad()
    def repack(self) -> None:
        """The masters from the per-key parameters: ``Part.pack`` with gamma, beta in the scale / shift slots."""
        net = self.net
        for part, theta in zip(net.parts, self.theta):
            layers = [tuple(net.get_parameter(stem + leaf) for leaf in leaves)
                      for stem, leaves in zip(part.stems, part.layer_leaves())]
            theta.copy_(part.pack(layers, [net.get_parameter(k) for k in part.tail]))
        if self.head is not None:
            self.head.copy_(torch.cat([net.get_parameter(k).reshape(-1) for k in self._head_keys()]))
        self.invalidate()

    def invalidate(self) -> None:
        """The next forward re-derives the packed buffers from the masters and the current running statistics."""
        self.mode = None

    @torch.no_grad()
    def sync(self) -> None:
        """The per-key parameters from the masters: ``Part.unpack``."""
        net = self.net
        for part, theta in zip(net.parts, self.theta):
            layers, tail = part.unpack(theta)
            for stem, leaves, layer in zip(part.stems, part.layer_leaves(), layers):
                for leaf, t in zip(leaves, layer):
                    net.get_parameter(stem + leaf).copy_(t)
            for key, t in zip(part.tail, tail):
                net.get_parameter(key).copy_(t)
        if self.head is not None:
            for key, t in zip(self._head_keys(), self.head_views()):
                net.get_parameter(key).copy_(t)

    def head_views(self):
        """(weight (2,256), bias (2,)) as views of the flat head leaf."""
        return self.head[:HEAD_FLOATS - 2].view(2, 256), self.head[HEAD_FLOATS - 2:]

    @torch.no_grad()
    def packed_for(self, bn: bool):
        """The packed buffers of a forward in BatchNorm mode ``bn`` (True: batch statistics), re-derived when the mode changed."""
        if self.mode != bn:
            net = self.net
            if not bn:
                stems = [stem for part in net.parts for stem in part.stems]
                torch.cat([t for stem in stems for t in net._stats(stem)], out=self.stats)
            nat.check(nat.load().occ_net_adamw_fold(C.byref(net._cfg(64)), nat.ptr(self.theta[0]), nat.ptr(self.out[0]),
                                                    nat.ptr(self.theta[1]), nat.ptr(self.out[1]), nat.ptr(self.stats), int(bn),
                                                    nat.stream_ptr(self.stats.device)), "occ_net_adamw_fold")
            self.mode = bn
        return self.out


class PackedAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` (decoupled decay, ``amsgrad`` and ``maximize`` off) on the packed leaves of ``net``, a
    ``fullnet.JointNet``; see the module docstring.  One param group; its ``lr``, ``betas``, ``eps`` and ``weight_decay`` are
    read at every step.  ``last_call``: the scalars the kernel took in the latest step."""

    def __init__(self, net, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-5):
        from .fullnet import JointNet

        if not isinstance(net, JointNet):
            raise ValueError("PackedAdamW needs a joint network (fullnet.TrainableFullNetwork or "
                             f"sepfullnet.TrainableSeparableFullNetwork), got {type(net).__name__}")
        if net._resident is None:
            net._resident = PackedState(net)
        self._res = net._resident
        self._init_leaves(self._res.leaves(), lr, betas, eps, weight_decay)

    def _init_leaves(self, leaves, lr, betas, eps, weight_decay):
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 < float(eps):
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= float(betas[0]) < 1.0 and 0.0 <= float(betas[1]) < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= float(weight_decay):
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        self.last_call = None
        super().__init__(leaves, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))

    @classmethod
    def _over_leaves(cls, leaves, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5):
        """The optimizer's bookkeeping (state, ``state_dict`` round trip) over given leaf tensors, without a net: it cannot step."""
        self = cls.__new__(cls)
        self._res = None
        self._init_leaves(list(leaves), lr, betas, eps, weight_decay)
        return self

    def moments(self, p):
        """The state of leaf ``p`` (``step``, ``exp_avg``, ``exp_avg_sq``, as ``torch.optim.AdamW`` names them), made on first use."""
        st = self.state[p]
        if not st:
            st["step"] = torch.tensor(0.0)
            st["exp_avg"] = torch.zeros_like(p, requires_grad=False)
            st["exp_avg_sq"] = torch.zeros_like(p, requires_grad=False)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        res = self._res
        if res is None:
            raise RuntimeError("this PackedAdamW was made over bare leaves: it has no network to step")
        if len(self.param_groups) != 1:
            raise RuntimeError("PackedAdamW keeps one param group, as the reference's optimizer does")
        group = self.param_groups[0]
        enc, dec = res.theta
        if enc.grad is None or dec.grad is None:
            return loss  # nothing was back-propagated
        head = res.head if res.head is not None and res.head.grad is not None else None
        states = [self.moments(p) for p in (enc, dec)] + ([self.moments(head)] if head is not None else [])
        step = int(states[0]["step"]) + 1
        beta1, beta2 = group["betas"]
        call = dict(lr=float(group["lr"]), beta1=float(beta1), beta2=float(beta2), eps=float(group["eps"]),
                    weight_decay=float(group["weight_decay"]), step=step, bn_mode=int(bool(res.mode)))
        args = []
        for p, st, out in zip((enc, dec), states, res.out):
            args += [nat.ptr(p), nat.ptr(st["exp_avg"]), nat.ptr(st["exp_avg_sq"]), nat.ptr(p.grad.contiguous()), nat.ptr(out)]
        args.append(nat.ptr(res.stats))
        if head is not None:
            st = states[2]
            args += [nat.ptr(head), nat.ptr(st["exp_avg"]), nat.ptr(st["exp_avg_sq"]), nat.ptr(head.grad.contiguous()), head.numel()]
        else:
            args += [None, None, None, None, 0]
        nat.check(nat.load().occ_net_adamw_step(C.byref(res.net._cfg(64)), *args, call["lr"], call["beta1"], call["beta2"],
                                                call["eps"], call["weight_decay"], step, call["bn_mode"],
                                                nat.stream_ptr(enc.device)), "occ_net_adamw_step")
        for st in states:
            st["step"] += 1
        res.net._version += 1  # the packed buffers a pending backward would read are gone
        self.last_call = call
        return loss
