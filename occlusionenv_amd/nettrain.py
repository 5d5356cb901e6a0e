"""The one host path of the native training wrappers: ``seghead.SegmentationHead`` (decoder and classifier),
``enctrain.TrainableEncoder`` (dense encoder), ``septrain.TrainableSeparableEncoder`` (separable encoder),
``fullnet.TrainableFullNetwork`` (dense encoder and decoder) and ``sepfullnet.TrainableSeparableFullNetwork`` (separable
encoder and decoder).  Each of them is a ``TrainableNet`` over one or two ``netlayout.Part``s, and one
``torch.autograd.Function`` runs them all: forward folds the current BatchNorm parameters on the device in f64
(``netlayout.fold_bn_vectors``), packs every part in the library's layout (``Part.pack``) and runs the native train forward;
backward runs the native backward and maps each part's packed gradient back to the parameters (``Part.unpack``).

BatchNorm keeps its running statistics (buffers); only its affine parameters train.  The joint networks
(``fullnet.JointNet``) also offer ``batch_stats=True``, ``nn.BatchNorm2d`` in train mode as pretrainer.py runs it: while
``net.training`` the step packs gamma / beta unfolded, runs the ``occ_fullnet_bn_*`` entry points (csrc/occ_bn_train.hpp),
which normalise every layer with the statistics of the batch and return d gamma / d beta themselves, and moves the running
buffers towards the batch's mean and unbiased variance (momentum 0.1) without a host sync; every layer must see at least two
values per channel, ``N (S / 32)^2 >= 2``.  After ``net.eval()`` the step is the running-statistics one, bit for bit.
A training call is one chunk (``N <= enc.max_chunk``), and the kept activations belong to the latest forward: a backward of
an earlier forward raises.

A joint network under ``netoptim.PackedAdamW`` is packed-resident (``net._resident``): its trainable leaves are one packed
master tensor per part, and a second autograd function, ``_PackedStep``, hands the packed buffers the optimizer's kernel
wrote to the same native forward and returns the packed gradients as they are; nothing is folded, packed or sliced per key.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _native as nat
from .encoder import FrozenEncoder
# the fold and the packed layout, as pure functions of tensors on any device: netlayout's, importable here as before
from .netlayout import (DECODER_PERM, ENCODER_PERM, FEATURES, LEAVES, SEP_LEAVES, Part, bn_layer_shapes, bn_param_grads,  # noqa: F401
                        decoder_part, encoder_part, fold_bn_vectors, pack_decoder_buffer, pack_encoder_buffer, pack_layers,
                        pack_sep_encoder_buffer, sep_encoder_part, unpack_decoder_buffer, unpack_encoder_buffer, unpack_layers,
                        unpack_sep_encoder_buffer)


def align256(b: int) -> int:
    """The 256-byte alignment of every part of a native workspace (include/occlusionenv_amd.h)."""
    return (b + 255) & ~255


BN_MOMENTUM = 0.1  # nn.BatchNorm2d's default, which the reference's layers keep


def register_under_key(module: torch.nn.Module, key: str, t: torch.Tensor, buffer: bool) -> None:
    """Register a copy of ``t`` on ``module`` under the dotted state-dict key, as a buffer or a parameter, creating the
    container modules on the way (the parameters of a ``TrainableNet`` sit under the checkpoint's keys)."""
    *path, leaf = key.split(".")
    m = module
    for name in path:
        if name not in m._modules:
            m.add_module(name, torch.nn.Module())
        m = m._modules[name]
    if buffer:
        m.register_buffer(leaf, t.clone())
    else:
        m.register_parameter(leaf, torch.nn.Parameter(t.clone()))


# ---- the module and its autograd function ------------------------------------------------------------------------------------
class TrainableNet(torch.nn.Module):
    """The trainable ``parts`` of a ``FrozenEncoder``: their tensors (``state``) as parameters, and as buffers for the
    running statistics, under the checkpoint's keys.  A subclass names its three native entry points (``SYMBOLS``: workspace
    query, train forward, backward), says which of (feats, prob) its step returns and which of them carry a gradient, and
    checks its checkpoint before it calls this constructor."""

    SYMBOLS: Tuple[str, str, str]
    RETURNS: Tuple[str, ...]           # of "feats" (N,256) and "prob" (N,1,S,S), in the order of the step's outputs
    DIFFERENTIABLE: Tuple[str, ...]    # those the native backward takes a gradient for, in its argument order
    RUNS_DECODER = True                # the decoder needs S a multiple of 32
    BN_SYMBOLS: Optional[Tuple[str, str, str]] = None  # the three for batch-statistics BatchNorm, where the step offers it

    def __init__(self, enc: FrozenEncoder, parts, state):
        if getattr(enc, "precision", "f32") != "f32":
            raise ValueError(f"training needs the f32 encoder: precision={enc.precision!r} is inference of the pooled feature "
                             "only; use enc.with_precision('f32')")
        super().__init__()
        self.enc = enc  # a plain attribute, not part of the state dict: the preset, the flags, the device and max_chunk
        self.parts = tuple(parts)
        for key, t in state.items():
            register_under_key(self, key, t.to(enc.device, torch.float32), buffer=key.endswith(("running_mean", "running_var")))
        self.batch_stats = False  # True (JointNet): while self.training, BatchNorm runs on the batch's statistics
        self._version = 0
        self._latest = None
        self._bufs = {}
        self._resident = None  # netoptim.PackedState once a PackedAdamW owns the parameters

    @classmethod
    def from_encoder(cls, enc: FrozenEncoder):
        return cls(enc)

    def _cfg(self, img: int):
        return self.enc._cfg(img)

    def _stats(self, stem: str):
        return self.get_buffer(stem + "bn.running_mean"), self.get_buffer(stem + "bn.running_var")

    def ordered_parameters(self):
        """[(key, parameter)] in packed order, part by part: per layer its leaves (dense: conv.weight, conv.bias, bn.weight,
        bn.bias), then the part's tail (the classifier's weight, bias).  A grad head is not among them."""
        names = []
        for part in self.parts:
            names += [stem + leaf for stem, leaves in zip(part.stems, part.layer_leaves()) for leaf in leaves]
            names += part.tail
        return [(k, self.get_parameter(k)) for k in names]

    def _bn_mode(self) -> bool:
        """Whether the next step normalises with batch statistics."""
        return bool(self.batch_stats and self.training)

    def _train_buffers(self, n: int, img: int, bn: bool = False):
        """(workspace, scratch) of a training call on n envs of side img, kept per shape and BatchNorm mode."""
        key = (n, img, bn)
        if key not in self._bufs:
            wsb, scb = C.c_size_t(), C.c_size_t()
            query = (self.BN_SYMBOLS if bn else self.SYMBOLS)[0]
            nat.check(getattr(nat.load(), query)(C.byref(self._cfg(img)), n, C.byref(wsb), C.byref(scb)), query)
            dev = self.enc.device
            self._bufs[key] = (torch.empty(int(wsb.value), dtype=torch.uint8, device=dev),
                               torch.empty(max(int(scb.value), 16), dtype=torch.uint8, device=dev))
        return self._bufs[key]

    def _native_forward(self, img, packed, obs, n, ws, outs, bn: bool = False):
        """The native train forward on the packed parts; ``outs``: feats and, when the step has one, prob (``bn``: and
        bn_stats)."""
        name = (self.BN_SYMBOLS if bn else self.SYMBOLS)[1]
        nat.check(getattr(nat.load(), name)(C.byref(self._cfg(img)), *[nat.ptr(p) for p in packed], nat.ptr(obs), n, nat.ptr(ws),
                                            ws.numel(), *[nat.ptr(o) for o in outs], nat.stream_ptr(obs.device)), name)

    def _native_backward(self, img, packed, n, ws, grads_in, scratch, grads_out, bn: bool = False):
        """The native backward of the latest forward: upstream ``grads_in`` -> one packed gradient per part."""
        name = (self.BN_SYMBOLS if bn else self.SYMBOLS)[2]
        nat.check(getattr(nat.load(), name)(C.byref(self._cfg(img)), *[nat.ptr(p) for p in packed], n, nat.ptr(ws), ws.numel(),
                                            *[nat.ptr(g) for g in grads_in], nat.ptr(scratch), scratch.numel(),
                                            *[nat.ptr(g) for g in grads_out], nat.stream_ptr(grads_in[0].device)), name)

    def _step(self, obs: torch.Tensor):
        """The checks of a training call and the autograd function on it -> the outputs named by ``RETURNS``."""
        self.enc._check_obs(obs, self.RUNS_DECODER)
        n = int(obs.shape[0])
        if n > self.enc.max_chunk:
            raise ValueError(f"a training call is one chunk: N = {n} > max_chunk = {self.enc.max_chunk}")
        if n < 1:
            raise ValueError("a training call needs at least one env")
        if self._bn_mode() and n * (int(obs.shape[2]) // 32) ** 2 < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(obs.shape)}: the "
                             "deepest BatchNorm sees N (S / 32)^2 values")
        obs = obs.detach().to(torch.float32).contiguous()
        if self._resident is not None:
            return _PackedStep.apply(obs, self, *self._resident.theta)
        return _NetStep.apply(obs, self, *[p for _k, p in self.ordered_parameters()])


def _update_running_stats(net, stats: torch.Tensor, n: int, img: int) -> None:
    """nn.BatchNorm2d's running-average rule on every layer of ``net`` from the forward's ``bn_stats``: the mean, and the
    biased variance made unbiased by M / (M - 1).  In place, on the device, no host sync."""
    stems = [stem for part in net.parts for stem in part.stems]
    means, variances, unbias, off = [], [], [], 0
    for c, plane in bn_layer_shapes(img):
        m = n * plane
        means.append(stats[off:off + c])
        variances.append(stats[off + c:off + 2 * c])
        unbias.append(BN_MOMENTUM * m / (m - 1))
        off += 2 * c
    running_mean, running_var = zip(*[net._stats(stem) for stem in stems])
    with torch.no_grad():
        torch._foreach_mul_(list(running_mean) + list(running_var), 1.0 - BN_MOMENTUM)
        torch._foreach_add_(list(running_mean), means, alpha=BN_MOMENTUM)
        torch._foreach_add_(list(running_var), torch._foreach_mul(variances, unbias))


def _native_step_forward(ctx, net, obs, packed, bn):
    """The native train forward of ``net`` on the ``packed`` parts (and, ``bn``, the move of the running buffers), kept on
    ``ctx`` for the backward -> the outputs ``net.RETURNS``."""
    n, img = int(obs.shape[0]), int(obs.shape[2])
    ws, _scratch = net._train_buffers(n, img, bn)
    out = {"feats": torch.empty(n, FEATURES, dtype=torch.float32, device=obs.device)}
    if "prob" in net.RETURNS:
        out["prob"] = torch.empty(n, 1, img, img, dtype=torch.float32, device=obs.device)
    net._version += 1
    net._latest = (n, img)
    if bn:
        stats = torch.empty(2 * sum(c for c, _plane in bn_layer_shapes(img)), dtype=torch.float32, device=obs.device)
        net._native_forward(img, packed, obs, n, ws, list(out.values()) + [stats], bn=True)
        _update_running_stats(net, stats, n, img)
        net.bn_stats = stats  # of the latest train-mode forward: mean[c] | var_biased[c] per layer, packed order
    else:
        net._native_forward(img, packed, obs, n, ws, list(out.values()))
    ctx.net, ctx.packed, ctx.version, ctx.shape, ctx.bn = net, packed, net._version, (n, img), bn
    if len(net.DIFFERENTIABLE) < len(net.RETURNS):
        ctx.mark_non_differentiable(*[out[k] for k in net.RETURNS if k not in net.DIFFERENTIABLE])
    return out[net.RETURNS[0]] if len(net.RETURNS) == 1 else tuple(out[k] for k in net.RETURNS)


def _native_step_backward(ctx, grads):
    """The native backward of the forward kept on ``ctx`` -> one packed gradient per part."""
    net = ctx.net
    if ctx.version != net._version:
        raise RuntimeError(f"{type(net).__name__}: backward of a forward that a later forward has superseded; the kept "
                           "activations belong to the latest forward (call backward before the next forward)")
    n, img = ctx.shape
    ws, scratch = net._train_buffers(n, img, ctx.bn)
    upstream = dict(zip(net.RETURNS, grads))
    grads_in = [upstream[k].to(torch.float32).contiguous() for k in net.DIFFERENTIABLE]
    grads_out = [torch.empty(part.floats, dtype=torch.float32, device=grads_in[0].device) for part in net.parts]
    net._native_backward(img, ctx.packed, n, ws, grads_in, scratch, grads_out, bn=ctx.bn)
    return grads_out


class _NetStep(torch.autograd.Function):
    """(obs, net, the parameters of ``net.ordered_parameters()``) -> the outputs ``net.RETURNS``; the gradient goes to the
    parameters only."""

    @staticmethod
    def forward(ctx, obs, net, *params):
        bn = net._bn_mode()
        folded, at = [], 0
        for part in net.parts:
            layers = []
            for stem, leaves in zip(part.stems, part.layer_leaves()):
                *conv, gamma, beta = params[at:at + len(leaves)]
                if bn:  # the kernels form scale and shift from the batch's statistics
                    scale, shift = gamma, beta
                else:
                    scale, shift, _rstd = fold_bn_vectors(gamma, beta, *net._stats(stem))
                layers.append((*conv, scale, shift))
                at += len(leaves)
            folded.append((layers, params[at:at + len(part.tail)]))
            at += len(part.tail)
        packed = [part.pack(layers, tail).contiguous() for part, (layers, tail) in zip(net.parts, folded)]
        return _native_step_forward(ctx, net, obs, packed, bn)

    @staticmethod
    def backward(ctx, *grads):
        net, grads_out = ctx.net, _native_step_backward(ctx, grads)
        result = [None, None]
        for part, gp in zip(net.parts, grads_out):
            layers, tail = part.unpack(gp)
            for stem, (*dconv, dscale, dshift) in zip(part.stems, layers):
                # batch statistics: the slots hold d gamma / d beta themselves
                dgamma, dbeta = (dscale.clone(), dshift.clone()) if ctx.bn else bn_param_grads(dscale, dshift, *net._stats(stem))
                result += [t.clone(memory_format=torch.contiguous_format) for t in dconv]
                result += [dgamma.to(torch.float32), dbeta.to(torch.float32)]
            result += [t.clone() for t in tail]
        return tuple(result)


class _PackedStep(torch.autograd.Function):
    """(obs, net, the packed master of every part) -> the outputs ``net.RETURNS`` of a packed-resident net: the forward reads
    the packed buffers ``net._resident`` keeps for the step's BatchNorm mode, the gradient of a master is the packed gradient
    of the native backward, unchanged (``netoptim.PackedAdamW``'s kernel takes it as it is)."""

    @staticmethod
    def forward(ctx, obs, net, *_theta):
        bn = net._bn_mode()
        return _native_step_forward(ctx, net, obs, net._resident.packed_for(bn), bn)

    @staticmethod
    def backward(ctx, *grads):
        return (None, None, *_native_step_backward(ctx, grads))
