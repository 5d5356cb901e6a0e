"""The one host path of the native training wrappers: ``seghead.SegmentationHead`` (decoder and classifier),
``enctrain.TrainableEncoder`` (dense encoder), ``septrain.TrainableSeparableEncoder`` (separable encoder),
``fullnet.TrainableFullNetwork`` (dense encoder and decoder) and ``sepfullnet.TrainableSeparableFullNetwork`` (separable
encoder and decoder).  Each of them is a ``TrainableNet`` over one or two ``Part``s,
and one ``torch.autograd.Function`` runs them all: forward folds the current
BatchNorm parameters on the device in f64, packs every part in the library's layout and runs the native train forward;
backward runs the native backward and maps each part's packed gradient back to the parameters.

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
from typing import Callable, NamedTuple, Optional, Tuple

import torch

from . import _native as nat
from .encoder import (BN_EPS, CH, DECODER_KEYS, FEATURES, PRESETS, FrozenEncoder, decoder_packed_floats, decoder_plan, layer_plan,
                      packed_floats)

LEAVES = ("conv.weight", "conv.bias", "bn.weight", "bn.bias")  # the four parameters of a dense layer, in packed order
# those of a separable layer: depthwise (3,1), depthwise (1,3), pointwise, its bias, then the BatchNorm affine
SEP_LEAVES = ("conv.0.weight", "conv.1.weight", "conv.2.weight", "conv.2.bias", "bn.weight", "bn.bias")
ENCODER_PERM, DECODER_PERM = (1, 2, 3, 0), (0, 2, 3, 1)  # conv (cout,cin,3,3) / transposed conv (cin,cout,3,3) -> (cin,3,3,cout)


# ---- the BatchNorm fold and the packed layout, as pure functions of tensors on any device ----------------------------------
def fold_bn_vectors(gamma, beta, mean, var):
    """-> (scale, shift, rstd) in f64: y = relu(.) * scale + shift (``encoder.fold_bn`` on c-vectors)."""
    rstd = 1.0 / torch.sqrt(var.double() + BN_EPS)
    scale = gamma.double() * rstd
    return scale, beta.double() - mean.double() * scale, rstd


def bn_param_grads(dscale, dshift, mean, var):
    """(dgamma, dbeta) in f64 from the gradients of the folded affine: scale = gamma rstd, shift = beta - mean gamma rstd."""
    rstd = 1.0 / torch.sqrt(var.double() + BN_EPS)
    return (dscale.double() - mean.double() * dshift.double()) * rstd, dshift.double()


def pack_layers(layers, perm, tail=()) -> torch.Tensor:
    """layers: (w, bias, scale, shift) each, ``w.permute(perm)`` being (cin,3,3,cout) -> the packed f32 buffer
    w[ci][ky * 3 + kx][co] | bias | scale | shift per layer, then the ``tail`` tensors."""
    parts = []
    for w, b, s, t in layers:
        parts += [w.permute(*perm).reshape(-1), b.reshape(-1), s.reshape(-1), t.reshape(-1)]
    parts += [x.reshape(-1) for x in tail]
    return torch.cat([p.to(torch.float32) for p in parts])


def unpack_layers(buf: torch.Tensor, plan, perm):
    """The inverse of ``pack_layers`` for layers of ``plan`` = [(cin, cout)] -> ([(w, bias, scale, shift)], views of ``buf``;
    the offset of the tail)."""
    inverse = [perm.index(d) for d in range(4)]
    layers, off = [], 0
    for cin, cout in plan:
        w = buf[off:off + 9 * cin * cout].reshape(cin, 3, 3, cout).permute(*inverse)
        off += 9 * cin * cout
        layers.append((w, buf[off:off + cout], buf[off + cout:off + 2 * cout], buf[off + 2 * cout:off + 3 * cout]))
        off += 3 * cout
    return layers, off


def _encoder_plan():
    return [(cin, cout) for _stem, cin, cout, _sep, _stride in layer_plan(False)]


def pack_encoder_buffer(layers) -> torch.Tensor:
    """layers: sixteen (w (cout,cin,3,3), bias, scale, shift) -> the packed f32 buffer of the dense encoder
    (``encoder.pack_state_dict``)."""
    buf = pack_layers(layers, ENCODER_PERM)
    assert buf.numel() == packed_floats(False)
    return buf


def unpack_encoder_buffer(buf: torch.Tensor):
    """The inverse of ``pack_encoder_buffer`` -> [(w (cout,cin,3,3), bias, scale, shift)] x 16, views of ``buf``."""
    if buf.numel() != packed_floats(False):
        raise ValueError(f"packed dense encoder buffer has {buf.numel()} floats, expected {packed_floats(False)}")
    return unpack_layers(buf, _encoder_plan(), ENCODER_PERM)[0]


def _sep_plan():
    return [(cin, cout, sep) for _stem, cin, cout, sep, _stride in layer_plan(True)]


def pack_sep_encoder_buffer(layers) -> torch.Tensor:
    """layers: sixteen tuples in packed order, a separable layer (wv (cin,1,3,1), wh (cin,1,1,3), pw (cout,cin,1,1), bias,
    scale, shift), a down (w (cout,cin,3,3), bias, scale, shift) -> the packed f32 buffer of the separable encoder
    (``encoder.pack_state_dict``): wv[ci][3] | wh[ci][3] | pw[ci][co] | bias | scale | shift per separable layer, the dense
    layout per down."""
    parts = []
    for layer in layers:
        if len(layer) == 6:
            wv, wh, pw, b, s, t = layer
            parts += [wv.reshape(-1), wh.reshape(-1), pw[:, :, 0, 0].t().reshape(-1), b.reshape(-1), s.reshape(-1), t.reshape(-1)]
        else:
            parts.append(pack_layers([layer], ENCODER_PERM))
    buf = torch.cat([p.to(torch.float32) for p in parts])
    assert buf.numel() == packed_floats(True)
    return buf


def unpack_sep_encoder_buffer(buf: torch.Tensor):
    """The inverse of ``pack_sep_encoder_buffer`` -> sixteen tuples of views of ``buf`` in the checkpoint's shapes."""
    if buf.numel() != packed_floats(True):
        raise ValueError(f"packed separable encoder buffer has {buf.numel()} floats, expected {packed_floats(True)}")
    layers, off = [], 0
    for cin, cout, sep in _sep_plan():
        if sep:
            wv = buf[off:off + 3 * cin].reshape(cin, 1, 3, 1)
            wh = buf[off + 3 * cin:off + 6 * cin].reshape(cin, 1, 1, 3)
            off += 6 * cin
            pw = buf[off:off + cin * cout].reshape(cin, cout).t().reshape(cout, cin, 1, 1)
            off += cin * cout
            layers.append((wv, wh, pw, buf[off:off + cout], buf[off + cout:off + 2 * cout], buf[off + 2 * cout:off + 3 * cout]))
            off += 3 * cout
        else:
            (layer,), used = unpack_layers(buf[off:], [(cin, cout)], ENCODER_PERM)
            layers.append(layer)
            off += used
    return layers


def pack_decoder_buffer(levels, cls_w, cls_b) -> torch.Tensor:
    """levels: five (w (2c,c,3,3), bias, scale, shift) -> the packed f32 buffer of the decoder, then cls_w[8] | cls_b
    (``encoder.pack_decoder``)."""
    buf = pack_layers(levels, DECODER_PERM, (cls_w, cls_b))
    assert buf.numel() == decoder_packed_floats()
    return buf


def unpack_decoder_buffer(buf: torch.Tensor):
    """The inverse of ``pack_decoder_buffer`` -> ([(w (2c,c,3,3), bias, scale, shift)] x 5, cls_w (1,8,1,1), cls_b (1,))."""
    if buf.numel() != decoder_packed_floats():
        raise ValueError(f"packed decoder buffer has {buf.numel()} floats, expected {decoder_packed_floats()}")
    levels, off = unpack_layers(buf, [(cin, cout) for _j, cin, cout in decoder_plan()], DECODER_PERM)
    return levels, buf[off:off + CH].reshape(1, CH, 1, 1), buf[off + CH:off + CH + 1]


def align256(b: int) -> int:
    """The 256-byte alignment of every part of a native workspace (include/occlusionenv_amd.h)."""
    return (b + 255) & ~255


BN_MOMENTUM = 0.1  # nn.BatchNorm2d's default, which the reference's layers keep


def bn_layer_shapes(img: int):
    """[(channels, pixels of one env's plane)] of the 21 BatchNorm layers of the joint network on side ``img``, in packed
    order (16 encoder layers, 5 decoder levels): the layout of ``bn_stats`` (mean[c] | var_biased[c] per layer)."""
    shapes, h = [], img
    for _stem, _cin, cout, _sep, stride in layer_plan(False):
        h = (h + stride - 1) // stride
        shapes.append((cout, h * h))
    return shapes + [(cout, ((img // 16) << j) ** 2) for j, _cin, cout in decoder_plan()]


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


# ---- a trainable part: where its tensors sit in the checkpoint and how they are packed -------------------------------------
class Part(NamedTuple):
    stems: Tuple[str, ...]  # per layer in packed order: stem + its leaves are its parameters, stem + "bn.running_*" its statistics
    tail: Tuple[str, ...]   # the parameters packed after the layers
    floats: int             # of the packed buffer
    pack: Callable          # (layers, tail tensors) -> packed buffer; a layer: (its conv leaves.., scale, shift)
    unpack: Callable        # packed buffer -> (layers, tail tensors)
    leaves: Optional[Tuple[Tuple[str, ...], ...]] = None  # per layer, ending in bn.weight, bn.bias; None: LEAVES for every layer

    def layer_leaves(self):
        return self.leaves if self.leaves is not None else (LEAVES,) * len(self.stems)


def encoder_part(preset: str) -> Part:
    """The 16 layers of the dense encoder under ``PRESETS[preset]``'s prefix."""
    stems = tuple(PRESETS[preset][0] + stem for stem, _ci, _co, _sep, _stride in layer_plan(False))
    return Part(stems, (), packed_floats(False), lambda layers, _tail: pack_encoder_buffer(layers),
                lambda buf: (unpack_encoder_buffer(buf), ()))


def sep_encoder_part(preset: str) -> Part:
    """The 16 layers of the separable encoder under ``PRESETS[preset]``'s prefix: eleven separable layers, five dense downs."""
    plan = layer_plan(True)
    stems = tuple(PRESETS[preset][0] + stem for stem, _ci, _co, _sep, _stride in plan)
    leaves = tuple(SEP_LEAVES if sep else LEAVES for _stem, _ci, _co, sep, _stride in plan)
    return Part(stems, (), packed_floats(True), lambda layers, _tail: pack_sep_encoder_buffer(layers),
                lambda buf: (unpack_sep_encoder_buffer(buf), ()), leaves)


def decoder_part(preset: str) -> Part:
    """The 5 up levels of the decoder and the 1x1 classifier under ``DECODER_KEYS[preset]``'s prefixes."""
    prefix, classifier = DECODER_KEYS[preset]
    stems = tuple(f"{prefix}{j}.up." for j, _ci, _co in decoder_plan())

    def unpack(buf):
        levels, cls_w, cls_b = unpack_decoder_buffer(buf)
        return levels, (cls_w, cls_b)

    return Part(stems, (classifier + "weight", classifier + "bias"), decoder_packed_floats(),
                lambda levels, tail: pack_decoder_buffer(levels, *tail), unpack)


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
