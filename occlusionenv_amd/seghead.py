"""Fine-tuning of the segmentation head on the device (csrc/occ_decoder_bwd.hpp): the decoder and the 1x1 classifier of a
``FullNetwork`` / ``Segmenter`` as trainable parameters on top of the frozen native encoder.

``SegmentationHead.from_encoder(enc)`` takes a ``FrozenEncoder`` whose checkpoint held the decoder.  ``head(obs)`` is the
predicted occlusion map (N,1,S,S), bitwise ``enc.segment(obs)`` while the parameters are the checkpoint's, and one
``torch.autograd.Function``: forward folds the current parameters into the packed layout on the device and runs
``occ_segment_train_forward``; backward runs ``occ_segment_backward`` and maps the packed gradient back to the parameters.
``obs`` gets no gradient and the encoder stays frozen.  Any torch optimizer works on ``head.parameters()``.

The parameters sit under the reference's state-dict keys (``encoder.DECODER_KEYS``), so ``head.state_dict()`` drops back into
the checkpoint it came from and ``enc.with_decoder(head.state_dict())`` is the fine-tuned network for inference.

Deviation from pretrainer.py, which trains in train mode: the decoder's BatchNorm keeps its running statistics (buffers
here); only its affine parameters train.  A training call is one chunk (``N <= enc.max_chunk``), and the kept activations
belong to the latest forward: a backward of an earlier forward raises.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as nat
from .encoder import BN_EPS, CH, DECODER_KEYS, FEATURES, LEVELS, FrozenEncoder, decoder_packed_floats, decoder_plan


# ---- the packed layout and the BatchNorm fold, as pure functions of tensors on any device ---------------------------------
def fold_bn_vectors(gamma, beta, mean, var):
    """-> (scale, shift, rstd) in f64: y = relu(.) * scale + shift (``encoder.fold_bn`` on c-vectors)."""
    rstd = 1.0 / torch.sqrt(var.double() + BN_EPS)
    scale = gamma.double() * rstd
    return scale, beta.double() - mean.double() * scale, rstd


def bn_param_grads(dscale, dshift, mean, var):
    """(dgamma, dbeta) in f64 from the gradients of the folded affine: scale = gamma rstd, shift = beta - mean gamma rstd."""
    rstd = 1.0 / torch.sqrt(var.double() + BN_EPS)
    return (dscale.double() - mean.double() * dshift.double()) * rstd, dshift.double()


def pack_decoder_buffer(levels, cls_w, cls_b) -> torch.Tensor:
    """levels: five (w (2c,c,3,3), bias, scale, shift) -> the packed f32 buffer: w[ci][ky * 3 + kx][co] | bias | scale |
    shift per level, then cls_w[8] | cls_b."""
    parts = []
    for w, b, s, t in levels:
        parts += [w.permute(0, 2, 3, 1).reshape(-1), b.reshape(-1), s.reshape(-1), t.reshape(-1)]
    parts += [cls_w.reshape(-1), cls_b.reshape(-1)]
    buf = torch.cat([p.to(torch.float32) for p in parts])
    assert buf.numel() == decoder_packed_floats()
    return buf


def unpack_decoder_buffer(buf: torch.Tensor):
    """The inverse of ``pack_decoder_buffer`` -> ([(w (2c,c,3,3), bias, scale, shift)] x 5, cls_w (1,8,1,1), cls_b (1,))."""
    if buf.numel() != decoder_packed_floats():
        raise ValueError(f"packed decoder buffer has {buf.numel()} floats, expected {decoder_packed_floats()}")
    levels, off = [], 0
    for _j, cin, cout in decoder_plan():
        w = buf[off:off + 9 * cin * cout].reshape(cin, 3, 3, cout).permute(0, 3, 1, 2)
        off += 9 * cin * cout
        levels.append((w, buf[off:off + cout], buf[off + cout:off + 2 * cout], buf[off + 2 * cout:off + 3 * cout]))
        off += 3 * cout
    return levels, buf[off:off + CH].reshape(1, CH, 1, 1), buf[off + CH:off + CH + 1]


def _align(b: int) -> int:
    return (b + 255) & ~255


def register_under_key(module: torch.nn.Module, key: str, t: torch.Tensor, buffer: bool) -> None:
    """Register a copy of ``t`` on ``module`` under the dotted state-dict key, as a buffer or a parameter, creating the
    container modules on the way (shared by ``SegmentationHead``, ``enctrain.TrainableEncoder`` and
    ``fullnet.TrainableFullNetwork``, whose parameters sit under the checkpoint's keys)."""
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


class _TrainStep(torch.autograd.Function):
    """(obs, head, 22 parameters) -> (prob, pooled features); the gradient goes to the parameters only."""

    @staticmethod
    def forward(ctx, obs, head, *params):
        levels = []
        for j in range(LEVELS):
            w, b, gamma, beta = params[4 * j:4 * j + 4]
            scale, shift, _rstd = fold_bn_vectors(gamma, beta, *head._stats(j))
            levels.append((w, b, scale, shift))
        packed = pack_decoder_buffer(levels, params[-2], params[-1]).contiguous()
        n, img = int(obs.shape[0]), int(obs.shape[2])
        ws, scratch = head._train_buffers(n, img)
        feats = torch.empty(n, FEATURES, dtype=torch.float32, device=obs.device)
        prob = torch.empty(n, 1, img, img, dtype=torch.float32, device=obs.device)
        enc = head.enc
        head._version += 1
        head._latest = (n, img)
        nat.check(nat.load().occ_segment_train_forward(C.byref(enc._cfg(img)), nat.ptr(enc.packed), nat.ptr(packed), nat.ptr(obs), n,
                                                       nat.ptr(ws), ws.numel(), nat.ptr(feats), nat.ptr(prob),
                                                       nat.stream_ptr(obs.device)), "occ_segment_train_forward")
        ctx.head, ctx.packed, ctx.version, ctx.shape = head, packed, head._version, (n, img)
        ctx.mark_non_differentiable(feats)
        return prob, feats

    @staticmethod
    def backward(ctx, grad_prob, _grad_feats):
        head = ctx.head
        if ctx.version != head._version:
            raise RuntimeError("SegmentationHead: backward of a forward that a later forward has superseded; the kept "
                               "activations belong to the latest forward (call backward before the next head(obs))")
        n, img = ctx.shape
        ws, scratch = head._train_buffers(n, img)
        g = grad_prob.to(torch.float32).contiguous()
        gp = torch.empty(decoder_packed_floats(), dtype=torch.float32, device=g.device)
        enc = head.enc
        nat.check(nat.load().occ_segment_backward(C.byref(enc._cfg(img)), nat.ptr(ctx.packed), n, nat.ptr(ws), ws.numel(), nat.ptr(g),
                                                  nat.ptr(scratch), scratch.numel(), nat.ptr(gp), nat.stream_ptr(g.device)),
                  "occ_segment_backward")
        levels, dcls_w, dcls_b = unpack_decoder_buffer(gp)
        grads = []
        for j, (dw, db, dscale, dshift) in enumerate(levels):
            dgamma, dbeta = bn_param_grads(dscale, dshift, *head._stats(j))
            grads += [dw.contiguous(), db.clone(), dgamma.to(torch.float32), dbeta.to(torch.float32)]
        return (None, None, *grads, dcls_w.clone(), dcls_b.clone())


class SegmentationHead(torch.nn.Module):
    """The trainable decoder and classifier over a frozen ``FrozenEncoder``; see the module docstring."""

    def __init__(self, enc: FrozenEncoder):
        super().__init__()
        if not isinstance(enc, FrozenEncoder):
            raise ValueError("SegmentationHead needs a FrozenEncoder")
        if not enc.has_decoder or enc.decoder_state is None:
            raise ValueError("this checkpoint has no segmentation decoder (no 'segmenter.0.features.*' / 'decoder.features.*' keys)")
        self.enc = enc  # a plain attribute: the frozen encoder is not part of the state dict
        self.decoder_prefix, self.classifier_prefix = DECODER_KEYS[enc.preset]
        for key, t in enc.decoder_state.items():
            t = t.to(enc.device, torch.float32)
            self._register(key, t, buffer=key.endswith(("running_mean", "running_var")))
        self._version = 0
        self._latest = None
        self._bufs = {}

    @classmethod
    def from_encoder(cls, enc: FrozenEncoder) -> "SegmentationHead":
        return cls(enc)

    def _register(self, key: str, t: torch.Tensor, buffer: bool):
        """Register ``t`` under the dotted state-dict key, creating the container modules on the way."""
        register_under_key(self, key, t, buffer)

    def _stats(self, j: int):
        stem = f"{self.decoder_prefix}{j}.up.bn."
        return self.get_buffer(stem + "running_mean"), self.get_buffer(stem + "running_var")

    def ordered_parameters(self):
        """The 22 parameters in packed order: per level conv.weight, conv.bias, bn.weight, bn.bias; classifier weight, bias."""
        names = [f"{self.decoder_prefix}{j}.up.{t}" for j in range(LEVELS) for t in ("conv.weight", "conv.bias", "bn.weight", "bn.bias")]
        names += [self.classifier_prefix + "weight", self.classifier_prefix + "bias"]
        return [(k, self.get_parameter(k)) for k in names]

    def _train_buffers(self, n: int, img: int):
        key = (n, img)
        if key not in self._bufs:
            wsb, scb = C.c_size_t(), C.c_size_t()
            nat.check(nat.load().occ_segment_train_workspace_query(C.byref(self.enc._cfg(img)), n, C.byref(wsb), C.byref(scb)),
                      "occ_segment_train_workspace_query")
            dev = self.enc.device
            self._bufs[key] = (torch.empty(int(wsb.value), dtype=torch.uint8, device=dev),
                               torch.empty(max(int(scb.value), 16), dtype=torch.uint8, device=dev))
        return self._bufs[key]

    def forward(self, obs: torch.Tensor, return_features: bool = False):
        """prob (N,1,S,S) f32; with ``return_features`` (pooled (N,256), prob), the pooled feature being ``enc(obs)``."""
        img = self.enc._check_obs(obs, True)
        n = int(obs.shape[0])
        if n > self.enc.max_chunk:
            raise ValueError(f"a training call is one chunk: N = {n} > max_chunk = {self.enc.max_chunk}")
        if n < 1:
            raise ValueError("a training call needs at least one env")
        obs = obs.detach().to(torch.float32).contiguous()
        prob, feats = _TrainStep.apply(obs, self, *[p for _k, p in self.ordered_parameters()])
        return (feats, prob) if return_features else prob

    def _kept_relu(self, j: int) -> torch.Tensor:
        """For tests: the kept r_j = relu(u_j) of the latest forward, (N, 128 >> j, S/16 << j, S/16 << j), a view of the
        workspace (layout: include/occlusionenv_amd.h)."""
        n, img = self._latest
        ws, _scratch = self._train_buffers(n, img)
        seg = C.c_size_t()
        nat.check(nat.load().occ_segment_workspace_query(C.byref(self.enc._cfg(img)), n, C.byref(seg)), "occ_segment_workspace_query")
        off = int(seg.value)
        for i in range(LEVELS):
            c, side = (CH << (LEVELS - 1)) >> i, (img >> (LEVELS - 1)) << i
            size = n * c * side * side * 4
            if i == j:
                lo = off + _align(size)
                return ws[lo:lo + size].view(torch.float32).view(n, c, side, side)
            off += 2 * _align(size)
        raise ValueError(f"level {j} outside [0, {LEVELS})")
