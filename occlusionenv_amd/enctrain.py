"""Training of the dense encoder on the device (csrc/occ_encoder_bwd.hpp): the 16 conv layers of a ``PredictorNet`` or of a
dense ``FullNetwork`` / ``Segmenter`` encoder as trainable parameters, driven by the gradient of the pooled 256-d feature.

``TrainableEncoder.from_encoder(enc)`` takes a ``FrozenEncoder``.  ``net(obs)`` is the pooled feature (N,256), bitwise
``enc(obs)`` while the parameters are the checkpoint's, and one ``torch.autograd.Function``: forward folds the current
BatchNorm parameters on the device in f64, packs them in the layout of ``encoder.pack_state_dict`` and runs
``occ_encoder_train_forward``; backward runs ``occ_encoder_backward`` and maps the packed gradient back to the parameters.
``obs`` gets no gradient.  ``net.predict_grad(obs)`` is the grad head (``Linear(256, 2)``, with tanh for ``PredictorNet``) in
torch on ``net(obs)``, so ``F.mse_loss(net.predict_grad(obs), target).backward()`` is one step of train_predict.py.  Any torch
optimizer works on ``net.parameters()``.

The parameters sit under the checkpoint's keys, so ``net.state_dict()`` drops back into the checkpoint it came from and
``enc.with_encoder(net.state_dict())`` is the trained network for inference.

Limits: dense 3x3 convs only (a separable checkpoint raises) at dilation 1.  Deviation from train_predict.py, which trains
in train mode: BatchNorm keeps its running statistics (buffers here); only its affine parameters train.  A training call is
one chunk (``N <= enc.max_chunk``), and the kept activations belong to the latest forward: a backward of an earlier forward
raises.  The gradient reaches the encoder through the pooled feature only; where the segmentation loss trains the encoder
too (the pretrainer's step), the decoder's skip and input gradients join the encoder's in ``fullnet.TrainableFullNetwork``.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as nat
from .encoder import FEATURES, PRESETS, FrozenEncoder, layer_plan, packed_floats
from .seghead import bn_param_grads, fold_bn_vectors, register_under_key


def pack_encoder_buffer(layers) -> torch.Tensor:
    """layers: sixteen (w (cout,cin,3,3), bias, scale, shift) -> the packed f32 buffer of the dense encoder:
    w[ci][ky * 3 + kx][co] | bias | scale | shift per layer (``encoder.pack_state_dict``)."""
    parts = []
    for w, b, s, t in layers:
        parts += [w.permute(1, 2, 3, 0).reshape(-1), b.reshape(-1), s.reshape(-1), t.reshape(-1)]
    buf = torch.cat([p.to(torch.float32) for p in parts])
    assert buf.numel() == packed_floats(False)
    return buf


def unpack_encoder_buffer(buf: torch.Tensor):
    """The inverse of ``pack_encoder_buffer`` -> [(w (cout,cin,3,3), bias, scale, shift)] x 16, views of ``buf``."""
    if buf.numel() != packed_floats(False):
        raise ValueError(f"packed dense encoder buffer has {buf.numel()} floats, expected {packed_floats(False)}")
    layers, off = [], 0
    for _stem, cin, cout, _sep, _stride in layer_plan(False):
        w = buf[off:off + 9 * cin * cout].reshape(cin, 3, 3, cout).permute(3, 0, 1, 2)
        off += 9 * cin * cout
        layers.append((w, buf[off:off + cout], buf[off + cout:off + 2 * cout], buf[off + 2 * cout:off + 3 * cout]))
        off += 3 * cout
    return layers


def _align(b: int) -> int:
    return (b + 255) & ~255


class _EncStep(torch.autograd.Function):
    """(obs, net, 64 parameters) -> pooled features; the gradient goes to the parameters only."""

    @staticmethod
    def forward(ctx, obs, net, *params):
        layers = []
        for i in range(len(net.stems)):
            w, b, gamma, beta = params[4 * i:4 * i + 4]
            scale, shift, _rstd = fold_bn_vectors(gamma, beta, *net._stats(i))
            layers.append((w, b, scale, shift))
        packed = pack_encoder_buffer(layers).contiguous()
        n, img = int(obs.shape[0]), int(obs.shape[2])
        ws, _scratch = net._train_buffers(n, img)
        feats = torch.empty(n, FEATURES, dtype=torch.float32, device=obs.device)
        net._version += 1
        net._latest = (n, img)
        nat.check(nat.load().occ_encoder_train_forward(C.byref(net._cfg(img)), nat.ptr(packed), nat.ptr(obs), n, nat.ptr(ws),
                                                       ws.numel(), nat.ptr(feats), nat.stream_ptr(obs.device)),
                  "occ_encoder_train_forward")
        ctx.net, ctx.packed, ctx.version, ctx.shape = net, packed, net._version, (n, img)
        return feats

    @staticmethod
    def backward(ctx, grad_feats):
        net = ctx.net
        if ctx.version != net._version:
            raise RuntimeError("TrainableEncoder: backward of a forward that a later forward has superseded; the kept "
                               "activations belong to the latest forward (call backward before the next net(obs))")
        n, img = ctx.shape
        ws, scratch = net._train_buffers(n, img)
        g = grad_feats.to(torch.float32).contiguous()
        gp = torch.empty(packed_floats(False), dtype=torch.float32, device=g.device)
        nat.check(nat.load().occ_encoder_backward(C.byref(net._cfg(img)), nat.ptr(ctx.packed), n, nat.ptr(ws), ws.numel(), nat.ptr(g),
                                                  nat.ptr(scratch), scratch.numel(), nat.ptr(gp), nat.stream_ptr(g.device)),
                  "occ_encoder_backward")
        grads = []
        for i, (dw, db, dscale, dshift) in enumerate(unpack_encoder_buffer(gp)):
            dgamma, dbeta = bn_param_grads(dscale, dshift, *net._stats(i))
            grads += [dw.contiguous(), db.clone(), dgamma.to(torch.float32), dbeta.to(torch.float32)]
        return (None, None, *grads)


class TrainableEncoder(torch.nn.Module):
    """The trainable dense encoder (and grad head) of a ``FrozenEncoder``; see the module docstring."""

    def __init__(self, enc: FrozenEncoder):
        super().__init__()
        if not isinstance(enc, FrozenEncoder):
            raise ValueError("TrainableEncoder needs a FrozenEncoder")
        if enc.separable:
            raise ValueError("the native encoder backward covers dense 3x3 convs only: this checkpoint is separable")
        if enc.dilation != 1:
            raise ValueError(f"the native encoder backward covers dilation 1 only, this encoder has dilation {enc.dilation}")
        if enc.encoder_state is None:
            raise ValueError("this FrozenEncoder keeps no unfolded encoder tensors (build it with from_state_dict)")
        self.enc = enc  # a plain attribute: the source of the preset, the flags, the device and max_chunk
        self.prefix, self.grad_prefix = PRESETS[enc.preset][0], PRESETS[enc.preset][1]
        self.stems = [self.prefix + stem for stem, _ci, _co, _sep, _stride in layer_plan(False)]
        for key, t in enc.encoder_state.items():
            t = t.to(enc.device, torch.float32)
            self._register(key, t, buffer=key.endswith(("running_mean", "running_var")))
        self.has_grad_head = self.grad_prefix is not None and self.grad_prefix + "weight" in enc.encoder_state
        self.grad_tanh = enc.grad_tanh
        self._version = 0
        self._latest = None
        self._bufs = {}

    @classmethod
    def from_encoder(cls, enc: FrozenEncoder) -> "TrainableEncoder":
        return cls(enc)

    def _register(self, key: str, t: torch.Tensor, buffer: bool):
        """Register ``t`` under the dotted state-dict key, creating the container modules on the way."""
        register_under_key(self, key, t, buffer)

    def _cfg(self, img: int):
        return self.enc._cfg(img)

    def _stats(self, i: int):
        return self.get_buffer(self.stems[i] + "bn.running_mean"), self.get_buffer(self.stems[i] + "bn.running_var")

    def ordered_parameters(self):
        """The 64 encoder parameters in packed order: per layer conv.weight, conv.bias, bn.weight, bn.bias."""
        names = [stem + t for stem in self.stems for t in ("conv.weight", "conv.bias", "bn.weight", "bn.bias")]
        return [(k, self.get_parameter(k)) for k in names]

    def _train_buffers(self, n: int, img: int):
        key = (n, img)
        if key not in self._bufs:
            wsb, scb = C.c_size_t(), C.c_size_t()
            nat.check(nat.load().occ_encoder_train_workspace_query(C.byref(self._cfg(img)), n, C.byref(wsb), C.byref(scb)),
                      "occ_encoder_train_workspace_query")
            dev = self.enc.device
            self._bufs[key] = (torch.empty(int(wsb.value), dtype=torch.uint8, device=dev),
                               torch.empty(max(int(scb.value), 16), dtype=torch.uint8, device=dev))
        return self._bufs[key]

    def forward(self, obs: torch.Tensor) -> torch.Tensor:
        """The pooled feature (N,256) f32 of the encoder with its current parameters."""
        self.enc._check_obs(obs, False)
        n = int(obs.shape[0])
        if n > self.enc.max_chunk:
            raise ValueError(f"a training call is one chunk: N = {n} > max_chunk = {self.enc.max_chunk}")
        if n < 1:
            raise ValueError("a training call needs at least one env")
        obs = obs.detach().to(torch.float32).contiguous()
        return _EncStep.apply(obs, self, *[p for _k, p in self.ordered_parameters()])

    def predict_grad(self, obs: torch.Tensor) -> torch.Tensor:
        """(N,2): the grad head on ``self(obs)`` in torch: ``FullNetwork.gradPredictor`` (no tanh, model.py:164) or
        ``tanh(PredictorNet.output(.))`` (model.py:81-85)."""
        if not self.has_grad_head:
            raise ValueError("this checkpoint has no gradPredictor / output head")
        g = torch.nn.functional.linear(self(obs), self.get_parameter(self.grad_prefix + "weight"),
                                       self.get_parameter(self.grad_prefix + "bias"))
        return torch.tanh(g) if self.grad_tanh else g

    def _kept_relu(self, i: int) -> torch.Tensor:
        """For tests: the kept r = relu(u) of layer i (packed order) of the latest forward, a view of the workspace (layout:
        include/occlusionenv_amd.h)."""
        n, img = self._latest
        ws, _scratch = self._train_buffers(n, img)

        def view(off, c, side):
            return ws[off:off + 4 * n * c * side * side].view(torch.float32).view(n, c, side, side)

        off = _align(4 * n * 4 * img * img)  # obs
        if i == 0:
            return view(off, 8, img)
        off += _align(4 * n * 8 * img * img)
        side = img
        for lv in range(5):
            c, half = 8 << lv, (side + 1) // 2
            act = _align(4 * n * c * side * side)
            r = {1: (off + act, c, side), 2: (off + 3 * act, c, side), 3: (off + 5 * act, 2 * c, half)}
            if (i - 1) // 3 == lv:
                return view(*r[(i - 1) % 3 + 1])
            off += 5 * act + _align(4 * n * 2 * c * half * half)
            side = half
        raise ValueError(f"layer {i} outside [0, 16)")
