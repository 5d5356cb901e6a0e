"""Joint training of a dense ``FullNetwork`` / ``Segmenter`` on the device (csrc/occ_fullnet_bwd.hpp): the 16 encoder layers,
the 5 up layers of the decoder, the 1x1 classifier and, when the checkpoint has one, the grad head as trainable parameters:
what ``PreTrainer.train()`` (pretrainer.py:112-159) back-propagates through.

``TrainableFullNetwork.from_encoder(enc)`` takes a ``FrozenEncoder`` whose checkpoint held the decoder (presets "ppo" and
"segmenter").  One ``torch.autograd.Function`` returns the pooled feature (N,256) and the predicted map (N,1,S,S), both
differentiable: forward folds the current BatchNorm parameters on the device in f64, packs encoder and decoder in the
layouts of ``encoder.pack_state_dict`` / ``encoder.pack_decoder`` and runs ``occ_fullnet_train_forward`` (the encoder runs
once); backward runs ``occ_fullnet_backward`` on both upstream gradients (an absent one arrives as zeros) and maps the two
packed gradients back to the parameters.  ``obs`` gets no gradient.  While the parameters are the checkpoint's the pooled
feature is bitwise ``enc(obs)`` and the map bitwise ``enc.segment(obs)``.

``net(obs)`` is ``FullNetwork.forward``'s triple ``(pooled, segm, grad_pred)`` for "ppo", the grad head
(``Linear(256, 2)``, no tanh) in torch on the pooled feature; for "segmenter" it is ``Segmenter.forward``'s pair with the
decoder feature left out, ``(None, segm)``.  ``net.features_and_map(obs)`` is the pair ``(pooled, segm)`` for either.
``action_head`` / ``value_head`` are not part of the network: the reference feeds them detached features.

The parameters sit under the checkpoint's keys, so ``net.state_dict()`` drops back into the checkpoint it came from and
``enc.with_state(net.state_dict())`` (``with_encoder(sd).with_decoder(sd)``) is the trained network for inference.

Limits: dense 3x3 convs only (a separable checkpoint raises) at dilation 1, the pretrainer's default configuration; S a
multiple of 32.  Deviation from pretrainer.py, which trains in train mode: BatchNorm keeps its running statistics (buffers
here) in all 21 layers; only its affine parameters train.  A training call is one chunk (``N <= enc.max_chunk``), and the
kept activations belong to the latest forward: a backward of an earlier forward raises.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as nat
from .encoder import DECODER_KEYS, FEATURES, LEVELS, PRESETS, FrozenEncoder, decoder_packed_floats, layer_plan, packed_floats
from .enctrain import pack_encoder_buffer, unpack_encoder_buffer
from .seghead import bn_param_grads, fold_bn_vectors, pack_decoder_buffer, register_under_key, unpack_decoder_buffer

N_ENC, N_DEC = 64, 22  # parameters of the packed encoder (16 x 4) and of the packed decoder (5 x 4 + 2)


class _FullStep(torch.autograd.Function):
    """(obs, net, 64 encoder parameters, 22 decoder parameters) -> (pooled features, prob), both differentiable."""

    @staticmethod
    def forward(ctx, obs, net, *params):
        enc_layers, dec_levels = [], []
        for i in range(N_ENC // 4):
            w, b, gamma, beta = params[4 * i:4 * i + 4]
            scale, shift, _rstd = fold_bn_vectors(gamma, beta, *net._enc_stats(i))
            enc_layers.append((w, b, scale, shift))
        dec = params[N_ENC:]
        for j in range(LEVELS):
            w, b, gamma, beta = dec[4 * j:4 * j + 4]
            scale, shift, _rstd = fold_bn_vectors(gamma, beta, *net._dec_stats(j))
            dec_levels.append((w, b, scale, shift))
        enc_packed = pack_encoder_buffer(enc_layers).contiguous()
        dec_packed = pack_decoder_buffer(dec_levels, dec[-2], dec[-1]).contiguous()
        n, img = int(obs.shape[0]), int(obs.shape[2])
        ws, _scratch = net._train_buffers(n, img)
        feats = torch.empty(n, FEATURES, dtype=torch.float32, device=obs.device)
        prob = torch.empty(n, 1, img, img, dtype=torch.float32, device=obs.device)
        net._version += 1
        net._latest = (n, img)
        nat.check(nat.load().occ_fullnet_train_forward(C.byref(net._cfg(img)), nat.ptr(enc_packed), nat.ptr(dec_packed), nat.ptr(obs),
                                                       n, nat.ptr(ws), ws.numel(), nat.ptr(feats), nat.ptr(prob),
                                                       nat.stream_ptr(obs.device)), "occ_fullnet_train_forward")
        ctx.net, ctx.packed, ctx.version, ctx.shape = net, (enc_packed, dec_packed), net._version, (n, img)
        return feats, prob

    @staticmethod
    def backward(ctx, grad_feats, grad_prob):
        net = ctx.net
        if ctx.version != net._version:
            raise RuntimeError("TrainableFullNetwork: backward of a forward that a later forward has superseded; the kept "
                               "activations belong to the latest forward (call backward before the next net(obs))")
        n, img = ctx.shape
        ws, scratch = net._train_buffers(n, img)
        gf = grad_feats.to(torch.float32).contiguous()
        gp = grad_prob.to(torch.float32).contiguous()
        enc_packed, dec_packed = ctx.packed
        ge = torch.empty(packed_floats(False), dtype=torch.float32, device=gf.device)
        gd = torch.empty(decoder_packed_floats(), dtype=torch.float32, device=gf.device)
        nat.check(nat.load().occ_fullnet_backward(C.byref(net._cfg(img)), nat.ptr(enc_packed), nat.ptr(dec_packed), n, nat.ptr(ws),
                                                  ws.numel(), nat.ptr(gf), nat.ptr(gp), nat.ptr(scratch), scratch.numel(),
                                                  nat.ptr(ge), nat.ptr(gd), nat.stream_ptr(gf.device)), "occ_fullnet_backward")
        grads = []
        for i, (dw, db, dscale, dshift) in enumerate(unpack_encoder_buffer(ge)):
            dgamma, dbeta = bn_param_grads(dscale, dshift, *net._enc_stats(i))
            grads += [dw.contiguous(), db.clone(), dgamma.to(torch.float32), dbeta.to(torch.float32)]
        levels, dcls_w, dcls_b = unpack_decoder_buffer(gd)
        for j, (dw, db, dscale, dshift) in enumerate(levels):
            dgamma, dbeta = bn_param_grads(dscale, dshift, *net._dec_stats(j))
            grads += [dw.contiguous(), db.clone(), dgamma.to(torch.float32), dbeta.to(torch.float32)]
        return (None, None, *grads, dcls_w.clone(), dcls_b.clone())


class TrainableFullNetwork(torch.nn.Module):
    """The trainable encoder, decoder, classifier and grad head of a dense ``FrozenEncoder``; see the module docstring."""

    def __init__(self, enc: FrozenEncoder):
        super().__init__()
        if not isinstance(enc, FrozenEncoder):
            raise ValueError("TrainableFullNetwork needs a FrozenEncoder")
        if enc.preset not in DECODER_KEYS:
            raise ValueError(f"preset {enc.preset!r} has no segmentation decoder; the presets are {sorted(DECODER_KEYS)}")
        if enc.separable:
            raise ValueError("the native joint backward covers dense 3x3 convs only: this checkpoint is separable")
        if enc.dilation != 1:
            raise ValueError(f"the native joint backward covers dilation 1 only, this encoder has dilation {enc.dilation}")
        if not enc.has_decoder or enc.decoder_state is None:
            raise ValueError("this checkpoint has no segmentation decoder (no 'segmenter.0.features.*' / 'decoder.features.*' keys)")
        if enc.encoder_state is None:
            raise ValueError("this FrozenEncoder keeps no unfolded encoder tensors (build it with from_state_dict)")
        self.enc = enc  # a plain attribute: the source of the preset, the flags, the device and max_chunk
        self.prefix, self.grad_prefix = PRESETS[enc.preset][0], PRESETS[enc.preset][1]
        self.decoder_prefix, self.classifier_prefix = DECODER_KEYS[enc.preset]
        self.stems = [self.prefix + stem for stem, _ci, _co, _sep, _stride in layer_plan(False)]
        for key, t in {**enc.encoder_state, **enc.decoder_state}.items():
            register_under_key(self, key, t.to(enc.device, torch.float32), buffer=key.endswith(("running_mean", "running_var")))
        self.has_grad_head = self.grad_prefix is not None and self.grad_prefix + "weight" in enc.encoder_state
        self._version = 0
        self._latest = None
        self._bufs = {}

    @classmethod
    def from_encoder(cls, enc: FrozenEncoder) -> "TrainableFullNetwork":
        return cls(enc)

    def _cfg(self, img: int):
        return self.enc._cfg(img)

    def _enc_stats(self, i: int):
        return self.get_buffer(self.stems[i] + "bn.running_mean"), self.get_buffer(self.stems[i] + "bn.running_var")

    def _dec_stats(self, j: int):
        stem = f"{self.decoder_prefix}{j}.up.bn."
        return self.get_buffer(stem + "running_mean"), self.get_buffer(stem + "running_var")

    def ordered_parameters(self):
        """The 86 parameters in packed order: the encoder's 64 (per layer conv.weight, conv.bias, bn.weight, bn.bias), then
        the decoder's 22 (the same four per level; classifier weight, bias).  The grad head is not among them."""
        leaves = ("conv.weight", "conv.bias", "bn.weight", "bn.bias")
        names = [stem + t for stem in self.stems for t in leaves]
        names += [f"{self.decoder_prefix}{j}.up.{t}" for j in range(LEVELS) for t in leaves]
        names += [self.classifier_prefix + "weight", self.classifier_prefix + "bias"]
        return [(k, self.get_parameter(k)) for k in names]

    def _train_buffers(self, n: int, img: int):
        key = (n, img)
        if key not in self._bufs:
            wsb, scb = C.c_size_t(), C.c_size_t()
            nat.check(nat.load().occ_fullnet_train_workspace_query(C.byref(self._cfg(img)), n, C.byref(wsb), C.byref(scb)),
                      "occ_fullnet_train_workspace_query")
            dev = self.enc.device
            self._bufs[key] = (torch.empty(int(wsb.value), dtype=torch.uint8, device=dev),
                               torch.empty(max(int(scb.value), 16), dtype=torch.uint8, device=dev))
        return self._bufs[key]

    def features_and_map(self, obs: torch.Tensor):
        """(pooled (N,256), segm (N,1,S,S)) f32 of the network with its current parameters, both differentiable."""
        self.enc._check_obs(obs, True)
        n = int(obs.shape[0])
        if n > self.enc.max_chunk:
            raise ValueError(f"a training call is one chunk: N = {n} > max_chunk = {self.enc.max_chunk}")
        if n < 1:
            raise ValueError("a training call needs at least one env")
        obs = obs.detach().to(torch.float32).contiguous()
        return _FullStep.apply(obs, self, *[p for _k, p in self.ordered_parameters()])

    def forward(self, obs: torch.Tensor):
        """"ppo": ``FullNetwork.forward`` (model.py:156-166) -> (pooled, segm, grad_pred (N,2)); "segmenter":
        ``Segmenter.forward`` (model.py:135-140) without the decoder feature -> (None, segm)."""
        feats, prob = self.features_and_map(obs)
        if self.enc.preset == "segmenter":
            return None, prob
        if not self.has_grad_head:
            raise ValueError("this checkpoint has no gradPredictor head; use features_and_map(obs)")
        grad_pred = torch.nn.functional.linear(feats, self.get_parameter(self.grad_prefix + "weight"),
                                               self.get_parameter(self.grad_prefix + "bias"))
        return feats, prob, grad_pred
