"""Training of the dense encoder on the device (csrc/occ_encoder_bwd.hpp): the 16 conv layers of a ``PredictorNet`` or of a
dense ``FullNetwork`` / ``Segmenter`` encoder as trainable parameters, driven by the gradient of the pooled 256-d feature.

``TrainableEncoder.from_encoder(enc)`` takes a ``FrozenEncoder``.  ``net(obs)`` is the pooled feature (N,256), bitwise
``enc(obs)`` while the parameters are the checkpoint's, and one ``torch.autograd.Function``: forward folds the current
BatchNorm parameters on the device in f64, packs them in the layout of ``netlayout.pack_state_dict`` and runs
``occ_encoder_train_forward``; backward runs ``occ_encoder_backward`` and maps the packed gradient back to the parameters.
``obs`` gets no gradient.  ``net.predict_grad(obs)`` is the grad head (``Linear(256, 2)``, with tanh for ``PredictorNet``) in
torch on ``net(obs)``, so ``F.mse_loss(net.predict_grad(obs), target).backward()`` is one step of train_predict.py.  Any torch
optimizer works on ``net.parameters()``.

The parameters sit under the checkpoint's keys, so ``net.state_dict()`` drops back into the checkpoint it came from and
``enc.with_encoder(net.state_dict())`` is the trained network for inference.

Limits: dense 3x3 convs only (a separable checkpoint raises) at dilation 1; the separable encoder, at dilation 1 or 2,
trains through ``septrain.TrainableSeparableEncoder``.  Deviation from train_predict.py, which trains
in train mode: BatchNorm keeps its running statistics (buffers here); only its affine parameters train.  A training call is
one chunk (``N <= enc.max_chunk``), and the kept activations belong to the latest forward: a backward of an earlier forward
raises.  The gradient reaches the encoder through the pooled feature only; where the segmentation loss trains the encoder
too (the pretrainer's step), the decoder's skip and input gradients join the encoder's in ``fullnet.TrainableFullNetwork``.

The host path (parameters under the checkpoint's keys, workspace, the autograd function) is ``nettrain.TrainableNet``'s,
shared with ``seghead`` and ``fullnet``, the fold and the packed layout are ``netlayout``'s; here are the guards, the native
symbols, the grad head and the view of the kept activations.
"""
from __future__ import annotations

import torch

from .encoder import PRESETS, FrozenEncoder
from .nettrain import TrainableNet, align256, encoder_part
from .netlayout import pack_encoder_buffer, unpack_encoder_buffer  # noqa: F401  (the encoder's packed layout, importable here)


class PooledFeatureNet(TrainableNet):
    """What the encoder-only nets share (``TrainableEncoder`` here, ``septrain.TrainableSeparableEncoder``): one encoder
    part whose step returns the pooled feature, the grad head in torch, and the view of the kept activations (both native
    paths keep them in the same workspace layout)."""

    RETURNS = DIFFERENTIABLE = ("feats",)
    RUNS_DECODER = False

    def __init__(self, enc: FrozenEncoder, part):
        if enc.encoder_state is None:
            raise ValueError("this FrozenEncoder keeps no unfolded encoder tensors (build it with from_state_dict)")
        super().__init__(enc, [part], enc.encoder_state)
        self.stems = self.parts[0].stems
        self.grad_prefix = PRESETS[enc.preset][1]
        self.has_grad_head = self.grad_prefix is not None and self.grad_prefix + "weight" in enc.encoder_state
        self.grad_tanh = enc.grad_tanh

    def forward(self, obs: torch.Tensor) -> torch.Tensor:
        """The pooled feature (N,256) f32 of the encoder with its current parameters."""
        return self._step(obs)

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

        off = align256(4 * n * 4 * img * img)  # obs
        if i == 0:
            return view(off, 8, img)
        off += align256(4 * n * 8 * img * img)
        side = img
        for lv in range(5):
            c, half = 8 << lv, (side + 1) // 2
            act = align256(4 * n * c * side * side)
            r = {1: (off + act, c, side), 2: (off + 3 * act, c, side), 3: (off + 5 * act, 2 * c, half)}
            if (i - 1) // 3 == lv:
                return view(*r[(i - 1) % 3 + 1])
            off += 5 * act + align256(4 * n * 2 * c * half * half)
            side = half
        raise ValueError(f"layer {i} outside [0, 16)")


class TrainableEncoder(PooledFeatureNet):
    """The trainable dense encoder (and grad head) of a ``FrozenEncoder``; see the module docstring."""

    SYMBOLS = ("occ_encoder_train_workspace_query", "occ_encoder_train_forward", "occ_encoder_backward")

    def __init__(self, enc: FrozenEncoder):
        if not isinstance(enc, FrozenEncoder):
            raise ValueError("TrainableEncoder needs a FrozenEncoder")
        if enc.separable:
            raise ValueError("the native encoder backward covers dense 3x3 convs only: this checkpoint is separable")
        if enc.dilation != 1:
            raise ValueError(f"the native encoder backward covers dilation 1 only, this encoder has dilation {enc.dilation}")
        super().__init__(enc, encoder_part(enc.preset))
