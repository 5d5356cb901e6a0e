"""Fine-tuning of the segmentation head on the device (csrc/occ_decoder_bwd.hpp): the decoder and the 1x1 classifier of a
``FullNetwork`` / ``Segmenter`` as trainable parameters on top of the frozen native encoder.

``SegmentationHead.from_encoder(enc)`` takes a ``FrozenEncoder`` whose checkpoint held the decoder.  ``head(obs)`` is the
predicted occlusion map (N,1,S,S), bitwise ``enc.segment(obs)`` while the parameters are the checkpoint's, and one
``torch.autograd.Function``: forward folds the current parameters into the packed layout on the device and runs
``occ_segment_train_forward``; backward runs ``occ_segment_backward`` and maps the packed gradient back to the parameters.
``obs`` gets no gradient and the encoder stays frozen.  Any torch optimizer works on ``head.parameters()``.

The parameters sit under the reference's state-dict keys (``netlayout.DECODER_KEYS``), so ``head.state_dict()`` drops back into
the checkpoint it came from and ``enc.with_decoder(head.state_dict())`` is the fine-tuned network for inference.

Deviation from pretrainer.py, which trains in train mode: the decoder's BatchNorm keeps its running statistics (buffers
here); only its affine parameters train.  A training call is one chunk (``N <= enc.max_chunk``), and the kept activations
belong to the latest forward: a backward of an earlier forward raises.

The host path (parameters under the checkpoint's keys, workspace, the autograd function) is ``nettrain.TrainableNet``'s,
shared with ``enctrain`` and ``fullnet``, the fold and the packed layout are ``netlayout``'s; here are the guards, the native
symbols, the outputs and the view of the kept activations.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as nat
from .encoder import CH, LEVELS, FrozenEncoder
from .nettrain import TrainableNet, align256, decoder_part
# importable here as before: the decoder's packed layout and the folds (netlayout), and what moved to nettrain
from .netlayout import bn_param_grads, fold_bn_vectors, pack_decoder_buffer, unpack_decoder_buffer  # noqa: F401
from .nettrain import register_under_key  # noqa: F401


class SegmentationHead(TrainableNet):
    """The trainable decoder and classifier over a frozen ``FrozenEncoder``; see the module docstring."""

    SYMBOLS = ("occ_segment_train_workspace_query", "occ_segment_train_forward", "occ_segment_backward")
    RETURNS, DIFFERENTIABLE = ("prob", "feats"), ("prob",)  # the pooled feature is the frozen encoder's

    def __init__(self, enc: FrozenEncoder):
        if not isinstance(enc, FrozenEncoder):
            raise ValueError("SegmentationHead needs a FrozenEncoder")
        if not enc.has_decoder or enc.decoder_state is None:
            raise ValueError("this checkpoint has no segmentation decoder (no 'segmenter.0.features.*' / 'decoder.features.*' keys)")
        super().__init__(enc, [decoder_part(enc.preset)], enc.decoder_state)

    def _native_forward(self, img, packed, obs, n, ws, outs):
        super()._native_forward(img, [self.enc.packed, *packed], obs, n, ws, outs)  # the frozen encoder's weights first

    def forward(self, obs: torch.Tensor, return_features: bool = False):
        """prob (N,1,S,S) f32; with ``return_features`` (pooled (N,256), prob), the pooled feature being ``enc(obs)``."""
        prob, feats = self._step(obs)
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
                lo = off + align256(size)
                return ws[lo:lo + size].view(torch.float32).view(n, c, side, side)
            off += 2 * align256(size)
        raise ValueError(f"level {j} outside [0, {LEVELS})")
