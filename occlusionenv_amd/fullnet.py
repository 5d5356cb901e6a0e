"""Joint training of a dense ``FullNetwork`` / ``Segmenter`` on the device (csrc/occ_fullnet_bwd.hpp): the 16 encoder layers,
the 5 up layers of the decoder, the 1x1 classifier and, when the checkpoint has one, the grad head as trainable parameters:
what ``PreTrainer.train()`` (pretrainer.py:112-159) back-propagates through.

``TrainableFullNetwork.from_encoder(enc)`` takes a ``FrozenEncoder`` whose checkpoint held the decoder (presets "ppo" and
"segmenter").  One ``torch.autograd.Function`` returns the pooled feature (N,256) and the predicted map (N,1,S,S), both
differentiable: forward folds the current BatchNorm parameters on the device in f64, packs encoder and decoder in the
layouts of ``netlayout.pack_state_dict`` / ``netlayout.pack_decoder`` and runs ``occ_fullnet_train_forward`` (the encoder runs
once); backward runs ``occ_fullnet_backward`` on both upstream gradients (an absent one arrives as zeros) and maps the two
packed gradients back to the parameters.  ``obs`` gets no gradient.  While the parameters are the checkpoint's the pooled
feature is bitwise ``enc(obs)`` and the map bitwise ``enc.segment(obs)``.

``net(obs)`` is ``FullNetwork.forward``'s triple ``(pooled, segm, grad_pred)`` for "ppo", the grad head
(``Linear(256, 2)``, no tanh) in torch on the pooled feature; for "segmenter" it is ``Segmenter.forward``'s pair with the
decoder feature left out, ``(None, segm)``.  ``net.features_and_map(obs)`` is the pair ``(pooled, segm)`` for either.
``action_head`` / ``value_head`` are not part of the network: the reference feeds them detached features.

The parameters sit under the checkpoint's keys, so ``net.state_dict()`` drops back into the checkpoint it came from and
``enc.with_state(net.state_dict())`` (``with_encoder(sd).with_decoder(sd)``) is the trained network for inference.

BatchNorm: by default it keeps its running statistics (buffers here) in all 21 layers and only its affine parameters
train, a deviation from pretrainer.py, which trains in train mode.  ``from_encoder(enc, batch_stats=True)`` is the
reference's train mode (csrc/occ_bn_train.hpp, ``occ_fullnet_bn_*``): while ``net.training`` every layer normalises with
the mean and the biased variance of the batch, the gradients go through those statistics, and the running buffers move as
``nn.BatchNorm2d`` moves them (momentum 0.1, unbiased variance; ``num_batches_tracked`` is not kept), so
``enc.with_state(net.state_dict())`` runs inference on learned statistics.  The envs of a batch are then coupled, feats and
prob are no longer those of ``enc`` and every layer needs two values per channel: ``N (S / 32)^2 >= 2``, else ``ValueError``
as in PyTorch.  After ``net.eval()`` the step is the running-statistics one, bit for bit.  Against an f64 model of the
network in train mode, evaluated with the step's own ReLU gates, the gradients were within 3.3e-5 of each tensor's largest
element on an MI355X (the tests' bar: max(1e-4, 4 e32) <= 4e-4, e32 being the error of PyTorch's own f32 run of the case;
tests/test_gpu_bn_train.py).

Limits: dense 3x3 convs only (a separable checkpoint raises) at dilation 1, the pretrainer's default configuration; S a
multiple of 32.  A training call is one chunk (``N <= enc.max_chunk``), and the kept activations belong to the latest
forward: a backward of an earlier forward raises.

``netoptim.PackedAdamW(net)`` moves the trainable values into packed masters and takes the optimizer step in one native
launch; ``net.sync_parameters()`` (and ``net.state_dict()``, which calls it) writes them back under the checkpoint's keys.

The host path (parameters under the checkpoint's keys, workspace, the autograd function) is ``nettrain.TrainableNet``'s on
two ``netlayout.Part``s, the encoder's and the decoder's, which hold the packed layouts; here are the guards, the native
symbols and the heads.  The heads and ``forward`` are ``JointNet``'s, which ``sepfullnet.TrainableSeparableFullNetwork`` (the separable
encoder's joint step) shares.
"""
from __future__ import annotations

import torch

from .encoder import DECODER_KEYS, PRESETS, FrozenEncoder
from .nettrain import TrainableNet, decoder_part, encoder_part


class JointNet(TrainableNet):
    """A ``TrainableNet`` over an encoder part and the decoder part whose step returns the pooled feature and the map,
    both differentiable, with the grad head of the checkpoint in torch on top: what the dense and the separable joint
    networks share.  A subclass checks its checkpoint and names its encoder part and its native symbols."""

    RETURNS = DIFFERENTIABLE = ("feats", "prob")
    BN_SYMBOLS = ("occ_fullnet_bn_train_workspace_query", "occ_fullnet_bn_train_forward", "occ_fullnet_bn_backward")

    def __init__(self, enc: FrozenEncoder, enc_part, batch_stats: bool = False):
        super().__init__(enc, [enc_part, decoder_part(enc.preset)], {**enc.encoder_state, **enc.decoder_state})
        self.batch_stats = bool(batch_stats)
        self.grad_prefix = PRESETS[enc.preset][1]
        self.has_grad_head = self.grad_prefix is not None and self.grad_prefix + "weight" in enc.encoder_state

    @classmethod
    def from_encoder(cls, enc: FrozenEncoder, batch_stats: bool = False):
        """``batch_stats``: BatchNorm in train mode while ``net.training`` (the module docstring of ``fullnet``)."""
        return cls(enc, batch_stats=batch_stats)

    def features_and_map(self, obs: torch.Tensor):
        """(pooled (N,256), segm (N,1,S,S)) f32 of the network with its current parameters, both differentiable."""
        return self._step(obs)

    def forward(self, obs: torch.Tensor):
        """"ppo": ``FullNetwork.forward`` (model.py:156-166) -> (pooled, segm, grad_pred (N,2)); "segmenter":
        ``Segmenter.forward`` (model.py:135-140) without the decoder feature -> (None, segm)."""
        feats, prob = self.features_and_map(obs)
        if self.enc.preset == "segmenter":
            return None, prob
        if not self.has_grad_head:
            raise ValueError("this checkpoint has no gradPredictor head; use features_and_map(obs)")
        if self._resident is not None:
            weight, bias = self._resident.head_views()
        else:
            weight, bias = self.get_parameter(self.grad_prefix + "weight"), self.get_parameter(self.grad_prefix + "bias")
        return feats, prob, torch.nn.functional.linear(feats, weight, bias)

    # ---- under netoptim.PackedAdamW the trained values live in packed masters (net._resident) --------------------------------
    def sync_parameters(self) -> None:
        """Write the packed masters of ``netoptim.PackedAdamW`` back to the parameters under the checkpoint's keys; nothing
        to do for a net without one."""
        if self._resident is not None:
            self._resident.sync()

    def state_dict(self, *args, **kwargs):
        self.sync_parameters()
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        result = super().load_state_dict(*args, **kwargs)
        if self._resident is not None:
            self._resident.repack()
        return result


class TrainableFullNetwork(JointNet):
    """The trainable encoder, decoder, classifier and grad head of a dense ``FrozenEncoder``; see the module docstring."""

    SYMBOLS = ("occ_fullnet_train_workspace_query", "occ_fullnet_train_forward", "occ_fullnet_backward")

    def __init__(self, enc: FrozenEncoder, batch_stats: bool = False):
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
        super().__init__(enc, encoder_part(enc.preset), batch_stats)
