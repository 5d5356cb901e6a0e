"""Joint training of a separable ``FullNetwork`` / ``Segmenter`` on the device (csrc/occ_sepfull_bwd.hpp): the network the
agent runs, ``FullNetwork(8, dilation=2, separable=True)`` (PPO.py:47), as ``pretrainer.py --separable --dilation 2`` trains
it: the 16 encoder layers (eleven separable, five dense downs), the 5 up layers of the decoder, the 1x1 classifier and, when
the checkpoint has one, the grad head, from the segmentation loss and the gradient loss at once.  It is the separable
counterpart of ``fullnet.TrainableFullNetwork`` and used the same way; ``harness.pretrain_epoch`` picks between the two by
the encoder's form.

``TrainableSeparableFullNetwork.from_encoder(enc)`` takes a separable ``FrozenEncoder`` (dilation 1 or 2, with or without
the residual) whose checkpoint held the decoder (presets "ppo" and "segmenter").  ``net(obs)``, ``net.features_and_map(obs)``
and the heads are ``fullnet.JointNet``'s: forward runs ``occ_sep_fullnet_train_forward`` (the encoder runs once), backward
``occ_sep_fullnet_backward`` on both upstream gradients (an absent one arrives as zeros).  ``obs`` gets no gradient.  While
the parameters are the checkpoint's the pooled feature is bitwise ``enc(obs)`` and the map bitwise ``enc.segment(obs)``.

The parameters sit under the checkpoint's keys (``septrain``'s six leaves per separable layer, four per down, then the
decoder's and the classifier's), so ``enc.with_state(net.state_dict())`` is the trained network for inference and
``BatchedPPO.from_fullnetwork(net.state_dict())`` the agent on it: the checkpoint's ``action_head`` / ``value_head``, which
pretraining does not touch (the reference feeds them detached features), ride along as buffers when the checkpoint had them.

BatchNorm: by default it keeps its running statistics (buffers here) in all 21 layers and only its affine parameters
train, a deviation from pretrainer.py.  ``from_encoder(enc, batch_stats=True)`` is the reference's train mode, as in
``fullnet``: batch statistics while ``net.training``, running buffers updated as ``nn.BatchNorm2d`` updates them,
``N (S / 32)^2 >= 2``, and the running-statistics step bit for bit after ``net.eval()``.  This is how a fresh
``FullNetwork(8, dilation=2, separable=True)`` is pretrained: its statistics are learned, not kept at mean 0, variance 1.

Limits: S a multiple of 32.  A training call is one chunk (``N <= enc.max_chunk``), and the kept activations belong to the
latest forward: a backward of an earlier forward raises.
"""
from __future__ import annotations

import torch

from .encoder import DECODER_KEYS, FrozenEncoder
from .fullnet import JointNet
from .nettrain import register_under_key, sep_encoder_part


class TrainableSeparableFullNetwork(JointNet):
    """The trainable encoder, decoder, classifier and grad head of a separable ``FrozenEncoder``; see the module
    docstring."""

    SYMBOLS = ("occ_sep_fullnet_train_workspace_query", "occ_sep_fullnet_train_forward", "occ_sep_fullnet_backward")

    def __init__(self, enc: FrozenEncoder, batch_stats: bool = False):
        if not isinstance(enc, FrozenEncoder):
            raise ValueError("TrainableSeparableFullNetwork needs a FrozenEncoder")
        if enc.preset not in DECODER_KEYS:
            raise ValueError(f"preset {enc.preset!r} has no segmentation decoder; the presets are {sorted(DECODER_KEYS)}")
        if not enc.separable:
            raise ValueError("the native separable joint backward needs a separable checkpoint: this one is dense "
                             "(use fullnet.TrainableFullNetwork)")
        if not enc.has_decoder or enc.decoder_state is None:
            raise ValueError("this checkpoint has no segmentation decoder (no 'segmenter.0.features.*' / 'decoder.features.*' keys)")
        if enc.encoder_state is None:
            raise ValueError("this FrozenEncoder keeps no unfolded encoder tensors (build it with from_state_dict)")
        super().__init__(enc, sep_encoder_part(enc.preset), batch_stats)
        for name, (w, b) in enc.heads.items():  # not trained here: carried so that state_dict() is the agent's checkpoint
            register_under_key(self, name + ".weight", w.to(enc.device, torch.float32), buffer=True)
            register_under_key(self, name + ".bias", b.to(enc.device, torch.float32), buffer=True)
