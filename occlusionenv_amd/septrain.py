"""Training of the separable encoder on the device (csrc/occ_sepenc_bwd.hpp): the 16 layers of a separable ``FullNetwork``
(the ``"ppo"`` preset, PPO.py:47) or ``PredictorNet(8, separable=True)`` (pred_train.py:35) encoder as trainable parameters,
at dilation 1 or 2, with or without the residual, driven by the gradient of the pooled 256-d feature.  It is the separable
counterpart of ``enctrain.TrainableEncoder`` and used the same way.

``TrainableSeparableEncoder.from_encoder(enc)`` takes a separable ``FrozenEncoder``.  ``net(obs)`` is the pooled feature
(N,256), bitwise ``enc(obs)`` while the parameters are the checkpoint's; forward runs ``occ_sep_encoder_train_forward``,
backward ``occ_sep_encoder_backward``.  ``obs`` gets no gradient.  ``net.predict_grad(obs)`` is the grad head in torch on
``net(obs)``.  The parameters sit under the checkpoint's keys: per separable layer ``conv.0.weight`` (cin,1,3,1),
``conv.1.weight`` (cin,1,1,3), ``conv.2.weight`` (cout,cin,1,1), ``conv.2.bias``, ``bn.weight``, ``bn.bias``, per down the four
dense leaves; ``enc.with_encoder(net.state_dict())`` is the trained network for inference.

Limits: as ``enctrain``'s: BatchNorm keeps its running statistics (buffers here), a training call is one chunk
(``N <= enc.max_chunk``), and the kept activations belong to the latest forward.  The gradient reaches this encoder
through the pooled feature only; the joint step with the segmentation decoder is ``sepfullnet.TrainableSeparableFullNetwork``.
"""
from __future__ import annotations

from .encoder import FrozenEncoder
from .enctrain import PooledFeatureNet
from .nettrain import sep_encoder_part
from .netlayout import pack_sep_encoder_buffer, unpack_sep_encoder_buffer  # noqa: F401  (the packed layout, importable here)


class TrainableSeparableEncoder(PooledFeatureNet):
    """The trainable separable encoder (and grad head) of a ``FrozenEncoder``; see the module docstring.  The grad head
    and the view of the kept activations are ``enctrain``'s: the training workspace has the dense layout."""

    SYMBOLS = ("occ_sep_encoder_train_workspace_query", "occ_sep_encoder_train_forward", "occ_sep_encoder_backward")

    def __init__(self, enc: FrozenEncoder):
        if not isinstance(enc, FrozenEncoder):
            raise ValueError("TrainableSeparableEncoder needs a FrozenEncoder")
        if not enc.separable:
            raise ValueError("the native separable-encoder backward needs a separable checkpoint: this one is dense "
                             "(use enctrain.TrainableEncoder)")
        super().__init__(enc, sep_encoder_part(enc.preset))
