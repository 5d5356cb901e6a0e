"""The packed weight layout of the native network, restated once in Python (the normative text is include/occlusionenv_amd.h).

One packed f32 buffer holds the 16 layers of the encoder and one the 5 up levels of the decoder with its 1x1 classifier:

  dense layer      w[ci][ky * 3 + kx][co] | bias | scale | shift                      9 cin cout + 3 cout floats
  separable layer  wv[ci][3] | wh[ci][3] | pw[ci][co] | bias | scale | shift          6 cin + cin cout + 3 cout floats

Here are the presets, plans and sizes, a layer's leaves in a checkpoint, a ``Part`` (where a net's tensors sit in a state dict
and how they are packed), the one pack / unpack pair, both BatchNorm folds and a checkpoint's checks.  ``FrozenEncoder`` loads
through ``pack_state_dict`` / ``pack_decoder`` (CPU, f64, one cast to f32); ``nettrain`` packs through the same ``Part.pack``.
"""
from __future__ import annotations

import re
from typing import Callable, NamedTuple, Optional, Tuple

import torch

CH, LEVELS, FEATURES = 8, 5, 256
BN_EPS = 1e-5
PRESETS = {
    # name: (key prefix, grad head, tanh on the grad head, dilation, residual)
    "ppo": ("encoder.", "gradPredictor.", False, 2, True),
    "predictor": ("features.", "output.", True, 1, False),
    "segmenter": ("encoder.", None, False, 1, True),
}
# name: (key prefix of Decoder.features, key prefix of the 1x1 classifier); "predictor" has no decoder
DECODER_KEYS = {
    "ppo": ("segmenter.0.features.", "segmenter.1."),
    "segmenter": ("decoder.features.", "classifier."),
}

LEAVES = ("conv.weight", "conv.bias", "bn.weight", "bn.bias")  # the four parameters of a dense layer, in packed order
# those of a separable layer: depthwise (3,1), depthwise (1,3), pointwise, its bias, then the BatchNorm affine
SEP_LEAVES = ("conv.0.weight", "conv.1.weight", "conv.2.weight", "conv.2.bias", "bn.weight", "bn.bias")
STATS = ("bn.running_mean", "bn.running_var")  # a layer's buffers, after its leaves
ENCODER_PERM, DECODER_PERM = (1, 2, 3, 0), (0, 2, 3, 1)  # conv (cout,cin,3,3) / transposed conv (cin,cout,3,3) -> (cin,3,3,cout)
CLASSIFIER_SHAPES = ((1, CH, 1, 1), (1,))  # the decoder's tail: weight, bias


def _numel(shape) -> int:
    n = 1
    for d in shape:
        n *= d
    return n


def _views(buf, off: int, shapes):
    """Consecutive views of ``buf`` from ``off`` on, in ``shapes`` -> (the views, the offset after them)."""
    views = []
    for shape in shapes:
        end = off + _numel(shape)
        views.append(buf[off:end].reshape(shape) if len(shape) > 1 else buf[off:end])
        off = end
    return views, off


# ---- plans and sizes ---------------------------------------------------------------------------------------------------------
def layer_plan(separable: bool):
    """[(state-dict stem relative to the encoder prefix, cin, cout, separable, stride)] in packed order."""
    plan = [("initial.", 4, CH, separable, 1)]
    for lv in range(LEVELS):
        c = CH << lv
        plan += [(f"features.{lv}.net.Layer 1.", c, c, separable, 1), (f"features.{lv}.net.Layer 2.", c, c, separable, 1),
                 (f"features.{lv}.down.", c, 2 * c, False, 2)]
    return plan


def decoder_plan():
    """[(index j in Decoder.features, cin = 2c, cout = c)] in packed (= decoder) order: c = 128, 64, 32, 16, 8."""
    return [(j, 2 * (CH << (LEVELS - 1 - j)), CH << (LEVELS - 1 - j)) for j in range(LEVELS)]


def _packed_shapes(cin: int, cout: int, separable: bool = False):
    """The pieces of one packed layer as they lie in the buffer (the depthwise taps with a checkpoint's unit dimensions)."""
    return ([(cin, 1, 3, 1), (cin, 1, 1, 3), (cin, cout)] if separable else [(cin, 3, 3, cout)]) + [(cout,)] * 3


def _leaf_shapes(cin: int, cout: int, separable: bool, perm):
    """The shapes a checkpoint holds a layer's leaves and statistics in, in the order ``SEP_LEAVES`` / ``LEAVES`` + ``STATS``."""
    conv = [(cin, 1, 3, 1), (cin, 1, 1, 3), (cout, cin, 1, 1)] if separable else [tuple((cin, 3, 3, cout)[perm.index(d)] for d in range(4))]
    return conv + [(cout,)] * 5


def layer_floats(cin: int, cout: int, separable: bool = False) -> int:
    return sum(_numel(s) for s in _packed_shapes(cin, cout, separable))


def layer_offsets(separable: bool):
    """The offset of every encoder layer in the packed buffer, in floats."""
    offsets, off = [], 0
    for _stem, cin, cout, sep, _stride in layer_plan(separable):
        offsets.append(off)
        off += layer_floats(cin, cout, sep)
    return offsets


def bn_layer_shapes(img: int):
    """[(channels, pixels of one env's plane)] of the 21 BatchNorm layers of the joint network on side ``img``, in packed
    order (16 encoder layers, 5 decoder levels): the layout of ``bn_stats`` (mean[c] | var_biased[c] per layer)."""
    shapes, h = [], img
    for _stem, _cin, cout, _sep, stride in layer_plan(False):
        h = (h + stride - 1) // stride
        shapes.append((cout, h * h))
    return shapes + [(cout, ((img // 16) << j) ** 2) for j, _cin, cout in decoder_plan()]


# ---- the two BatchNorm folds -------------------------------------------------------------------------------------------------
# BN after the ReLU (model.py:21-22) as y = relu(.) * scale + shift.  One quantity, two expressions, and both stay: the
# checkpoint's defines the features of every checkpoint in use, the training path's is the one ``occ_adamw_kernel``
# reproduces to the bit (netoptim.py, tests/test_gpu_adamw.py).  Rounded to f32 they agree on every BatchNorm element of the
# tests' checkpoints, with f64 and with f32 inputs; a one-ulp difference on some other checkpoint remains possible.
def fold_bn_checkpoint(gamma, beta, mean, var):
    """-> (scale, shift) of a checkpoint load, on f64 vectors."""
    scale = gamma / torch.sqrt(var + BN_EPS)
    return scale, beta - mean * scale


def fold_bn_vectors(gamma, beta, mean, var):
    """-> (scale, shift, rstd) in f64 of a training step, on vectors on any device."""
    rstd = 1.0 / torch.sqrt(var.double() + BN_EPS)
    scale = gamma.double() * rstd
    return scale, beta.double() - mean.double() * scale, rstd


def bn_param_grads(dscale, dshift, mean, var):
    """(dgamma, dbeta) in f64 from the gradients of the folded affine: scale = gamma rstd, shift = beta - mean gamma rstd."""
    rstd = 1.0 / torch.sqrt(var.double() + BN_EPS)
    return (dscale.double() - mean.double() * dshift.double()) * rstd, dshift.double()


# ---- the generic pack / unpack pair, on tensors on any device ----------------------------------------------------------------
def pack_layers(layers, perm, tail=()) -> torch.Tensor:
    """layers: (w, bias, scale, shift), ``w.permute(perm)`` being (cin,3,3,cout), or for a separable layer (wv (cin,1,3,1),
    wh (cin,1,1,3), pw (cout,cin,1,1), bias, scale, shift) -> the packed f32 buffer, then the ``tail`` tensors."""
    parts = []
    for *conv, b, s, t in layers:
        if len(conv) == 3:
            conv[2] = conv[2][:, :, 0, 0].t()
        else:
            conv[0] = conv[0].permute(*perm)
        parts += [*conv, b, s, t]
    return torch.cat([p.reshape(-1).to(torch.float32) for p in [*parts, *tail]])


def unpack_layers(buf: torch.Tensor, plan, perm):
    """The inverse of ``pack_layers`` for layers of ``plan`` = [(cin, cout)] or [(cin, cout, separable)] -> (the layers in the
    checkpoint's shapes, views of ``buf``; the offset of the tail)."""
    inverse = [perm.index(d) for d in range(4)]
    layers, off = [], 0
    for cin, cout, *sep in plan:
        pieces, off = _views(buf, off, _packed_shapes(cin, cout, bool(sep and sep[0])))
        if len(pieces) == 6:
            pieces[2] = pieces[2].t().reshape(cout, cin, 1, 1)
        else:
            pieces[0] = pieces[0].permute(*inverse)
        layers.append(tuple(pieces))
    return layers, off


# ---- a part: where its tensors sit in the checkpoint and how they are packed -------------------------------------------------
class Part(NamedTuple):
    stems: Tuple[str, ...]  # per layer in packed order: stem + its leaves are its parameters, stem + STATS its statistics
    tail: Tuple[str, ...]   # the parameters packed after the layers
    floats: int             # of the packed buffer
    pack: Callable          # (layers, tail tensors) -> packed buffer; a layer: (its conv leaves.., scale, shift)
    unpack: Callable        # packed buffer -> (layers, tail tensors)
    leaves: Optional[Tuple[Tuple[str, ...], ...]] = None  # per layer, ending in bn.weight, bn.bias; None: LEAVES for every layer
    shapes: Tuple = ()      # per layer the checkpoint's shapes of its leaves and statistics, then those of the tail

    def layer_leaves(self):
        return self.leaves if self.leaves is not None else (LEAVES,) * len(self.stems)


def _part(what: str, stems, plan, perm, tail=(), tail_shapes=()) -> Part:
    """The part of ``plan`` = [(cin, cout, separable)] under ``stems``; ``what`` names its buffer in an error."""
    floats = sum(layer_floats(*layer) for layer in plan) + sum(_numel(s) for s in tail_shapes)

    def pack(layers, tail_tensors=()):
        buf = pack_layers(layers, perm, tail_tensors)
        assert buf.numel() == floats
        return buf

    def unpack(buf):
        if buf.numel() != floats:
            raise ValueError(f"packed {what} buffer has {buf.numel()} floats, expected {floats}")
        layers, off = unpack_layers(buf, plan, perm)
        return layers, tuple(_views(buf, off, tail_shapes)[0])

    leaves = tuple(SEP_LEAVES if sep else LEAVES for _ci, _co, sep in plan) if any(sep for _ci, _co, sep in plan) else None
    shapes = tuple(_leaf_shapes(*layer, perm) for layer in plan) + tuple(tail_shapes)
    return Part(tuple(stems), tuple(tail), floats, pack, unpack, leaves, shapes)


def _encoder_part(prefix: str, separable: bool) -> Part:
    plan = layer_plan(separable)
    return _part("separable encoder" if separable else "dense encoder", [prefix + stem for stem, *_ in plan],
                 [(cin, cout, sep) for _stem, cin, cout, sep, _stride in plan], ENCODER_PERM)


def _decoder_part(prefix: str, classifier: str) -> Part:
    plan = decoder_plan()
    return _part("decoder", [f"{prefix}{j}.up." for j, _ci, _co in plan], [(cin, cout, False) for _j, cin, cout in plan], DECODER_PERM,
                 (classifier + "weight", classifier + "bias"), CLASSIFIER_SHAPES)


def encoder_part(preset: str) -> Part:
    """The 16 layers of the dense encoder under ``PRESETS[preset]``'s prefix."""
    return _encoder_part(PRESETS[preset][0], False)


def sep_encoder_part(preset: str) -> Part:
    """The 16 layers of the separable encoder under ``PRESETS[preset]``'s prefix: eleven separable layers, five dense downs."""
    return _encoder_part(PRESETS[preset][0], True)


def decoder_part(preset: str) -> Part:
    """The 5 up levels of the decoder and the 1x1 classifier under ``DECODER_KEYS[preset]``'s prefixes."""
    return _decoder_part(*DECODER_KEYS[preset])


def packed_floats(separable: bool) -> int:
    return _encoder_part("", separable).floats


def decoder_packed_floats() -> int:
    return _decoder_part("", "").floats


# the packed buffers without a checkpoint's keys: layers in, buffer out, and back (views of ``buf``)
def pack_encoder_buffer(layers) -> torch.Tensor:
    """layers: sixteen (w (cout,cin,3,3), bias, scale, shift) -> the packed f32 buffer of the dense encoder."""
    return _encoder_part("", False).pack(layers)


def unpack_encoder_buffer(buf: torch.Tensor):
    return _encoder_part("", False).unpack(buf)[0]


def pack_sep_encoder_buffer(layers) -> torch.Tensor:
    """layers: sixteen tuples in packed order, six tensors for a separable layer, four for a down -> the packed f32 buffer."""
    return _encoder_part("", True).pack(layers)


def unpack_sep_encoder_buffer(buf: torch.Tensor):
    return _encoder_part("", True).unpack(buf)[0]


def pack_decoder_buffer(levels, cls_w, cls_b) -> torch.Tensor:
    """levels: five (w (2c,c,3,3), bias, scale, shift) -> the packed f32 buffer of the decoder, then cls_w[8] | cls_b."""
    return _decoder_part("", "").pack(levels, (cls_w, cls_b))


def unpack_decoder_buffer(buf: torch.Tensor):
    """-> ([(w (2c,c,3,3), bias, scale, shift)] x 5, cls_w (1,8,1,1), cls_b (1,))."""
    levels, (cls_w, cls_b) = _decoder_part("", "").unpack(buf)
    return levels, cls_w, cls_b


# ---- loading a checkpoint: the checks, the fold, the pack (CPU, f64, one cast to f32) ----------------------------------------
def _get(sd, key, shape=None):
    if key not in sd:
        raise ValueError(f"encoder state dict: missing key {key!r}")
    t = torch.as_tensor(sd[key]).detach().to("cpu", torch.float64)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"encoder state dict: {key!r} has shape {tuple(t.shape)}, expected {tuple(shape)} "
                         "(only ch=8, levels=5, layers=2, k=3 give the 256 features)")
    return t


def _check_structure(sd, prefix: str):
    """The rejections of the contract: levels != 5, a third layer, a missing encoder -> whether the encoder is separable."""
    stems = [k[len(prefix):] for k in sd if k.startswith(prefix)]
    if not stems:
        raise ValueError(f"encoder state dict: no key starts with {prefix!r} (wrong preset?)")
    levels = {int(m.group(1)) for s in stems for m in [re.match(r"features\.(\d+)\.", s)] if m}
    if levels != set(range(LEVELS)):
        raise ValueError(f"encoder state dict: levels {sorted(levels)}; only levels=5 gives 256 features")
    layers = {m.group(1) for s in stems for m in [re.match(r"features\.\d+\.net\.Layer (\d+)\.", s)] if m}
    if layers != {"1", "2"}:
        raise ValueError(f"encoder state dict: layers {sorted(layers)} per block; only layers=2 is supported")
    if prefix + "initial." + SEP_LEAVES[0] in sd:
        return True
    if prefix + "initial." + LEAVES[0] in sd:
        return False
    raise ValueError(f"encoder state dict: missing key {prefix + 'initial.' + LEAVES[0]!r}")


def _check_up_weight(sd, wkey: str, shape) -> None:
    """What the decoder says about an ``up`` weight before its shape is compared (ConvTranspose2d: input channels first)."""
    if wkey not in sd:
        raise ValueError(f"decoder state dict: missing key {wkey!r}")
    w = torch.as_tensor(sd[wkey])
    if w.dim() == 4 and tuple(w.shape[:2]) != tuple(shape[:2]):
        raise ValueError(f"decoder state dict: {wkey!r} maps {w.shape[0]} -> {w.shape[1]} channels, expected {shape[0]} -> {shape[1]} "
                         "(only ch=8, levels=5 is supported)")


def _packed_checkpoint(sd, part: Part, check_weight=None):
    """``part.pack`` of the tensors of ``sd``, read layer by layer in the order of the part's keys, each checked against its
    shape, the BatchNorm folded as a checkpoint load folds it -> numpy f32."""
    layers = []
    for stem, leaves, shapes in zip(part.stems, part.layer_leaves(), part.shapes):
        if check_weight is not None:
            check_weight(sd, stem + leaves[0], shapes[0])
        *conv, gamma, beta, mean, var = [_get(sd, stem + leaf, shape) for leaf, shape in zip(leaves + STATS, shapes)]
        layers.append((*conv, *fold_bn_checkpoint(gamma, beta, mean, var)))
    tail = [_get(sd, key, shape) for key, shape in zip(part.tail, part.shapes[len(part.stems):])]
    return part.pack(layers, tail).numpy()


def pack_state_dict(sd, prefix: str):
    """Parse, check and fold a state dict -> (separable, packed f32 numpy buffer, [offset of every layer])."""
    separable = _check_structure(sd, prefix)
    w0 = _get(sd, prefix + "initial." + (SEP_LEAVES[2] if separable else LEAVES[0]))
    if w0.shape[0] != CH:
        raise ValueError(f"encoder state dict: ch = {w0.shape[0]}; only ch=8 gives 256 features")
    return separable, _packed_checkpoint(sd, _encoder_part(prefix, separable)), layer_offsets(separable)


def pack_decoder(sd, prefix: str, classifier: str):
    """Parse, check and fold the decoder of a state dict -> packed f32 numpy buffer.

    Only the ``up`` TrConv of every block is read: TrConvBlock.forward returns ``self.up(x)`` and discards what its
    ``net`` layers computed (model.py:63-67), so ``{prefix}{j}.net.*`` keys are neither needed nor used."""
    stems = [k[len(prefix):] for k in sd if k.startswith(prefix)]
    if not stems:
        raise ValueError(f"decoder state dict: no key starts with {prefix!r}")
    levels = {int(m.group(1)) for s in stems for m in [re.match(r"(\d+)\.", s)] if m}
    if levels != set(range(LEVELS)):
        raise ValueError(f"decoder state dict: levels {sorted(levels)}; only levels=5 matches the encoder's five skips")
    return _packed_checkpoint(sd, _decoder_part(prefix, classifier), _check_up_weight)


def _unfolded(sd, part: Part, extra=()) -> dict:
    """The tensors of ``part`` as the checkpoint holds them, under their full keys: per layer its leaves and statistics, then
    the tail, then ``extra``.  This order is the registration order of a ``nettrain.TrainableNet``'s parameters."""
    keys = [stem + leaf for stem, leaves in zip(part.stems, part.layer_leaves()) for leaf in leaves + STATS]
    return {k: torch.as_tensor(sd[k]).detach().to("cpu").clone() for k in [*keys, *part.tail, *extra]}


def decoder_tensors(sd, prefix: str, classifier: str) -> dict:
    """The unfolded tensors ``pack_decoder`` reads (what ``seghead.SegmentationHead`` trains and
    ``FrozenEncoder.with_decoder`` takes back); call after ``pack_decoder`` has checked them."""
    return _unfolded(sd, _decoder_part(prefix, classifier))


def encoder_tensors(sd, prefix: str, separable: bool, grad_head: Optional[str] = None) -> dict:
    """The unfolded tensors ``pack_state_dict`` reads, plus the grad head's when it is there (what
    ``enctrain.TrainableEncoder`` trains and ``FrozenEncoder.with_encoder`` takes back); call after ``pack_state_dict``."""
    head = (grad_head + "weight", grad_head + "bias") if grad_head is not None and grad_head + "weight" in sd else ()
    return _unfolded(sd, _encoder_part(prefix, separable), head)
