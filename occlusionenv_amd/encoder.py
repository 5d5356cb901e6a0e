"""The frozen FullNetwork / PredictorNet encoder as native inference (csrc/occ_encoder.hpp).

The reference's agent runs every observation through a frozen, pretrained ``FullNetwork`` and keeps the 256-d average
pool of the encoder's last ``down`` output (PPO.py:47,152-162; model.py:142-171); the gradient predictors read the same
feature (``FullNetwork.gradPredictor``, model.py:164, no tanh; ``PredictorNet.output`` + tanh, model.py:81-85).
``FrozenEncoder`` loads such a network's weights once (parsed, checked, BatchNorm folded to a per-channel affine and packed
on the CPU by ``netlayout``, whose names are importable here, in the layout include/occlusionenv_amd.h documents, uploaded)
and runs ``occ_encoder_forward`` on the caller's stream: no host sync, no allocation once the workspace of a batch size
exists, capturable in a HIP graph.

Presets (model.py: a state dict stores neither the dilation nor the residual flag):

  ``"ppo"``        FullNetwork(8, dilation=2, separable=True), residual=True, keys ``encoder.*`` (PPO.py:47, test.py)
  ``"predictor"``  PredictorNet(8): dense 3x3, dilation 1, no residual, keys ``features.*`` (train_predict.py:27)

  ``"segmenter"``  Segmenter(8): dense 3x3, dilation 1, residual=True, keys ``encoder.*``, ``decoder.features.*``,
                   ``classifier.*``; no grad head (train_segm.py:28)

The segmentation decoder (csrc/occ_decoder.hpp; model.py:109-125,147-150) is picked up when its keys are in the state dict
(``enc.has_decoder``): ``enc.segment(obs)`` is the predicted occlusion map, ``enc.forward_full(obs)`` the triple of
``FullNetwork.forward`` from one pass over the encoder, ``enc.occlusion_metrics(pred, target)`` the accuracy / IoU counts
of pretrainer.py:127-141, ``enc.validation_losses(...)`` one batch of ``PreTrainer.val()`` (losses and metrics from one read
of the maps, csrc/occ_criterion.hpp); both hand on to ``segmentation.py``, the home of everything that consumes a predicted map.

Every forward call takes ``skip=`` and ``out=``: a caller who holds a batch of which only some rows have changed passes an
(N,) int32 or bool mask on the device, and the rows it marks are left alone (``occ_encoder_forward_masked``,
``occ_segment_forward_masked``: their blocks return at once, nothing of them is read or written).  With ``out=`` such rows
keep the bits they held; without it they are zero.  The grid stays sized for N and the mask is read on the device, so the
host needs no count of the active rows and a captured call follows the mask it finds at replay.

``precision="bf16"`` (separable encoders only; csrc/occ_encoder_bf16.hpp) is a reduced-precision inference mode of the
pooled feature: activations are stored as bfloat16, the contractions take bf16 operands (on the matrix cores from 16 input
channels up) and accumulate in f32; the observation, the depthwise taps, biases, the BN affine, every epilogue and ``feats``
stay f32, and the heads run in torch f32 on the f32 ``feats``.  ``enc(obs, skip=, out=)`` and ``enc.predict_grad`` work as
in f32, with the same guarantees on bits (repeat calls, batch position, chunking); ``segment``, ``forward_full`` and the
training wrappers need the f32 mode (``enc.with_precision("f32")``).

Whole-module checkpoints (``torch.save(model)``, as pretrainer.py writes them) need the reference's ``model.py`` to
unpickle; with it on the path use ``FrozenEncoder.from_module(torch.load(path, weights_only=False))``.
"""
from __future__ import annotations

import copy
import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _native as nat
from . import segmentation
from .netlayout import (BN_EPS, CH, DECODER_KEYS, FEATURES, LEVELS, PRESETS, _get, decoder_packed_floats, decoder_plan,  # noqa: F401
                        decoder_tensors, encoder_tensors, layer_plan, pack_decoder, pack_state_dict, packed_floats)
from .segmentation import seg_counts  # noqa: F401

PRECISIONS = ("f32", "bf16")
# (the decoder runs, a skip mask is given) -> the f32 entry point of a forward call
FORWARD_ENTRY = {(False, False): "occ_encoder_forward", (False, True): "occ_encoder_forward_masked",
                 (True, False): "occ_segment_forward", (True, True): "occ_segment_forward_masked"}


def _check_precision(precision: str, separable: bool, what: str) -> None:
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
    if precision == "bf16" and not separable:
        raise ValueError(f"precision='bf16' exists for the separable encoder only; {what} the dense one")


class FrozenEncoder:
    """Native inference of the frozen encoder: ``enc(obs)`` (N,4,S,S) f32 on the GPU -> (N,256) f32 pooled features,
    the callable ``BatchedPPO(encoder=...)`` takes; ``enc.predict_grad(obs)`` -> (N,2) from the grad head.

    Calls are split into chunks of at most ``max_chunk`` envs (one workspace per (chunk size, S), kept and reused);
    every env's features are computed independently, so the chunking changes no bit."""

    takes_skip_mask = True  # ppo.BatchedPPO.features: this encoder is called with skip= and out=
    precision = "f32"       # the mode: "f32", or "bf16" (inference of the pooled feature only; the module docstring)
    packed_bf16 = None      # the bf16 mode's packed buffer on the device

    def __init__(self, packed: np.ndarray, separable: bool, dilation: int, residual: bool, preset: str, grad_head=None,
                 heads: Optional[dict] = None, device="cuda", max_chunk: int = 256, offsets=None, decoder=None,
                 decoder_state: Optional[dict] = None, encoder_state: Optional[dict] = None, precision: str = "f32"):
        _check_precision(precision, separable, "this state dict holds")
        if dilation not in (1, 2):
            raise ValueError(f"dilation must be 1 or 2, got {dilation}")
        if int(max_chunk) < 1:
            raise ValueError("max_chunk must be >= 1")
        self.preset = preset
        self.separable, self.dilation, self.residual = bool(separable), int(dilation), bool(residual)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise nat.NativeError("FrozenEncoder runs in the HIP library: it needs a CUDA/ROCm device; there is no CPU fallback")
        self.max_chunk = int(max_chunk)
        self.layer_offsets = list(offsets or [])
        lib = nat.load()
        cfg = self._cfg(64)
        if lib.occ_encoder_packed_floats(C.byref(cfg)) != np.size(packed):
            raise nat.NativeError("packed encoder weights do not match the library's layout")
        self.packed_host, self.packed = self._upload(packed)
        self.precision = precision
        self.packed_bf16 = self._pack_bf16() if precision == "bf16" else None
        self.grad_tanh = PRESETS[preset][2] if preset in PRESETS else False
        self.grad_w = self.grad_b = None
        if grad_head is not None:
            self.grad_w, self.grad_b = self._head(grad_head)
        self.heads = heads or {}
        self._ws = {}  # (kind, chunk size, S) -> workspace
        self.dec_packed_host = self.dec_packed = None
        self.decoder_state = decoder_state  # the decoder's unfolded tensors by state-dict key (None without a decoder)
        self.encoder_state = encoder_state  # the encoder's (and the grad head's) unfolded tensors by state-dict key
        if decoder is not None:
            if lib.occ_decoder_packed_floats(C.byref(cfg)) != np.size(decoder):
                raise nat.NativeError("packed decoder weights do not match the library's layout")
            self.dec_packed_host, self.dec_packed = self._upload(decoder)

    def _upload(self, packed):
        """A packed host buffer as (contiguous f32 numpy array, its copy on the device)."""
        host = np.ascontiguousarray(packed, dtype=np.float32)
        return host, torch.from_numpy(host).to(self.device)

    def _head(self, weight_bias):
        return tuple(t.to(self.device, torch.float32).contiguous() for t in weight_bias)

    def _pack_bf16(self) -> torch.Tensor:
        """The bf16 mode's packed buffer (include/occlusionenv_amd.h) of ``packed_host``, on the device: made on the host by
        ``occ_encoder_bf16_pack``."""
        lib, cfg = nat.load(), self._cfg(64)
        nbytes = int(lib.occ_encoder_bf16_packed_bytes(C.byref(cfg)))
        if nbytes <= 0:
            raise nat.NativeError("occ_encoder_bf16_packed_bytes rejected the configuration")
        host = np.empty(nbytes, dtype=np.uint8)
        nat.check(lib.occ_encoder_bf16_pack(C.byref(cfg), self.packed_host.ctypes.data_as(C.c_void_p),
                                            host.ctypes.data_as(C.c_void_p)), "occ_encoder_bf16_pack")
        return torch.from_numpy(host).to(self.device)

    def _derived(self, packed=None, decoder=None, **fields) -> "FrozenEncoder":
        """A copy of this encoder with ``fields`` replaced; what is not replaced is shared, not copied.  It starts with no
        workspaces; ``packed`` / ``decoder`` are new packed host buffers, uploaded here, and the bf16 buffer is packed again
        whenever ``packed`` or the precision changed.  This encoder is left as it is."""
        new = copy.copy(self)
        new._ws = {}
        for name, value in fields.items():
            setattr(new, name, value)
        if packed is not None:
            new.packed_host, new.packed = self._upload(packed)
        if decoder is not None:
            new.dec_packed_host, new.dec_packed = self._upload(decoder)
        if packed is not None or "precision" in fields:
            new.packed_bf16 = new._pack_bf16() if new.precision == "bf16" else None
        return new

    def with_precision(self, precision: str) -> "FrozenEncoder":
        """A ``FrozenEncoder`` over this one's state (weights, heads, decoder: shared, not copied) that runs in ``precision``
        ("f32" or "bf16").  This encoder is left as it is."""
        _check_precision(precision, self.separable, "this encoder is")
        return self._derived(precision=precision)

    def _f32_only(self, what: str) -> None:
        if self.precision != "f32":
            raise ValueError(f"{what}: precision={self.precision!r} is inference of the pooled feature only; "
                             "use enc.with_precision('f32')")

    @property
    def has_decoder(self) -> bool:
        """Whether the checkpoint held the segmentation decoder (``segment`` / ``forward_full`` need it)."""
        return self.dec_packed is not None

    # ---- construction ------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, preset: str = "ppo", dilation: Optional[int] = None, residual: Optional[bool] = None,
                        device="cuda", max_chunk: int = 256, precision: str = "f32") -> "FrozenEncoder":
        """A ``FullNetwork`` (preset "ppo"), ``PredictorNet`` (preset "predictor") or ``Segmenter`` (preset "segmenter")
        state dict.  The dilation and the residual flag are not in a state dict: they come from the preset unless given.
        The segmentation decoder is loaded when its keys are there (``has_decoder``).  ``precision``: "f32", or "bf16" for
        the reduced-precision inference mode of a separable encoder (the module docstring)."""
        if preset not in PRESETS:
            raise ValueError(f"unknown preset {preset!r}; one of {sorted(PRESETS)}")
        if preset == "segmenter" and any(k.startswith(("segmenter.0.", "gradPredictor.")) for k in sd):
            # both networks keep their encoder under "encoder.": without this a FullNetwork would load with the Segmenter's
            # dilation and without its decoder
            raise ValueError("state dict holds FullNetwork keys ('segmenter.0.*' / 'gradPredictor.*'): unknown preset "
                             "'segmenter' for such a checkpoint, use preset='ppo'")
        prefix, ghead, _tanh, d0, r0 = PRESETS[preset]
        separable, packed, offsets = pack_state_dict(sd, prefix)
        decoder = decoder_state = None
        if preset in DECODER_KEYS:
            dprefix, dcls = DECODER_KEYS[preset]
            if any(k.startswith(dprefix) or k.startswith(dcls) for k in sd):
                decoder = pack_decoder(sd, dprefix, dcls)
                decoder_state = decoder_tensors(sd, dprefix, dcls)
        grad_head = None
        if ghead is not None and ghead + "weight" in sd:
            grad_head = (_get(sd, ghead + "weight", (2, FEATURES)), _get(sd, ghead + "bias", (2,)))
        heads = {}
        for name, rows in (("action_head.", 2), ("value_head.", 1)):
            if name + "weight" in sd:
                heads[name[:-1]] = (_get(sd, name + "weight", (rows, FEATURES)), _get(sd, name + "bias", (rows,)))
        return cls(packed, separable, d0 if dilation is None else int(dilation), r0 if residual is None else bool(residual),
                   preset, grad_head, heads, device, max_chunk, offsets, decoder, decoder_state,
                   encoder_tensors(sd, prefix, separable, ghead), precision)

    def with_decoder(self, sd) -> "FrozenEncoder":
        """A ``FrozenEncoder`` with this one's encoder (the packed weights are shared, not copied) and the decoder of
        ``sd``, a state dict holding the decoder and classifier keys of this preset (``DECODER_KEYS``), such as
        ``seghead.SegmentationHead.state_dict()`` after fine-tuning.  This encoder is left as it is."""
        if self.preset not in DECODER_KEYS:
            raise ValueError(f"preset {self.preset!r} has no segmentation decoder")
        dprefix, dcls = DECODER_KEYS[self.preset]
        return self._derived(decoder=pack_decoder(sd, dprefix, dcls), decoder_state=decoder_tensors(sd, dprefix, dcls))

    def with_encoder(self, sd) -> "FrozenEncoder":
        """A ``FrozenEncoder`` with the encoder (and, when its keys are in ``sd``, the grad head) of ``sd``, a state dict
        under this preset's keys such as ``enctrain.TrainableEncoder.state_dict()`` after training, and this one's dilation,
        residual flag and decoder.  This encoder is left as it is."""
        prefix, ghead = PRESETS[self.preset][0], PRESETS[self.preset][1]
        separable, packed, offsets = pack_state_dict(sd, prefix)
        if separable != self.separable:
            raise ValueError("with_encoder: the state dict's encoder is " + ("separable" if separable else "dense") +
                             ", this encoder is not")
        fields = dict(layer_offsets=list(offsets))
        if ghead is not None and ghead + "weight" in sd:
            fields["grad_w"], fields["grad_b"] = self._head((_get(sd, ghead + "weight", (2, FEATURES)), _get(sd, ghead + "bias", (2,))))
        return self._derived(packed=packed, encoder_state=encoder_tensors(sd, prefix, separable, ghead), **fields)

    def with_state(self, sd) -> "FrozenEncoder":
        """``with_encoder(sd).with_decoder(sd)``: the whole trained network of ``fullnet.TrainableFullNetwork.state_dict()``."""
        return self.with_encoder(sd).with_decoder(sd)

    @classmethod
    def from_module(cls, m, device="cuda", max_chunk: int = 256, precision: str = "f32") -> "FrozenEncoder":
        """A ``FullNetwork``, ``PredictorNet`` or ``Segmenter`` module: dilation and residual are read from the module
        (the dilation of the first block's Layer 1 conv, ``ConvBlock.residual``)."""
        if hasattr(m, "encoder") and hasattr(m, "gradPredictor"):
            preset, enc = "ppo", m.encoder
        elif hasattr(m, "encoder") and hasattr(m, "decoder") and hasattr(m, "classifier"):
            preset, enc = "segmenter", m.encoder
        elif hasattr(m, "features") and hasattr(m, "output"):
            preset, enc = "predictor", m.features
        else:
            raise ValueError("from_module expects a FullNetwork, a PredictorNet or a Segmenter")
        block = enc.features[0]
        conv = block.net[0].conv
        dil = conv[0].dilation[0] if isinstance(conv, torch.nn.Sequential) else conv.dilation[0]
        return cls.from_state_dict(m.state_dict(), preset, int(dil), bool(block.residual), device, max_chunk, precision)

    @classmethod
    def from_file(cls, path, preset: str = "ppo", dilation: Optional[int] = None, residual: Optional[bool] = None,
                  device="cuda", max_chunk: int = 256, precision: str = "f32") -> "FrozenEncoder":
        """A state dict saved with ``torch.save(model.state_dict(), path)`` (loaded with weights_only=True)."""
        sd = torch.load(path, map_location="cpu", weights_only=True)
        return cls.from_state_dict(sd, preset, dilation, residual, device, max_chunk, precision)

    # ---- inference -------------------------------------------------------------------------------------------------
    def _cfg(self, img: int) -> nat.OccEncoderConfig:
        cfg = nat.OccEncoderConfig()
        cfg.img, cfg.dilation, cfg.residual, cfg.separable = int(img), self.dilation, int(self.residual), int(self.separable)
        return cfg

    def _check_obs(self, obs: torch.Tensor, decoder: bool) -> int:
        """The checks of a forward call, before anything native is touched -> the image side.  ``decoder``: the call runs the
        segmentation decoder, whose skip additions need a side that is a multiple of 32."""
        if not isinstance(obs, torch.Tensor) or not obs.is_cuda:
            raise nat.NativeError("FrozenEncoder needs CUDA/ROCm tensors; there is no CPU fallback")
        if decoder and not self.has_decoder:
            raise ValueError("this checkpoint has no segmentation decoder (no 'segmenter.0.features.*' / 'decoder.features.*' keys)")
        if obs.dim() != 4 or obs.shape[1] != 4 or obs.shape[2] != obs.shape[3]:
            raise ValueError(f"obs must be (N,4,S,S), got {tuple(obs.shape)}")
        if obs.device != self.packed.device:
            raise ValueError(f"obs is on {obs.device}, the encoder's weights on {self.packed.device}")
        img = int(obs.shape[2])
        if decoder and not (32 <= img <= 1024 and img % 32 == 0):
            raise ValueError(f"image side {img}: the decoder's skip additions need a multiple of 32 in [32, 1024]")
        if not 32 <= img <= 1024:
            raise ValueError(f"image side {img} outside [32, 1024]")
        return img

    def _workspace(self, kind: str, n: int, img: int):
        """The kept workspace of ``occ_<kind>_forward`` (kind "encoder" or "segment") for a chunk of n envs."""
        key = (kind, n, img)
        ws = self._ws.get(key)
        if ws is None:
            nbytes, what = C.c_size_t(), f"occ_{kind}_workspace_query"
            nat.check(getattr(nat.load(), what)(C.byref(self._cfg(img)), n, C.byref(nbytes)), what)
            ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
        return ws

    @staticmethod
    def _check_skip(skip, obs: torch.Tensor):
        """The skip mask of a forward call as a contiguous (N,) int32 tensor (None stays None); ValueError otherwise."""
        if skip is None:
            return None
        if not isinstance(skip, torch.Tensor) or skip.dtype not in (torch.int32, torch.bool):
            raise ValueError("skip must be an int32 or bool tensor, got " +
                             (str(skip.dtype) if isinstance(skip, torch.Tensor) else type(skip).__name__))
        if skip.dim() != 1 or skip.shape[0] != obs.shape[0]:
            raise ValueError(f"skip must be ({int(obs.shape[0])},), one entry per row of obs, got {tuple(skip.shape)}")
        if skip.device != obs.device:
            raise ValueError(f"skip is on {skip.device}, obs on {obs.device}")
        return skip.detach().to(torch.int32).contiguous()

    @staticmethod
    def _check_out(name: str, out, shape, device) -> None:
        """``out`` is a tensor a native call can write rows of in place: f32, contiguous, of ``shape``, on ``device``."""
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32:
            raise ValueError(f"out ({name}) must be a float32 tensor")
        if tuple(out.shape) != tuple(shape):
            raise ValueError(f"out ({name}) must be {tuple(shape)}, got {tuple(out.shape)}")
        if out.device != device:
            raise ValueError(f"out ({name}) is on {out.device}, obs on {device}")
        if not out.is_contiguous():
            raise ValueError(f"out ({name}) must be contiguous")

    @staticmethod
    def _out_tuple(out, names) -> tuple:
        """``out`` of a call that returns ``names`` -> one entry per name (None: no ``out`` given)."""
        if out is None:
            return (None,) * len(names)
        if isinstance(out, torch.Tensor):
            out = (out,)
        if not isinstance(out, (tuple, list)) or len(out) != len(names):
            raise ValueError(f"out must hold {len(names)} tensor(s) in the call's return order ({', '.join(names)})")
        return tuple(out)

    def _forward(self, obs: torch.Tensor, decoder: bool, want_logits: bool = False, want_features: bool = False, skip=None,
                 out=(None, None, None, None)):
        """-> (pooled (N,256), prob (N,1,S,S), logits, decoder feature (N,8,S,S)), None for what was not asked for: one
        occ_segment_forward (``decoder``) or occ_encoder_forward per chunk on the caller's stream.  ``skip``: the (N,) mask of
        rows to leave alone (the ``_masked`` entry points; every chunk takes its slice).  ``out``: the tensors to write into,
        in the order of the return value (None: a fresh one, zero where a row is skipped); their skipped rows keep their
        bits.  Everything is checked before anything native runs."""
        if decoder:
            self._f32_only("the segmentation decoder")
        img = self._check_obs(obs, decoder)
        bf16 = self.precision == "bf16"
        n_all = int(obs.shape[0])
        skip = self._check_skip(skip, obs)
        shapes = ((n_all, FEATURES), (n_all, 1, img, img), (n_all, 1, img, img), (n_all, CH, img, img))
        wanted = (True, decoder, want_logits, want_features)
        for name, o, shape, want in zip(("features", "prob", "logits", "decoder feature"), out, shapes, wanted):
            if o is not None and want:
                self._check_out(name, o, shape, obs.device)
        obs = obs.detach().to(torch.float32).contiguous()
        alloc = torch.empty if skip is None else torch.zeros
        feats, prob, logits, dfeat = (
            (alloc(shape, dtype=torch.float32, device=obs.device) if o is None else o) if want else None
            for o, shape, want in zip(out, shapes, wanted))
        if n_all == 0:
            return feats, prob, logits, dfeat
        # the entry point, its workspace and the packed weights it reads (bf16 is encoder only: the decoder needs f32)
        masked = bf16 or skip is not None  # the bf16 entry point takes the mask always, None when no row is skipped
        kind = "encoder_bf16" if bf16 else "segment" if decoder else "encoder"
        name = "occ_encoder_forward_bf16" if bf16 else FORWARD_ENTRY[decoder, masked]
        weights = [self.packed_bf16] if bf16 else [self.packed, self.dec_packed] if decoder else [self.packed]
        entry, cfg, stream = getattr(nat.load(), name), self._cfg(img), nat.stream_ptr(obs.device)
        pix = 4 * img * img  # bytes of one f32 map
        for lo, n in nat.row_chunks(n_all, self.max_chunk):
            ws = self._workspace(kind, n, img)
            outs = [nat.ptr(feats, lo * 4 * FEATURES)]
            if decoder:
                outs += [nat.ptr(prob, lo * pix), nat.ptr(logits, lo * pix), nat.ptr(dfeat, lo * CH * pix)]
            if masked:
                outs.append(None if skip is None else nat.ptr(skip, 4 * lo))
            nat.check(entry(C.byref(cfg), *[nat.ptr(w) for w in weights], nat.ptr(obs, lo * 4 * pix), n, nat.ptr(ws), ws.numel(),
                            *outs, stream), name)
        return feats, prob, logits, dfeat

    @torch.no_grad()
    def __call__(self, obs: torch.Tensor, skip=None, out=None) -> torch.Tensor:
        """The pooled (N,256) feature.  ``skip``: an (N,) int32 or bool tensor on the encoder's device; a row with a non-zero
        entry is left alone: its blocks return at once and nothing of it is read or written (the mask is read on the device
        when the kernels run, so a captured call follows the values it finds at replay).  ``out``: the (N,256) f32
        contiguous tensor to write into, whose skipped rows keep their bits; without it skipped rows of the result are zero."""
        (o,) = self._out_tuple(out, ("features",))
        return self._forward(obs, False, skip=skip, out=(o, None, None, None))[0]

    def _masked_head(self, feats: torch.Tensor, skip, out):
        """``grad_head(feats)`` on all rows (no count of the active ones, no sync); a skipped row keeps the bits of ``out``
        or, without ``out``, is zero."""
        g = self.grad_head(feats)
        if skip is None:
            return g if out is None else out.copy_(g)
        keep = (skip != 0).unsqueeze(1)
        if out is None:
            return torch.where(keep, torch.zeros_like(g), g)
        return out.copy_(torch.where(keep, out, g))

    @torch.no_grad()
    def predict_grad(self, obs: torch.Tensor, skip=None, out=None) -> torch.Tensor:
        """(N,2): ``FullNetwork.gradPredictor(pooled)`` (no tanh, model.py:164) or ``tanh(PredictorNet.output(pooled))``
        (model.py:81-85).  ``skip`` as in ``__call__``; ``out``: the (N,2) f32 contiguous tensor to write into."""
        if self.grad_w is None:
            raise ValueError("this checkpoint has no gradPredictor / output head")
        (o,) = self._out_tuple(out, ("grad",))
        if o is not None:
            self._check_obs(obs, False)
            self._check_out("grad", o, (int(obs.shape[0]), 2), obs.device)
        return self._masked_head(self(obs, skip=skip), skip, o)

    @torch.no_grad()
    def grad_head(self, feats: torch.Tensor) -> torch.Tensor:
        """The head of ``predict_grad`` alone, on pooled features (N,256) that a caller already holds."""
        if self.grad_w is None:
            raise ValueError("this checkpoint has no gradPredictor / output head")
        g = torch.addmm(self.grad_b, feats, self.grad_w.t())
        return torch.tanh(g) if self.grad_tanh else g

    # ---- segmentation decoder --------------------------------------------------------------------------------------
    def _segment(self, obs: torch.Tensor, want_logits: bool, want_features: bool, skip=None, out=(None, None, None, None)):
        """-> (pooled (N,256), prob (N,1,S,S), logits or None, decoder feature (N,8,S,S) or None): one occ_segment_forward
        per chunk on the caller's stream."""
        return self._forward(obs, True, want_logits, want_features, skip, out)

    @torch.no_grad()
    def segment(self, obs: torch.Tensor, return_logits: bool = False, return_features: bool = False, skip=None, out=None):
        """The predicted occlusion map ``sigmoid(segmenter(encoder(obs)))`` (model.py:159), (N,1,S,S) f32; S a multiple of
        32.  With ``return_features`` the (N,8,S,S) decoder feature comes first, as in ``Segmenter.forward`` (model.py:
        135-140): ``(features, predictions)``; with ``return_logits`` the classifier's output before the sigmoid comes last.
        ``skip`` as in ``__call__``; ``out``: the tensors to write into, a tuple in the order of the return value (a lone
        tensor when only the map is returned)."""
        self._f32_only("segment")
        names = (("decoder feature",) if return_features else ()) + ("prob",) + (("logits",) if return_logits else ())
        given = dict(zip(names, self._out_tuple(out, names)))
        _f, prob, logits, dfeat = self._segment(obs, return_logits, return_features, skip,
                                                (None, given.get("prob"), given.get("logits"), given.get("decoder feature")))
        res = ((dfeat,) if return_features else ()) + (prob,) + ((logits,) if return_logits else ())
        return res[0] if len(res) == 1 else res

    @torch.no_grad()
    def forward_full(self, obs: torch.Tensor, skip=None, out=None):
        """``FullNetwork.forward`` (model.py:156-166) from one pass over the encoder: (pooled (N,256), segm (N,1,S,S),
        grad (N,2)).  The pooled feature is bitwise ``self(obs)``.  ``skip`` as in ``__call__``; ``out``: a tuple
        (pooled, segm, grad) to write into."""
        self._f32_only("forward_full")
        if self.grad_w is None:
            raise ValueError("this checkpoint has no gradPredictor / output head")
        o_feats, o_prob, o_grad = self._out_tuple(out, ("features", "prob", "grad"))
        if o_grad is not None:
            self._check_obs(obs, True)
            self._check_out("grad", o_grad, (int(obs.shape[0]), 2), obs.device)
        feats, prob, _l, _d = self._segment(obs, False, False, skip, (o_feats, o_prob, None, None))
        return feats, prob, self._masked_head(feats, skip, o_grad)

    def occlusion_metrics(self, pred: torch.Tensor, target: torch.Tensor) -> dict:
        """The judgement of pretrainer.py:133-141 on a batch: both maps thresholded at 0.5; per-env int64 counts
        ``correct`` (pixels where they agree), ``intersection``, ``union`` on the device, and over the whole batch
        ``accuracy`` = sum(correct) / pixels and ``iou`` = sum(intersection) / sum(union) as 0-d f64 tensors (0 / 0 = nan,
        as in the reference).  pred (N,1,S,S) or (N,S,S); target likewise, any float tensor; a strided view such as
        ``full_state[..., 3]`` is read in place."""
        return segmentation.occlusion_metrics(pred, target)

    def validation_losses(self, segm: torch.Tensor, grad_pred: torch.Tensor, occlusion: torch.Tensor, grad: torch.Tensor,
                          use_dice: bool = True, use_l1: bool = False) -> dict:
        """One batch of ``PreTrainer.val()`` (pretrainer.py:176-189) on the outputs of ``forward_full``: ``segm_loss`` =
        BinaryDiceLoss() (``use_dice``) or nn.BCELoss() of the predicted map against ``occlusion``, ``grad_loss`` =
        nn.MSELoss() or nn.SmoothL1Loss(beta=0.01) (``use_l1``) of the (N,2) gradient prediction, ``loss`` their sum,
        ``accuracy`` and ``iou`` as fractions over the batch (0 / 0 = nan, as in the reference), all 0-d f64 tensors on the
        device, plus the per-env int64 ``correct``, ``intersection``, ``union``.  The maps are read once
        (``segmentation.seg_criterion``); no host sync."""
        return segmentation.validation_losses(segm, grad_pred, occlusion, grad, use_dice, use_l1)
