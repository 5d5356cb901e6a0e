"""The frozen FullNetwork / PredictorNet encoder as native inference (csrc/occ_encoder.hpp).

The reference's agent runs every observation through a frozen, pretrained ``FullNetwork`` and keeps the 256-d average
pool of the encoder's last ``down`` output (PPO.py:47,152-162; model.py:142-171); the gradient predictors read the same
feature (``FullNetwork.gradPredictor``, model.py:164, no tanh; ``PredictorNet.output`` + tanh, model.py:81-85).
``FrozenEncoder`` loads such a network's weights once (parsed and checked on the CPU, BatchNorm folded to a per-channel
affine, packed in the layout include/occlusionenv_amd.h documents, uploaded) and runs ``occ_encoder_forward`` on the
caller's stream: no host sync, no allocation once the workspace of a batch size exists, capturable in a HIP graph.

Presets (model.py: a state dict stores neither the dilation nor the residual flag):

  ``"ppo"``        FullNetwork(8, dilation=2, separable=True), residual=True, keys ``encoder.*`` (PPO.py:47, test.py)
  ``"predictor"``  PredictorNet(8): dense 3x3, dilation 1, no residual, keys ``features.*`` (train_predict.py:27)

Whole-module checkpoints (``torch.save(model)``, as pretrainer.py writes them) need the reference's ``model.py`` to
unpickle; with it on the path use ``FrozenEncoder.from_module(torch.load(path, weights_only=False))``.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Optional

import numpy as np
import torch

from . import _native as nat

CH, LEVELS, FEATURES = 8, 5, 256
BN_EPS = 1e-5
PRESETS = {
    # name: (key prefix, grad head, tanh on the grad head, dilation, residual)
    "ppo": ("encoder.", "gradPredictor.", False, 2, True),
    "predictor": ("features.", "output.", True, 1, False),
}


def _layer_floats(cin: int, cout: int, separable: bool) -> int:
    return 6 * cin + cin * cout + 3 * cout if separable else 9 * cin * cout + 3 * cout


def layer_plan(separable: bool):
    """[(state-dict stem relative to the encoder prefix, cin, cout, separable, stride)] in packed order."""
    plan = [("initial.", 4, CH, separable, 1)]
    for lv in range(LEVELS):
        c = CH << lv
        plan += [(f"features.{lv}.net.Layer 1.", c, c, separable, 1), (f"features.{lv}.net.Layer 2.", c, c, separable, 1),
                 (f"features.{lv}.down.", c, 2 * c, False, 2)]
    return plan


def packed_floats(separable: bool) -> int:
    return sum(_layer_floats(ci, co, sep) for _, ci, co, sep, _ in layer_plan(separable))


def _get(sd, key, shape=None):
    if key not in sd:
        raise ValueError(f"encoder state dict: missing key {key!r}")
    t = torch.as_tensor(sd[key]).detach().to("cpu", torch.float64)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"encoder state dict: {key!r} has shape {tuple(t.shape)}, expected {tuple(shape)} "
                         "(only ch=8, levels=5, layers=2, k=3 give the 256 features)")
    return t


def fold_bn(sd, stem: str, cout: int):
    """BN after the ReLU (model.py:21-22) as y = relu(.) * scale + shift, in f64."""
    g = _get(sd, stem + "bn.weight", (cout,))
    b = _get(sd, stem + "bn.bias", (cout,))
    m = _get(sd, stem + "bn.running_mean", (cout,))
    v = _get(sd, stem + "bn.running_var", (cout,))
    scale = g / torch.sqrt(v + BN_EPS)
    return scale, b - m * scale


def _check_structure(sd, prefix: str):
    """The rejections of the contract: levels != 5, a third layer, a missing encoder."""
    stems = [k[len(prefix):] for k in sd if k.startswith(prefix)]
    if not stems:
        raise ValueError(f"encoder state dict: no key starts with {prefix!r} (wrong preset?)")
    levels = {int(m.group(1)) for s in stems for m in [re.match(r"features\.(\d+)\.", s)] if m}
    if levels != set(range(LEVELS)):
        raise ValueError(f"encoder state dict: levels {sorted(levels)}; only levels=5 gives 256 features")
    layers = {m.group(1) for s in stems for m in [re.match(r"features\.\d+\.net\.Layer (\d+)\.", s)] if m}
    if layers != {"1", "2"}:
        raise ValueError(f"encoder state dict: layers {sorted(layers)} per block; only layers=2 is supported")
    if prefix + "initial.conv.0.weight" in sd:
        return True
    if prefix + "initial.conv.weight" in sd:
        return False
    raise ValueError(f"encoder state dict: missing key {prefix + 'initial.conv.weight'!r}")


def pack_state_dict(sd, prefix: str):
    """Parse, check and fold a state dict -> (separable, packed f32 numpy buffer, [offset of every layer])."""
    separable = _check_structure(sd, prefix)
    w0 = _get(sd, prefix + ("initial.conv.2.weight" if separable else "initial.conv.weight"))
    if w0.shape[0] != CH:
        raise ValueError(f"encoder state dict: ch = {w0.shape[0]}; only ch=8 gives 256 features")
    parts, offsets, off = [], [], 0
    for stem, cin, cout, sep, _stride in layer_plan(separable):
        stem = prefix + stem
        if sep:
            dv = _get(sd, stem + "conv.0.weight", (cin, 1, 3, 1))[:, 0, :, 0]
            dh = _get(sd, stem + "conv.1.weight", (cin, 1, 1, 3))[:, 0, 0, :]
            pw = _get(sd, stem + "conv.2.weight", (cout, cin, 1, 1))[:, :, 0, 0].t()
            bias = _get(sd, stem + "conv.2.bias", (cout,))
            body = [dv.reshape(-1), dh.reshape(-1), pw.reshape(-1)]
        else:
            w = _get(sd, stem + "conv.weight", (cout, cin, 3, 3))
            bias = _get(sd, stem + "conv.bias", (cout,))
            body = [w.permute(1, 2, 3, 0).reshape(-1)]
        scale, shift = fold_bn(sd, stem, cout)
        offsets.append(off)
        layer = torch.cat(body + [bias, scale, shift])
        assert layer.numel() == _layer_floats(cin, cout, sep)
        parts.append(layer)
        off += layer.numel()
    return separable, torch.cat(parts).to(torch.float32).numpy(), offsets


class FrozenEncoder:
    """Native inference of the frozen encoder: ``enc(obs)`` (N,4,S,S) f32 on the GPU -> (N,256) f32 pooled features,
    the callable ``BatchedPPO(encoder=...)`` takes; ``enc.predict_grad(obs)`` -> (N,2) from the grad head.

    Calls are split into chunks of at most ``max_chunk`` envs (one workspace per (chunk size, S), kept and reused);
    every env's features are computed independently, so the chunking changes no bit."""

    def __init__(self, packed: np.ndarray, separable: bool, dilation: int, residual: bool, preset: str, grad_head=None,
                 heads: Optional[dict] = None, device="cuda", max_chunk: int = 256, offsets=None):
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
        self.packed_host = np.ascontiguousarray(packed, dtype=np.float32)
        self.layer_offsets = list(offsets or [])
        lib = nat.load()
        cfg = self._cfg(64)
        if lib.occ_encoder_packed_floats(C.byref(cfg)) != self.packed_host.size:
            raise nat.NativeError("packed encoder weights do not match the library's layout")
        self.packed = torch.from_numpy(self.packed_host).to(self.device)
        self.grad_tanh = PRESETS[preset][2] if preset in PRESETS else False
        self.grad_w = self.grad_b = None
        if grad_head is not None:
            self.grad_w = grad_head[0].to(self.device, torch.float32).contiguous()
            self.grad_b = grad_head[1].to(self.device, torch.float32).contiguous()
        self.heads = heads or {}
        self._ws = {}

    # ---- construction ------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, preset: str = "ppo", dilation: Optional[int] = None, residual: Optional[bool] = None,
                        device="cuda", max_chunk: int = 256) -> "FrozenEncoder":
        """A ``FullNetwork`` (preset "ppo") or ``PredictorNet`` (preset "predictor") state dict.  The dilation and the
        residual flag are not in a state dict: they come from the preset unless given."""
        if preset not in PRESETS:
            raise ValueError(f"unknown preset {preset!r}; one of {sorted(PRESETS)}")
        prefix, ghead, _tanh, d0, r0 = PRESETS[preset]
        separable, packed, offsets = pack_state_dict(sd, prefix)
        grad_head = None
        if ghead + "weight" in sd:
            grad_head = (_get(sd, ghead + "weight", (2, FEATURES)), _get(sd, ghead + "bias", (2,)))
        heads = {}
        for name, rows in (("action_head.", 2), ("value_head.", 1)):
            if name + "weight" in sd:
                heads[name[:-1]] = (_get(sd, name + "weight", (rows, FEATURES)), _get(sd, name + "bias", (rows,)))
        return cls(packed, separable, d0 if dilation is None else int(dilation), r0 if residual is None else bool(residual),
                   preset, grad_head, heads, device, max_chunk, offsets)

    @classmethod
    def from_module(cls, m, device="cuda", max_chunk: int = 256) -> "FrozenEncoder":
        """A ``FullNetwork`` or ``PredictorNet`` module: dilation and residual are read from the module (the dilation of
        the first block's Layer 1 conv, ``ConvBlock.residual``)."""
        if hasattr(m, "encoder") and hasattr(m, "gradPredictor"):
            preset, enc = "ppo", m.encoder
        elif hasattr(m, "features") and hasattr(m, "output"):
            preset, enc = "predictor", m.features
        else:
            raise ValueError("from_module expects a FullNetwork or a PredictorNet")
        block = enc.features[0]
        conv = block.net[0].conv
        dil = conv[0].dilation[0] if isinstance(conv, torch.nn.Sequential) else conv.dilation[0]
        return cls.from_state_dict(m.state_dict(), preset, int(dil), bool(block.residual), device, max_chunk)

    @classmethod
    def from_file(cls, path, preset: str = "ppo", dilation: Optional[int] = None, residual: Optional[bool] = None,
                  device="cuda", max_chunk: int = 256) -> "FrozenEncoder":
        """A state dict saved with ``torch.save(model.state_dict(), path)`` (loaded with weights_only=True)."""
        sd = torch.load(path, map_location="cpu", weights_only=True)
        return cls.from_state_dict(sd, preset, dilation, residual, device, max_chunk)

    # ---- inference -------------------------------------------------------------------------------------------------
    def _cfg(self, img: int) -> nat.OccEncoderConfig:
        cfg = nat.OccEncoderConfig()
        cfg.img, cfg.dilation, cfg.residual, cfg.separable = int(img), self.dilation, int(self.residual), int(self.separable)
        return cfg

    def _workspace(self, n: int, img: int):
        key = (n, img)
        ws = self._ws.get(key)
        if ws is None:
            nbytes = C.c_size_t()
            nat.check(nat.load().occ_encoder_workspace_query(C.byref(self._cfg(img)), n, C.byref(nbytes)),
                      "occ_encoder_workspace_query")
            ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
        return ws

    @torch.no_grad()
    def __call__(self, obs: torch.Tensor) -> torch.Tensor:
        if not isinstance(obs, torch.Tensor) or not obs.is_cuda:
            raise nat.NativeError("FrozenEncoder needs CUDA/ROCm tensors; there is no CPU fallback")
        if obs.dim() != 4 or obs.shape[1] != 4 or obs.shape[2] != obs.shape[3]:
            raise ValueError(f"obs must be (N,4,S,S), got {tuple(obs.shape)}")
        if obs.device != self.packed.device:
            raise ValueError(f"obs is on {obs.device}, the encoder's weights on {self.packed.device}")
        img = int(obs.shape[2])
        if not 32 <= img <= 1024:
            raise ValueError(f"image side {img} outside [32, 1024]")
        obs = obs.detach().to(torch.float32).contiguous()
        n_all = int(obs.shape[0])
        feats = torch.empty(n_all, FEATURES, dtype=torch.float32, device=obs.device)
        if n_all == 0:
            return feats
        lib = nat.load()
        cfg = self._cfg(img)
        stream = C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        per_env = 4 * img * img
        for lo in range(0, n_all, self.max_chunk):
            n = min(self.max_chunk, n_all - lo)
            ws = self._workspace(n, img)
            nat.check(lib.occ_encoder_forward(C.byref(cfg), C.c_void_p(self.packed.data_ptr()),
                                              C.c_void_p(obs.data_ptr() + 4 * lo * per_env), n, C.c_void_p(ws.data_ptr()),
                                              ws.numel(), C.c_void_p(feats.data_ptr() + 4 * lo * FEATURES), stream),
                      "occ_encoder_forward")
        return feats

    @torch.no_grad()
    def predict_grad(self, obs: torch.Tensor) -> torch.Tensor:
        """(N,2): ``FullNetwork.gradPredictor(pooled)`` (no tanh, model.py:164) or ``tanh(PredictorNet.output(pooled))``
        (model.py:81-85)."""
        if self.grad_w is None:
            raise ValueError("this checkpoint has no gradPredictor / output head")
        g = torch.addmm(self.grad_b, self(obs), self.grad_w.t())
        return torch.tanh(g) if self.grad_tanh else g
