"""Host model of the bf16 inference mode of the separable encoder (csrc/occ_encoder_bf16.hpp): ``tests/encoder_model.encode``
with the roundings of the mode's numeric contract (include/occlusionenv_amd.h), in f64 arithmetic.

Rounded to bfloat16: the depthwise pair's result before the pointwise contraction, the pointwise and the dense down weights,
and every stored activation (after the BN affine and the residual).  The last down's output is pooled unrounded.  Everything
else keeps the working ``dtype``.  ``rounding``: "rne" (the contract), "trunc" (what a test must be able to tell from it), or
None (no rounding at all: the model is then ``encode`` op for op).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from tests.encoder_model import LEVELS


def round_bf16(x: torch.Tensor, rounding="rne") -> torch.Tensor:
    """``x`` rounded to the nearest bfloat16 value (8 significant bits), straight from its own precision: ties to even
    ("rne") or towards zero ("trunc").  The result keeps x's dtype.  Normal range only (no bf16 subnormals, no overflow)."""
    if rounding is None:
        return x
    a = x.detach().to(torch.float64).numpy()
    m, e = np.frexp(a)  # a = m * 2^e, 0.5 <= |m| < 1: m * 256 holds the 8 significant bits before the point
    if rounding == "rne":
        q = np.round(m * 256.0)  # numpy rounds halves to even
    elif rounding == "trunc":
        q = np.trunc(m * 256.0)
    else:
        raise ValueError(f"rounding must be 'rne', 'trunc' or None, got {rounding!r}")
    return torch.from_numpy(np.ldexp(q / 256.0, e)).to(x.dtype).reshape(x.shape)


def _bn(x, sd, stem):
    return F.batch_norm(x, sd[stem + "bn.running_mean"], sd[stem + "bn.running_var"], sd[stem + "bn.weight"], sd[stem + "bn.bias"],
                        False, 0.0, 1e-5)


def _sep(x, sd, stem, dilation, rounding):
    """relu(pointwise(round(dw_h(dw_v(x)))) + bias) -> BN; the pointwise weight rounded."""
    p, c = (3 + dilation - 1) // 2, x.shape[1]
    x = F.conv2d(x, sd[stem + "conv.0.weight"], None, 1, (p, 0), (dilation, 1), c)
    x = F.conv2d(x, sd[stem + "conv.1.weight"], None, 1, (0, p), (1, dilation), c)
    x = F.conv2d(round_bf16(x, rounding), round_bf16(sd[stem + "conv.2.weight"], rounding), sd[stem + "conv.2.bias"])
    return _bn(torch.relu(x), sd, stem)


def _down(x, sd, stem, rounding):
    x = F.conv2d(x, round_bf16(sd[stem + "conv.weight"], rounding), sd[stem + "conv.bias"], 2, 1, 1)
    return _bn(torch.relu(x), sd, stem)


def encode_bf16(sd, obs, prefix="encoder.", dilation=2, residual=True, rounding="rne", dtype=torch.float64):
    """(N,4,S,S) -> (N,256) of the separable encoder in the bf16 mode.  ``dtype``: the working precision of everything that
    is not bf16 (torch.float64: the yardstick; torch.float32: the same model with f32 accumulation, a second
    implementation whose distance from the yardstick is the noise a correct implementation may show)."""
    sd = {k: v.to(dtype) for k, v in sd.items() if k.startswith(prefix) and v.is_floating_point()}
    x = round_bf16(_sep(obs.to(dtype), sd, prefix + "initial.", 1, rounding), rounding)
    for lv in range(LEVELS):
        stem = f"{prefix}features.{lv}."
        y = round_bf16(_sep(x, sd, stem + "net.Layer 1.", dilation, rounding), rounding)
        y = _sep(y, sd, stem + "net.Layer 2.", dilation, rounding)
        if residual:
            y = y + x
        y = round_bf16(y, rounding)
        x = _down(y, sd, stem + "down.", rounding)
        if lv < LEVELS - 1:
            x = round_bf16(x, rounding)
    return x.mean(dim=(2, 3))


def err(got, want):
    """max |got - want| / max(1, max |want|), as tests/test_gpu_encoder.py measures."""
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max()) / max(1.0, float(want.abs().max()))
