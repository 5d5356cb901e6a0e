"""Generates tests/golden/criterion_golden.npz from the reference's own loss.py and torch's nn losses, in f64 with
autograd.  Run once, at authoring time only, with the reference's directory given (its loss.py is imported from there,
nothing of it is copied):

    python tests/golden/make_criterion_golden.py /path/to/reference

Per input (N = 3, S = 32; one binary and one soft target; pred with exact 0.0, 1.0 and 0.5 entries, regenerated from the
seed by tests/criterion_model.py: make_maps): BinaryDiceLoss() with every reduction and nn.BCELoss(), each with its gradient
with respect to pred; and nn.MSELoss() / nn.SmoothL1Loss(beta=0.01) on seeded (3,2) tensors.  Only the seeds, the losses
(f64) and the (3,32,32) gradients are stored.  To keep the fixture below 100 kB the gradients are stored as the float32
rounding of the f64 result (keys ending in ``_f32``): eight f64 maps of random mantissas do not fit, and half an f32 ulp
(6e-8 relative) is far below the 1e-4 bar they are used at.  For reduction "none" the backward runs with the upstream
vector NONE_UPSTREAM, so that a per-env mix-up shows.

A degenerate fixture would let a broken criterion pass, so this script asserts per env: 10-90 % of the target pixels set
(> 0.5), 10-90 % of pred above 0.5, and at least one pixel with a clamped log (pred exactly 0 or 1).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, sys.argv[1])
import loss as ref_loss  # noqa: E402

from tests.criterion_model import make_grad_pairs, make_maps  # noqa: E402

N, S = 3, 32
INPUTS = {"binary": 20261101, "soft": 20261102}  # name: seed
GRAD_SEED = 20261103
NONE_UPSTREAM = [0.5, -1.25, 2.0]

out = {"n_img": np.array([N, S]), "names": np.array(list(INPUTS)), "seeds": np.array(list(INPUTS.values())),
       "grad_seed": np.array(GRAD_SEED), "none_upstream": np.array(NONE_UPSTREAM)}
for name, seed in INPUTS.items():
    pred32, target32 = make_maps(seed, N, S, soft=name == "soft")
    for i in range(N):
        share_t, share_p = float((target32[i] > 0.5).double().mean()), float((pred32[i] > 0.5).double().mean())
        clamped = int(((pred32[i] == 0) | (pred32[i] == 1)).sum())
        print(name, i, "target set %.3f" % share_t, "pred > 0.5 %.3f" % share_p, "clamped pixels", clamped,
              "pred == 0.5:", int((pred32[i] == 0.5).sum()))
        assert 0.1 <= share_t <= 0.9 and 0.1 <= share_p <= 0.9 and clamped >= 1 and int((pred32[i] == 0.5).sum()) >= 1
    if name == "soft":
        assert bool(((target32 > 0) & (target32 < 1)).any())
    target = target32.double()[:, None]
    for key, crit, upstream in [("dice_mean", ref_loss.BinaryDiceLoss(), None),
                                ("dice_sum", ref_loss.BinaryDiceLoss(reduction="sum"), None),
                                ("dice_none", ref_loss.BinaryDiceLoss(reduction="none"), torch.tensor(NONE_UPSTREAM, dtype=torch.float64)),
                                ("bce", torch.nn.BCELoss(), None)]:
        pred = pred32.double()[:, None].requires_grad_(True)
        value = crit(pred, target)
        if upstream is None:
            value.backward()
        else:
            value.backward(upstream)
        out[f"{name}_{key}_loss"] = value.detach().numpy()
        out[f"{name}_{key}_grad_f32"] = pred.grad[:, 0].numpy().astype(np.float32)
        print(name, key, value.detach().numpy(), "max |grad| %.3g" % float(pred.grad.abs().max()))

gp, g = make_grad_pairs(GRAD_SEED, N)
assert bool(((gp - g).abs() < 0.01).any()) and bool(((gp - g).abs() > 0.01).any())
out["mse_loss"] = torch.nn.MSELoss()(gp, g).numpy()
out["smooth_l1_loss"] = torch.nn.SmoothL1Loss(beta=0.01)(gp, g).numpy()

path = os.path.join(HERE, "criterion_golden.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
assert os.path.getsize(path) < 100_000
