"""Host-side checks of the packed AdamW step (csrc/occ_adamw.hpp, occlusionenv_amd/netoptim.py): the host model of
tests/adamw_model.py in its f32-rounded form follows ``torch.optim.AdamW`` on CPU tensors, and two deliberate breaks of the
model are caught by that check; the size query is the restated layout; the entry points refuse bad arguments before anything
is launched; ``PackedAdamW`` refuses a net that is not joint and its ``state_dict`` round-trips.  No GPU.

The bar of the f32 comparison.  Model and ``torch.optim.AdamW`` apply the same f32 operations in the same order to the same
gradient bits; what may differ is whether a multiply-add is fused.  Per step that is at most one rounding of the parameter
(one ulp at the tensor's largest element) and a few roundings of the update, which is at most about lr in size; the moments
take two fusable operations per step.  So, per tensor over K steps:
    parameter  K (ulp32(max |p|) + 8 eps32 lr_max)        moments  2 K ulp32(max |moment|)
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from occlusionenv_amd import _native as nat
from tests import adamw_model as am
from tests import train_model as tm

P16 = C.c_void_p(4096)  # never dereferenced: every call below is rejected before a launch
EPS32 = float(np.finfo(np.float32).eps)
STEPS = 5
LRS = [1e-3, 8e-4, 1.2e-3, 5e-4, 9e-4]
WEIGHT_DECAY = 1e-2


def _cfg(img=64, dilation=2, residual=1, separable=1):
    cfg = nat.OccEncoderConfig()
    cfg.img, cfg.dilation, cfg.residual, cfg.separable = img, dilation, residual, separable
    return cfg


def _random_grads(model, seed):
    """Per step: the packed gradient of each part and the head's, f32; the BatchNorm slots read as (d scale, d shift)."""
    gen = torch.Generator().manual_seed(seed)
    steps = []
    for _ in range(STEPS):
        packed = [torch.randn(t.size, generator=gen) * 0.05 for t in model.theta]
        steps.append((packed, torch.randn(model.head.size, generator=gen) * 0.05))
    return steps


def _follows_torch(form, mutate=None):
    sd = tm.joint_state_dict("golden", form == "separable")
    model = am.PackedModel(form, sd, dtype=np.float32)
    steps = _random_grads(model, 7)
    per_key = [am.grads_per_key(model, packed, head, 0) for packed, head in steps]
    want_p, want_m, want_v = am.torch_adamw_reference(form, sd, per_key, LRS, WEIGHT_DECAY)
    for (packed, head), lr in zip(steps, LRS):
        model.step(packed, head, lr, WEIGHT_DECAY, 0, mutate=mutate)
    assert model.step_count == STEPS
    worst = 0.0
    for what, want in (("theta", want_p), ("m", want_m), ("v", want_v)):
        got = model.per_key(what)
        assert set(got) == set(want)
        for k, w in want.items():
            top = float(w.abs().max())
            bar = STEPS * (am.ulp32(top) + 8 * EPS32 * max(LRS)) if what == "theta" else 2 * STEPS * am.ulp32(top)
            err = float((got[k].double() - w.double()).abs().max())
            worst = max(worst, err / bar)
            assert got[k].shape == w.shape and err <= bar, (what, k, err, bar)
    return worst


@pytest.mark.parametrize("form", ["dense", "separable"])
def test_f32_model_follows_torch_adamw(form):
    worst = _follows_torch(form)
    print(f"{form}: worst error / bar {worst:.3g}")


@pytest.mark.parametrize("mutate", ["decay_on_scale", "no_bias_correction"])
def test_the_check_catches_a_broken_model(mutate):
    with pytest.raises(AssertionError):
        _follows_torch("separable", mutate=mutate)


def test_the_f64_model_and_its_f32_form_agree_to_f32_rounding():
    sd = tm.joint_state_dict("golden", separable=False)
    m64, m32 = am.PackedModel("dense", sd), am.PackedModel("dense", sd, dtype=np.float32)
    for (packed, head), lr in zip(_random_grads(m64, 11), LRS):
        m64.step(packed, head, lr, WEIGHT_DECAY, 1)
        m32.step(packed, head, lr, WEIGHT_DECAY, 1)
    a, b = m64.per_key(), m32.per_key()
    for k, w in a.items():
        assert float((b[k].double() - w).abs().max()) <= STEPS * (am.ulp32(float(w.abs().max())) + 8 * EPS32 * max(LRS)), k
    # batch statistics: the packed output is the masters, running statistics: their fold
    for part, out, theta in zip(m32.parts, m32.packed_output(1), m32.theta):
        assert np.array_equal(out.numpy(), theta)
    assert not np.array_equal(m32.packed_output(0)[0].numpy(), m32.theta[0])


def test_query_is_the_restated_layout():
    from occlusionenv_amd.encoder import decoder_packed_floats, packed_floats
    from occlusionenv_amd.nettrain import bn_layer_shapes

    lib = nat.load()
    for separable in (0, 1):
        for img in (32, 64, 256):
            sizes = [C.c_int64(), C.c_int64(), C.c_int64()]
            cfg = _cfg(img, dilation=2 if separable else 1, separable=separable)
            assert lib.occ_net_adamw_query(C.byref(cfg), *[C.byref(s) for s in sizes]) == 0
            assert [int(s.value) for s in sizes] == [packed_floats(bool(separable)), decoder_packed_floats(),
                                                     2 * sum(c for c, _plane in bn_layer_shapes(img))]
    assert packed_floats(False) % 4 == 0 and packed_floats(True) % 4 == 0  # the decoder starts a 16-byte run in no buffer's middle
    sizes = [C.c_int64(), C.c_int64(), C.c_int64()]
    assert lib.occ_net_adamw_query(None, *[C.byref(s) for s in sizes]) == 1
    assert lib.occ_net_adamw_query(C.byref(_cfg(separable=2)), *[C.byref(s) for s in sizes]) == 1
    assert lib.occ_net_adamw_query(C.byref(_cfg(16)), *[C.byref(s) for s in sizes]) == 1
    for i in range(3):
        args = [C.byref(s) for s in sizes]
        args[i] = None
        assert lib.occ_net_adamw_query(C.byref(_cfg()), *args) == 1


def test_symbols_declared_exported_and_abi_stays_12():
    import os

    lib = C.CDLL(nat.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "occlusionenv_amd.h")).read()
    for name in ("occ_net_adamw_query", "occ_net_adamw_step", "occ_net_adamw_fold"):
        assert hasattr(lib, name) and name in nat.SYMBOLS and f"int {name}(" in header
    assert nat.load().occ_abi_version() == 12 == nat.ABI_VERSION


def test_argument_checks_need_no_gpu():
    lib = nat.load()
    # occ_net_adamw_step(cfg, enc theta m v grad packed, dec theta m v grad packed, stats, head theta m v grad, head_count,
    #                    lr, beta1, beta2, eps, weight_decay, step, bn_mode, stream)
    full = [C.byref(_cfg())] + [P16] * 15 + [514, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 0, None]
    for i in range(16):
        args = list(full)
        args[i] = None
        assert lib.occ_net_adamw_step(*args) == 1, i
    for i in range(1, 16):
        args = list(full)
        args[i] = C.c_void_p(4096 + 4)  # not 16-byte aligned
        assert lib.occ_net_adamw_step(*args) == 1, i
    for i, bad in ((16, -1), (17, -1e-3), (17, float("nan")), (18, 1.0), (18, -0.1), (19, 1.0), (20, 0.0), (20, -1e-8),
                   (20, float("nan")), (21, -1e-2), (22, 0), (22, -3), (23, 2), (23, -1)):
        args = list(full)
        args[i] = bad
        assert lib.occ_net_adamw_step(*args) == 1, (i, bad)
    for bad in (_cfg(separable=2), _cfg(dilation=3), _cfg(16), _cfg(residual=2)):
        assert lib.occ_net_adamw_step(C.byref(bad), *full[1:]) == 1
    # occ_net_adamw_fold(cfg, enc_theta, enc_packed, dec_theta, dec_packed, stats, bn_mode, stream)
    full = [C.byref(_cfg())] + [P16] * 5 + [0, None]
    for i in range(6):
        args = list(full)
        args[i] = None
        assert lib.occ_net_adamw_fold(*args) == 1, i
    assert lib.occ_net_adamw_fold(*full[:6], 2, None) == 1
    assert lib.occ_net_adamw_fold(C.byref(_cfg(separable=2)), *full[1:]) == 1


def test_packed_adamw_refuses_a_net_that_is_not_joint():
    from occlusionenv_amd.netoptim import PackedAdamW

    with pytest.raises(ValueError, match="joint network"):
        PackedAdamW(torch.nn.Linear(4, 2))
    with pytest.raises(ValueError, match="joint network"):
        PackedAdamW([torch.nn.Parameter(torch.zeros(3))])


def test_optimizer_state_dict_round_trips_on_cpu_tensors():
    from occlusionenv_amd.netoptim import PackedAdamW

    gen = torch.Generator().manual_seed(3)

    def leaves():
        return [torch.zeros(n, requires_grad=True) for n in (40, 24, 514)]

    opt = PackedAdamW._over_leaves(leaves(), lr=2e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=1e-2)
    for p in opt.param_groups[0]["params"]:
        st = opt.moments(p)
        st["step"] += 4
        st["exp_avg"].copy_(torch.randn(p.numel(), generator=gen))
        st["exp_avg_sq"].copy_(torch.rand(p.numel(), generator=gen))
    saved = copy.deepcopy(opt.state_dict())  # as a file would hold it: load_state_dict keeps tensors that already fit
    assert saved["param_groups"][0]["lr"] == 2e-3 and saved["param_groups"][0]["betas"] == (0.8, 0.99)
    assert sorted(saved["state"]) == [0, 1, 2] and all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in saved["state"].values())
    fresh = PackedAdamW._over_leaves(leaves())
    fresh.load_state_dict(saved)
    group = fresh.param_groups[0]
    assert (group["lr"], group["betas"], group["eps"], group["weight_decay"]) == (2e-3, (0.8, 0.99), 1e-7, 1e-2)
    for p, q in zip(opt.param_groups[0]["params"], group["params"]):
        a, b = opt.state[p], fresh.moments(q)
        assert float(b["step"]) == 4.0 and torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
    with pytest.raises(RuntimeError, match="no network to step"):
        fresh.step()
    with pytest.raises(ValueError, match="Invalid epsilon"):
        PackedAdamW._over_leaves(leaves(), eps=0.0)
