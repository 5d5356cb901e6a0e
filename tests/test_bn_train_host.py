"""Host-side checks of the joint training step with batch-statistics BatchNorm (csrc/occ_bn_train.hpp,
``from_encoder(enc, batch_stats=True)``): the A / B / C form of the BatchNorm backward is the gradient, the running-average
rule of ``nettrain`` is nn.BatchNorm2d's, the workspace query is the documented layout, the statistics the train-mode model
records are those of its relu outputs, and every case whose gradients the GPU
test judges is well conditioned: PyTorch's own f32 run of it agrees with the f64 model within 1e-4 for every tensor.  The
argument contract of the three entry points is checked from the table of tests/train_abi.py by
tests/test_train_abi_host.py.  No GPU."""
import ctypes as C

import pytest
import torch

from occlusionenv_amd import _native as nat
from occlusionenv_amd import nettrain
from tests import train_layout as tl
from tests import train_model as m

SYMBOLS = ("occ_fullnet_bn_train_workspace_query", "occ_fullnet_bn_train_forward", "occ_fullnet_bn_backward")
FORMS = {"dense": dict(dilation=1, separable=0), "separable": dict(dilation=2, separable=1)}


def _net(form, residual=True, batch_stats=True):
    return m.Net("ppo", form == "separable", FORMS[form]["dilation"], residual, True, batch_stats)


def _cfg(img=64, dilation=2, residual=1, separable=1):
    cfg = nat.OccEncoderConfig()
    cfg.img, cfg.dilation, cfg.residual, cfg.separable = img, dilation, residual, separable
    return cfg


def _query(lib, name, img, n, **kw):
    ws, sc = C.c_size_t(), C.c_size_t()
    rc = getattr(lib, name)(C.byref(_cfg(img, **kw)), n, C.byref(ws), C.byref(sc))
    return rc, int(ws.value), int(sc.value)


def test_abc_form_is_the_batchnorm_gradient():
    """dR = A dY + C r + B, dgamma and dbeta against f64 autograd through F.batch_norm in training mode; channel 2 is dead
    (r = 0 everywhere, variance 0), channel 3 is constant."""
    gen = torch.Generator().manual_seed(5)
    for shape in ((2, 5, 1, 1), (3, 5, 3, 3), (2, 5, 8, 8)):
        r = torch.relu(torch.randn(shape, generator=gen, dtype=torch.float64)).requires_grad_()
        with torch.no_grad():
            r[:, 2] = 0.0
            r[:, 3] = 0.75
        gamma = (torch.rand(5, generator=gen, dtype=torch.float64) + 0.5).requires_grad_()
        beta = torch.randn(5, generator=gen, dtype=torch.float64).requires_grad_()
        dy = torch.randn(shape, generator=gen, dtype=torch.float64)
        y = torch.nn.functional.batch_norm(r, None, None, gamma, beta, True, 0.1, m.EPS)
        want = torch.autograd.grad(y, (r, gamma, beta), dy)
        got = m.bn_backward_abc(r.detach(), dy, gamma.detach())
        for g, w in zip(got, want):
            assert float((g - w).abs().max()) <= 1e-9 * max(1.0, float(w.abs().max())), shape
        assert float(got[1][2].abs()) == 0.0  # the dead channel: dgamma = rstd (0 - 0)


def test_running_average_rule_is_batchnorm2d():
    """nettrain._update_running_stats, two steps, against nn.BatchNorm2d in f64 on the same activations."""
    n, img = 2, 32
    stems = [f"l{i}." for i in range(21)]
    shapes = tl.layer_shapes(img)
    assert [(c, s * s) for c, s in shapes] == nettrain.bn_layer_shapes(img) and sum(c for c, _s in shapes) == tl.CHANNELS
    gen = torch.Generator().manual_seed(9)
    bns = [torch.nn.BatchNorm2d(c).double().train() for c, _s in shapes]
    buffers = {}
    for st, bn, (c, _s) in zip(stems, bns, shapes):
        with torch.no_grad():
            bn.running_mean.copy_(torch.randn(c, generator=gen))
            bn.running_var.copy_(torch.rand(c, generator=gen) + 0.5)
        buffers[st] = (bn.running_mean.clone(), bn.running_var.clone())

    class Net:
        parts = (nettrain.Part(tuple(stems), (), 0, None, None),)

        @staticmethod
        def _stats(stem):
            return buffers[stem]

    for _step in range(2):
        stats = []
        for bn, (c, side) in zip(bns, shapes):
            r = torch.relu(torch.randn(n, c, side, side, generator=gen, dtype=torch.float64))
            bn(r)
            stats += [r.mean(dim=(0, 2, 3)), r.var(dim=(0, 2, 3), unbiased=False)]
        nettrain._update_running_stats(Net, torch.cat(stats), n, img)
        for st, bn in zip(stems, bns):
            assert torch.allclose(buffers[st][0], bn.running_mean, rtol=1e-12, atol=1e-14), st
            assert torch.allclose(buffers[st][1], bn.running_var, rtol=1e-12, atol=1e-14), st


@pytest.mark.parametrize("form", sorted(FORMS))
def test_workspace_query_is_the_documented_layout(form):
    lib = nat.load()
    joint = "occ_fullnet_train_workspace_query" if form == "dense" else "occ_sep_fullnet_train_workspace_query"
    for img, n in ((32, 2), (64, 3), (96, 2), (64, 4), (256, 8)):
        rc, ws_b, sc_b = _query(lib, SYMBOLS[0], img, n, **FORMS[form])
        rcj, ws_j, sc_j = _query(lib, joint, img, n, **FORMS[form])
        assert rc == 0 and rcj == 0
        assert ws_j == tl.ws_bytes(_net(form, batch_stats=False), img, n) and sc_b == sc_j == tl.scratch_bytes(_net(form), img, n)
        assert ws_b == tl.ws_bytes(_net(form), img, n) and ws_b - ws_j == tl.extra_ws_bytes(img, n) > 0, (img, n)
        assert ws_b % 256 == 0
    # coef 24 bytes per channel, abc 3 x 256 floats, the partials of the largest layer: the last down (256 channels, one
    # chunk) until level 0 (8 channels) has more than 32 chunks
    assert tl.extra_ws_bytes(256, 8) == 29952 + 3072 + 256 * 8 * 1 * 2 * 8
    assert tl.extra_ws_bytes(1024, 2) == 29952 + 3072 + 8 * 2 * 256 * 2 * 8
    assert tl.extra_ws_bytes(32, 2) == 29952 + 3072 + 256 * 2 * 1 * 2 * 8


def test_python_keyword_and_modes_need_no_gpu():
    """``batch_stats`` is off by default, is taken by both joint classes and by the harness, and only counts while
    training."""
    import inspect

    from occlusionenv_amd import harness
    from occlusionenv_amd.fullnet import JointNet, TrainableFullNetwork
    from occlusionenv_amd.sepfullnet import TrainableSeparableFullNetwork

    for cls in (TrainableFullNetwork, TrainableSeparableFullNetwork):
        assert inspect.signature(cls.from_encoder).parameters["batch_stats"].default is False
        assert cls.BN_SYMBOLS == SYMBOLS and issubclass(cls, JointNet)
    assert inspect.signature(harness.pretrain_epoch).parameters["batch_stats"].default is False
    assert nettrain.TrainableNet.BN_SYMBOLS is None and nettrain.BN_MOMENTUM == m.MOMENTUM


def test_recorded_statistics_are_those_of_the_relu_outputs():
    """With ``running`` a copy of the checkpoint's statistics, the train-mode forward's ``stats`` are the mean and the biased
    variance of relu(u) for the u's it hands out, layer by layer, and ``running`` moves by momentum 0.1 towards them (the
    variance unbiased), for one dense and one separable net at 2 x 32^2: 32 is the smallest S the decoder takes, N = 2 the
    smallest batch with N (S/32)^2 >= 2 values per channel at the deepest layer."""
    for form in sorted(FORMS):
        net = _net(form)
        host = m.HostModel(m.joint_state_dict("golden", net.separable), net, m.case_obs((32, 2)))
        before = {k: v.clone() for k, v in host.running.items()}
        us = []
        with torch.no_grad():
            host.forward(None, us)
        assert len(us) == len(host.stats) == 21 and host.packed_stats().shape == (2 * tl.CHANNELS,)
        assert [(u.shape[1], u.shape[-1]) for u in us] == tl.layer_shapes(32)
        for stem, u, (mean, var) in zip(m.bn_stems(net), us, host.stats):
            r = torch.relu(u)
            cnt = r.numel() // r.shape[1]
            assert torch.equal(mean, r.mean(dim=(0, 2, 3))) and torch.equal(var, r.var(dim=(0, 2, 3), unbiased=False)), stem
            for leaf, want in (("bn.running_mean", mean), ("bn.running_var", var * cnt / (cnt - 1))):
                moved = (1 - m.MOMENTUM) * before[stem + leaf] + m.MOMENTUM * want
                assert torch.allclose(host.running[stem + leaf], moved, rtol=1e-12, atol=1e-14), stem + leaf
        assert all(torch.equal(host.sd[k], v) for k, v in before.items())  # the checkpoint's own statistics stay


@pytest.mark.parametrize("case", m.BN_GRAD_CASES, ids=m.BN_IDS[:len(m.BN_GRAD_CASES)])
def test_conditioning_of_the_judged_cases(case):
    """Every tensor of every judged case: PyTorch's f32 CPU autograd run is within 1e-4 of the plain f64 model, so the
    bar max(1e-4, 4 e32) never exceeds 4e-4.  Measured worst e32: 1.6e-5 (golden separable S=64 N=3), 1.5e-5 (dense
    S=64 N=4), 1.7e-5 (seeded separable S=96 N=2); worst band share 0.11 %, 0.19 %, 0.34 %."""
    e, net = m.e32(case), m.bn_net(case)
    assert len(e) == len(m.enc_keys(net)) + 22
    worst = {}
    for k, v in e.items():
        worst[m.kind(net, k)] = max(worst.get(m.kind(net, k), 0.0), v)
    print(case, {k: f"{v:.3g}" for k, v in sorted(worst.items())})
    assert all(v <= m.E32_CAP for v in e.values()), {k: v for k, v in e.items() if v > m.E32_CAP}
    assert all(m.TOL <= m.bar(case, k) <= m.MARGIN * m.E32_CAP for k in e)
    # no layer has more than 1 % of its pixels where an f32 evaluation may flip the gate
    shares = m.band_shares(m.plain_f64(case)[2])
    assert len(shares) == 21 and max(shares) <= m.BAND_CAP, shares
    # the deepest layer sees M >= 2 values per channel (18 in the S=96 N=2 case, whose deepest plane is 3 x 3)
    assert case[5] * (case[4] // 32) ** 2 >= 2
