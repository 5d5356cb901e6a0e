"""GPU tests of the packed AdamW step (csrc/occ_adamw.hpp, ``netoptim.PackedAdamW``, ``harness.pretrain_epoch(..,
native_optimizer=True)``, ``harness.pretrain``) against tests/adamw_model.py.

The network's parameter count is fixed, so the smallest observations do: N = 2, S = 32 under running statistics, N = 1,
S = 64 under batch statistics (N (S / 32)^2 = 4 values per channel in the deepest layer).  Every case runs the dense network
at dilation 1 and the separable one at dilation 2, both with the residual, on the "golden" checkpoints of
tests/train_model.py (joint_state_dict).

Bars.
  * The packed output against torch's own fold and ``Part.pack`` of the synced parameters: bitwise.  It is a permutation
    and IEEE f64 multiply, subtract, sqrt and divide, rounded to f32 once.
  * Masters and moments against the f64 model fed the same packed gradient bits, per tensor:
    max |native - f64| <= 4 max |torch.optim.AdamW in f32 on the CPU - f64| + one f32 ulp of the tensor's largest element.
    The factor 4 allows for fused multiply-adds and a differently ordered lerp; the bar comes from the reference optimizer,
    never from the code under test.
  * The per-key path (``torch.optim.AdamW`` on the ~110 parameters) against the packed path after the same three steps: the
    same bar, its first term from the packed run's own captured gradients; the five reported numbers to 1e-5 relative.

Measured on an MI355X (``-s`` prints every figure; DESIGN.md section 4.4, "The optimizer"): worst error / bar against the
f64 model over the four cases, masters 0.53, exp_avg 0.23, exp_avg_sq 0.77.  Against the per-key path the state dicts, the
running buffers and the five numbers were equal bit for bit in all four cases: the kernel's f32 rule has the roundings of
torch's foreach AdamW on the device written out, and everything before it (fold, forward, backward) is bitwise the per-key
path's.  With the rule left to the compiler's contraction the two paths differed by one ulp after the first step and by up to
289 ulp of a tensor's largest element after the third (1.9e5 under batch statistics at N = 1, S = 64): Adam's normalised
update amplifies a gradient's rounding noise, so this comparison only holds because the first step is exact.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests import adamw_model as am
from tests import train_model as tm
from tests.encoder_model import make_obs

pytestmark = pytest.mark.gpu

FORMS = [("dense", 1, 1), ("separable", 2, 1)]  # (form, dilation, residual)
FORM_IDS = [f"{f}-d{d}" for f, d, _r in FORMS]
MODES = [(False, 2, 32), (True, 1, 64)]  # (batch statistics, N, S)
MODE_IDS = ["running", "batch"]
K = 3
WEIGHT_DECAY = 1e-2
WORST = {}


def _net_class(form):
    from occlusionenv_amd.fullnet import TrainableFullNetwork
    from occlusionenv_amd.sepfullnet import TrainableSeparableFullNetwork

    return TrainableFullNetwork if form == "dense" else TrainableSeparableFullNetwork


def _batches(n, img, count=2, seed=90):
    """``count`` stored batches (obs, occlusion, grad, None) of n x img^2, on the CPU."""
    gen = torch.Generator().manual_seed(seed + img + n)
    out = []
    for b in range(count):
        occl = (torch.rand(n, 1, img // 8, img // 8, generator=gen) > 0.5).float().repeat_interleave(8, 2).repeat_interleave(8, 3)
        out.append((make_obs(700 + b, n, img).float(), occl, torch.randn(n, 2, generator=gen) * 0.5, None))
    return out


def _loss(net, batch):
    from occlusionenv_amd import segmentation

    obs, occl, grad, _ = batch
    _pooled, segm, pred = net(obs.cuda())
    return segmentation.binary_dice_loss(segm, occl.cuda()) + F.mse_loss(pred, grad.cuda())


@pytest.fixture(scope="module")
def encs():
    """form -> (sd32, FrozenEncoder)."""
    from occlusionenv_amd.encoder import FrozenEncoder

    out = {}
    for form, d, res in FORMS:
        sd32 = tm.joint_state_dict("golden", form == "separable")
        out[form] = (sd32, FrozenEncoder.from_state_dict(sd32, preset="ppo", dilation=d, residual=bool(res)))
    return out


@pytest.fixture(scope="module")
def runs(encs):
    """Per (form, batch statistics), computed once and left unchanged: K native steps with weight decay 1e-2 and a
    scheduler that changes lr every step; the packed gradients and the lr of every step are kept."""
    from occlusionenv_amd.netoptim import PackedAdamW

    cache = {}

    def get(form, bn):
        if (form, bn) not in cache:
            _bn, n, img = MODES[int(bn)]
            sd32, enc = encs[form]
            net = _net_class(form).from_encoder(enc, batch_stats=bn)
            opt = PackedAdamW(net, lr=1e-3, weight_decay=WEIGHT_DECAY)
            sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.7)
            batches = _batches(n, img)
            res, grads, lrs = net._resident, [], []
            for i in range(K):
                opt.zero_grad()
                _loss(net, batches[i % 2]).backward()
                grads.append(([t.grad.detach().cpu().clone() for t in res.theta], res.head.grad.detach().cpu().clone()))
                lrs.append(float(opt.param_groups[0]["lr"]))
                opt.step()
                assert opt.last_call["lr"] == lrs[-1] and opt.last_call["step"] == i + 1 and opt.last_call["bn_mode"] == int(bn)
                sched.step()
            assert lrs[0] == 1e-3 and abs(lrs[2] - 0.49e-3) < 1e-12
            cache[form, bn] = dict(net=net, opt=opt, grads=grads, lrs=lrs, sd=sd32, enc=enc, batches=batches)
        return cache[form, bn]

    return get


def _native_per_key(parts, bufs, head):
    out = {}
    for part, buf in zip(parts, bufs):
        out.update({k: t.clone() for k, t in am.unpack_raw(part, buf.detach().cpu()).items()})
    head = head.detach().cpu()
    out[am.HEAD_KEYS[0]], out[am.HEAD_KEYS[1]] = head[:512].reshape(2, 256), head[512:]
    return out


def _reference_errors(form, sd, grads, lrs, bn):
    """The f64 model after the steps, and per quantity {key: max |torch f32 CPU AdamW - f64|}."""
    model = am.PackedModel(form, sd)
    per_key = [am.grads_per_key(model, packed, head, int(bn)) for packed, head in grads]
    for (packed, head), lr in zip(grads, lrs):
        model.step(packed, head, lr, WEIGHT_DECAY, int(bn))
    ref = dict(zip(("theta", "m", "v"), am.torch_adamw_reference(form, sd, per_key, lrs, WEIGHT_DECAY)))
    e32 = {what: {k: float((ref[what][k].double() - w).abs().max()) for k, w in model.per_key(what).items()} for what in ref}
    return model, e32


def _check_against_model(what, got, want, e32):
    """got: {key: f32 tensor}; want: {key: f64 tensor}; the bar of the module docstring, per tensor."""
    assert set(got) == set(want)
    worst = 0.0
    for k, w in want.items():
        err = float((got[k].double() - w.double()).abs().max())
        bar = 4.0 * e32[k] + am.ulp32(float(w.abs().max()))
        worst = max(worst, err / bar)
        assert got[k].shape == w.shape and err <= bar, (what, k, err, bar, e32[k])
    WORST[what] = max(WORST.get(what, 0.0), worst)
    print(f"{what}: worst error / bar {worst:.3g}; worst so far {WORST}")


@pytest.mark.parametrize("bn", [False, True], ids=MODE_IDS)
@pytest.mark.parametrize("form", [f for f, _d, _r in FORMS], ids=FORM_IDS)
def test_packed_output_is_the_fold_of_the_synced_parameters_bitwise(runs, form, bn):
    from occlusionenv_amd.nettrain import fold_bn_vectors

    r = runs(form, bn)
    net = r["net"]
    net.sync_parameters()
    params = dict(net.named_parameters())
    for part, out, theta in zip(net.parts, net._resident.out, net._resident.theta):
        layers = []
        for stem, leaves in zip(part.stems, part.layer_leaves()):
            *conv, gamma, beta = [params[stem + leaf].detach() for leaf in leaves]
            if bn:
                layers.append((*conv, gamma, beta))
            else:
                scale, shift, _rstd = fold_bn_vectors(gamma, beta, *net._stats(stem))
                layers.append((*conv, scale, shift))
        want = part.pack(layers, [params[k].detach() for k in part.tail])
        assert want.is_cuda and torch.equal(out, want)
        assert torch.equal(out, theta.detach()) == bn  # running statistics: the output is folded, the master is not
        assert not torch.equal(theta.detach().cpu(), am.pack_raw(part, r["sd"]))  # and the steps moved it


@pytest.mark.parametrize("bn", [False, True], ids=MODE_IDS)
@pytest.mark.parametrize("form", [f for f, _d, _r in FORMS], ids=FORM_IDS)
def test_update_against_the_f64_model(runs, form, bn):
    r = runs(form, bn)
    res, opt = r["net"]._resident, r["opt"]
    model, e32 = _reference_errors(form, r["sd"], r["grads"], r["lrs"], bn)
    leaves = res.theta + [res.head]
    for what, bufs in (("theta", leaves), ("m", [opt.state[p]["exp_avg"] for p in leaves]),
                       ("v", [opt.state[p]["exp_avg_sq"] for p in leaves])):
        got = _native_per_key(model.parts, bufs[:2], bufs[2])
        _check_against_model(f"{form} {MODE_IDS[int(bn)]} {what}", got, model.per_key(what), e32[what])
    assert all(float(opt.state[p]["step"]) == K for p in leaves)


@pytest.mark.parametrize("bn", [False, True], ids=MODE_IDS)
@pytest.mark.parametrize("form", [f for f, _d, _r in FORMS], ids=FORM_IDS)
def test_same_training_as_the_per_key_path(encs, form, bn):
    """K steps of pretrain_epoch on two stored batches from one checkpoint, with torch.optim.AdamW and with
    native_optimizer=True: the state dicts agree within the bar of the f64 comparison, the numbers to 1e-5."""
    from torch.optim.optimizer import register_optimizer_step_pre_hook

    from occlusionenv_amd import harness
    from occlusionenv_amd.netoptim import PackedAdamW

    _bn, n, img = MODES[int(bn)]
    sd32, enc = encs[form]
    stored = _batches(n, img)
    batches = [stored[i % 2] for i in range(K)]
    cls = _net_class(form)
    ref = harness.pretrain_epoch(cls.from_encoder(enc, batch_stats=bn), batches, weight_decay=WEIGHT_DECAY)
    captured = []

    def keep(opt, _args, _kwargs):
        res = opt._res
        captured.append(([t.grad.detach().cpu().clone() for t in res.theta], res.head.grad.detach().cpu().clone()))

    handle = register_optimizer_step_pre_hook(keep)
    try:
        nat_ = harness.pretrain_epoch(cls.from_encoder(enc, batch_stats=bn), batches, weight_decay=WEIGHT_DECAY,
                                      native_optimizer=True)
    finally:
        handle.remove()
    assert isinstance(nat_["optimizer"], PackedAdamW) and isinstance(ref["optimizer"], torch.optim.AdamW)
    assert len(captured) == K and nat_["batches"] == ref["batches"] == K
    for k in ("loss", "segm_loss", "grad_loss", "accuracy", "iou"):
        print(f"{k}: native {nat_[k]:.9g}, per key {ref[k]:.9g}")
        assert abs(nat_[k] - ref[k]) <= 1e-5 * abs(ref[k]), k
    _model, e32 = _reference_errors(form, sd32, captured, [1e-3] * K, bn)
    got, want = nat_["net"].state_dict(), ref["net"].state_dict()
    assert list(got) == list(want)
    worst = 0.0
    for k, w in want.items():
        err = float((got[k].double() - w.double()).abs().max())
        bar = 4.0 * e32["theta"].get(k, 0.0) + am.ulp32(float(w.abs().max()))
        worst = max(worst, err / bar)
        print(f"{k}: error {err:.3g}, bar {bar:.3g}")
    print(f"{form} {MODE_IDS[int(bn)]}: worst error / bar against the per-key path {worst:.3g}")
    for k, w in want.items():
        err = float((got[k].double() - w.double()).abs().max())
        assert err <= 4.0 * e32["theta"].get(k, 0.0) + am.ulp32(float(w.abs().max())), (k, err)
    moved = [k for k in want if "running_" in k and not torch.equal(want[k].cpu(), sd32[k])]
    assert len(moved) == (42 if bn else 0)


@pytest.mark.parametrize("form", [f for f, _d, _r in FORMS], ids=FORM_IDS)
def test_trained_network_reaches_inference(encs, form):
    """After native train-mode steps, enc.with_state(net.state_dict()) infers the bits of the net's own eval-mode forward."""
    enc = encs[form][1]
    batches = _batches(1, 64)
    net, opt = _fresh(encs, form, True, weight_decay=WEIGHT_DECAY)
    for batch in batches:
        _backward(net, opt, batch)
        opt.step()
    obs = batches[0][0].cuda()
    trained = enc.with_state(net.state_dict())
    net.eval()
    with torch.no_grad():
        feats, prob, pred = net(obs)
    f2, s2, g2 = trained.forward_full(obs)
    assert torch.equal(feats, f2) and torch.equal(prob, s2)
    assert torch.allclose(pred, g2, rtol=1e-5, atol=1e-6)
    assert not torch.equal(f2, enc(obs))  # the checkpoint's network is another one
    # back in train mode the packed buffers are the raw masters again, and the moments were kept
    net.train()
    _backward(net, opt, batches[0])
    assert all(torch.equal(o, t.detach()) for o, t in zip(net._resident.out, net._resident.theta))
    opt.step()
    assert opt.last_call["step"] == 3 and opt.last_call["bn_mode"] == 1


def _fresh(encs, form, bn, **hyper):
    from occlusionenv_amd.netoptim import PackedAdamW

    net = _net_class(form).from_encoder(encs[form][1], batch_stats=bn)
    return net, PackedAdamW(net, **hyper)


def _backward(net, opt, batch, zero=True):
    if zero:
        opt.zero_grad()
    _loss(net, batch).backward()


@pytest.mark.parametrize("form", [f for f, _d, _r in FORMS], ids=FORM_IDS)
def test_gradient_accumulation(encs, form):
    """Two backward calls and one step are one step on the summed packed gradient, bitwise."""
    batches = _batches(2, 32)
    a, opt_a = _fresh(encs, form, False, weight_decay=WEIGHT_DECAY)
    _backward(a, opt_a, batches[0])
    _backward(a, opt_a, batches[1], zero=False)
    opt_a.step()
    b, opt_b = _fresh(encs, form, False, weight_decay=WEIGHT_DECAY)
    leaves = b._resident.leaves()
    _backward(b, opt_b, batches[0])
    first = [t.grad.clone() for t in leaves]
    _backward(b, opt_b, batches[1])
    assert not torch.equal(first[0], leaves[0].grad)
    for t, g in zip(leaves, first):
        t.grad = g + t.grad
    opt_b.step()
    for x, y in zip(a._resident.leaves() + a._resident.out, leaves + b._resident.out):
        assert torch.equal(x.detach(), y.detach())


@pytest.mark.parametrize("bn", [False, True], ids=MODE_IDS)
@pytest.mark.parametrize("form", [f for f, _d, _r in FORMS], ids=FORM_IDS)
def test_saved_state_continues_to_the_same_bits(encs, form, bn):
    _bn, n, img = MODES[int(bn)]
    batches = _batches(n, img)
    a, opt_a = _fresh(encs, form, bn, lr=2e-3, weight_decay=WEIGHT_DECAY)
    for i in range(2):
        _backward(a, opt_a, batches[i])
        opt_a.step()
    net_sd = {k: v.clone() for k, v in a.state_dict().items()}
    opt_sd = copy.deepcopy(opt_a.state_dict())
    _backward(a, opt_a, batches[0])
    opt_a.step()
    b, opt_b = _fresh(encs, form, bn)
    b.load_state_dict(net_sd)
    opt_b.load_state_dict(opt_sd)
    assert opt_b.param_groups[0]["lr"] == 2e-3 and opt_b.param_groups[0]["weight_decay"] == WEIGHT_DECAY
    _backward(b, opt_b, batches[0])
    opt_b.step()
    assert opt_b.last_call["step"] == 3
    for x, y in zip(a._resident.leaves() + a._resident.out, b._resident.leaves() + b._resident.out):
        assert torch.equal(x.detach(), y.detach())
    for p, q in zip(a._resident.leaves(), b._resident.leaves()):
        assert torch.equal(opt_a.state[p]["exp_avg"], opt_b.state[q]["exp_avg"])
        assert torch.equal(opt_a.state[p]["exp_avg_sq"], opt_b.state[q]["exp_avg_sq"])
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.mark.parametrize("form", [f for f, _d, _r in FORMS], ids=FORM_IDS)
def test_a_step_with_lr_0_and_no_decay_moves_only_the_moments(encs, form):
    net, opt = _fresh(encs, form, False, lr=0.0, weight_decay=0.0)
    res = net._resident
    _backward(net, opt, _batches(2, 32)[0])
    before = [t.detach().clone() for t in res.leaves() + res.out]
    opt.step()
    assert all(torch.equal(x, y.detach()) for x, y in zip(before, res.leaves() + res.out))
    for p in res.leaves():
        assert float(opt.state[p]["exp_avg"].abs().max()) > 0.0 and float(opt.state[p]["exp_avg_sq"].max()) > 0.0
    # the per-key optimizer of a packed-resident net would train nothing: refused
    from occlusionenv_amd import harness

    with pytest.raises(ValueError, match="packed-resident"):
        harness.pretrain_epoch(net, _batches(2, 32))
    with pytest.raises(RuntimeError, match="superseded"):
        loss = _loss(net, _batches(2, 32)[0])
        opt.step()
        loss.backward()


@pytest.mark.parametrize("form", [f for f, _d, _r in FORMS], ids=FORM_IDS)
def test_pretrain_runs_the_cosine_schedule_and_keeps_the_best_epoch(encs, form):
    import math

    from occlusionenv_amd import harness
    from occlusionenv_amd.netoptim import PackedAdamW

    enc = encs[form][1]
    train, val = _batches(2, 32), _batches(2, 32, seed=190)
    out = harness.pretrain(enc, lambda: iter(train), val, epochs=2, lr=1e-3)
    opt, rows = out["optimizer"], out["rows"]
    assert isinstance(opt, PackedAdamW) and len(rows) == 2 and [r["epoch"] for r in rows] == [0, 1]
    cosine = 1e-4 + (1e-3 - 1e-4) * (1 + math.cos(math.pi * 1 / 2)) / 2
    assert rows[0]["lr"] == 1e-3 and abs(rows[1]["lr"] - cosine) < 1e-15
    assert opt.last_call["lr"] == rows[1]["lr"] and opt.last_call["step"] == 4  # what the kernel took in epoch 2
    ious = [r["val"]["iou"] for r in rows]
    assert all(i == i for i in ious)
    best = 1 if ious[1] > ious[0] else 0
    assert out["best_epoch"] == best and out["best_iou"] == ious[best]
    again = harness.validate_pretrained(enc.with_state(out["best_state"]), val)
    assert again["iou"] == ious[best] and again["loss"] == rows[best]["val"]["loss"]
    if best == 0:  # the returned state is the first epoch's, not the net's final one
        assert any(not torch.equal(out["best_state"][k], v) for k, v in out["net"].state_dict().items())
    # the per-key optimizer drives the same loop
    out2 = harness.pretrain(enc, train, val, epochs=1, native_optimizer=False)
    assert isinstance(out2["optimizer"], torch.optim.AdamW) and out2["best_epoch"] == 0
