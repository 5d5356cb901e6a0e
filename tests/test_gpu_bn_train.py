"""GPU tests of the joint training step with batch-statistics BatchNorm (csrc/occ_bn_train.hpp,
``from_encoder(enc, batch_stats=True)``, ``harness.pretrain_epoch(.., batch_stats=True)``) against tests/train_model.py (a joint
``Net`` with ``batch_stats``): the network in train mode in f64 on the CPU with torch autograd.

Cases (weights, form, dilation, residual, S, N), weights rounded to f32 and used as exactly those values by the model:
golden separable d2 res S=64 N=3; golden dense d1 res S=64 N=4; seeded separable d2 no residual S=96 N=2 (M = 18 at the
deepest layer, whose plane is 3 x 3; level 0 has 2.25 chunks; no plane below level 0 is a multiple of 4 pixels, so the
one-pixel-per-lane kernels run next to the 16-byte ones).  Golden separable S=32 N=2 (M = 2 at the deepest layer) gets the
forward and determinism checks only: PyTorch's own f32 run misses the f64 model by 6e-4 there.  Two cases take their
observation from another seed than the other training tests' (train_model.OBS_SEEDS says which and why: conditioning and
the gate band, both settled on the CPU).

Bars.  Forward: bn_stats, feats and prob within 1e-4 max(1, max |want|) per tensor; kept relu outputs within
1e-4 max(1, max |r64|); gates r > 0 may differ from the f64 gate only where |u64| <= 1e-4 max(1, max |u64|), a band that
holds at most 1 % of any layer's pixels.  Gradients, per tensor, the f64 model evaluated with the GPU's own 21 gates:
max |got - want| <= max(1e-4, 4 e32) max |want|, e32 being the same relative error of PyTorch's f32 CPU autograd run of the
case against the plain f64 model; every judged case has e32 <= 1e-4 for every tensor (tests/test_bn_train_host.py asserts
it without a GPU), so the bar never exceeds 4e-4.  Running buffers: within 1e-4 max(1, max |want|).

Every gradient test prints its relative errors, its e32 and the worst so far per parameter kind (``-s``); DESIGN.md section
4.4, "Batch-statistics BatchNorm", records the measured figures.

Measured on an MI355X against the f64 model (worst relative error per parameter kind over the three judged cases and the
real losses; the bar is max(1e-4, 4 e32); worst e32 of the cases 1.6e-5, 1.5e-5, 1.7e-5):
  separable layers  conv.0.w 1.4e-5  conv.1.w 2.3e-5  conv.2.w 3.2e-5  conv.2.b 1.2e-5  bn.w 1.2e-5  bn.b 1.3e-5
  dense layers      conv.w 7.1e-6  conv.b 1.1e-5       downs  conv.w 1.5e-5  conv.b 1.8e-5  bn.w 1.1e-5  bn.b 9.7e-6
  decoder           conv.w 9.1e-6  conv.b 8.2e-6  bn.w 7.8e-6  bn.b 3.0e-6    classifier w 2.8e-6  b 5.1e-7    head w 5.7e-6  b 1.5e-7
Forward: bn_stats 5.8e-6, feats 4.0e-5 (S=32 N=2), prob 5.8e-6; kept relu 2.6e-5; one gate in the four cases differed from the
f64 model's, inside the band; worst band share 0.34 %.  Running buffers after one, two steps and after pretrain_epoch: 7.9e-6;
pretrain_epoch's mean losses against two f64 AdamW steps: 6e-8.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import train_gpu_suite as suite
from tests import train_layout as tl
from tests import train_model as m
from tests.train_utils import dice64 as _dice64
from tests.train_utils import grads as _grads
from tests.train_utils import guarded as _guarded
from tests.train_utils import guards_intact

pytestmark = pytest.mark.gpu

TOL = m.TOL
CASES, IDS = m.BN_CASES, m.BN_IDS
GRAD_CASES, GRAD_IDS = m.BN_GRAD_CASES, m.BN_IDS[:len(m.BN_GRAD_CASES)]
WORST = {}  # measured worst relative error per parameter kind (printed with -s)
# what the shared bodies of tests/train_gpu_suite.py are given; this module keeps its own ``runs`` (batch_stats, OBS_SEEDS, bn_stats)
FORM = suite.Form(model=m.bn_net, label=str, gate_label=lambda case: "", tol=TOL, nonzero_scale=True, band_cap=m.BAND_CAP, e32=m.e32)


def _net_class(form):
    from occlusionenv_amd.fullnet import TrainableFullNetwork
    from occlusionenv_amd.sepfullnet import TrainableSeparableFullNetwork

    return TrainableFullNetwork if form == "dense" else TrainableSeparableFullNetwork


@pytest.fixture(scope="module")
def nets():
    """(weights, form, dilation, residual) -> (sd32, FrozenEncoder)."""
    from occlusionenv_amd.encoder import FrozenEncoder

    out = {}
    for weights, form, d, res in sorted({c[:4] for c in CASES}):
        sd32 = m.joint_state_dict(weights, form == "separable")
        enc = FrozenEncoder.from_state_dict(sd32, preset="ppo", dilation=d, residual=bool(res))
        assert enc.separable == (form == "separable") and enc.dilation == d and enc.has_decoder
        out[weights, form, d, res] = (sd32, enc)
    return out


@pytest.fixture(scope="module")
def runs(nets):
    """Per case, computed once and left unchanged: one native train-mode forward + backward with the case's randn upstream
    gradients, bn_stats, the 21 kept relu outputs, the running buffers after that step, and a fresh host model."""
    cache = {}

    def get(case):
        case = tuple(case)
        if case not in cache:
            weights, form, d, res, img, n = case
            sd32, enc = nets[case[:4]]
            obs = m.case_obs(case).float().cuda()
            net = _net_class(form).from_encoder(enc, batch_stats=True)
            assert net.batch_stats and net.training
            feats, prob = net.features_and_map(obs)
            gf, gp = m.upstream(img, n)
            net.zero_grad()
            torch.autograd.backward([feats, prob], [gf.cuda(), gp.cuda()])
            kept = [tl.kept_relu(net, i).cpu().clone() for i in range(21)]
            cache[case] = dict(enc=enc, net=net, obs=obs, feats=feats.detach().cpu(), prob=prob.detach().cpu(), gf=gf, gp=gp,
                               kept=kept, gates=[(k > 0).double() for k in kept], stats=net.bn_stats.cpu().clone(),
                               grads={k: v.cpu() for k, v in _grads(net).items()},
                               buffers={k: v.cpu().clone() for k, v in net.named_buffers() if "running_" in k},
                               host=m.HostModel(sd32, m.bn_net(case), obs.cpu()))
        return cache[case]

    return get


def _close(got, want, what):
    err = float((got.double().cpu() - want).abs().max()) / max(1.0, float(want.abs().max()))
    print(f"{what}: max|want| {float(want.abs().max()):.3g}, error {err:.3g}")
    assert got.shape == want.shape and err <= TOL, (what, err)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_against_the_f64_model(runs, case):
    r = runs(case)
    _w, _form, _d, _res, img, n = case
    host = m.plain_f64(case)[0]
    pooled, prob = host.first
    assert r["stats"].shape == (2 * tl.CHANNELS,) and r["feats"].shape == (n, 256) and r["prob"].shape == (n, 1, img, img)
    _close(r["stats"], host.packed_stats(), "bn_stats")
    _close(r["feats"], pooled, "feats")
    _close(r["prob"], prob, "prob")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kept_relu_and_gates(runs, case):
    us = m.plain_f64(case)[2]
    assert len(us) == 21
    suite.kept_relu_and_gates(FORM, runs(case), case, us)


@pytest.mark.parametrize("case", GRAD_CASES, ids=GRAD_IDS)
def test_gradients_against_f64_autograd(runs, case):
    r = runs(case)
    host = r["host"]
    pooled, prob, _pred = host.forward(r["gates"])
    want = host.grads((pooled * r["gf"].double()).sum() + (prob * r["gp"].double()).sum())
    assert len(want) == len(m.enc_keys(m.bn_net(case))) + 22 and set(want) <= set(r["grads"])
    suite.check_grads(FORM, WORST, str(case), case, r["grads"], want)


def test_gradients_through_the_real_losses(runs):
    """pretrainer.py:127-141 on net(obs) in train mode: Dice on the map plus MSE on the head's prediction."""
    from occlusionenv_amd import segmentation

    case = GRAD_CASES[0]
    _w, _form, _d, _res, img, n = case
    r = runs(case)
    net, host = r["net"], r["host"]
    gen = torch.Generator().manual_seed(m.obs_seed(img, n) + 2)
    occl = (torch.rand(n, 1, img, img, generator=gen) > 0.5).float()
    grad = torch.randn(n, 2, generator=gen) * 0.05
    net.zero_grad()
    _pooled, segm, pred = net(r["obs"])
    loss = segmentation.binary_dice_loss(segm, occl.cuda()) + F.mse_loss(pred, grad.cuda())
    loss.backward()
    got = _grads(net)
    gates = [(tl.kept_relu(net, i).cpu() > 0).double() for i in range(21)]
    _p64, prob64, pred64 = host.forward(gates)
    loss64 = _dice64(prob64, occl) + F.mse_loss(pred64, grad.double())
    want = host.grads(loss64, head=True)
    assert len(want) == len(m.enc_keys(m.bn_net(case))) + 22 + 2
    assert abs(float(loss.detach()) - float(loss64.detach())) <= TOL * max(1.0, abs(float(loss64.detach())))
    suite.check_grads(FORM, WORST, f"dice+mse {case}", case, got, want)


@pytest.mark.parametrize("case", [GRAD_CASES[0], GRAD_CASES[1]], ids=GRAD_IDS[:2])
def test_running_buffers_and_eval_mode(nets, runs, case):
    """After one train-mode step and after two the running buffers are the f64 model's; net.eval() is then the
    running-statistics step on the learned statistics, bitwise the inference of enc.with_state(net.state_dict())."""
    weights, form, d, res, img, n = case
    r = runs(case)
    sd32, enc = nets[case[:4]]
    host = m.HostModel(sd32, m.bn_net(case), r["obs"].cpu())
    with torch.no_grad():
        host.forward()
    for k, want in host.running.items():
        _close(r["buffers"][k], want, f"after one step {k}")
    assert any(not torch.equal(r["buffers"][k], sd32[k]) for k in host.running)
    net = _net_class(form).from_encoder(enc, batch_stats=True)
    obs2 = torch.roll(r["obs"], 1, 0) * 0.5
    with torch.no_grad():
        net.features_and_map(r["obs"])
        net.features_and_map(obs2)
        host.forward(obs=obs2.double().cpu())
    buffers = dict(net.named_buffers())
    for k, want in host.running.items():
        _close(buffers[k], want, f"after two steps {k}")
    net.eval()
    before = {k: v.clone() for k, v in buffers.items()}
    with torch.no_grad():
        feats, prob = net.features_and_map(r["obs"])
    assert all(torch.equal(v, before[k]) for k, v in net.named_buffers())  # eval mode moves nothing
    f2, s2, _g2 = enc.with_state(net.state_dict()).forward_full(r["obs"])
    assert torch.equal(feats, f2) and torch.equal(prob, s2)
    assert not torch.equal(prob.cpu(), r["prob"])  # the train-mode map is another one
    # and the default net never leaves the running-statistics path, whatever its mode
    plain = _net_class(form).from_encoder(enc)
    assert not plain.batch_stats
    with torch.no_grad():
        f3, s3 = plain.features_and_map(r["obs"])
    assert torch.equal(f3, enc(r["obs"])) and torch.equal(s3, enc.segment(r["obs"]))
    assert all(torch.equal(v.cpu(), sd32[k]) for k, v in plain.named_buffers() if "running_" in k)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_two_calls_give_the_same_bits(runs, case):
    r = runs(case)
    _w, form, _d, _res, _img, _n = case
    net = _net_class(form).from_encoder(r["enc"], batch_stats=True)
    feats, prob = net.features_and_map(r["obs"])
    torch.autograd.backward([feats, prob], [r["gf"].cuda(), r["gp"].cuda()])
    again = _grads(net)
    assert torch.equal(net.bn_stats.cpu(), r["stats"])
    assert torch.equal(feats.detach().cpu(), r["feats"]) and torch.equal(prob.detach().cpu(), r["prob"])
    assert len(again) == len(r["grads"]) and all(torch.equal(v.cpu(), r["grads"][k]) for k, v in again.items())
    assert all(bool(torch.isfinite(v).all()) for v in again.values())


@pytest.mark.parametrize("case", [GRAD_CASES[1], GRAD_CASES[2]], ids=GRAD_IDS[1:])
def test_nothing_outside_the_reported_sizes(runs, case):
    """The native calls on buffers of exactly the queried sizes, each the middle of a larger allocation that is inspected
    afterwards; the gradients are those of the autograd function, bitwise."""
    from occlusionenv_amd import _native as nat
    from occlusionenv_amd.encoder import FEATURES, decoder_packed_floats, packed_floats

    _w, form, _d, _res, img, n = case
    r = runs(case)
    enc, net, obs = r["enc"], r["net"], r["obs"]
    gf, gp = r["gf"].cuda(), r["gp"].cuda()
    lib, cfg, st = nat.load(), enc._cfg(img), nat.stream_ptr(obs.device)
    wsb, scb = C.c_size_t(), C.c_size_t()
    nat.check(lib.occ_fullnet_bn_train_workspace_query(C.byref(cfg), n, C.byref(wsb), C.byref(scb)), "query")
    sizes = dict(ws=int(wsb.value), scratch=int(scb.value), grad_enc=4 * packed_floats(form == "separable"),
                 grad_dec=4 * decoder_packed_floats(), prob=4 * n * img * img, feats=4 * n * FEATURES, stats=8 * tl.CHANNELS)
    assert sizes["ws"] == tl.ws_bytes(m.bn_net(case), img, n) and sizes["scratch"] == tl.scratch_bytes(m.bn_net(case), img, n)
    bufs = {k: _guarded(b) for k, b in sizes.items()}
    mid = {k: whole[lo:lo + sizes[k]] for k, (whole, lo) in bufs.items()}
    # the packed buffers of the train-mode step: gamma / beta unfolded in the scale / shift slots
    params = dict(net.named_parameters())
    packed = []
    for part in net.parts:
        layers = [tuple(params[stem + leaf].detach() for leaf in leaves) for stem, leaves in zip(part.stems, part.layer_leaves())]
        packed.append(part.pack(layers, [params[k].detach() for k in part.tail]).contiguous())
    nat.check(lib.occ_fullnet_bn_train_forward(C.byref(cfg), nat.ptr(packed[0]), nat.ptr(packed[1]), nat.ptr(obs), n,
                                               nat.ptr(mid["ws"]), sizes["ws"], nat.ptr(mid["feats"]), nat.ptr(mid["prob"]),
                                               nat.ptr(mid["stats"]), st), "occ_fullnet_bn_train_forward")
    nat.check(lib.occ_fullnet_bn_backward(C.byref(cfg), nat.ptr(packed[0]), nat.ptr(packed[1]), n, nat.ptr(mid["ws"]), sizes["ws"],
                                          nat.ptr(gf), nat.ptr(gp), nat.ptr(mid["scratch"]), sizes["scratch"],
                                          nat.ptr(mid["grad_enc"]), nat.ptr(mid["grad_dec"]), st), "occ_fullnet_bn_backward")
    torch.cuda.synchronize()
    assert torch.equal(mid["stats"].view(torch.float32).cpu(), r["stats"])
    assert torch.equal(mid["feats"].view(torch.float32).view(n, FEATURES).cpu(), r["feats"])
    assert torch.equal(mid["prob"].view(torch.float32).view(n, 1, img, img).cpu(), r["prob"])
    packed_grads = [mid[key].view(torch.float32) for key in ("grad_enc", "grad_dec")]
    # d gamma / d beta sit in the scale / shift slots as they are
    assert suite.packed_gradients_are_the_modules(net, packed_grads, r["grads"], folded=False) == len(m.enc_keys(m.bn_net(case))) + 22
    guards_intact(bufs, sizes)


def test_batch_coupling_and_the_one_value_limit(nets, runs):
    """In train mode another env's observation changes an env's map; in eval mode it does not.  One value per channel
    (N = 1 at S = 32) raises as PyTorch does."""
    case = GRAD_CASES[0]
    r = runs(case)
    net = _net_class(case[1]).from_encoder(r["enc"], batch_stats=True)
    obs2 = r["obs"].clone()
    obs2[0] = torch.flip(obs2[0], (1,)) * 0.25
    with torch.no_grad():
        a, b = net.features_and_map(r["obs"])[1], net.features_and_map(obs2)[1]
        assert not torch.equal(a[1], b[1]) and not torch.equal(a[2], b[2])
        net.eval()
        a, b = net.features_and_map(r["obs"])[1], net.features_and_map(obs2)[1]
        assert torch.equal(a[1:], b[1:]) and not torch.equal(a[0], b[0])
        net.train()
        with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
            net.features_and_map(r["obs"][:1, :, :32, :32].contiguous())
        net.features_and_map(r["obs"][:2, :, :32, :32].contiguous())  # two values are enough
        net.eval()
        net.features_and_map(r["obs"][:1, :, :32, :32].contiguous())  # the running-statistics step has no such limit


def test_pretrain_epoch_with_batch_stats(nets):
    """harness.pretrain_epoch(enc, two batches of 3 x 64^2, batch_stats=True): its mean losses are those of the same two
    AdamW steps (Dice + MSE) taken in f64 on the host model, within 1e-4 max(1, |want|), and the running statistics it
    leaves are no longer the checkpoint's."""
    from occlusionenv_amd import harness
    from tests.encoder_model import make_obs

    weights, form, d, res = "golden", "separable", 2, 1
    sd32, enc = nets[weights, form, d, res]
    n, img = 3, 64
    gen = torch.Generator().manual_seed(78)
    batches = []
    for b in range(2):
        occl = (torch.rand(n, 1, img // 8, img // 8, generator=gen) > 0.5).float().repeat_interleave(8, 2).repeat_interleave(8, 3)
        batches.append((make_obs(600 + b, n, img).float(), occl, torch.randn(n, 2, generator=gen) * 0.5, None))
    res_ = harness.pretrain_epoch(enc, batches, batch_stats=True)
    net = res_["net"]
    assert isinstance(net, _net_class(form)) and net.batch_stats and res_["batches"] == 2
    host = m.HostModel(sd32, m.Net("ppo", True, d, bool(res), True, True), batches[0][0])
    opt = torch.optim.AdamW(list(host.params.values()), lr=1e-3, weight_decay=1e-5)
    rows = []
    for obs, occl, grad, _ in batches:
        opt.zero_grad()
        _pooled, prob, pred = host.forward(obs=obs.double())
        segm_loss, grad_loss = _dice64(prob, occl), F.mse_loss(pred, grad.double())
        (segm_loss + grad_loss).backward()
        opt.step()
        rows.append((float((segm_loss + grad_loss).detach()), float(segm_loss.detach()), float(grad_loss.detach())))
    for i, k in enumerate(("loss", "segm_loss", "grad_loss")):
        want = sum(row[i] for row in rows) / len(rows)
        print(f"{k}: {res_[k]:.8g} against {want:.8g}")
        assert res_[k] == res_[k] and abs(res_[k]) < float("inf")
        assert abs(res_[k] - want) <= TOL * max(1.0, abs(want)), k
    buffers = {k: v.cpu() for k, v in net.named_buffers() if "running_" in k}
    assert len(buffers) == 42 and all(not torch.equal(v, sd32[k]) for k, v in buffers.items())
    for k, want in host.running.items():
        _close(buffers[k], want, f"after the epoch {k}")
    # the learned statistics reach inference
    trained = enc.with_state(net.state_dict())
    net.eval()
    with torch.no_grad():
        feats, prob = net.features_and_map(batches[0][0].cuda())
    assert torch.equal(trained(batches[0][0].cuda()), feats) and torch.equal(trained.segment(batches[0][0].cuda()), prob)
