"""GPU tests of the native joint backward (csrc/occ_fullnet_bwd.hpp, occlusionenv_amd/fullnet.py, harness.pretrain_epoch)
against tests/fullnet_train_model.py in f64 on the CPU with torch autograd.

Weights: fullnet_train_model.state_dict rounded to f32 (what a checkpoint on disk holds), used as exactly those values in
f64 by the host model.  Inputs: encoder_model.make_obs.  Upstream: a randn grad_feats and a randn grad_prob together.

Shapes: S=32 N=2 (the deepest decoder plane is 1 x 1: the new input gradient of the deepest level), S=64 N=3, S=96 N=2 (sides
96 / 48 / 24 / 12 / 6 / 3), presets "ppo" and "segmenter", residual 1 and 0.  Split cases: "ppo" 129 x 32^2 (the encoder's)
and "ppo" 65 x 96^2 (the decoder's), where the dW slices span several tiles and cross env boundaries on both sides
(asserted below from the two split models), also with both upstream gradients non-zero in one env alone.

Bar: per tensor max |got - want| <= 1e-4 max |want| (no floor), the oracle evaluated with the GPU's own 21 gates
(relu(u) replaced by u * gate), as in the encoder's and the decoder's tests.

Every gradient test prints its relative errors and the worst so far per parameter kind (``-s``); DESIGN.md section 4.4,
"Joint training", is where measured figures are recorded."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import decoder_split_model as dsm
from tests import encoder_train_model as etm
from tests import fullnet_train_model as m
from tests.encoder_model import make_obs
from tests.train_utils import GUARD
from tests.train_utils import bce64 as _bce64
from tests.train_utils import dice64 as _dice64
from tests.train_utils import grads as _grads
from tests.train_utils import guarded as _guarded

pytestmark = pytest.mark.gpu

TOL = 1e-4
CASES = m.GRAD_CASES + m.SPLIT_CASES
IDS = [f"{p}-res{r}-S{s}-N{n}" for p, r, s, n in CASES]
WORST = {}  # measured worst relative error per parameter kind (printed with -s)


def _seed(img, n):
    return 9000 + img + n


@pytest.fixture(scope="module")
def nets():
    from occlusionenv_amd.encoder import FrozenEncoder

    out = {}
    for preset in m.PRESETS:
        sd32 = {k: v.float() for k, v in m.state_dict(preset).items()}
        sd64 = {k: v.double() for k, v in sd32.items()}
        for residual in (1, 0):
            out[preset, residual] = (sd32, sd64, FrozenEncoder.from_state_dict(sd32, preset=preset, dilation=1, residual=bool(residual)))
    return out


def _gates(net):
    return [(m.kept_relu(net, i).cpu() > 0).double() for i in range(21)]


@pytest.fixture(scope="module")
def runs(nets):
    """Per case, computed once and left unchanged: one native forward + backward with seeded randn upstream gradients, the
    gates of the 21 kept relu outputs, and the host model."""
    from occlusionenv_amd.fullnet import TrainableFullNetwork

    cache = {}

    def get(preset, residual, img, n):
        key = (preset, residual, img, n)
        if key not in cache:
            _sd32, sd64, enc = nets[preset, residual]
            obs64 = make_obs(_seed(img, n), n, img)
            obs = obs64.float().cuda()
            net = TrainableFullNetwork.from_encoder(enc)
            feats, prob = net.features_and_map(obs)
            gen = torch.Generator().manual_seed(_seed(img, n) + 1)
            gf, gp = torch.randn(n, 256, generator=gen), torch.randn(n, 1, img, img, generator=gen)
            net.zero_grad()
            torch.autograd.backward([feats, prob], [gf.cuda(), gp.cuda()])
            cache[key] = dict(enc=enc, net=net, obs=obs, feats=feats.detach(), prob=prob.detach(), gf=gf, gp=gp, gates=_gates(net),
                              grads={k: v.cpu() for k, v in _grads(net).items()},
                              host=m.HostModel(sd64, preset, residual, obs.double().cpu()))
        return cache[key]

    return get


def _check_grads(what, preset, got, want):
    for k, w in want.items():
        scale = float(w.abs().max())
        err = float((got[k].double().cpu() - w).abs().max()) / scale
        WORST[m.kind(preset, k)] = max(WORST.get(m.kind(preset, k), 0.0), err)
        print(f"{what} {k}: max|want| {scale:.3g}, relative error {err:.3g}")
    for k, w in want.items():
        assert got[k].shape == w.shape and got[k].dtype == torch.float32
        assert float((got[k].double().cpu() - w).abs().max()) <= TOL * float(w.abs().max()), (what, k)
    print("worst so far:", {k: f"{v:.3g}" for k, v in sorted(WORST.items())})


def test_split_cases_reach_the_tile_loops_on_both_sides():
    """What the split cases have to reach, from the two split models alone: at least two tiles per slice in some encoder
    layer and in some decoder level of each, slices that cross env boundaries on both sides, and a short last slice."""
    for _p, _r, img, n in m.SPLIT_CASES:
        enc, dec = etm.dw_plans(img, n), dsm.dw_plans(img, n)
        assert max(p["tps"] for p in enc) >= 2 and max(p["tps"] for p in dec) >= 2, (img, n)
        assert any(p["tps"] >= 2 and p["straddles"] for p in enc) and any(p["short_last"] for p in enc)
        # a decoder slice of more tiles than an env has crosses env boundaries whatever its start
        assert any(p["tps"] >= 2 and (p["straddles"] or p["tps"] > p["tiles_env"]) for p in dec)
    assert [p["tps"] for p in etm.dw_plans(32, 129)] == [5, 5, 5, 2, 2, 2, 1, 1, 1, 1, 1, 1, 2, 3, 3, 5]
    assert [p["tps"] for p in dsm.dw_plans(32, 129)] == [3, 1, 1, 1, 2]
    assert [p["tps"] for p in etm.dw_plans(96, 65)] == [19, 19, 19, 5, 5, 5, 2, 2, 2, 2, 3, 3, 3, 5, 5, 3]
    assert [p["tps"] for p in dsm.dw_plans(96, 65)] == [2, 2, 2, 2, 5]
    assert any(p["short_last"] for p in dsm.dw_plans(96, 65)) and sum(p["straddles"] for p in dsm.dw_plans(96, 65)) == 3


@pytest.mark.parametrize("preset,residual,img,n", CASES, ids=IDS)
def test_forward_identity(runs, preset, residual, img, n):
    r = runs(preset, residual, img, n)
    assert r["feats"].shape == (n, 256) and r["prob"].shape == (n, 1, img, img)
    assert torch.equal(r["feats"], r["enc"](r["obs"]))
    assert torch.equal(r["prob"], r["enc"].segment(r["obs"]))


@pytest.mark.parametrize("preset,residual,img,n", CASES, ids=IDS)
def test_gradients_against_f64_autograd(runs, preset, residual, img, n):
    r = runs(preset, residual, img, n)
    host = r["host"]
    pooled, prob, _pred = host.forward(r["gates"])
    want = host.grads((pooled * r["gf"].double()).sum() + (prob * r["gp"].double()).sum())
    assert len(want) == 86 and set(want) <= set(r["grads"])
    _check_grads(f"{preset} res{residual} S={img} N={n}", preset, r["grads"], want)


@pytest.mark.parametrize("losses", ["dice+mse", "bce+smoothl1"])
def test_gradients_through_the_real_losses(runs, losses):
    """pretrainer.py:127-131 on net(obs): the segmentation loss plus the gradient loss on the head, 88 parameters."""
    from occlusionenv_amd import segmentation

    preset, residual, img, n = "ppo", 1, 64, 3
    r = runs(preset, residual, img, n)
    net, host = r["net"], r["host"]
    gen = torch.Generator().manual_seed(_seed(img, n) + 2)
    occl = (torch.rand(n, 1, img, img, generator=gen) > 0.5).float()
    grad = torch.randn(n, 2, generator=gen) * 0.05  # both sides of SmoothL1's beta = 0.01
    net.zero_grad()
    _pooled, segm, pred = net(r["obs"])
    if losses == "dice+mse":
        loss = segmentation.binary_dice_loss(segm, occl.cuda()) + F.mse_loss(pred, grad.cuda())
    else:
        loss = segmentation.binary_cross_entropy(segm, occl.cuda()) + F.smooth_l1_loss(pred, grad.cuda(), beta=0.01)
    loss.backward()
    got = _grads(net)
    _p64, prob64, pred64 = host.forward(_gates(net))
    if losses == "dice+mse":
        loss64 = _dice64(prob64, occl) + F.mse_loss(pred64, grad.double())
    else:
        loss64 = _bce64(prob64, occl) + F.smooth_l1_loss(pred64, grad.double(), beta=0.01)
    want = host.grads(loss64, head=True)
    assert len(want) == 88
    assert abs(float(loss.detach()) - float(loss64.detach())) <= TOL * max(1.0, abs(float(loss64.detach())))
    _check_grads(f"{losses} {preset} S={img} N={n}", preset, got, want)


@pytest.mark.parametrize("which", ["last", "one"])
@pytest.mark.parametrize("preset,residual,img,n", m.SPLIT_CASES, ids=IDS[-2:])
def test_gradients_of_one_env(runs, preset, residual, img, n, which):
    """Both upstream gradients are randn in one env and zero in the others: a tile given to the wrong env or dropped from a
    short last slice is the whole signal."""
    env = n - 1 if which == "last" else 1
    r = runs(preset, residual, img, n)
    net, host = r["net"], r["host"]
    gen = torch.Generator().manual_seed(_seed(img, n) + 3 + env)
    gf, gp = torch.zeros(n, 256), torch.zeros(n, 1, img, img)
    gf[env], gp[env] = torch.randn(256, generator=gen), torch.randn(1, img, img, generator=gen)
    net.zero_grad()
    feats, prob = net.features_and_map(r["obs"])
    assert torch.equal(prob.detach(), r["prob"])
    torch.autograd.backward([feats, prob], [gf.cuda(), gp.cuda()])
    pooled64, prob64, _pred = host.forward(_gates(net))
    want = host.grads((pooled64 * gf.double()).sum() + (prob64 * gp.double()).sum())
    _check_grads(f"env {env} alone {preset} S={img} N={n}", preset, _grads(net), want)


@pytest.mark.parametrize("preset,residual,img,n", [("ppo", 1, 32, 2), ("ppo", 1, 96, 2), ("segmenter", 0, 64, 3)])
def test_the_join_itself(runs, preset, residual, img, n):
    """grad_feats = 0: whatever reaches the encoder came through the decoder's skip and input gradients."""
    r = runs(preset, residual, img, n)
    net, host = r["net"], r["host"]
    net.zero_grad()
    _feats, prob = net.features_and_map(r["obs"])
    prob.backward(r["gp"].cuda())  # the absent gradient of feats arrives as zeros
    got = _grads(net)
    assert all(float(got[k].abs().max()) > 0.0 for k in m.enc_keys(preset))
    _pooled64, prob64, _pred = host.forward(_gates(net))
    want = host.grads((prob64 * r["gp"].double()).sum())
    _check_grads(f"join {preset} res{residual} S={img} N={n}", preset, got, want)


@pytest.mark.parametrize("preset,residual,img,n", [("ppo", 1, 64, 3), ("segmenter", 0, 96, 2), ("ppo", 1, 32, 129)])
def test_bitwise_against_the_two_single_passes(runs, preset, residual, img, n):
    from occlusionenv_amd.enctrain import TrainableEncoder
    from occlusionenv_amd.seghead import SegmentationHead

    r = runs(preset, residual, img, n)
    net, enc, obs = r["net"], r["enc"], r["obs"]
    # the decoder and classifier gradients are SegmentationHead's for the same grad_prob, whatever grad_feats is
    head = SegmentationHead.from_encoder(enc)
    head(obs).backward(r["gp"].cuda())
    hg = _grads(head)
    assert len(hg) == 22 and all(torch.equal(v.cpu(), r["grads"][k]) for k, v in hg.items())
    # with grad_prob = 0 the encoder gradients are TrainableEncoder's
    tenc = TrainableEncoder.from_encoder(enc)
    tenc(obs).backward(r["gf"].cuda())
    eg = {k: v for k, v in _grads(tenc).items() if k in m.enc_keys(preset)}
    net.zero_grad()
    feats, _prob = net.features_and_map(obs)
    feats.backward(r["gf"].cuda())
    got = _grads(net)
    assert len(eg) == 64 and all(torch.equal(v, got[k]) for k, v in eg.items())
    assert all(float(got[k].abs().max()) == 0.0 for k in m.dec_keys(preset))
    # two backward calls give the same bits
    net.zero_grad()
    feats, prob = net.features_and_map(obs)
    torch.autograd.backward([feats, prob], [r["gf"].cuda(), r["gp"].cuda()])
    again = _grads(net)
    assert len(again) >= 86 and all(torch.equal(v.cpu(), r["grads"][k]) for k, v in again.items())


@pytest.mark.parametrize("preset,residual,img,n", [("ppo", 1, 96, 2), ("ppo", 1, 32, 129)])
def test_no_stale_reads_and_nothing_outside_the_reported_sizes(runs, preset, residual, img, n):
    """The native calls on buffers of exactly the queried sizes, each the middle of a larger allocation that is inspected
    afterwards; then the backward again after everything it may only write (scratch, the gradient part of the workspace,
    both gradient outputs) and the forward's outputs feats and prob, which it must neither read nor write, have been filled
    with NaNs: the same bits."""
    from occlusionenv_amd import _native as nat
    from occlusionenv_amd.encoder import FEATURES, decoder_packed_floats, packed_floats

    r = runs(preset, residual, img, n)
    enc, obs = r["enc"], r["obs"]
    gf, gp = r["gf"].cuda(), r["gp"].cuda()
    lib, cfg, st = nat.load(), enc._cfg(img), nat.stream_ptr(obs.device)
    wsb, scb = C.c_size_t(), C.c_size_t()
    nat.check(lib.occ_fullnet_train_workspace_query(C.byref(cfg), n, C.byref(wsb), C.byref(scb)), "occ_fullnet_train_workspace_query")
    sizes = dict(ws=int(wsb.value), scratch=int(scb.value), grad_enc=4 * packed_floats(False), grad_dec=4 * decoder_packed_floats(),
                 prob=4 * n * img * img, feats=4 * n * FEATURES)
    assert sizes["ws"] == m.ws_bytes(img, n) and sizes["scratch"] == m.scratch_bytes(img, n)
    bufs = {k: _guarded(b) for k, b in sizes.items()}
    mid = {k: whole[lo:lo + sizes[k]] for k, (whole, lo) in bufs.items()}
    assert all(v.data_ptr() % 256 == 0 for v in mid.values())

    def backward():
        nat.check(lib.occ_fullnet_backward(C.byref(cfg), nat.ptr(enc.packed), nat.ptr(enc.dec_packed), n, nat.ptr(mid["ws"]),
                                           sizes["ws"], nat.ptr(gf), nat.ptr(gp), nat.ptr(mid["scratch"]), sizes["scratch"],
                                           nat.ptr(mid["grad_enc"]), nat.ptr(mid["grad_dec"]), st), "occ_fullnet_backward")
        return mid["grad_enc"].view(torch.float32).clone(), mid["grad_dec"].view(torch.float32).clone()

    nat.check(lib.occ_fullnet_train_forward(C.byref(cfg), nat.ptr(enc.packed), nat.ptr(enc.dec_packed), nat.ptr(obs), n,
                                            nat.ptr(mid["ws"]), sizes["ws"], nat.ptr(mid["feats"]), nat.ptr(mid["prob"]), st),
              "occ_fullnet_train_forward")
    prob, feats = mid["prob"].clone(), mid["feats"].clone()
    assert torch.equal(prob.view(torch.float32).view(n, 1, img, img), r["prob"])
    assert torch.equal(feats.view(torch.float32).view(n, FEATURES), r["feats"])
    a = backward()
    nan = 0x7FC00000
    # what the backward only writes: g0 | g1 | g2 at the end of the encoder's part, dlast | dskip at the end of the workspace
    buf = dsm.align(4 * n * 8 * img * img)
    e_end = m.encoder_ws_bytes(img, n)
    mid["ws"][e_end - 3 * buf:e_end].view(torch.int32).fill_(nan)
    tail = dsm.align(4 * n * 256 * (img // 32) ** 2) + sum(dsm.level_bytes(img, n)[:4])
    mid["ws"][sizes["ws"] - tail:].view(torch.int32).fill_(nan)
    for k in ("scratch", "grad_enc", "grad_dec", "feats", "prob"):  # the outputs too: the backward reads the prob kept in ws
        mid[k].view(torch.int32).fill_(nan)
    b = backward()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in a)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    assert bool((mid["prob"].view(torch.int32) == nan).all()) and bool((mid["feats"].view(torch.int32) == nan).all())  # writes neither
    # the same bits as through the autograd function
    from occlusionenv_amd.enctrain import unpack_encoder_buffer
    from occlusionenv_amd.seghead import unpack_decoder_buffer

    ek, dk = m.enc_keys(preset), m.dec_keys(preset)
    for i, layer in enumerate(unpack_encoder_buffer(a[0])):
        assert torch.equal(layer[0].cpu(), r["grads"][ek[4 * i]]) and torch.equal(layer[1].cpu(), r["grads"][ek[4 * i + 1]])
    levels, dcw, dcb = unpack_decoder_buffer(a[1])
    for j, level in enumerate(levels):
        assert torch.equal(level[0].cpu(), r["grads"][dk[4 * j]]) and torch.equal(level[1].cpu(), r["grads"][dk[4 * j + 1]])
    assert torch.equal(dcw.cpu(), r["grads"][dk[-2]]) and torch.equal(dcb.cpu(), r["grads"][dk[-1]])
    for k, (whole, lo) in bufs.items():
        assert lo >= GUARD and whole.numel() - (lo + sizes[k]) >= GUARD
        assert bool((whole[:lo] == 0xA5).all()), f"bytes in front of {k} were written"
        assert bool((whole[lo + sizes[k]:] == 0xA5).all()), f"bytes behind {k} were written"


def test_errors(nets, runs):
    from occlusionenv_amd._native import NativeError
    from occlusionenv_amd.encoder import FrozenEncoder
    from occlusionenv_amd.fullnet import TrainableFullNetwork
    from tests.segmenter_model import golden_seg_state_dict

    import numpy as np

    sd32, _sd64, enc = nets["ppo", 1]
    r = runs("ppo", 1, 64, 3)
    net = r["net"]
    with pytest.raises(ValueError, match="dilation 1 only"):
        TrainableFullNetwork.from_encoder(FrozenEncoder.from_state_dict(sd32, preset="ppo"))  # the preset's dilation 2
    sep = {k: v.float() for k, v in golden_seg_state_dict(np.load(m.GOLDEN), "ppo").items()}
    with pytest.raises(ValueError, match="dense 3x3 convs only"):
        TrainableFullNetwork.from_encoder(FrozenEncoder.from_state_dict(sep, preset="ppo", dilation=1))
    bare = FrozenEncoder.from_state_dict({k: v for k, v in sd32.items() if not k.startswith("segmenter.")}, preset="ppo", dilation=1)
    with pytest.raises(ValueError, match="no segmentation decoder"):
        TrainableFullNetwork.from_encoder(bare)
    enc.max_chunk = 2
    try:
        with pytest.raises(ValueError, match="max_chunk"):
            net(r["obs"])
    finally:
        enc.max_chunk = 256
    with pytest.raises(ValueError, match="multiple of 32"):
        net(torch.zeros(1, 4, 48, 48, device="cuda"))
    with pytest.raises(NativeError):
        net(torch.zeros(1, 4, 64, 64))
    first = net.features_and_map(r["obs"])
    second = net.features_and_map(r["obs"][:1])
    with pytest.raises(RuntimeError, match="superseded"):
        (first[0].sum() + first[1].sum()).backward()
    net.zero_grad()
    (second[0].sum() + second[1].sum()).backward()  # the latest forward still has its activations
    assert all(p.grad is not None for _k, p in net.ordered_parameters())
    # "segmenter": Segmenter.forward's pair without the decoder feature
    seg = TrainableFullNetwork.from_encoder(nets["segmenter", 1][2])
    none, prob = seg(r["obs"])
    assert none is None and prob.shape == (3, 1, 64, 64) and prob.requires_grad and not seg.has_grad_head


@pytest.fixture(scope="module")
def trained(nets):
    """Forty AdamW steps at lr 1e-3 on a fixed batch (N=4, S=64), Dice + MSE as in pretrainer.py."""
    from occlusionenv_amd import segmentation
    from occlusionenv_amd.fullnet import TrainableFullNetwork

    enc = nets["ppo", 1][2]
    n, img = 4, 64
    obs = make_obs(_seed(img, n), n, img).float().cuda()
    gen = torch.Generator().manual_seed(_seed(img, n) + 5)
    occl = (torch.rand(n, 1, img // 8, img // 8, generator=gen) > 0.5).float().repeat_interleave(8, 2).repeat_interleave(8, 3).cuda()
    grad = (torch.randn(n, 2, generator=gen) * 0.5).cuda()
    net = TrainableFullNetwork.from_encoder(enc)
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-5)
    losses = []
    for _ in range(41):  # forty steps, and the loss after the fortieth
        opt.zero_grad()
        _pooled, segm, pred = net(obs)
        loss = segmentation.binary_dice_loss(segm, occl) + F.mse_loss(pred, grad)
        losses.append(loss.detach())
        if len(losses) <= 40:
            loss.backward()
            opt.step()
    return dict(net=net, enc=enc, obs=obs, before=before, losses=torch.stack(losses).cpu().tolist())


def test_learning(trained):
    losses = trained["losses"]
    print("Dice + MSE:", [f"{v:.4f}" for v in losses[::5]])
    assert all(v == v for v in losses) and losses[-1] < losses[0]
    assert all(not torch.equal(v, trained["before"][k]) for k, v in trained["net"].named_parameters())


def test_round_trip_into_a_frozen_encoder(trained):
    net, enc, obs = trained["net"], trained["enc"], trained["obs"]
    sd = net.state_dict()
    assert len(sd) == 16 * 6 + 5 * 6 + 2 + 2 and "segmenter.0.features.0.up.conv.weight" in sd and "gradPredictor.bias" in sd
    tuned = enc.with_encoder(sd).with_decoder(sd)
    with torch.no_grad():
        pooled, segm, pred = net(obs)
    f2, s2, g2 = tuned.forward_full(obs)
    assert torch.equal(f2, pooled) and torch.equal(s2, segm)
    assert torch.allclose(g2, pred, rtol=1e-5, atol=1e-6)  # addmm against F.linear
    both = enc.with_state(sd)
    assert torch.equal(both.segment(obs), segm) and torch.equal(both(obs), pooled)
    assert not torch.equal(enc.segment(obs), segm) and not torch.equal(enc(obs), pooled)  # the source is left as it is


def test_pretrain_epoch(nets):
    from occlusionenv_amd import harness, segmentation
    from occlusionenv_amd.fullnet import TrainableFullNetwork

    enc = nets["ppo", 1][2]
    n, img = 4, 64
    gen = torch.Generator().manual_seed(77)
    batches = []
    for b in range(3):
        occl = (torch.rand(n, 1, img // 8, img // 8, generator=gen) > 0.5).float().repeat_interleave(8, 2).repeat_interleave(8, 3)
        batches.append((make_obs(500 + b, n, img).float(), occl, torch.randn(n, 2, generator=gen) * 0.5, None))
    # the predictions each step learns from, by the same steps taken by hand
    ref = TrainableFullNetwork.from_encoder(enc)
    opt = torch.optim.AdamW(ref.parameters(), lr=1e-3, weight_decay=1e-5)
    acc, iou = [], []
    for obs, occl, grad, _ in batches:
        opt.zero_grad()
        _pooled, segm, pred = ref(obs.cuda())
        (segmentation.binary_dice_loss(segm, occl.cuda()) + F.mse_loss(pred, grad.cuda())).backward()
        opt.step()
        c = segmentation.seg_criterion(segm.detach(), occl.cuda())
        acc.append(float(c["correct"].sum()) / segm.numel())
        iou.append(float(c["intersection"].sum()) / float(c["union"].sum()))
    res = harness.pretrain_epoch(enc, batches)
    assert isinstance(res["net"], TrainableFullNetwork) and res["batches"] == 3 and res["pixels"] == 3 * n * img * img
    for k in ("loss", "segm_loss", "grad_loss", "accuracy", "iou"):
        assert res[k] == res[k] and abs(res[k]) < float("inf"), k
    assert abs(res["loss"] - (res["segm_loss"] + res["grad_loss"])) <= 1e-6
    assert abs(res["accuracy"] - 100.0 * sum(acc) / 3) <= 1e-9 and abs(res["iou"] - 100.0 * sum(iou) / 3) <= 1e-9
    assert all(torch.equal(v, dict(ref.named_parameters())[k]) for k, v in res["net"].named_parameters())
    res2 = harness.pretrain_epoch(res["net"], batches, use_dice=False, use_l1=True, optimizer=res["optimizer"])
    assert res2["net"] is res["net"] and all(res2[k] == res2[k] for k in ("loss", "segm_loss", "grad_loss", "accuracy", "iou"))
