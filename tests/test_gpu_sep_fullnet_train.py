"""GPU tests of the native joint backward of the separable network (csrc/occ_fullnet_bwd.hpp,
occlusionenv_amd/sepfullnet.py, harness.pretrain_epoch) against tests/sep_fullnet_train_model.py in f64 on the CPU with torch
autograd.

Weights, rounded to f32 (what a checkpoint on disk holds) and used as exactly those values in f64 by the host model:
"golden" = the fixture tests/golden/segmenter_golden.npz ("ppo" keys), the reference's own FullNetwork(8, dilation=2,
separable=True) with its decoder, run at dilation 2 with the residual and once at dilation 1; "seeded" =
sep_fullnet_train_model.seeded_state_dict, at dilation 2 without the residual.  Inputs: encoder_model.make_obs.  Upstream: a
randn grad_feats and a randn grad_prob together.

Shapes: S=32 N=2 (the deepest plane is 1 x 1, a dilation-2 halo there is all padding, and Ho = 16 is the smallest side the
level-0 join variant accepts), S=64 N=3, S=96 N=2.  Split cases: 130 x 64^2 (the pointwise weight gradient runs 3 tiles per
slice on the initial layer and on both layers of levels 0 and 1, the level-0 down 5, slices crossing env boundaries, a last
slice of one tile) and 65 x 96^2 (the decoder's split shape; the separable layers of levels 3 and 4 straddle envs too), both
asserted without a GPU in tests/test_sep_fullnet_train_host.py, also with both upstream gradients non-zero in one env alone.

Bars (those of the existing training tests).  Gradients: per tensor max |got - want| <= 1e-4 max |want| (no floor; no
wanted tensor is all zero), the oracle evaluated with the GPU's own 21 gates (relu(u) replaced by u * gate).  Kept relu
outputs: within 1e-4 max(1, max |r64|) of the f64 relu(u).  Gates r > 0: may differ from the f64 gate only where
|u64| <= 1e-4 max(1, max |u64|); that band holds at most 1 % of any layer's pixels (asserted here; at most 0.5 % by the
host test, from the model alone).

Every gradient test prints its relative errors and the worst so far per parameter kind (``-s``); DESIGN.md section 4.4,
"Joint training of the separable network", is where measured figures are recorded.

Measured on an MI355X against the f64 model (worst relative error per parameter kind; the bar is 1e-4; "encoder" = the
separable layers, "down" = the dense downs):
                     enc conv.0.w conv.1.w conv.2.w conv.2.b bn.w    bn.b  | down conv.w conv.b bn.w    bn.b  | dec conv.w conv.b bn.w    bn.b  | cls w    cls b
  golden, both grads   7.7e-7   7.5e-7   1.0e-6   4.7e-7   6.6e-7  5.9e-7 |  5.5e-7    4.9e-7  6.3e-7  5.0e-7 |  8.7e-7   8.8e-7  8.6e-7  6.9e-7 | 3.0e-7  3.1e-7
  seeded, both grads   8.3e-6   7.4e-6   1.2e-5   8.7e-6   1.7e-5  1.1e-5 |  6.7e-6    6.8e-6  7.0e-6  1.3e-5 |  1.1e-5   2.5e-5  1.6e-5  2.1e-5 | 1.0e-5  4.3e-6
  real losses          4.8e-7   5.9e-7   6.2e-7   5.2e-7   3.0e-7  4.2e-7 |  3.7e-7    2.6e-7  5.4e-7  4.0e-7 |  8.3e-7   3.5e-7  4.1e-7  3.3e-7 | 6.1e-8  8.8e-9   (head w 2.9e-7, b 5.0e-8)
  the join itself      5.8e-5   3.6e-5   3.2e-5   6.3e-5   4.7e-5  5.2e-5 |  4.7e-5    3.5e-5  3.6e-5  6.7e-5 |  1.1e-5   2.5e-5  1.6e-5  2.1e-5 | 1.0e-5  4.3e-6
  split cases          7.8e-7   1.7e-6   1.3e-6   7.4e-7   1.1e-6  1.1e-6 |  6.8e-7    5.6e-7  5.8e-7  2.9e-7 |  1.0e-6   9.3e-7  6.5e-7  5.2e-7 | 6.4e-8  9.1e-9
  one env alone        8.0e-7   7.8e-7   1.0e-6   9.4e-7   1.0e-6  7.4e-7 |  4.6e-7    6.3e-7  7.1e-7  6.1e-7 |  8.4e-7   5.7e-7  9.5e-7  6.0e-7 | 2.0e-7  1.9e-7
Every figure above 2.5e-5 belongs to the seeded weights at S=64 N=3 with grad_feats absent (the golden join cases stay below
1.1e-6): those weights were fixed before the first run and are kept.  Kept relu outputs: 2.0e-6; no gate differed from the
f64 gate in any case; worst band share 0.24 %.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import decoder_split_model as dsm
from tests import sep_fullnet_train_model as m
from tests.train_utils import GUARD
from tests.train_utils import bce64 as _bce64
from tests.train_utils import dice64 as _dice64
from tests.train_utils import grads as _grads
from tests.train_utils import guarded as _guarded

pytestmark = pytest.mark.gpu

TOL = m.TOL
BAND_CAP = 0.01
CASES = m.CASES
IDS = [f"{w}-d{d}-res{r}-S{s}-N{n}" for w, d, r, s, n in CASES]
SPLIT_IDS = IDS[len(m.GRAD_CASES):]
WORST = {}  # measured worst relative error per parameter kind (printed with -s)
N_ENC, N_DEC = 11 * 6 + 5 * 4, 22


@pytest.fixture(scope="module")
def nets():
    """(weights, dilation, residual) -> (sd32, FrozenEncoder)."""
    from occlusionenv_amd.encoder import FrozenEncoder

    out = {}
    for weights, d, res in sorted({c[:3] for c in CASES}):
        sd32 = m.state_dict(weights)
        enc = FrozenEncoder.from_state_dict(sd32, preset="ppo", dilation=d, residual=bool(res))
        assert enc.separable and enc.dilation == d and enc.residual == bool(res) and enc.has_decoder
        out[weights, d, res] = (sd32, enc)
    return out


def _kept(net):
    return [m.kept_relu(net, i).cpu().clone() for i in range(21)]


def _gates(net):
    return [(m.kept_relu(net, i).cpu() > 0).double() for i in range(21)]


@pytest.fixture(scope="module")
def runs(nets):
    """Per case, computed once and left unchanged: one native forward + backward with seeded randn upstream gradients, the
    21 kept relu outputs, and the host model."""
    from occlusionenv_amd.sepfullnet import TrainableSeparableFullNetwork

    cache = {}

    def get(weights, d, res, img, n):
        key = (weights, d, res, img, n)
        if key not in cache:
            sd32, enc = nets[weights, d, res]
            obs = m.case_obs(img, n).float().cuda()
            net = TrainableSeparableFullNetwork.from_encoder(enc)
            feats, prob = net.features_and_map(obs)
            gen = torch.Generator().manual_seed(m.obs_seed(img, n) + 1)
            gf, gp = torch.randn(n, 256, generator=gen), torch.randn(n, 1, img, img, generator=gen)
            net.zero_grad()
            torch.autograd.backward([feats, prob], [gf.cuda(), gp.cuda()])
            kept = _kept(net)
            cache[key] = dict(enc=enc, net=net, obs=obs, feats=feats.detach(), prob=prob.detach(), gf=gf, gp=gp, kept=kept,
                              gates=[(k > 0).double() for k in kept], grads={k: v.cpu() for k, v in _grads(net).items()},
                              host=m.HostModel(sd32, d, res, obs.double().cpu()))
        return cache[key]

    return get


def _check_grads(what, got, want):
    for k, w in want.items():
        scale = float(w.abs().max())
        assert scale > 0.0, (what, k, "the oracle's gradient is all zero")
        err = float((got[k].double().cpu() - w).abs().max()) / scale
        WORST[m.kind(k)] = max(WORST.get(m.kind(k), 0.0), err)
        print(f"{what} {k}: max|want| {scale:.3g}, relative error {err:.3g}")
    for k, w in want.items():
        assert got[k].shape == w.shape and got[k].dtype == torch.float32
        assert float((got[k].double().cpu() - w).abs().max()) <= TOL * float(w.abs().max()), (what, k)
    print("worst so far:", {k: f"{v:.3g}" for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("weights,d,res,img,n", CASES, ids=IDS)
def test_forward_identity(runs, weights, d, res, img, n):
    r = runs(weights, d, res, img, n)
    assert r["feats"].shape == (n, 256) and r["prob"].shape == (n, 1, img, img)
    assert torch.equal(r["feats"], r["enc"](r["obs"]))
    assert torch.equal(r["prob"], r["enc"].segment(r["obs"]))


@pytest.mark.parametrize("weights,d,res,img,n", CASES, ids=IDS)
def test_kept_relu_and_gates(runs, weights, d, res, img, n):
    r = runs(weights, d, res, img, n)
    us = []
    with torch.no_grad():
        r["host"].forward(None, us)
    assert len(us) == 21
    total, worst_band, worst_err = 0, 0.0, 0.0
    for i, (u64, got) in enumerate(zip(us, r["kept"])):
        assert got.shape == u64.shape
        r64 = torch.relu(u64)
        err = float((got.double() - r64).abs().max()) / max(1.0, float(r64.abs().max()))
        band = u64.abs() <= TOL * max(1.0, float(u64.abs().max()))
        share = float(band.double().mean())
        differ = (got > 0) != (u64 > 0)
        total += int(differ.sum())
        worst_band, worst_err = max(worst_band, share), max(worst_err, err)
        print(f"{IDS[CASES.index((weights, d, res, img, n))]} layer {i}: relu error {err:.3g}, band share {share:.3g}, "
              f"gates differing {int(differ.sum())}")
        assert err <= TOL, (i, err)
        assert share <= BAND_CAP, (i, share)
        assert not bool((differ & ~band).any()), (i, int((differ & ~band).sum()))
    print(f"{weights} d={d} res{res} S={img} N={n}: relu error {worst_err:.3g}, {total} gates differ from the f64 model's, "
          f"worst band share {worst_band:.3g}")


@pytest.mark.parametrize("weights,d,res,img,n", CASES, ids=IDS)
def test_gradients_against_f64_autograd(runs, weights, d, res, img, n):
    r = runs(weights, d, res, img, n)
    host = r["host"]
    pooled, prob, _pred = host.forward(r["gates"])
    want = host.grads((pooled * r["gf"].double()).sum() + (prob * r["gp"].double()).sum())
    assert len(want) == N_ENC + N_DEC and set(want) <= set(r["grads"])
    _check_grads(f"{weights} d={d} res{res} S={img} N={n}", r["grads"], want)


@pytest.mark.parametrize("losses", ["dice+mse", "bce+smoothl1"])
def test_gradients_through_the_real_losses(runs, losses):
    """pretrainer.py:127-141 on net(obs): the segmentation loss plus the gradient loss on the head."""
    from occlusionenv_amd import segmentation

    weights, d, res, img, n = "golden", 2, 1, 64, 3
    r = runs(weights, d, res, img, n)
    net, host = r["net"], r["host"]
    gen = torch.Generator().manual_seed(m.obs_seed(img, n) + 2)
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
    assert len(want) == N_ENC + N_DEC + 2
    assert abs(float(loss.detach()) - float(loss64.detach())) <= TOL * max(1.0, abs(float(loss64.detach())))
    _check_grads(f"{losses} {weights} S={img} N={n}", got, want)


@pytest.mark.parametrize("weights,d,res,img,n", [CASES[0], CASES[2], CASES[5]], ids=[IDS[0], IDS[2], IDS[5]])
def test_the_join_itself(runs, weights, d, res, img, n):
    """grad_feats absent: whatever reaches the encoder came through the decoder's skip and input gradients, down to both
    depthwise weights of the initial layer."""
    r = runs(weights, d, res, img, n)
    net, host = r["net"], r["host"]
    net.zero_grad()
    _feats, prob = net.features_and_map(r["obs"])
    prob.backward(r["gp"].cuda())  # the absent gradient of feats arrives as zeros
    got = _grads(net)
    assert len(m.enc_keys()) == N_ENC and all(float(got[k].abs().max()) > 0.0 for k in m.enc_keys())
    assert {"encoder.initial.conv.0.weight", "encoder.initial.conv.1.weight"} <= set(m.enc_keys())
    _pooled64, prob64, _pred = host.forward(_gates(net))
    want = host.grads((prob64 * r["gp"].double()).sum())
    _check_grads(f"join {weights} d={d} res{res} S={img} N={n}", got, want)


@pytest.mark.parametrize("which", ["last", "one"])
@pytest.mark.parametrize("weights,d,res,img,n", m.SPLIT_CASES, ids=SPLIT_IDS)
def test_gradients_of_one_env(runs, weights, d, res, img, n, which):
    """Both upstream gradients are randn in one env and zero in the others: a tile given to the wrong env or dropped from a
    short last slice is the whole signal."""
    env = n - 1 if which == "last" else 1
    r = runs(weights, d, res, img, n)
    net, host = r["net"], r["host"]
    gen = torch.Generator().manual_seed(m.obs_seed(img, n) + 3 + env)
    gf, gp = torch.zeros(n, 256), torch.zeros(n, 1, img, img)
    gf[env], gp[env] = torch.randn(256, generator=gen), torch.randn(1, img, img, generator=gen)
    net.zero_grad()
    feats, prob = net.features_and_map(r["obs"])
    assert torch.equal(prob.detach(), r["prob"])
    torch.autograd.backward([feats, prob], [gf.cuda(), gp.cuda()])
    pooled64, prob64, _pred = host.forward(_gates(net))
    want = host.grads((pooled64 * gf.double()).sum() + (prob64 * gp.double()).sum())
    _check_grads(f"env {env} alone {weights} S={img} N={n}", _grads(net), want)


@pytest.mark.parametrize("weights,d,res,img,n", [CASES[1], CASES[4], CASES[6]], ids=[IDS[1], IDS[4], IDS[6]])
def test_bitwise_against_the_single_passes(runs, weights, d, res, img, n):
    from occlusionenv_amd.seghead import SegmentationHead
    from occlusionenv_amd.septrain import TrainableSeparableEncoder

    r = runs(weights, d, res, img, n)
    net, enc, obs = r["net"], r["enc"], r["obs"]
    # the decoder and classifier gradients are SegmentationHead's for the same grad_prob, whatever grad_feats is
    head = SegmentationHead.from_encoder(enc)
    head(obs).backward(r["gp"].cuda())
    hg = _grads(head)
    assert len(hg) == N_DEC and set(hg) == set(m.dec_keys()) and all(torch.equal(v.cpu(), r["grads"][k]) for k, v in hg.items())
    # with grad_prob absent the encoder gradients are TrainableSeparableEncoder's and the decoder's exactly zero
    tenc = TrainableSeparableEncoder.from_encoder(enc)
    tenc(obs).backward(r["gf"].cuda())
    eg = {k: v for k, v in _grads(tenc).items() if k in m.enc_keys()}
    net.zero_grad()
    feats, _prob = net.features_and_map(obs)
    feats.backward(r["gf"].cuda())
    got = _grads(net)
    assert len(eg) == N_ENC and all(torch.equal(v, got[k]) for k, v in eg.items())
    assert all(float(got[k].abs().max()) == 0.0 for k in m.dec_keys())
    # two joint backward calls give the same bits
    net.zero_grad()
    feats, prob = net.features_and_map(obs)
    torch.autograd.backward([feats, prob], [r["gf"].cuda(), r["gp"].cuda()])
    again = _grads(net)
    assert len(again) >= N_ENC + N_DEC and all(torch.equal(v.cpu(), r["grads"][k]) for k, v in again.items())


@pytest.mark.parametrize("weights,d,res,img,n", [CASES[2], CASES[6]], ids=[IDS[2], IDS[6]])
def test_no_stale_reads_and_nothing_outside_the_reported_sizes(runs, weights, d, res, img, n):
    """The native calls on buffers of exactly the queried sizes, each the middle of a larger allocation that is inspected
    afterwards; then the backward again after everything it may only write (scratch, the gradient part of the workspace,
    dlast / dskip, both gradient outputs) and the forward's outputs feats and prob, which it must neither read nor write,
    have been filled with NaNs: the same bits."""
    from occlusionenv_amd import _native as nat
    from occlusionenv_amd.encoder import FEATURES, decoder_packed_floats, packed_floats
    from occlusionenv_amd.nettrain import unpack_decoder_buffer, unpack_sep_encoder_buffer

    r = runs(weights, d, res, img, n)
    enc, net, obs = r["enc"], r["net"], r["obs"]
    gf, gp = r["gf"].cuda(), r["gp"].cuda()
    lib, cfg, st = nat.load(), enc._cfg(img), nat.stream_ptr(obs.device)
    wsb, scb = C.c_size_t(), C.c_size_t()
    nat.check(lib.occ_sep_fullnet_train_workspace_query(C.byref(cfg), n, C.byref(wsb), C.byref(scb)),
              "occ_sep_fullnet_train_workspace_query")
    sizes = dict(ws=int(wsb.value), scratch=int(scb.value), grad_enc=4 * packed_floats(True), grad_dec=4 * decoder_packed_floats(),
                 prob=4 * n * img * img, feats=4 * n * FEATURES)
    assert sizes["ws"] == m.ws_bytes(img, n) and sizes["scratch"] == m.scratch_bytes(img, n)
    bufs = {k: _guarded(b) for k, b in sizes.items()}
    mid = {k: whole[lo:lo + sizes[k]] for k, (whole, lo) in bufs.items()}
    assert all(v.data_ptr() % 256 == 0 for v in mid.values())

    def backward():
        nat.check(lib.occ_sep_fullnet_backward(C.byref(cfg), nat.ptr(enc.packed), nat.ptr(enc.dec_packed), n, nat.ptr(mid["ws"]),
                                               sizes["ws"], nat.ptr(gf), nat.ptr(gp), nat.ptr(mid["scratch"]), sizes["scratch"],
                                               nat.ptr(mid["grad_enc"]), nat.ptr(mid["grad_dec"]), st), "occ_sep_fullnet_backward")
        return mid["grad_enc"].view(torch.float32).clone(), mid["grad_dec"].view(torch.float32).clone()

    nat.check(lib.occ_sep_fullnet_train_forward(C.byref(cfg), nat.ptr(enc.packed), nat.ptr(enc.dec_packed), nat.ptr(obs), n,
                                                nat.ptr(mid["ws"]), sizes["ws"], nat.ptr(mid["feats"]), nat.ptr(mid["prob"]), st),
              "occ_sep_fullnet_train_forward")
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
    # the same bits as through the autograd function: the conv weights and biases as they are
    part = net.parts[0]
    for layer, stem, leaves in zip(unpack_sep_encoder_buffer(a[0].cpu()), part.stems, part.layer_leaves()):
        for t, leaf in zip(layer[:-2], leaves[:-2]):
            assert torch.equal(t, r["grads"][stem + leaf]), stem + leaf
    dk = m.dec_keys()
    levels, dcw, dcb = unpack_decoder_buffer(a[1].cpu())
    for j, level in enumerate(levels):
        assert torch.equal(level[0], r["grads"][dk[4 * j]]) and torch.equal(level[1], r["grads"][dk[4 * j + 1]])
    assert torch.equal(dcw, r["grads"][dk[-2]]) and torch.equal(dcb, r["grads"][dk[-1]])
    for k, (whole, lo) in bufs.items():
        assert lo >= GUARD and whole.numel() - (lo + sizes[k]) >= GUARD
        assert bool((whole[:lo] == 0xA5).all()), f"bytes in front of {k} were written"
        assert bool((whole[lo + sizes[k]:] == 0xA5).all()), f"bytes behind {k} were written"


def test_errors(nets, runs):
    from occlusionenv_amd._native import NativeError
    from occlusionenv_amd.encoder import FrozenEncoder
    from occlusionenv_amd.fullnet import TrainableFullNetwork
    from occlusionenv_amd.sepfullnet import TrainableSeparableFullNetwork
    from tests import fullnet_train_model as ftm

    sd32, enc = nets["golden", 2, 1]
    r = runs("golden", 2, 1, 64, 3)
    net = r["net"]
    with pytest.raises(ValueError, match="FrozenEncoder"):
        TrainableSeparableFullNetwork.from_encoder(object())
    dense = FrozenEncoder.from_state_dict({k: v.float() for k, v in ftm.state_dict("ppo").items()}, preset="ppo", dilation=1)
    assert not dense.separable
    with pytest.raises(ValueError, match=r"dense \(use fullnet.TrainableFullNetwork\)"):
        TrainableSeparableFullNetwork.from_encoder(dense)
    bare = FrozenEncoder.from_state_dict({k: v for k, v in sd32.items() if not k.startswith("segmenter.")}, preset="ppo")
    with pytest.raises(ValueError, match="no segmentation decoder"):
        TrainableSeparableFullNetwork.from_encoder(bare)
    import copy

    folded = copy.copy(enc)
    folded.encoder_state = None
    with pytest.raises(ValueError, match="keeps no unfolded encoder tensors"):
        TrainableSeparableFullNetwork.from_encoder(folded)
    # the dense joint network still refuses this checkpoint
    with pytest.raises(ValueError, match="dense 3x3 convs only"):
        TrainableFullNetwork.from_encoder(enc)
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
    net.zero_grad()


@pytest.fixture(scope="module")
def trained(nets):
    """Twenty AdamW steps at lr 1e-3 on a fixed batch (N=4, S=64), Dice + MSE as in pretrainer.py."""
    from occlusionenv_amd import segmentation
    from occlusionenv_amd.sepfullnet import TrainableSeparableFullNetwork

    enc = nets["golden", 2, 1][1]
    n, img = 4, 64
    obs = m.case_obs(img, n).float().cuda()
    gen = torch.Generator().manual_seed(m.obs_seed(img, n) + 5)
    occl = (torch.rand(n, 1, img // 8, img // 8, generator=gen) > 0.5).float().repeat_interleave(8, 2).repeat_interleave(8, 3).cuda()
    grad = (torch.randn(n, 2, generator=gen) * 0.5).cuda()
    net = TrainableSeparableFullNetwork.from_encoder(enc)
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-5)
    losses = []
    for _ in range(21):  # twenty steps, and the loss after the twentieth
        opt.zero_grad()
        _pooled, segm, pred = net(obs)
        loss = segmentation.binary_dice_loss(segm, occl) + F.mse_loss(pred, grad)
        losses.append(loss.detach())
        if len(losses) <= 20:
            loss.backward()
            opt.step()
    return dict(net=net, enc=enc, obs=obs, before=before, losses=torch.stack(losses).cpu().tolist())


def test_learning(trained):
    losses = trained["losses"]
    print("Dice + MSE:", [f"{v:.4f}" for v in losses[::5]])
    assert all(v == v for v in losses) and losses[-1] < losses[0]
    assert all(not torch.equal(v, trained["before"][k]) for k, v in trained["net"].named_parameters())


def test_round_trip_into_a_frozen_encoder_and_the_agent(trained):
    from occlusionenv_amd.ppo import BatchedPPO

    net, enc, obs = trained["net"], trained["enc"], trained["obs"]
    sd = net.state_dict()
    assert "segmenter.0.features.0.up.conv.weight" in sd and "gradPredictor.bias" in sd and "action_head.weight" in sd
    assert tuple(sd["encoder.features.4.net.Layer 2.conv.0.weight"].shape) == (128, 1, 3, 1)
    assert len(list(net.named_parameters())) == N_ENC + N_DEC + 2
    with torch.no_grad():
        pooled, segm, pred = net(obs)
    both = enc.with_state(sd)
    assert torch.equal(both(obs), pooled) and torch.equal(both.segment(obs), segm)
    f2, s2, g2 = both.forward_full(obs)
    assert torch.equal(f2, pooled) and torch.equal(s2, segm)
    assert torch.allclose(g2, pred, rtol=1e-5, atol=1e-6)  # addmm against F.linear
    assert not torch.equal(enc.segment(obs), segm) and not torch.equal(enc(obs), pooled)  # the source is left as it is
    agent = BatchedPPO.from_fullnetwork(sd)
    assert agent.encoder.separable and agent.encoder.dilation == 2 and agent.encoder.residual
    assert torch.equal(agent.encoder(obs), pooled)
    assert torch.equal(agent.policy.action_head.weight.detach().cpu(), enc.heads["action_head"][0].float())


def test_pretrain_epoch(nets):
    from occlusionenv_amd import harness, segmentation
    from occlusionenv_amd.sepfullnet import TrainableSeparableFullNetwork
    from tests.encoder_model import make_obs

    enc = nets["golden", 2, 1][1]
    n, img = 4, 64
    gen = torch.Generator().manual_seed(77)
    batches = []
    for b in range(3):  # the stored format: (img, occlusion, grad, _) on the host
        occl = (torch.rand(n, 1, img // 8, img // 8, generator=gen) > 0.5).float().repeat_interleave(8, 2).repeat_interleave(8, 3)
        batches.append((make_obs(500 + b, n, img).float(), occl, torch.randn(n, 2, generator=gen) * 0.5, None))
    # the predictions each step learns from, by the same steps taken by hand
    ref = TrainableSeparableFullNetwork.from_encoder(enc)
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
    res = harness.pretrain_epoch(enc, batches)  # from a separable encoder: the separable net is made
    assert isinstance(res["net"], TrainableSeparableFullNetwork) and res["batches"] == 3 and res["pixels"] == 3 * n * img * img
    for k in ("loss", "segm_loss", "grad_loss", "accuracy", "iou"):
        assert res[k] == res[k] and abs(res[k]) < float("inf"), k
    assert abs(res["loss"] - (res["segm_loss"] + res["grad_loss"])) <= 1e-6
    assert abs(res["accuracy"] - 100.0 * sum(acc) / 3) <= 1e-9 and abs(res["iou"] - 100.0 * sum(iou) / 3) <= 1e-9
    assert 0 <= res["intersection"] <= res["union"] <= res["pixels"] and 0 <= res["correct"] <= res["pixels"]
    assert all(torch.equal(v, dict(ref.named_parameters())[k]) for k, v in res["net"].named_parameters())
    res2 = harness.pretrain_epoch(res["net"], batches, use_dice=False, use_l1=True, optimizer=res["optimizer"])
    assert res2["net"] is res["net"] and res2["optimizer"] is res["optimizer"] and res2["batches"] == 3
    assert all(res2[k] == res2[k] for k in ("loss", "segm_loss", "grad_loss", "accuracy", "iou"))
    assert abs(res2["loss"] - (res2["segm_loss"] + res2["grad_loss"])) <= 1e-6
