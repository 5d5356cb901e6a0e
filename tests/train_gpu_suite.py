"""The bodies shared by the GPU tests of the native training paths: tests/test_gpu_encoder_train.py and
tests/test_gpu_sep_encoder_train.py (the encoder through its pooled feature), tests/test_gpu_fullnet_train.py and
tests/test_gpu_sep_fullnet_train.py (the joint step), tests/test_gpu_decoder_train.py (the decoder over the frozen encoder)
and, for the gate, gradient and packed-gradient checks, tests/test_gpu_bn_train.py (the joint step with batch statistics).
Each body is a plain function of a ``Form``, what varies between those modules; the modules keep their fixtures, their cases
and their ``WORST`` dictionary and call in here.  Nothing is cached in this module: what lives on the device is what the
calling module's fixtures hold.

A case is a tuple that ends in (img, n); what is in front of it selects the weights (the key of the module's ``nets``, whose
entries are (the f32 state dict, the FrozenEncoder)).  What a step returns, which of that takes an upstream gradient, which
packed weights the two native calls read and how many relu layers are kept is read off the net class (``RETURNS``,
``DIFFERENTIABLE``, ``parts``), not off the form: the encoder nets return feats, the joint nets (feats, prob), both with a
gradient, the decoder head both with a gradient for prob alone.  The oracle is tests/train_model.HostModel on the case's
f32 weights, the workspace layout tests/train_layout.py."""
import ctypes as C
import functools
from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_layout as tl
from tests import train_model as tm
from tests.encoder_model import make_obs
from tests.train_utils import bce64, dice64, grads, guarded, guards_intact

FEATURES = 256
NAN = 0x7FC00000


class Form(NamedTuple):
    model: Callable               # case -> the train_model.Net it runs
    label: Callable               # case -> what a printed line starts with
    tol: float
    # what the fixtures and the native-call bodies read; a module that calls kept_relu_and_gates and check_grads alone
    # (tests/test_gpu_bn_train.py, which has its own ``runs``) leaves these five out
    net: Optional[type] = None    # the trainable net
    symbols: Tuple[str, ...] = ()  # workspace query, train forward, backward
    n_params: int = 0             # tensors that receive a gradient, without the head's two
    seed: int = 0                 # 4000, 7000 or 9000: a case's seed is seed + img + n
    steps: int = 0                # AdamW steps of ``trained``
    encoder_net: Optional[type] = None   # joint: the single encoder pass the joint step is compared with
    gate_label: Optional[Callable] = None  # case -> the start of a gate line, where it is not ``label``
    one_env_seed: int = 3             # a one-env upstream gradient is drawn from the case's seed + this + the env
    host_obs_f64: bool = False        # the host model reads make_obs's f64 values, the device their f32 roundings
    # what one form asserts and the other does not
    nonzero_scale: bool = False       # no wanted gradient is all zero
    band_cap: Optional[float] = None  # the largest share of a layer's pixels inside the gate band
    gate_cap: Optional[float] = None  # the largest share of a layer's gates that differ from the f64 model's
    e32: Optional[Callable] = None    # case -> {key: PyTorch's f32 error}: such a key's bar is train_model.bar's, its line shows it
    head_is_the_decoder: bool = False  # SegmentationHead's gradients are exactly the decoder keys
    finite_losses: bool = False       # the losses of ``trained`` are finite, not only not NaN


# What varies with the step a net class runs, keyed by what that class says of itself.  An output's name also names the packed
# weights it needs (feats: the encoder's, prob: the decoder's): the train forward takes those of the outputs it returns, the
# backward those of the outputs it differentiates.
OUTPUTS = ("feats", "prob")  # the order of the library's arguments, and of ``outs`` and ``ups`` below
STEP = {("feats",): lambda net, obs: (net(obs),),  # RETURNS -> the public call that gives (feats, prob), whichever there are
        ("feats", "prob"): lambda net, obs: net.features_and_map(obs),
        ("prob", "feats"): lambda net, obs: net(obs, return_features=True)}


def case_seed(f, case):
    return f.seed + case[-2] + case[-1]


def _named(names, feats, prob):
    """Of (feats, prob), those that ``names`` (a net's ``RETURNS`` or ``DIFFERENTIABLE``) holds."""
    return [t for k, t in zip(OUTPUTS, (feats, prob)) if k in names]


def _step(net, obs):
    return STEP[net.RETURNS](net, obs)


def _diff(net, outs):
    """Of a step's outputs, those that take an upstream gradient."""
    return [o for k, o in zip(_named(net.RETURNS, *OUTPUTS), outs) if k in net.DIFFERENTIABLE]


def _total(outs):
    total = outs[0].sum()
    for o in outs[1:]:
        total = total + o.sum()
    return total


def _n_relu(net):
    return sum(len(part.stems) for part in net.parts)


def gates_of(net):
    return [(tl.kept_relu(net, i).cpu() > 0).double() for i in range(_n_relu(net))]


def _host_outs(net, host, gates):
    pooled, prob, _pred = host.forward(gates)
    return _named(net.DIFFERENTIABLE, pooled, prob)


def _dot(outs64, ups):
    loss = (outs64[0] * ups[0].double()).sum()
    for o, u in zip(outs64[1:], ups[1:]):
        loss = loss + (o * u.double()).sum()
    return loss


def _shapes(names, img, n):
    return _named(names, (n, FEATURES), (n, 1, img, img))


def make_runs(f, nets):
    """The ``runs`` fixture of a module: case -> computed once and left unchanged, one native forward + backward with seeded
    randn upstream gradients, the kept relu outputs and their gates, and the host model."""
    cache = {}

    def get(*case):
        if case not in cache:
            img, n = case[-2:]
            key = case[:-2]
            sd32, enc = nets[key if len(key) > 1 else key[0]]
            obs64 = make_obs(case_seed(f, case), n, img)
            obs = obs64.float().cuda()
            net = f.net.from_encoder(enc)
            outs = _step(net, obs)
            assert [o.requires_grad for o in outs] == [k in net.DIFFERENTIABLE for k in _named(net.RETURNS, *OUTPUTS)]
            gen = torch.Generator().manual_seed(case_seed(f, case) + 1)
            ups = [torch.randn(*s, generator=gen) for s in _shapes(net.DIFFERENTIABLE, img, n)]
            net.zero_grad()
            torch.autograd.backward(_diff(net, outs), [u.cuda() for u in ups])
            kept = [tl.kept_relu(net, i).cpu().clone() for i in range(_n_relu(net))]
            cache[case] = dict(sd=sd32, enc=enc, net=net, obs=obs, outs=[o.detach() for o in outs], feats=outs[0].detach(), ups=ups,
                               kept=kept, gates=[(k > 0).double() for k in kept],
                               grads={k: v.cpu() for k, v in grads(net).items()},
                               host=tm.HostModel(sd32, f.model(case), obs64 if f.host_obs_f64 else obs.double().cpu()))
        return cache[case]

    return get


def check_grads(f, worst, what, case, got, want):
    e32 = f.e32(case) if f.e32 else {}
    for k, w in want.items():
        scale = float(w.abs().max())
        if f.nonzero_scale:
            assert scale > 0.0, (what, k, "the oracle's gradient is all zero")
        err = float((got[k].double().cpu() - w).abs().max()) / scale
        kind = tm.kind(f.model(case), k)
        worst[kind] = max(worst.get(kind, 0.0), err)
        print(f"{what} {k}: max|want| {scale:.3g}, relative error {err:.3g}" + (f", e32 {e32.get(k, 0.0):.3g}" if f.e32 else ""))
    for k, w in want.items():
        assert got[k].shape == w.shape and got[k].dtype == torch.float32
        bar = tm.bar(case, k) if k in e32 else f.tol  # the head's two tensors sit above the pooled feature: the plain bar
        assert float((got[k].double().cpu() - w).abs().max()) <= bar * float(w.abs().max()), (what, k, bar)
    print("worst so far:", {k: f"{v:.3g}" for k, v in sorted(worst.items())})


def forward_identity(f, r, case):
    img, n = case[-2:]
    net, frozen = r["net"], (r["enc"], r["enc"].segment)
    assert [tuple(o.shape) for o in r["outs"]] == _shapes(net.RETURNS, img, n)
    for o, inference in zip(r["outs"], _named(net.RETURNS, *frozen)):
        assert torch.equal(o, inference(r["obs"]))


def kept_relu_and_gates(f, r, case, us=None):
    """``us``: the f64 model's pre-activations, where the calling module already has them."""
    if us is None:
        us = []
        with torch.no_grad():
            r["host"].forward(None, us)
    assert len(us) == len(r["kept"]) == _n_relu(r["net"])
    start = (f.gate_label or f.label)(case)
    start = start + " " if start else ""  # a module whose gate lines begin with "layer"
    total, worst_band, worst_err = 0, 0.0, 0.0
    for i, (u64, got) in enumerate(zip(us, r["kept"])):
        assert got.shape == u64.shape
        r64 = torch.relu(u64)
        err = float((got.double() - r64).abs().max()) / max(1.0, float(r64.abs().max()))
        band = u64.abs() <= f.tol * max(1.0, float(u64.abs().max()))
        share = float(band.double().mean())
        differ = (got > 0) != (u64 > 0)
        total += int(differ.sum())
        worst_band, worst_err = max(worst_band, share), max(worst_err, err)
        print(f"{start}layer {i}: relu error {err:.3g}, band share {share:.3g}, gates differing {int(differ.sum())}")
        assert err <= f.tol, (i, err)
        if f.band_cap is not None:
            assert share <= f.band_cap, (i, share)  # a property of the seeds, checked on the f64 model alone
        assert not bool((differ & ~band).any()), (i, int((differ & ~band).sum()))
        if f.gate_cap is not None:
            assert float(differ.double().mean()) <= f.gate_cap, (i, int(differ.sum()))
    print(f"{f.label(case)}: relu error {worst_err:.3g}, {total} gates differ from the f64 model's, "
          f"worst band share {worst_band:.3g}")


def gradients_against_f64_autograd(f, worst, r, case):
    host = r["host"]
    want = host.grads(_dot(_host_outs(r["net"], host, r["gates"]), r["ups"]))
    assert len(want) == f.n_params and set(want) <= set(r["grads"])
    check_grads(f, worst, f.label(case), case, r["grads"], want)


def gradients_through_the_head_and_mse(f, worst, r, case):
    img, n = case[-2:]
    net, host = r["net"], r["host"]
    target = torch.randn(n, 2, generator=torch.Generator().manual_seed(case_seed(f, case) + 2)).clamp(-1, 1)
    net.zero_grad()
    loss = F.mse_loss(net.predict_grad(r["obs"]), target.cuda())
    loss.backward()
    got = grads(net)
    loss64 = F.mse_loss(host.predict(gates_of(net)), target.double())
    want = host.grads(loss64, head=True)
    assert len(want) == f.n_params + 2
    assert abs(float(loss.detach()) - float(loss64.detach())) <= f.tol * max(1.0, abs(float(loss64.detach())))
    check_grads(f, worst, f"mse {f.label(case)}", case, got, want)


MAP_LOSS = {"dice": ("binary_dice_loss", dice64), "bce": ("binary_cross_entropy", bce64)}  # the native loss, its f64 model
HEAD_LOSS = {"mse": F.mse_loss, "smoothl1": functools.partial(F.smooth_l1_loss, beta=0.01)}


def gradients_through_the_real_losses(f, worst, r, case, losses, occl=None):
    """``losses``: "dice" or "bce" on the map of ``net(obs)`` (towards ``occl``, or a seeded random map), "+mse" or
    "+smoothl1": plus that loss on the grad head's prediction, ``net(obs)`` being (pooled, map, prediction)."""
    from occlusionenv_amd import segmentation

    img, n = case[-2:]
    net, host = r["net"], r["host"]
    on_map, _, on_head = losses.partition("+")
    gen = torch.Generator().manual_seed(case_seed(f, case) + 2)
    if occl is None:
        occl = (torch.rand(n, 1, img, img, generator=gen) > 0.5).float()
    net.zero_grad()
    out = net(r["obs"])
    loss = getattr(segmentation, MAP_LOSS[on_map][0])(out[1] if on_head else out, occl.cuda())
    if on_head:
        grad = torch.randn(n, 2, generator=gen) * 0.05  # both sides of SmoothL1's beta = 0.01
        loss = loss + HEAD_LOSS[on_head](out[2], grad.cuda())
    loss.backward()
    got = grads(net)
    _p64, prob64, pred64 = host.forward(gates_of(net))
    loss64 = MAP_LOSS[on_map][1](prob64, occl)
    if on_head:
        loss64 = loss64 + HEAD_LOSS[on_head](pred64, grad.double())
    want = host.grads(loss64, head=bool(on_head))
    assert len(want) == f.n_params + (2 if on_head else 0)
    assert abs(float(loss.detach()) - float(loss64.detach())) <= f.tol * max(1.0, abs(float(loss64.detach())))
    check_grads(f, worst, f"{losses} {case[0]} S={img} N={n}", case, got, want)


def gradients_of_one_env(f, worst, r, case, env):
    """Every upstream gradient is randn in one env and zero in the others: a tile given to the wrong env or dropped from a
    short last slice is the whole signal."""
    img, n = case[-2:]
    net, host = r["net"], r["host"]
    gen = torch.Generator().manual_seed(case_seed(f, case) + f.one_env_seed + env)
    ups = [torch.zeros(*s) for s in _shapes(net.DIFFERENTIABLE, img, n)]
    for u in ups:
        u[env] = torch.randn(*u.shape[1:], generator=gen)
    net.zero_grad()
    outs = _step(net, r["obs"])
    assert torch.equal(outs[-1].detach(), r["outs"][-1])
    torch.autograd.backward(_diff(net, outs), [u.cuda() for u in ups])
    got = grads(net)
    want = host.grads(_dot(_host_outs(net, host, gates_of(net)), ups))
    assert len(want) == f.n_params
    both = f"env {env} alone {case[0]} S={img} N={n}"  # what the modules whose step takes two upstream gradients print
    check_grads(f, worst, both if len(ups) == 2 else f"one-hot env {env} {f.label(case)}", case, got, want)


def reproducible_and_accumulating(r):
    net, obs, up = r["net"], r["obs"], r["ups"][0].cuda()
    net.zero_grad()
    net(obs).backward(up)
    once = grads(net)
    assert all(torch.equal(once[k].cpu(), r["grads"][k]) for k in once)  # the same bits as the fixture's call
    net(obs).backward(up)  # without zero_grad the second pass accumulates as torch does: g + g, exact
    assert all(torch.equal(v, once[k] + once[k]) for k, v in grads(net).items())
    net.zero_grad()
    net(obs).backward(up)
    assert all(torch.equal(v, once[k]) for k, v in grads(net).items())
    net.zero_grad()


def the_join_itself(f, worst, r, case):
    """grad_feats absent: whatever reaches the encoder came through the decoder's skip and input gradients."""
    net, host = r["net"], r["host"]
    net.zero_grad()
    _feats, prob = net.features_and_map(r["obs"])
    prob.backward(r["ups"][1].cuda())  # the absent gradient of feats arrives as zeros
    got = grads(net)
    assert all(float(got[k].abs().max()) > 0.0 for k in tm.enc_keys(f.model(case)))
    _pooled64, prob64, _pred = host.forward(gates_of(net))
    want = host.grads((prob64 * r["ups"][1].double()).sum())
    check_grads(f, worst, f"join {f.label(case)}", case, got, want)


def bitwise_against_the_single_passes(f, r, case):
    from occlusionenv_amd.seghead import SegmentationHead

    net, enc, obs = r["net"], r["enc"], r["obs"]
    gf, gp = (u.cuda() for u in r["ups"])
    enc_keys, dec_keys = tm.enc_keys(f.model(case)), tm.dec_keys(f.model(case))
    n_dec = len(dec_keys)
    # the decoder and classifier gradients are SegmentationHead's for the same grad_prob, whatever grad_feats is
    head = SegmentationHead.from_encoder(enc)
    head(obs).backward(gp)
    hg = grads(head)
    assert len(hg) == n_dec == 22 and all(torch.equal(v.cpu(), r["grads"][k]) for k, v in hg.items())
    if f.head_is_the_decoder:
        assert set(hg) == set(dec_keys)
    # with grad_prob absent the encoder gradients are the single encoder pass's and the decoder's exactly zero
    tenc = f.encoder_net.from_encoder(enc)
    tenc(obs).backward(gf)
    eg = {k: v for k, v in grads(tenc).items() if k in enc_keys}
    net.zero_grad()
    feats, _prob = net.features_and_map(obs)
    feats.backward(gf)
    got = grads(net)
    assert len(eg) == f.n_params - n_dec and all(torch.equal(v, got[k]) for k, v in eg.items())
    assert all(float(got[k].abs().max()) == 0.0 for k in dec_keys)
    # two joint backward calls give the same bits
    net.zero_grad()
    feats, prob = net.features_and_map(obs)
    torch.autograd.backward([feats, prob], [gf, gp])
    again = grads(net)
    assert len(again) >= f.n_params and all(torch.equal(v.cpu(), r["grads"][k]) for k, v in again.items())


def no_stale_reads_and_nothing_outside_the_reported_sizes(f, r, case):
    """The native calls on buffers of exactly the queried sizes, each the middle of a larger allocation that is inspected
    afterwards; then the backward again after everything it may only write (scratch, train_layout.only_written of the
    workspace, the packed gradients) and the forward's outputs, which it must neither read nor write, have been filled with
    NaNs: the same bits, so nothing read was left over from before."""
    from occlusionenv_amd import _native as nat

    img, n = case[-2:]
    m, enc, net, obs = f.model(case), r["enc"], r["net"], r["obs"]
    ups = [u.cuda() for u in r["ups"]]
    out_names = _named(net.RETURNS, *OUTPUTS)
    grad_names = [f"grad_packed_{i}" for i in range(len(net.parts))]
    forward_packed = _named(net.RETURNS, enc.packed, enc.dec_packed)
    backward_packed = _named(net.DIFFERENTIABLE, enc.packed, enc.dec_packed)
    lib, cfg, st = nat.load(), enc._cfg(img), nat.stream_ptr(obs.device)
    query, forward_name, backward_name = f.symbols
    wsb, scb = C.c_size_t(), C.c_size_t()
    nat.check(getattr(lib, query)(C.byref(cfg), n, C.byref(wsb), C.byref(scb)), query)
    sizes = dict(ws=int(wsb.value), scratch=int(scb.value))
    sizes.update(zip(grad_names, (4 * part.floats for part in net.parts)))
    sizes.update(zip(out_names, _named(net.RETURNS, 4 * n * FEATURES, 4 * n * img * img)))
    assert sizes["scratch"] == tl.scratch_bytes(m, img, n) and sizes["ws"] == tl.ws_bytes(m, img, n)
    bufs = {k: guarded(b) for k, b in sizes.items()}
    mid = {k: whole[lo:lo + sizes[k]] for k, (whole, lo) in bufs.items()}
    assert all(v.data_ptr() % 256 == 0 for v in mid.values())

    def backward():
        nat.check(getattr(lib, backward_name)(C.byref(cfg), *[nat.ptr(p) for p in backward_packed], n, nat.ptr(mid["ws"]),
                                              sizes["ws"], *[nat.ptr(u) for u in ups], nat.ptr(mid["scratch"]), sizes["scratch"],
                                              *[nat.ptr(mid[k]) for k in grad_names], st), backward_name)
        return [mid[k].view(torch.float32).clone() for k in grad_names]

    nat.check(getattr(lib, forward_name)(C.byref(cfg), *[nat.ptr(p) for p in forward_packed], nat.ptr(obs), n, nat.ptr(mid["ws"]),
                                         sizes["ws"], *[nat.ptr(mid[k]) for k in out_names], st), forward_name)
    for k, want in zip(out_names, r["outs"]):
        assert torch.equal(mid[k].view(torch.float32).view(want.shape), want)
    a, again = backward(), backward()
    for lo, hi in tl.only_written(m, img, n):
        mid["ws"][lo:hi].view(torch.int32).fill_(NAN)
    for k in ["scratch"] + grad_names + out_names:  # the outputs too: the backward reads the prob kept in ws
        mid[k].view(torch.int32).fill_(NAN)
    b = backward()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in a)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), z.view(torch.int32))
               for x, y, z in zip(a, again, b))
    assert all(bool((mid[k].view(torch.int32) == NAN).all()) for k in out_names)  # the backward writes none of them
    # through the autograd function the BN affine goes through the fold: every conv leaf and the classifier as they are
    packed_gradients_are_the_modules(net, a, r["grads"], folded=True)
    guards_intact(bufs, sizes)


def packed_gradients_are_the_modules(net, packed_grads, module_grads, folded):
    """The packed gradients of the native backward, one per part, hold the bits that the autograd function gave the
    parameters -> the number of tensors compared.  ``folded``: the BatchNorm slots hold d scale / d shift of the folded
    affine and are left out; otherwise (batch statistics) they hold d gamma / d beta as they are."""
    assert len(net.parts) == len(packed_grads)
    compared = 0
    for part, packed_grad in zip(net.parts, packed_grads):
        layers, tail = part.unpack(packed_grad.cpu())
        for layer, stem, leaves in zip(layers, part.stems, part.layer_leaves()):
            for t, leaf in zip(layer, leaves[:-2] if folded else leaves):
                assert torch.equal(t, module_grads[stem + leaf]), stem + leaf
                compared += 1
        assert len(tail) == len(part.tail)
        for t, k in zip(tail, part.tail):
            assert torch.equal(t, module_grads[k]), k
            compared += 1
    return compared


def errors_tail(f, r):
    """What every form refuses in the same words, on a case's net: a chunk limit below the batch, a side that is no multiple
    of 32 (where the decoder runs), a CPU tensor, and the backward of a forward that a later one has superseded."""
    from occlusionenv_amd._native import NativeError

    net, enc = r["net"], r["enc"]
    enc.max_chunk = 2
    try:
        with pytest.raises(ValueError, match="max_chunk"):
            net(r["obs"])
    finally:
        enc.max_chunk = 256
    if net.RUNS_DECODER:
        with pytest.raises(ValueError, match="multiple of 32"):
            net(torch.zeros(1, 4, 48, 48, device="cuda"))
    with pytest.raises(NativeError):
        net(torch.zeros(1, 4, 64, 64))
    first = _diff(net, _step(net, r["obs"]))
    second = _diff(net, _step(net, r["obs"][:1]))
    with pytest.raises(RuntimeError, match="superseded"):
        _total(first).backward()
    net.zero_grad()
    _total(second).backward()  # the latest forward still has its activations
    assert all(p.grad is not None for _k, p in net.ordered_parameters())
    net.zero_grad()


def train(f, net, loss_of, **adamw):
    """``f.steps`` AdamW steps at lr 1e-3 on a fixed batch -> (the parameters before, the loss in front of every step and after
    the last one)."""
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, **adamw)
    losses = []
    for _ in range(f.steps + 1):
        opt.zero_grad()
        loss = loss_of(net)
        losses.append(loss.detach())
        if len(losses) <= f.steps:
            loss.backward()
            opt.step()
    return before, torch.stack(losses).cpu().tolist()


def trained_encoder(f, r):
    """The ``trained`` fixture of an encoder form, on the case of ``r``, towards fixed unit targets."""
    net = f.net.from_encoder(r["enc"])
    target = F.normalize(torch.randn(3, 2, generator=torch.Generator().manual_seed(5)), dim=1).cuda()
    before, losses = train(f, net, lambda net: F.mse_loss(net.predict_grad(r["obs"]), target))
    return dict(net=net, before=before, losses=losses, obs=r["obs"], enc=r["enc"], feats0=r["feats"])


def _blocky(n, img, gen):
    """A random occlusion map of 8 x 8 blocks."""
    return (torch.rand(n, 1, img // 8, img // 8, generator=gen) > 0.5).float().repeat_interleave(8, 2).repeat_interleave(8, 3)


def trained_joint(f, enc):
    """The ``trained`` fixture of a joint form: a fixed batch (N=4, S=64), Dice + MSE as in pretrainer.py."""
    from occlusionenv_amd import segmentation

    n, img = 4, 64
    obs = make_obs(f.seed + img + n, n, img).float().cuda()
    gen = torch.Generator().manual_seed(f.seed + img + n + 5)
    occl = _blocky(n, img, gen).cuda()
    grad = (torch.randn(n, 2, generator=gen) * 0.5).cuda()
    net = f.net.from_encoder(enc)

    def loss_of(net):
        _pooled, segm, pred = net(obs)
        return segmentation.binary_dice_loss(segm, occl) + F.mse_loss(pred, grad)

    before, losses = train(f, net, loss_of, weight_decay=1e-5)
    return dict(net=net, enc=enc, obs=obs, before=before, losses=losses)


def learning(f, trained):
    losses = trained["losses"]
    assert all(np.isfinite(v) if f.finite_losses else v == v for v in losses) and losses[-1] < losses[0]
    assert all(not torch.equal(v, trained["before"][k]) for k, v in trained["net"].named_parameters())


def pretrain_epoch(f, enc):
    """harness.pretrain_epoch on three stored batches against the same steps taken by hand -> (the first epoch's result, a
    second epoch's on its net and optimizer with the other two losses)."""
    from occlusionenv_amd import harness, segmentation

    n, img = 4, 64
    gen = torch.Generator().manual_seed(77)
    batches = []
    for b in range(3):  # the stored format: (img, occlusion, grad, _) on the host
        occl = _blocky(n, img, gen)
        batches.append((make_obs(500 + b, n, img).float(), occl, torch.randn(n, 2, generator=gen) * 0.5, None))
    # the predictions each step learns from, by the same steps taken by hand
    ref = f.net.from_encoder(enc)
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
    res = harness.pretrain_epoch(enc, batches)  # from an encoder: the net of its form is made
    assert isinstance(res["net"], f.net) and res["batches"] == 3 and res["pixels"] == 3 * n * img * img
    for k in ("loss", "segm_loss", "grad_loss", "accuracy", "iou"):
        assert res[k] == res[k] and abs(res[k]) < float("inf"), k
    assert abs(res["loss"] - (res["segm_loss"] + res["grad_loss"])) <= 1e-6
    assert abs(res["accuracy"] - 100.0 * sum(acc) / 3) <= 1e-9 and abs(res["iou"] - 100.0 * sum(iou) / 3) <= 1e-9
    assert all(torch.equal(v, dict(ref.named_parameters())[k]) for k, v in res["net"].named_parameters())
    res2 = harness.pretrain_epoch(res["net"], batches, use_dice=False, use_l1=True, optimizer=res["optimizer"])
    assert res2["net"] is res["net"] and all(res2[k] == res2[k] for k in ("loss", "segm_loss", "grad_loss", "accuracy", "iou"))
    return res, res2
