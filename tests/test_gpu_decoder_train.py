"""GPU tests of the native decoder backward (csrc/occ_decoder_bwd.hpp, occlusionenv_amd/seghead.py, harness.
finetune_segmentation) against tests/segmenter_model.py in f64 on the CPU: the encoder detached, the decoder and the
classifier with requires_grad tensors, torch autograd supplying the gradients.

Weights: the fixture's seeded state dict rounded to f32 (what a checkpoint on disk holds, and what the head's f32
parameters can represent), used as exactly those values in f64 by the host model.  Inputs: encoder_model.make_obs.

Shapes (the smallest that reach every code path): S=32 N=1 (deepest level 1x1: every neighbour is the zero edge; one tile per
level), S=64 N=3 (several envs in the K split of the weight gradient), S=96 N=2 (H = 3, 6, 12, 24, 48: partial 4-, 8- and
16-tiles); preset "ppo" on all three, "segmenter" on S=64.  In all of these a block of the weight gradient
(occ_dec_bwd_dw_kernel) owns one pixel tile.  The split cases give it a slice of several (tests/decoder_split_model.py, whose
reach is asserted without a GPU in tests/test_decoder_train_host.py): "ppo" S=96 N=65 has 2, 2, 2, 2, 5 tiles per slice on
levels 0 to 4, a short last slice on levels 0, 2 and 3 and slices that cross an env boundary on levels 2 to 4 (9 and 36 tiles
per env); "segmenter" S=64 N=130 has 3, 1, 2, 2, 5 with a short last slice on level 0 (the dense preset's f64 encode is
cheap, so the large N is there).  At "ppo" S=96 N=65 the backward also runs with an upstream gradient in one env alone,
where a tile given to the wrong env or dropped from the last slice is the whole signal; at "segmenter" S=64 N=130 it runs
through the C entry points on guarded buffers of exactly the queried sizes, and again after everything it may only write was
filled with NaNs; at "ppo" S=64 N=3 with the classifier scaled until the stored f32 p is exactly 0 or 1.

Bars.  Kept relu outputs: within 1e-4 max(1, max |r64|) of the f64 relu(u).  Gates r > 0: may differ from the f64 gate only
where |u64| <= 1e-4 max(1, max |u64|), on at most 1e-3 of the elements; the band itself holds at most 1e-3 of the elements
for these seeds (asserted).  Gradients: per tensor max |got - want| <= 1e-4 max |want| (no floor), the oracle evaluated with
the GPU's own gate (relu(u) replaced by u * gate), so that a flipped borderline pixel is judged by the gate test and not
smeared into every weight sum.

Measured on an MI355X against the f64 model (worst relative error per tensor kind; the bar is 1e-4):
                     conv.weight  conv.bias  bn.weight  bn.bias  classifier weight  bias
  one tile per block   8.8e-7      5.6e-7     1.5e-6    5.5e-7       5.1e-7        1.8e-7
  split cases          7.2e-7      7.5e-7     7.1e-7    5.3e-7       2.1e-7        1.8e-7
  one env alone        1.3e-6      3.2e-7     7.9e-7    5.8e-7       1.1e-7        2.4e-8
  saturated p          1.5e-6      3.3e-7     3.3e-7    2.5e-7       6.6e-8        8.2e-8
Kept relu outputs at the split cases: 1.9e-6; one gate differed from the f64 gate ("ppo" S=96 N=65, level 1), inside the
band.  Largest band share 3.7e-4 and 4.1e-4.  With `env` taken from the slice's first tile, or with the tile loop ended after
one tile, every gradient test of the split cases and both one-env tests fail and every one-tile case still passes."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import criterion_model, decoder_split_model
from tests.encoder_model import make_obs
from tests.segmenter_model import PRESETS, encode_full, golden_seg_state_dict, up_conv
from tests.train_utils import GUARD, bce64, dice64
from tests.train_utils import guarded as _guarded

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segmenter_golden.npz")
TOL = 1e-4
BAND_SHARE = 1e-3
SPLIT_CASES = [("ppo", 96, 65), ("segmenter", 64, 130)]  # several tiles per block of the weight gradient, see the docstring
assert SPLIT_CASES == decoder_split_model.SPLIT_CASES  # what they reach is asserted on the host (test_decoder_train_host.py)
CASES = [("ppo", 32, 1), ("ppo", 64, 3), ("ppo", 96, 2), ("segmenter", 64, 3)] + SPLIT_CASES
IDS = [f"{p}-S{s}-N{n}" for p, s, n in CASES]
WORST = {}  # measured worst relative error per tensor kind (printed with -s)


def _seed(img, n):
    return 4000 + img + n


@pytest.fixture(scope="module")
def nets():
    from occlusionenv_amd.encoder import FrozenEncoder

    g = np.load(GOLDEN)
    out = {}
    for preset in ("ppo", "segmenter"):
        sd32 = {k: (v.float() if v.is_floating_point() else v) for k, v in golden_seg_state_dict(g, preset).items()}
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd32.items()}
        out[preset] = (sd64, FrozenEncoder.from_state_dict(sd32, preset=preset))
    return out


def _param_keys(preset):
    p = PRESETS[preset]
    keys = [f"{p['decoder']}{j}.up.{t}" for j in range(5) for t in ("conv.weight", "conv.bias", "bn.weight", "bn.bias")]
    return keys + [p["classifier"] + "weight", p["classifier"] + "bias"]


class HostModel:
    """The f64 model with the encoder detached: ``forward(gates)`` -> prob with autograd through the 22 parameters."""

    def __init__(self, sd, preset, obs64):
        self.sd, self.preset, self.p = dict(sd), preset, PRESETS[preset]
        sep = (self.p["prefix"] + "initial.conv.0.weight") in sd
        with torch.no_grad():
            self.x_last, self.skips = encode_full(sd, obs64, self.p["prefix"], sep, self.p["dilation"], self.p["residual"])
        self.pooled = self.x_last.mean(dim=(2, 3))
        self.params = {k: sd[k].clone().requires_grad_() for k in _param_keys(preset)}
        self.sd.update(self.params)

    def forward(self, gates=None):
        """-> (prob, [u_j detached]); ``gates``: relu(u) is replaced by u * gate."""
        logit, us = self.logit(gates)
        return torch.sigmoid(logit), us

    def logit(self, gates=None):
        """-> (logit, [u_j detached]): ``forward`` before the sigmoid."""
        sd, x, us = self.sd, self.x_last, []
        for j, y in enumerate(self.skips[::-1]):
            stem = f"{self.p['decoder']}{j}.up."
            u = up_conv(x, sd, stem)
            us.append(u.detach())
            r = torch.relu(u) if gates is None else u * gates[j]
            x = F.batch_norm(r, sd[stem + "bn.running_mean"], sd[stem + "bn.running_var"], sd[stem + "bn.weight"],
                             sd[stem + "bn.bias"], False, 0.0, 1e-5) + y
        return F.conv2d(x, sd[self.p["classifier"] + "weight"], sd[self.p["classifier"] + "bias"]), us

    def grads(self, loss):
        for v in self.params.values():
            v.grad = None
        loss.backward()
        return {k: v.grad.clone() for k, v in self.params.items()}


def _head_grads(head):
    return {k: p.grad.detach().clone() for k, p in head.named_parameters()}


@pytest.fixture(scope="module")
def runs(nets):
    """Per case, computed once and left unchanged: one native forward + backward with a seeded randn upstream gradient, the
    kept relu outputs, and the host model."""
    from occlusionenv_amd.seghead import SegmentationHead

    cache = {}

    def get(preset, img, n):
        key = (preset, img, n)
        if key not in cache:
            sd, enc = nets[preset]
            obs64 = make_obs(_seed(img, n), n, img)
            obs = obs64.float().cuda()
            head = SegmentationHead.from_encoder(enc)
            feats, prob = head(obs, return_features=True)
            gen = torch.Generator().manual_seed(_seed(img, n) + 1)
            up = torch.randn(n, 1, img, img, generator=gen)
            target = (torch.rand(n, 1, img, img, generator=gen) > 0.5).float()
            head.zero_grad()
            prob.backward(up.cuda())
            kept = [head._kept_relu(j).cpu().clone() for j in range(5)]
            cache[key] = dict(sd=sd, enc=enc, head=head, obs=obs, feats=feats.detach(), prob=prob.detach(), up=up, target=target,
                              kept=kept, grads={k: v.cpu() for k, v in _head_grads(head).items()}, host=HostModel(sd, preset, obs64))
        return cache[key]

    return get


def _check_grads(what, got, want):
    for k, w in want.items():
        scale = float(w.abs().max())
        err = float((got[k].double().cpu() - w).abs().max()) / scale
        kind = k.rsplit(".", 2)[-2] + "." + k.rsplit(".", 1)[-1]
        WORST[kind] = max(WORST.get(kind, 0.0), err)
        print(f"{what} {k}: max|want| {scale:.3g}, relative error {err:.3g}")
    for k, w in want.items():
        scale = float(w.abs().max())
        assert got[k].shape == w.shape and got[k].dtype == torch.float32
        assert float((got[k].double().cpu() - w).abs().max()) <= TOL * scale, (what, k)


@pytest.mark.parametrize("preset,img,n", CASES, ids=IDS)
def test_forward_identity(runs, preset, img, n):
    r = runs(preset, img, n)
    assert r["prob"].shape == (n, 1, img, img)
    assert torch.equal(r["prob"], r["enc"].segment(r["obs"]))
    assert torch.equal(r["feats"], r["enc"](r["obs"]))


@pytest.mark.parametrize("preset,img,n", CASES, ids=IDS)
def test_kept_relu_and_gate(runs, preset, img, n):
    r = runs(preset, img, n)
    with torch.no_grad():
        _prob, us = r["host"].forward()
    for j, (u64, got) in enumerate(zip(us, r["kept"])):
        assert got.shape == u64.shape
        r64 = torch.relu(u64)
        err = float((got.double() - r64).abs().max()) / max(1.0, float(r64.abs().max()))
        band = u64.abs() <= TOL * max(1.0, float(u64.abs().max()))
        share = float(band.double().mean())
        differ = (got > 0) != (u64 > 0)
        print(f"{preset} S={img} N={n} level {j}: relu error {err:.3g}, band share {share:.3g}, gates differing {int(differ.sum())}")
        assert share <= BAND_SHARE, (j, share)  # a property of the seeds, checked on the f64 model alone
        assert err <= TOL, (j, err)
        assert not bool((differ & ~band).any()), (j, int((differ & ~band).sum()))
        assert float(differ.double().mean()) <= BAND_SHARE


@pytest.mark.parametrize("preset,img,n", CASES, ids=IDS)
def test_gradients_against_f64_autograd(runs, preset, img, n):
    r = runs(preset, img, n)
    host = r["host"]
    gates = [(k > 0).double() for k in r["kept"]]
    prob, _us = host.forward(gates)
    want = host.grads((prob * r["up"].double()).sum())
    assert len(want) == 22
    _check_grads(f"{preset} S={img} N={n}", r["grads"], want)
    print("worst so far:", {k: f"{v:.3g}" for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("loss", ["dice", "bce"])
@pytest.mark.parametrize("preset,img,n", CASES, ids=IDS)
def test_gradients_through_the_losses(runs, preset, img, n, loss):
    from occlusionenv_amd import segmentation

    r = runs(preset, img, n)
    head, host = r["head"], r["host"]
    head.zero_grad()
    prob = head(r["obs"])
    native = segmentation.binary_dice_loss if loss == "dice" else segmentation.binary_cross_entropy
    value = native(prob, r["target"].cuda())
    value.backward()
    got = _head_grads(head)
    gates = [(head._kept_relu(j).cpu() > 0).double() for j in range(5)]
    p64, _us = host.forward(gates)
    value64 = (dice64 if loss == "dice" else bce64)(p64, r["target"])
    want = host.grads(value64)
    assert abs(float(value.detach()) - float(value64.detach())) <= TOL * max(1.0, abs(float(value64.detach())))
    _check_grads(f"{loss} {preset} S={img} N={n}", got, want)


def test_reproducible_overwrite_and_accumulation(runs):
    import ctypes as C

    from occlusionenv_amd import _native as nat
    from occlusionenv_amd.encoder import decoder_packed_floats

    r = runs("ppo", 64, 3)
    head, obs, up = r["head"], r["obs"], r["up"].cuda()
    head.zero_grad()
    head(obs).backward(up)
    once = _head_grads(head)
    assert all(torch.equal(once[k].cpu(), r["grads"][k]) for k in once)  # the same bits as the fixture's call
    # without zero_grad the second pass accumulates as torch does: g + g, exact
    head(obs).backward(up)
    twice = _head_grads(head)
    assert all(torch.equal(twice[k], once[k] + once[k]) for k in once)
    head.zero_grad()
    head(obs).backward(up)
    assert all(torch.equal(v, once[k]) for k, v in _head_grads(head).items())
    # the native call overwrites grad_packed: garbage in the buffer changes no bit
    n, img = 3, 64
    ws, scratch = head._train_buffers(n, img)
    enc = head.enc
    outs = []
    for fill in (0.0, 123.0):
        gp = torch.full((decoder_packed_floats(),), fill, device="cuda")
        nat.check(nat.load().occ_segment_backward(C.byref(enc._cfg(img)), nat.ptr(enc.dec_packed), n, nat.ptr(ws), ws.numel(),
                                                  nat.ptr(up), nat.ptr(scratch), scratch.numel(), nat.ptr(gp),
                                                  nat.stream_ptr(up.device)), "occ_segment_backward")
        outs.append(gp)
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())


@pytest.mark.parametrize("env", [64, 1])
def test_gradients_of_one_env(runs, env):
    """The upstream gradient is randn in one env and zero in the others, so that env's tiles are the whole signal: env 64
    alone fills the short last slice of level 0; env 1 is where the first slices that cross an env boundary on levels 2 to
    4 end (asserted on the host model, test_decoder_train_host.py)."""
    preset, img, n = SPLIT_CASES[0]
    r = runs(preset, img, n)
    head, host = r["head"], r["host"]
    up = torch.zeros(n, 1, img, img)
    up[env] = torch.randn(1, img, img, generator=torch.Generator().manual_seed(_seed(img, n) + 2 + env))
    head.zero_grad()
    prob = head(r["obs"])
    assert torch.equal(prob.detach(), r["prob"])
    prob.backward(up.cuda())
    got = _head_grads(head)
    gates = [(head._kept_relu(j).cpu() > 0).double() for j in range(5)]
    p64, _us = host.forward(gates)
    want = host.grads((p64 * up.double()).sum())
    assert len(want) == 22
    _check_grads(f"one-hot env {env} {preset} S={img} N={n}", got, want)


def test_no_stale_reads_and_nothing_outside_the_reported_sizes(runs):
    """The native calls on buffers of exactly the queried sizes, each the middle of a larger allocation that is inspected
    afterwards; then the backward again after everything it may only write (scratch, the two gradient buffers at the end of
    the workspace, grad_packed) has been filled with NaNs: the same bits, so nothing read was left over from before."""
    import ctypes as C

    from occlusionenv_amd import _native as nat
    from occlusionenv_amd.encoder import FEATURES, decoder_packed_floats

    preset, img, n = SPLIT_CASES[1]
    r = runs(preset, img, n)
    enc, obs, up = r["enc"], r["obs"], r["up"].cuda()
    lib, cfg, st = nat.load(), enc._cfg(img), nat.stream_ptr(obs.device)
    wsb, scb = C.c_size_t(), C.c_size_t()
    nat.check(lib.occ_segment_train_workspace_query(C.byref(cfg), n, C.byref(wsb), C.byref(scb)), "occ_segment_train_workspace_query")
    sizes = dict(ws=int(wsb.value), scratch=int(scb.value), grad_packed=4 * decoder_packed_floats(), prob=4 * n * img * img,
                 feats=4 * n * FEATURES)
    assert sizes["scratch"] == decoder_split_model.scratch_bytes(img, n)
    bufs = {k: _guarded(b) for k, b in sizes.items()}
    mid = {k: whole[lo:lo + sizes[k]] for k, (whole, lo) in bufs.items()}
    assert all(m.data_ptr() % 256 == 0 for m in mid.values())

    def backward():
        nat.check(lib.occ_segment_backward(C.byref(cfg), nat.ptr(enc.dec_packed), n, nat.ptr(mid["ws"]), sizes["ws"], nat.ptr(up),
                                           nat.ptr(mid["scratch"]), sizes["scratch"], nat.ptr(mid["grad_packed"]), st),
                  "occ_segment_backward")
        return mid["grad_packed"].view(torch.float32).clone()

    nat.check(lib.occ_segment_train_forward(C.byref(cfg), nat.ptr(enc.packed), nat.ptr(enc.dec_packed), nat.ptr(obs), n,
                                            nat.ptr(mid["ws"]), sizes["ws"], nat.ptr(mid["feats"]), nat.ptr(mid["prob"]), st),
              "occ_segment_train_forward")
    prob, feats = mid["prob"].clone(), mid["feats"].clone()
    assert torch.equal(prob.view(torch.float32).view(n, 1, img, img), r["prob"])
    assert torch.equal(feats.view(torch.float32).view(n, FEATURES), r["feats"])
    a = backward()
    lvl = decoder_split_model.level_bytes(img, n)
    nan = 0x7FC00000
    assert sizes["scratch"] % 4 == 0
    mid["scratch"].view(torch.int32).fill_(nan)
    tail = lvl[4] + lvl[3]  # g0 | g1, the end of the layout in include/occlusionenv_amd.h
    mid["ws"][sizes["ws"] - tail:].view(torch.int32).fill_(nan)
    mid["grad_packed"].view(torch.int32).fill_(nan)
    assert bool(torch.isnan(mid["grad_packed"].view(torch.float32)).all())
    b = backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(mid["prob"], prob) and torch.equal(mid["feats"], feats)  # the backward writes neither
    for k, (whole, lo) in bufs.items():
        assert lo >= GUARD and whole.numel() - (lo + sizes[k]) >= GUARD
        assert bool((whole[:lo] == 0xA5).all()), f"bytes in front of {k} were written"
        assert bool((whole[lo + sizes[k]:] == 0xA5).all()), f"bytes behind {k} were written"


@pytest.mark.parametrize("loss", ["dice", "bce"])
@pytest.mark.parametrize("factor", [64, 512])
def test_saturated_probabilities(runs, factor, loss):
    """Classifier weight and bias times ``factor``: the stored f32 p is exactly 1 (and, at 512, exactly 0) on many pixels.
    The contract is dz = g p (1 - p) from the stored p, so dz = 0 there although BCE's g is of order 1e12 x coef: the oracle
    takes the GPU's p, g from criterion_model at that p, dz in f64, and back-propagates sum(logit dz) through the host model.

    1 / (1 + expf(-z)) is exactly 1 for z > 17.4 and exactly 0 only once expf overflows, z < -88.8.  This case's logits lie
    in [-0.262, 1.102], so 64 saturates the upper end only ([-16.8, 70.5]); 512 ([-134, 564]) saturates both."""
    from occlusionenv_amd import segmentation
    from occlusionenv_amd.seghead import SegmentationHead

    preset, img, n = "ppo", 64, 3
    r = runs(preset, img, n)
    sd, cls = dict(r["sd"]), PRESETS[preset]["classifier"]
    head = SegmentationHead.from_encoder(r["enc"])
    with torch.no_grad():
        for t in ("weight", "bias"):
            head.get_parameter(cls + t).mul_(float(factor))
            sd[cls + t] = sd[cls + t] * float(factor)  # a power of two: the same values in f32 and in f64
    target = r["target"]
    prob = head(r["obs"])
    p32 = prob.detach().cpu()
    one, zero = p32 == 1.0, p32 == 0.0
    print(f"factor {factor}: {int(one.sum())} pixels with p == 1, {int(zero.sum())} with p == 0, of {p32.numel()}")
    assert bool((target[one] == 1).any()) and bool((target[one] == 0).any())
    if factor == 512:
        assert bool((target[zero] == 1).any()) and bool((target[zero] == 0).any())
    native = segmentation.binary_dice_loss if loss == "dice" else segmentation.binary_cross_entropy
    native(prob, target.cuda()).backward()
    got = _head_grads(head)
    assert len(got) == 22 and all(bool(torch.isfinite(v).all()) for v in got.values())
    g = (criterion_model.dice_grad if loss == "dice" else criterion_model.bce_grad)(p32, target)
    dz = g * p32.double() * (1.0 - p32.double())
    assert bool((dz[one] == 0).all()) and bool((dz[zero] == 0).all())
    host = HostModel(sd, preset, r["obs"].double().cpu())
    gates = [(head._kept_relu(j).cpu() > 0).double() for j in range(5)]
    logit, _us = host.logit(gates)
    want = host.grads((logit * dz).sum())
    _check_grads(f"saturated x{factor} {loss} {preset} S={img} N={n}", got, want)


@pytest.fixture(scope="module")
def trained(runs):
    """Five AdamW steps at lr 1e-3 on a fixed batch (S=64, N=3): the f64 host model first, then the native head."""
    from occlusionenv_amd import segmentation
    from occlusionenv_amd.seghead import SegmentationHead

    r = runs("ppo", 64, 3)
    sd, enc = r["sd"], r["enc"]
    host = HostModel(sd, "ppo", r["obs"].double().cpu())
    opt = torch.optim.AdamW(list(host.params.values()), lr=1e-3, weight_decay=1e-5)
    host_losses = []
    for _ in range(6):  # five steps, and the loss after the fifth
        opt.zero_grad()
        loss = dice64(host.forward()[0], r["target"])
        host_losses.append(float(loss))
        if len(host_losses) <= 5:
            loss.backward()
            opt.step()
    head = SegmentationHead.from_encoder(enc)
    before = {k: v.detach().clone() for k, v in head.named_parameters()}
    opt = torch.optim.AdamW(head.parameters(), lr=1e-3, weight_decay=1e-5)
    target = r["target"].cuda()
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = segmentation.binary_dice_loss(head(r["obs"]), target)
        losses.append(float(loss))
        if len(losses) <= 5:
            loss.backward()
            opt.step()
    return dict(head=head, before=before, host_losses=host_losses, losses=losses, obs=r["obs"], enc=enc, prob0=r["prob"])


def test_learning(trained):
    print("host Dice:", trained["host_losses"], "native Dice:", trained["losses"])
    assert trained["host_losses"][-1] < trained["host_losses"][0]
    assert trained["losses"][-1] < trained["losses"][0]
    assert all(not torch.equal(v, trained["before"][k]) for k, v in trained["head"].named_parameters())


def test_round_trip_into_a_frozen_encoder(trained):
    from occlusionenv_amd.encoder import DECODER_KEYS

    head, enc, obs = trained["head"], trained["enc"], trained["obs"]
    sd = head.state_dict()
    dp, dc = DECODER_KEYS["ppo"]
    assert dp + "0.up.conv.weight" in sd and dp + "4.up.bn.running_var" in sd and dc + "bias" in sd
    assert tuple(sd[dp + "0.up.conv.weight"].shape) == (256, 128, 3, 3)
    assert all(k.startswith("ckpt.") for k in head.state_dict(prefix="ckpt."))
    tuned = enc.with_decoder(sd)
    with torch.no_grad():
        now = head(obs)
    assert torch.equal(tuned.segment(obs), now)
    assert not torch.equal(now, trained["prob0"])
    assert torch.equal(enc.segment(obs), trained["prob0"])  # the untouched encoder keeps its map
    assert torch.equal(tuned(obs), enc(obs))


def test_errors(nets, runs):
    from occlusionenv_amd._native import NativeError
    from occlusionenv_amd.encoder import FrozenEncoder
    from occlusionenv_amd.seghead import SegmentationHead

    sd, enc = nets["ppo"]
    r = runs("ppo", 64, 3)
    head = r["head"]
    enc.max_chunk = 2
    try:
        with pytest.raises(ValueError, match="max_chunk"):
            head(r["obs"])
    finally:
        enc.max_chunk = 256
    with pytest.raises(ValueError, match="multiple of 32"):
        head(torch.zeros(1, 4, 48, 48, device="cuda"))
    with pytest.raises(NativeError):
        head(torch.zeros(1, 4, 64, 64))
    bare = FrozenEncoder.from_state_dict({k: v for k, v in sd.items() if not k.startswith("segmenter.")}, preset="ppo")
    with pytest.raises(ValueError, match="no segmentation decoder"):
        SegmentationHead.from_encoder(bare)
    first = head(r["obs"])
    second = head(r["obs"][:1])
    with pytest.raises(RuntimeError, match="superseded"):
        first.sum().backward()
    head.zero_grad()
    second.sum().backward()  # the latest forward still has its activations
    assert all(p.grad is not None for p in head.parameters())


def test_finetune_segmentation_harness(nets):
    from environment import OcclusionEnv
    from occlusionenv_amd import environment, harness
    from occlusionenv_amd.meshes import SyntheticShapeNet
    from occlusionenv_amd.seghead import SegmentationHead
    from SubProcVecEnv import SimpleVecEnv

    ds = SyntheticShapeNet(n_models=8, seed=1234)
    environment.seed_scene_rng(77)
    np.random.seed(77)
    torch.manual_seed(77)
    venv = SimpleVecEnv([lambda: OcclusionEnv(ds, img_size=128) for _ in range(16)])
    head = SegmentationHead.from_encoder(nets["ppo"][1])
    before = {k: v.detach().clone() for k, v in head.named_parameters()}
    res = harness.finetune_segmentation(venv, head, 3)
    assert res["head"] is head and res["steps"] == 3
    for key in ("losses", "accuracy", "iou"):
        assert len(res[key]) == 3
    assert all(np.isfinite(v) for v in res["losses"]) and all(0.0 <= v <= 100.0 for v in res["accuracy"])
    assert all(not torch.equal(v, before[k]) for k, v in head.named_parameters())
    # from an encoder: a head is made, with BCE
    res = harness.finetune_segmentation(venv, nets["ppo"][1], 1, use_dice=False)
    assert isinstance(res["head"], SegmentationHead) and np.isfinite(res["losses"][0])
