"""GPU tests of the fused pretrainer criterion (occlusionenv_amd/ops.py: seg_criterion, binary_dice_loss,
binary_cross_entropy; encoder.py: validation_losses; harness.py: validate_pretrained; csrc/occ_criterion.hpp) against the
f64 host model (tests/criterion_model.py) and the reference-produced fixture (tests/golden/criterion_golden.npz).

Shapes: S = 32 (fewer pixels than one block's 4 096), S = 96 (three blocks, the last one ragged: 9 216 = 2 x 4 096 + 1 024),
S = 33 (an odd pixel count: the 4-byte load path, ragged inside a group of four), N in {1, 3, 5}; targets contiguous, with
pixel stride 4 (``(N,S,S,4)[..., 3]``, read in place) and transposed (no pixel stride describes it: the wrapper's
contiguous fallback).

Bars.  Counts: exact.  Sums and losses: TOL = 1e-4 relative to max(1, |value|), the bar of this kernel family
(tests/test_gpu_encoder.py, tests/test_gpu_segmenter.py), with S_bce compared as its per-pixel mean.  Gradients: 1e-4
relative with an absolute floor of 1e-4 x the env's max |model gradient|.  What the kernels should reach is far tighter
(csrc/occ_criterion.hpp: every addition is f64, the only f32 roundings are two logf per pixel and the final rounding of the
gradient), so the gradient is ALSO held to 2e-7 x |model| + 1e-12 x the env's max: one f32 rounding (2^-24 = 6e-8) with a
factor 3 of slack, plus the f64 error of the coefficients where a t + b p cancels.

Worst errors measured on an MI355X (printed with -s): see DESIGN.md §4.4."""
import os

import numpy as np
import pytest
import torch

from tests import criterion_model as cm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "criterion_golden.npz")
SEG_GOLDEN = os.path.join(HERE, "golden", "segmenter_golden.npz")
TOL = 1e-4
LAYOUTS = ["contiguous", "stride4", "transposed"]
WORST = {}


def _note(key, err):
    WORST[key] = max(WORST.get(key, 0.0), float(err))
    print(f"{key}: {float(err):.3g} (worst so far {WORST[key]:.3g})")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


_CASES = {}


def case(n, img, soft):
    """(pred f32 (n,1,S,S) on the GPU, target f32 (n,S,S) on the host, the host model's sums), computed once."""
    key = (n, img, soft)
    if key not in _CASES:
        pred, target = cm.make_maps(1000 + 10 * img + n + (500 if soft else 0), n, img, soft)
        _CASES[key] = (pred, target, cm.sums(pred, target))
    pred, target, want = _CASES[key]
    return pred.clone(), target.clone(), want


def lay_out(target, layout):
    """``target`` (n,S,S) on the GPU in the given memory layout; the values are the same."""
    t = target.cuda()
    if layout == "contiguous":
        return t
    if layout == "stride4":
        fs = torch.rand(*t.shape, 4, device="cuda")
        fs[..., 3] = t
        v = fs[..., 3]
        assert v.stride(2) == 4 and not v.is_contiguous()
        return v
    v = t.transpose(1, 2).contiguous().transpose(1, 2)
    assert v.stride(2) == t.shape[1] and v.stride(1) == 1
    return v


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.double().cpu()
    return float(((got - want).abs() / want.abs().clamp_min(1.0)).max())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("img", [32, 96, 33])
def test_counts_sums_and_losses(img, n, layout):
    from occlusionenv_amd import ops
    from occlusionenv_amd.encoder import seg_counts

    soft = (n + img) % 2 == 0
    pred, target, want = case(n, img, soft)
    pred_d, tgt = pred[:, None].cuda(), lay_out(target, layout)
    got = ops.seg_criterion(pred_d, tgt)
    for k in ("correct", "intersection", "union"):
        assert got[k].dtype == torch.int64 and got[k].is_cuda and torch.equal(got[k].cpu(), want[k]), k
    assert torch.equal(torch.stack([got["correct"], got["intersection"], got["union"]], 1), seg_counts(pred_d, tgt))
    for k in ("s_pt", "s_pp", "s_tt"):
        assert got[k].dtype == torch.float64 and got[k].shape == (n,)
        e = _rel(got[k], want[k])
        _note("sums", e)
        assert e <= TOL, (k, e)
    e = _rel(got["s_bce"] / (img * img), want["s_bce"] / (img * img))
    _note("bce mean", e)
    assert e <= TOL, e
    for red in ("mean", "sum", "none"):
        e = _rel(ops.binary_dice_loss(pred_d, tgt, reduction=red), cm.dice_loss(pred, target, reduction=red))
        _note("dice loss", e)
        assert e <= TOL, (red, e)
    e = _rel(ops.binary_dice_loss(pred_d, tgt, smooth=0.25), cm.dice_loss(pred, target, smooth=0.25))
    assert e <= TOL, e
    loss = ops.binary_cross_entropy(pred_d, tgt)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    e = _rel(loss, cm.bce_loss(pred, target))
    _note("bce loss", e)
    assert e <= TOL, e


def _sums(pred, target):
    from occlusionenv_amd import ops

    c = ops.seg_criterion(pred, target)
    return torch.stack([c["s_pt"], c["s_pp"], c["s_tt"], c["s_bce"]], 1)


@pytest.mark.parametrize("img", [96, 33])
def test_sums_are_bitwise_reproducible(img):
    pred, target, _want = case(5, img, True)
    pred, target = pred.cuda(), target.cuda()
    a = _sums(pred, target)
    assert torch.equal(_sums(pred, target), a)  # two runs of the same call
    for i in range(5):
        assert torch.equal(_sums(pred[i:i + 1], target[i:i + 1])[0], a[i]), i  # the env alone
    perm = torch.roll(torch.arange(5), 2)
    assert torch.equal(_sums(pred[perm], target[perm]), a[perm])  # at another position
    assert torch.equal(_sums(pred[1:4], target[1:4]), a[1:4])  # in a smaller batch
    # the load width is chosen from alignment and stride: it changes no bit either
    for layout in ("stride4", "transposed"):
        assert torch.equal(_sums(pred, lay_out(target.cpu(), layout)), a), layout
    buf = torch.empty(pred.numel() + 1, device="cuda")
    shifted = buf[1:].view_as(pred).copy_(pred)  # 4 bytes off the 16-byte alignment
    assert shifted.data_ptr() % 16 == 4 and torch.equal(_sums(shifted, target), a)


def _check_grad(key, got, want):
    """The issue's bar, then the derived one (module docstring)."""
    assert got.dtype == torch.float32 and got.shape == want.shape
    got, want = got.double().cpu(), want.double()
    n = want.shape[0]
    env_max = want.reshape(n, -1).abs().max(1).values.reshape(n, *([1] * (want.dim() - 1)))
    err = (got - want).abs()
    _note(key + " grad / env max", float((err / env_max).max()))
    assert bool((err <= torch.maximum(TOL * want.abs(), TOL * env_max)).all()), key
    tight = err - (2e-7 * want.abs() + 1e-12 * env_max)
    _note(key + " grad rel (nonzero entries)", float((err / want.abs().clamp_min(1e-300))[want != 0].max()))
    assert float(tight.max()) <= 0.0, (key, float(tight.max()))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("img", [32, 96, 33])
def test_gradient_against_host_model(img, layout):
    from occlusionenv_amd import ops

    for soft in (False, True):
        pred, target, _want = case(3, img, soft)
        assert int((pred == 0).sum()) >= 3 and int((pred == 1).sum()) >= 3  # the BCE floor and the clamp are reached
        tgt = lay_out(target, layout)
        for red in ("mean", "sum"):
            p = pred[:, None].cuda().requires_grad_(True)
            ops.binary_dice_loss(p, tgt, reduction=red).backward()
            _check_grad("dice", p.grad, cm.dice_grad(pred[:, None], target, reduction=red))
        up = torch.tensor([0.5, -1.25, 2.0], dtype=torch.float64)
        p = pred.cuda().requires_grad_(True)  # the (N,S,S) form
        ops.binary_dice_loss(p, tgt, reduction="none").backward(up.float().cuda())
        _check_grad("dice", p.grad, cm.dice_grad(pred, target, reduction="none", upstream=up))
        p = pred[:, None].cuda().requires_grad_(True)
        ops.binary_cross_entropy(p, tgt).backward()
        _check_grad("bce", p.grad, cm.bce_grad(pred[:, None], target))
        assert not tgt.requires_grad


@pytest.mark.parametrize("name", ["binary", "soft"])
def test_autograd_ops_against_reference_fixture(golden, name):
    from occlusionenv_amd import ops

    n, img = (int(v) for v in golden["n_img"])
    seed = int(golden["seeds"][list(golden["names"]).index(name)])
    pred, target = cm.make_maps(seed, n, img, soft=name == "soft")
    up = torch.from_numpy(golden["none_upstream"])
    for layout in LAYOUTS:
        tgt = lay_out(target, layout)[:, None]  # (N,1,S,S) target, as the dataset yields it
        for red in ("mean", "sum", "none"):
            p = pred[:, None].cuda().requires_grad_(True)
            loss = ops.binary_dice_loss(p, tgt, reduction=red)
            assert loss.shape == ((n,) if red == "none" else ())
            e = _rel(loss, torch.from_numpy(golden[f"{name}_dice_{red}_loss"]))
            _note("fixture dice loss", e)
            assert e <= TOL, (red, e)
            if red == "none":
                loss.backward(up.float().cuda())
            else:
                loss.backward()
            _check_grad("fixture dice", p.grad[:, 0], torch.from_numpy(golden[f"{name}_dice_{red}_grad_f32"]))
        p = pred[:, None].cuda().requires_grad_(True)
        loss = ops.binary_cross_entropy(p, tgt)
        e = _rel(loss, torch.from_numpy(golden[f"{name}_bce_loss"]))
        _note("fixture bce loss", e)
        assert e <= TOL, e
        loss.backward()
        _check_grad("fixture bce", p.grad[:, 0], torch.from_numpy(golden[f"{name}_bce_grad_f32"]))


def test_upstream_scalar_scales_the_gradient():
    """A power-of-two upstream factor scales every f64 coefficient, hence every f32 gradient, exactly (no value here is
    near the subnormal range); any other factor to within the roundings of the coefficient and of the result."""
    from occlusionenv_amd import ops

    pred, target, _want = case(3, 96, True)
    tgt = target.cuda()
    for fn in (ops.binary_dice_loss, ops.binary_cross_entropy):
        p = pred[:, None].cuda().requires_grad_(True)
        (base,) = torch.autograd.grad(fn(p, tgt), p)
        for factor in (0.25, -8.0):
            (g,) = torch.autograd.grad(fn(p, tgt), p, grad_outputs=torch.tensor(factor, device="cuda"))
            assert torch.equal(g, base * factor), (fn.__name__, factor)
        (g,) = torch.autograd.grad(fn(p, tgt) * 3.0, p)  # through another node
        assert float(((g.double() - 3.0 * base.double()).abs() / (3.0 * base.double().abs()).clamp_min(1e-300))[base != 0].max()) <= 2e-7
        assert bool((base != 0).any())


def test_rejections():
    from occlusionenv_amd import ops
    from occlusionenv_amd._native import NativeError

    a = torch.zeros(2, 1, 32, 32, device="cuda")
    with pytest.raises(NativeError):
        ops.seg_criterion(a, torch.zeros(2, 32, 32))
    with pytest.raises(ValueError, match="differ"):
        ops.binary_dice_loss(a, torch.zeros(2, 64, 64, device="cuda"))
    with pytest.raises(ValueError, match="differ"):
        ops.binary_cross_entropy(a, torch.zeros(3, 32, 32, device="cuda"))
    with pytest.raises(ValueError, match=r"\(N,S,S\)"):
        ops.seg_criterion(torch.zeros(2, 3, 32, 32, device="cuda"), a)
    empty = ops.seg_criterion(a[:0], a[:0])
    assert empty["s_pt"].shape == (0,) and empty["union"].shape == (0,)


def test_validate_pretrained_against_f64_chain():
    """Three batches of 4, 4 and 1 observations at 64^2 through the "ppo" network of the segmenter fixture: the five
    numbers of PreTrainer.val() against encode_full -> decode -> the host criterion in f64.  A pixel inside the exempt
    band of the f64 logits (segmenter_model.exempt_band: the only pixels on which the f32 map may threshold differently)
    takes the native map's side in the expected counts; the band holds at most 0.1 % of the pixels."""
    from occlusionenv_amd import harness
    from occlusionenv_amd.encoder import FrozenEncoder
    from tests.encoder_model import make_obs
    from tests.segmenter_model import exempt_band, full_forward, golden_seg_state_dict

    sd = golden_seg_state_dict(np.load(SEG_GOLDEN), "ppo")
    enc = FrozenEncoder.from_state_dict(sd, preset="ppo")
    batches = []
    for b, n in enumerate((4, 4, 1)):
        obs = make_obs(4100 + b, n, 64).float()
        _pred, occl = cm.make_maps(4200 + b, n, 64, soft=b == 1)
        gp, g = cm.make_grad_pairs(4300 + b, n)
        batches.append((obs, occl[:, None], (gp * 40).float(), g))  # host tensors; the dataset's fourth item is not read
    seen = []
    orig = enc.forward_full

    def spy(obs):
        out = orig(obs)
        seen.append(out[1].clone())
        return out

    enc.forward_full = spy
    try:
        for use_dice, use_l1 in ((True, False), (False, True)):
            del seen[:]
            res = harness.validate_pretrained(enc, batches, use_dice=use_dice, use_l1=use_l1)
            assert len(seen) == 3 and res["batches"] == 3 and res["pixels"] == 9 * 64 * 64
            rows, counts = [], np.zeros(3, dtype=np.int64)
            for (obs, occl, grad, _), segm in zip(batches, seen):
                want = full_forward(sd, obs.double(), "ppo")
                band = exempt_band(want["logit"])
                share = float(band.double().mean())
                assert share <= 1e-3, share
                native_map = segm.cpu() > 0.5
                assert not bool(((native_map != (want["logit"] > 0)) & ~band).any())
                v = cm.validation(want["prob"], want["grad"], occl, grad, use_dice, use_l1)
                p = torch.where(band, native_map, want["logit"] > 0).reshape(-1)
                t = (occl > 0.5).reshape(-1)
                c = np.array([int((p == t).sum()), int((p & t).sum()), int((p | t).sum())])
                counts += c
                rows.append([v["loss"], v["segm_loss"], v["grad_loss"], c[0] / p.numel(), c[1] / c[2]])
            mean = np.mean(np.array(rows), axis=0) * np.array([1, 1, 1, 100.0, 100.0])
            print("validate_pretrained", use_dice, use_l1, res, "f64 chain", mean)
            assert (res["correct"], res["intersection"], res["union"]) == tuple(int(x) for x in counts)
            for k, w in zip(("loss", "segm_loss", "grad_loss", "accuracy", "iou"), mean):
                e = abs(res[k] - w) / max(1.0, abs(w))
                _note("validate_pretrained " + k, e)
                assert e <= TOL, (k, res[k], w)
            assert 0.0 < res["iou"] < 100.0 and 0.0 < res["accuracy"] < 100.0 and res["grad_loss"] > 0
    finally:
        del enc.forward_full
