"""GPU tests of the skip mask of the native encoder and decoder (encoder.FrozenEncoder ``skip=`` / ``out=``,
occ_encoder_forward_masked, occ_segment_forward_masked): a skipped row is neither read nor written.

Shapes.  n = 9 envs with max_chunk = 4: a chunk boundary inside the batch, the last chunk a single env, so every chunk
must take its own slice of the mask.  Image side 64 runs the 16-pixel tile kernels at three levels (64, 32, 16) and the
multi-group 8-pixel ones at three (8, 4, 2); side 32 ends at a 1 x 1 last down.  The decoder runs at side 32 (its 8-pixel
kernel at 1, 2, 4, 8, the fused 16-pixel last level at 16).  Both encoder forms: separable, dilation 2, residual (preset
"ppo": occ_enc_sep_kernel, the dense downs, the pooling down) and dense, dilation 1 (preset "predictor": every layer
through occ_enc_dense_kernel); the segmenting calls run the pooling down that also keeps its output.

Every comparison is bitwise, on the int32 view: the sentinel that pre-fills ``out`` is a NaN pattern, and the obs of every
skipped row is NaN, so a block that read a skipped row or wrote one shows."""
import os

import numpy as np
import pytest
import torch

from tests.encoder_model import golden_state_dict, make_obs
from tests.segmenter_model import golden_seg_state_dict

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N, CHUNK = 9, 4
SENTINEL = 0x7FC5A5A5  # a quiet NaN with a payload no kernel produces
MASKS = {
    "none": [0] * N,
    "all": [1] * N,
    "alternating": [i % 2 for i in range(N)],
    "last_active": [1] * (N - 1) + [0],
    "first_skipped": [1] + [0] * (N - 1),
}


@pytest.fixture(scope="module")
def encs():
    """preset -> a FrozenEncoder with max_chunk = 4: both encoder forms, and the FullNetwork with its decoder."""
    from occlusionenv_amd.encoder import FrozenEncoder

    g = np.load(os.path.join(HERE, "golden", "encoder_golden.npz"))
    gs = np.load(os.path.join(HERE, "golden", "segmenter_golden.npz"))
    out = {p: FrozenEncoder.from_state_dict(golden_state_dict(g, p), preset=p, max_chunk=CHUNK) for p in ("ppo", "predictor")}
    out["full"] = FrozenEncoder.from_state_dict(golden_seg_state_dict(gs, "ppo"), preset="ppo", max_chunk=CHUNK)
    assert out["ppo"].separable and out["ppo"].dilation == 2 and out["ppo"].residual
    assert not out["predictor"].separable and out["predictor"].dilation == 1
    assert out["full"].has_decoder and out["full"].grad_w is not None
    return out


_OBS = {}


def _obs(img):
    if img not in _OBS:
        _OBS[img] = make_obs(500 + img, N, img).float().cuda()
    return _OBS[img]


def _mask(name, dtype=torch.int32):
    return torch.tensor(MASKS[name], dtype=dtype, device="cuda")


def _holed(obs, mask):
    """obs with every skipped row NaN."""
    o = obs.clone()
    o[mask != 0] = float("nan")
    return o


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_rows(what, got, ref, mask, untouched=SENTINEL):
    """Skipped rows of ``got`` hold ``untouched`` in every word, the others the bits of ``ref``."""
    m = mask != 0
    g, r = _bits(got), _bits(ref)
    assert g.shape == r.shape, what
    assert bool((g[m] == untouched).all()), f"{what}: a skipped row was written"
    assert torch.equal(g[~m], r[~m]), f"{what}: an active row differs from the unmasked call"


@pytest.mark.parametrize("mask_name", list(MASKS))
@pytest.mark.parametrize("img", [32, 64])
@pytest.mark.parametrize("preset", ["ppo", "predictor"])
def test_encoder_leaves_skipped_rows_alone(encs, preset, img, mask_name):
    enc = encs[preset]
    mask = _mask(mask_name)
    obs = _holed(_obs(img), mask)
    ref_f, ref_g = enc(obs), enc.predict_grad(obs)  # the unmasked call on the same obs
    out = _sentinel(N, 256)
    got = enc(obs, skip=mask, out=out)
    torch.cuda.synchronize()  # (the all-one mask: nothing may have been raised, on the device either)
    assert got.data_ptr() == out.data_ptr()
    _check_rows("features", out, ref_f, mask)
    if mask_name == "none":
        assert torch.equal(_bits(out), _bits(ref_f))
    # a bool mask is the same mask
    out_b = _sentinel(N, 256)
    enc(obs, skip=_mask(mask_name, torch.bool), out=out_b)
    assert torch.equal(_bits(out_b), _bits(out))
    # the grad head: applied to all rows, the skipped ones put back
    gout = _sentinel(N, 2)
    assert enc.predict_grad(obs, skip=mask, out=gout).data_ptr() == gout.data_ptr()
    _check_rows("grad", gout, ref_g, mask)
    # without out: skipped rows are exactly zero (all bits)
    _check_rows("features, fresh", enc(obs, skip=mask), ref_f, mask, untouched=0)
    _check_rows("grad, fresh", enc.predict_grad(obs, skip=mask), ref_g, mask, untouched=0)


@pytest.mark.parametrize("mask_name", list(MASKS))
def test_decoder_leaves_skipped_rows_alone(encs, mask_name):
    enc, img = encs["full"], 32
    mask = _mask(mask_name)
    obs = _holed(_obs(img), mask)
    ref_d, ref_p, ref_l = enc.segment(obs, return_logits=True, return_features=True)
    ref_f, ref_p2, ref_g = enc.forward_full(obs)
    assert torch.equal(_bits(ref_p), _bits(ref_p2))
    out = (_sentinel(N, 8, img, img), _sentinel(N, 1, img, img), _sentinel(N, 1, img, img))
    got = enc.segment(obs, return_logits=True, return_features=True, skip=mask, out=out)
    torch.cuda.synchronize()
    assert [t.data_ptr() for t in got] == [t.data_ptr() for t in out]
    for what, o, r in zip(("decoder feature", "prob", "logits"), out, (ref_d, ref_p, ref_l)):
        _check_rows(what, o, r, mask)
        if mask_name == "none":
            assert torch.equal(_bits(o), _bits(r)), what
    # the map alone: out may be the lone tensor
    lone = _sentinel(N, 1, img, img)
    assert enc.segment(obs, skip=mask, out=lone).data_ptr() == lone.data_ptr()
    assert torch.equal(_bits(lone), _bits(out[1]))
    # forward_full: pooled feature, map and grad head
    fout = (_sentinel(N, 256), _sentinel(N, 1, img, img), _sentinel(N, 2))
    got = enc.forward_full(obs, skip=mask, out=fout)
    assert [t.data_ptr() for t in got] == [t.data_ptr() for t in fout]
    for what, o, r in zip(("pooled", "segm", "grad"), fout, (ref_f, ref_p, ref_g)):
        _check_rows("forward_full " + what, o, r, mask)
    # without out: zeros
    for what, o, r in zip(("decoder feature", "prob", "logits"),
                          enc.segment(obs, return_logits=True, return_features=True, skip=mask), (ref_d, ref_p, ref_l)):
        _check_rows(what + ", fresh", o, r, mask, untouched=0)
    for what, o, r in zip(("pooled", "segm", "grad"), enc.forward_full(obs, skip=mask), (ref_f, ref_p, ref_g)):
        _check_rows("forward_full " + what + ", fresh", o, r, mask, untouched=0)


def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()  # warm-up: the workspaces exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


@pytest.mark.parametrize("kind", ["encoder", "segment"])
def test_graph_replay_follows_the_mask_it_finds(encs, kind):
    """One captured masked forward; the mask tensor is overwritten in place between replays."""
    img = 32
    enc = encs["ppo"] if kind == "encoder" else encs["full"]
    obs = _obs(img)
    mask = _mask("alternating")
    out = (_sentinel(N, 256),) if kind == "encoder" else (_sentinel(N, 1, img, img),)
    run = (lambda o, m: enc(obs, skip=m, out=o[0])) if kind == "encoder" else (lambda o, m: enc.segment(obs, skip=m, out=o[0]))
    graph = _capture(lambda: run(out, mask))
    for name in ("alternating", "first_skipped", "all", "none"):
        mask.copy_(_mask(name))
        out[0].copy_(_sentinel(*out[0].shape))
        graph.replay()
        torch.cuda.synchronize()
        eager = (_sentinel(*out[0].shape),)
        run(eager, _mask(name))
        assert torch.equal(_bits(out[0]), _bits(eager[0])), name
        assert bool((_bits(out[0])[mask != 0] == SENTINEL).all()), name
        assert not bool((_bits(out[0])[mask == 0] == SENTINEL).any()), name


def test_batched_ppo_features_and_actions(encs):
    from occlusionenv_amd import ppo

    gs = np.load(os.path.join(HERE, "golden", "segmenter_golden.npz"))
    agent = ppo.BatchedPPO.from_fullnetwork(golden_seg_state_dict(gs, "ppo"), max_chunk=CHUNK, seed=0)
    pooled = ppo.BatchedPPO(device="cuda", seed=0)  # no encoder: 8 x 8 average pooling
    mask = _mask("alternating")
    clean = _obs(32)
    obs = _holed(clean, mask)
    for what, a in (("encoder", agent), ("pooled", pooled)):
        ref = a.features(clean)
        out = _sentinel(N, 256)
        assert a.features(obs, skip=mask, out=out).data_ptr() == out.data_ptr()
        _check_rows(what + " features", out, ref, mask)
        _check_rows(what + " features, fresh", a.features(obs, skip=mask), ref, mask, untouched=0)
        _check_rows(what + " features, bool", a.features(obs, skip=mask.bool()), ref, mask, untouched=0)
    # select_action: the noise is drawn for all rows, mask or no mask
    gen = torch.Generator(device="cuda").manual_seed(3)
    f0, a0, lp0 = agent.select_action(clean, gen)
    state0 = gen.get_state()
    gen.manual_seed(3)
    f1, a1, lp1 = agent.select_action(obs, gen, skip=mask)
    assert torch.equal(gen.get_state(), state0)
    m = mask != 0
    assert torch.equal(_bits(a1)[~m], _bits(a0)[~m]) and torch.equal(_bits(lp1)[~m], _bits(lp0)[~m])
    _check_rows("select_action features", f1, f0, mask, untouched=0)
    assert bool(torch.isfinite(a1).all())  # a skipped row's action comes from zero features, not from its NaN obs
    # ... and it is the action of zero features under the same noise: mean = bias
    pol = agent.policy_old
    eps = (a0 - pol.action_head(f0)) / pol.action_var.sqrt()
    want = pol.action_head.bias + eps * pol.action_var.sqrt()
    assert torch.allclose(a1[m], want[m], rtol=1e-4, atol=1e-5)


def test_argument_errors_come_before_any_launch(encs, monkeypatch):
    from occlusionenv_amd import _native as nat
    from occlusionenv_amd import ppo

    lib = nat.load()
    reached = []
    for name in ("occ_encoder_forward", "occ_encoder_forward_masked", "occ_segment_forward", "occ_segment_forward_masked"):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: reached.append(_n) or 0)
    enc, img = encs["full"], 32
    obs = _obs(img)
    ok = _mask("alternating")
    f32 = dict(dtype=torch.float32, device="cuda")
    bad_skips = {
        "float mask": ok.float(), "int64 mask": ok.long(), "short mask": ok[:-1].contiguous(), "long mask": torch.cat([ok, ok]),
        "2-d mask": ok.reshape(N, 1), "host mask": ok.cpu(), "list": MASKS["alternating"],
    }
    for what, s in bad_skips.items():
        for call in (lambda: enc(obs, skip=s), lambda: enc.predict_grad(obs, skip=s), lambda: enc.segment(obs, skip=s),
                     lambda: enc.forward_full(obs, skip=s)):
            with pytest.raises(ValueError):
                call()
    bad_feats = {
        "wrong rows": torch.empty(N + 1, 256, **f32), "wrong columns": torch.empty(N, 255, **f32),
        "f64": torch.empty(N, 256, dtype=torch.float64, device="cuda"), "host": torch.empty(N, 256),
        "non-contiguous": torch.empty(256, N, **f32).t(), "strided rows": torch.empty(N, 512, **f32)[:, ::2], "no tensor": [0.0],
    }
    for what, o in bad_feats.items():
        with pytest.raises(ValueError):
            enc(obs, skip=ok, out=o)
        with pytest.raises(ValueError):
            enc(obs, out=o)
        with pytest.raises(ValueError):
            enc.forward_full(obs, skip=ok, out=(o, torch.empty(N, 1, img, img, **f32), torch.empty(N, 2, **f32)))
    good_map = lambda: torch.empty(N, 1, img, img, **f32)  # noqa: E731
    bad_maps = {"wrong shape": torch.empty(N, img, img, **f32), "non-contiguous": torch.empty(N, 1, img, 2 * img, **f32)[..., ::2],
                "f16": torch.empty(N, 1, img, img, dtype=torch.float16, device="cuda"), "host": torch.empty(N, 1, img, img)}
    for what, o in bad_maps.items():
        with pytest.raises(ValueError):
            enc.segment(obs, skip=ok, out=o)
        with pytest.raises(ValueError):
            enc.segment(obs, return_logits=True, skip=ok, out=(good_map(), o))
        with pytest.raises(ValueError):
            enc.forward_full(obs, skip=ok, out=(torch.empty(N, 256, **f32), o, torch.empty(N, 2, **f32)))
    with pytest.raises(ValueError):  # the tuple follows the return order: two tensors for a call that returns three
        enc.segment(obs, return_logits=True, return_features=True, skip=ok, out=(good_map(), good_map()))
    with pytest.raises(ValueError):
        enc.segment(obs, skip=ok, out=(good_map(), good_map()))
    with pytest.raises(ValueError):
        enc.forward_full(obs, skip=ok, out=(torch.empty(N, 256, **f32), good_map(), torch.empty(N, 3, **f32)))
    with pytest.raises(ValueError):
        enc.predict_grad(obs, skip=ok, out=torch.empty(N, 3, **f32))
    agent = ppo.BatchedPPO(device="cuda", seed=0, encoder=enc)
    with pytest.raises(ValueError):
        agent.features(obs, skip=ok.long())
    with pytest.raises(ValueError):
        agent.features(obs, skip=ok, out=torch.empty(N, 255, **f32))
    with pytest.raises(ValueError):
        ppo.BatchedPPO(device="cuda", seed=0).features(obs, skip=ok[:-1].contiguous())
    assert reached == [], reached
    # the stand-ins do get reached by a good call (so the list above was able to show a launch)
    enc(obs, skip=ok)
    enc.segment(obs)
    assert reached == ["occ_encoder_forward_masked"] * 3 + ["occ_segment_forward"] * 3
