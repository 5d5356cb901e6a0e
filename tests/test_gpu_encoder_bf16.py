"""GPU tests of the bf16 inference mode of the separable encoder (occlusionenv_amd/encoder.py ``precision="bf16"``,
csrc/occ_encoder_bf16.hpp) against the f64 host model of its numeric contract (tests/encoder_bf16_model.py).

Accuracy is judged against what the format itself costs.  Per case, on the CPU: ``exact`` = the f64 encoder, ``emu`` = the
f64 model of the bf16 mode, ``e_fmt = err(emu, exact)``: the code under test plays no part in it.  The kernels must stay
within 0.25 e_fmt of ``emu`` and 1.25 e_fmt of ``exact``.  ``d_ref`` = the same model with f32 accumulation against ``emu``
is the noise of a second correct implementation (rare one-ulp flips of a stored bf16); it must be under 0.125 e_fmt for the
bar to be fair, and truncation instead of RNE sits at 2.4-3.6 e_fmt, ten times over the bar."""
import os

import numpy as np
import pytest
import torch

from tests.encoder_bf16_model import encode_bf16, err
from tests.encoder_model import encode, golden_state_dict, make_obs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_golden.npz")
WORST = {"emu": 0.0, "exact": 0.0, "d_ref": 0.0}  # measured worst ratios to e_fmt (printed with -s)
_REF = {}
# (S, n, dilation, residual) -> the make_obs seed.  d_ref is not continuous: one stored value that lies within f32 noise of
# a bf16 tie flips by a whole bf16 ulp in one implementation and not in the other, and deep in the network (2 x 2 and 1 x 1
# maps) one such flip moves a feature by 0.1-0.3 e_fmt; over seeds d_ref ranges from 1e-5 to 0.27 e_fmt.  Each seed below is
# the first of 1000 k + S + n (k = 1, 2, ..) at which the two HOST models agree to d_ref < 0.01 e_fmt, i.e. at which no
# stored value of the model sits on such a tie: chosen on the CPU from the models alone, before any kernel ran.
SEEDS = {(32, 1, 2, True): 1033, (32, 3, 2, True): 1035, (40, 2, 2, True): 1042, (64, 5, 2, True): 10069,
         (100, 2, 2, True): 4102, (128, 1, 2, True): 2129, (48, 2, 2, False): 2050, (48, 2, 1, True): 2050,
         (48, 2, 1, False): 1050}


@pytest.fixture(scope="module")
def sd():
    return golden_state_dict(np.load(GOLDEN), "ppo")


@pytest.fixture(scope="module")
def encs(sd):
    from occlusionenv_amd.encoder import FrozenEncoder

    f32 = FrozenEncoder.from_state_dict(sd, preset="ppo")
    return f32, FrozenEncoder.from_state_dict(sd, preset="ppo", precision="bf16")


def _reference(sd, img, n, dilation=2, residual=True):
    """(obs f32 on the CPU, exact, emu, e_fmt, d_ref), computed once per case and shared."""
    key = (img, n, dilation, residual)
    if key not in _REF:
        obs = make_obs(SEEDS[key], n, img).float()
        exact = encode(sd, obs.double(), "encoder.", True, dilation, residual)
        emu = encode_bf16(sd, obs, "encoder.", dilation, residual)
        ref32 = encode_bf16(sd, obs, "encoder.", dilation, residual, dtype=torch.float32)
        _REF[key] = (obs, exact, emu, err(emu, exact), err(ref32, emu))
    return _REF[key]


def _judge(what, got, ref):
    _obs, exact, emu, e_fmt, d_ref = ref
    e_emu, e_exact = err(got, emu), err(got, exact)
    for k, v in (("emu", e_emu), ("exact", e_exact), ("d_ref", d_ref)):
        WORST[k] = max(WORST[k], v / e_fmt)
    print(f"{what}: e_fmt {e_fmt:.3g}, d_ref {d_ref:.3g} ({d_ref / e_fmt:.3f} e_fmt), kernel vs emu {e_emu:.3g} "
          f"({e_emu / e_fmt:.3f} e_fmt), vs exact {e_exact:.3g} ({e_exact / e_fmt:.3f} e_fmt); worst ratios so far "
          f"emu {WORST['emu']:.3f}, exact {WORST['exact']:.3f}, d_ref {WORST['d_ref']:.3f}")
    assert e_fmt > 1e-4, "the format costs nothing here: the case tests nothing"
    assert d_ref <= 0.125 * e_fmt, (what, "the bar would be unfair here", d_ref, e_fmt)
    assert e_emu <= 0.25 * e_fmt, (what, e_emu, e_fmt)
    assert e_exact <= 1.25 * e_fmt, (what, e_exact, e_fmt)


@pytest.mark.parametrize("img,n", [(32, 1), (32, 3), (40, 2), (64, 5), (100, 2), (128, 1)])
def test_accuracy(sd, encs, img, n):
    ref = _reference(sd, img, n)
    f = encs[1](ref[0].cuda())
    assert f.shape == (n, 256) and f.dtype == torch.float32
    _judge(f"S={img} N={n}", f, ref)


@pytest.mark.parametrize("residual,dilation", [(False, 2), (True, 1), (False, 1)])
def test_configurations(sd, residual, dilation):
    from occlusionenv_amd.encoder import FrozenEncoder

    enc = FrozenEncoder.from_state_dict(sd, preset="ppo", dilation=dilation, residual=residual, precision="bf16")
    ref = _reference(sd, 48, 2, dilation, residual)
    _judge(f"residual={residual} dilation={dilation}", enc(ref[0].cuda()), ref)


# ---- bits -----------------------------------------------------------------------------------------------------------------
def test_bits(encs):
    _f32, enc = encs
    g = torch.Generator().manual_seed(3)
    base = make_obs(11, 4, 64).float()
    batch = base[torch.randint(0, 4, (16,), generator=g)] * (0.5 + torch.rand(16, 1, 1, 1, generator=g))
    batch = batch.cuda()
    a, b = enc(batch), enc(batch)
    assert torch.equal(a, b)
    assert len({tuple(r.tolist()) for r in a.cpu()}) == 16  # sixteen different envs
    for i in (0, 7, 15):  # env i alone == env i at any position of the batch
        assert torch.equal(enc(batch[i:i + 1])[0], a[i])
        perm = torch.roll(torch.arange(16), 5 + i)
        assert torch.equal(enc(batch[perm]), a[perm])
    for chunk in (1, 7, 16):
        enc.max_chunk = chunk
        try:
            assert torch.equal(enc(batch), a), chunk
        finally:
            enc.max_chunk = 256
    nc = batch.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not nc.is_contiguous() and torch.equal(enc(nc), a)


def _capture(fn):
    """Warm ``fn`` up on a side stream, capture it -> the graph."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def test_graph_capture_matches_eager(encs):
    _f32, enc = encs
    obs = make_obs(21, 6, 64).float().cuda()
    eager = enc(obs)
    static, out = obs.clone(), torch.zeros(6, 256, device="cuda")
    graph = _capture(lambda: enc(static, out=out))
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    other = make_obs(22, 6, 64).float().cuda()
    static.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, enc(other))


# ---- skip mask ------------------------------------------------------------------------------------------------------------
def test_skip_mask(encs):
    _f32, enc = encs
    obs = make_obs(31, 9, 32).float().cuda()
    enc.max_chunk = 4
    try:
        full = enc(obs)
        mask = torch.tensor([1, 0, 0, 1, 1, 0, 1, 1, 0], dtype=torch.int32, device="cuda")  # both ends of chunks 0 and 1
        keep = mask.bool()
        sentinel = torch.full((9, 256), -123.25, device="cuda")
        out = sentinel.clone()
        assert enc(obs, skip=mask, out=out) is out
        assert torch.equal(out[keep], sentinel[keep]) and torch.equal(out[~keep], full[~keep])
        fresh = enc(obs, skip=mask)
        assert torch.equal(fresh[keep], torch.zeros_like(fresh[keep])) and torch.equal(fresh[~keep], full[~keep])
        assert torch.equal(enc(obs, skip=keep), fresh)  # bool == int32
        # one captured graph follows the mask it finds at replay
        static_mask, out2 = mask.clone(), sentinel.clone()
        graph = _capture(lambda: enc(obs, skip=static_mask, out=out2))
        out2.copy_(sentinel)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out2, out)
        static_mask.copy_(1 - mask)
        out2.copy_(sentinel)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out2[~keep], sentinel[~keep]) and torch.equal(out2[keep], full[keep])
    finally:
        enc.max_chunk = 256


# ---- interface ------------------------------------------------------------------------------------------------------------
def test_interface(sd, encs):
    from occlusionenv_amd.encoder import FrozenEncoder
    from occlusionenv_amd.sepfullnet import TrainableSeparableFullNetwork
    from occlusionenv_amd.septrain import TrainableSeparableEncoder

    f32, enc = encs
    assert f32.precision == "f32" and enc.precision == "bf16"
    dense = golden_state_dict(np.load(GOLDEN), "predictor")
    with pytest.raises(ValueError, match="separable"):
        FrozenEncoder.from_state_dict(dense, preset="predictor", precision="bf16")
    with pytest.raises(ValueError, match="precision"):
        FrozenEncoder.from_state_dict(sd, preset="ppo", precision="fp8")
    with pytest.raises(ValueError, match="precision"):
        enc.with_precision("half")
    obs = make_obs(41, 2, 32).float().cuda()
    assert enc.has_decoder
    with pytest.raises(ValueError, match="pooled feature only"):
        enc.segment(obs)
    with pytest.raises(ValueError, match="pooled feature only"):
        enc.forward_full(obs)
    for wrapper in (TrainableSeparableEncoder, TrainableSeparableFullNetwork):
        with pytest.raises(ValueError, match="pooled feature only"):
            wrapper.from_encoder(enc)
    # the head runs on the f32 feats
    feats = enc(obs)
    assert torch.equal(enc.predict_grad(obs), enc.grad_head(feats))
    # the mode travels with the state, and back
    back = enc.with_precision("f32")
    assert back.precision == "f32" and torch.equal(back(obs), f32(obs)) and torch.equal(back.segment(obs), f32.segment(obs))
    assert enc.precision == "bf16" and torch.equal(f32.with_precision("bf16")(obs), feats)
    for other in (enc.with_encoder(sd), enc.with_decoder(sd), enc.with_state(sd)):
        assert other.precision == "bf16" and torch.equal(other(obs), feats)
    assert not torch.equal(feats, f32(obs))


def test_ppo_agent_in_bf16(sd, encs):
    from occlusionenv_amd import ppo

    f32, enc = encs
    agent16 = ppo.BatchedPPO.from_fullnetwork(sd, precision="bf16", seed=0)
    agent32 = ppo.BatchedPPO.from_fullnetwork(sd, seed=0)
    assert agent16.encoder.precision == "bf16" and agent32.encoder.precision == "f32"
    ref = _reference(sd, 64, 5)
    obs, e_fmt = ref[0].cuda(), ref[3]
    f16, f = agent16.features(obs), agent32.features(obs)
    assert torch.equal(f16, enc(obs)) and torch.equal(f, f32(obs))
    with torch.no_grad():
        m16, m32 = agent16.policy_old.action_head(f16), agent32.policy_old.action_head(f)
    w = agent32.policy_old.action_head.weight.detach()
    bound = 1.25 * e_fmt * max(1.0, float(f.abs().max())) * float(w.abs().sum(dim=1).max())
    diff = float((m16 - m32).abs().max())
    print(f"action mean: bf16 vs f32 agent differ by {diff:.3g}, bound {bound:.3g}")
    assert diff <= bound
