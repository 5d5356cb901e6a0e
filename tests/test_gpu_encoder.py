"""GPU tests of the native frozen encoder (occlusionenv_amd/encoder.py, csrc/occ_encoder.hpp): against the f64 host
model (tests/encoder_model.py) and the reference's fixture (tests/golden/encoder_golden.npz), bitwise reproducibility
(repeat calls, batch position, chunking, graph replay), real observations, and the PPO agent built from a FullNetwork
checkpoint."""
import os

import numpy as np
import pytest
import torch

from tests.encoder_model import encode, golden_state_dict, make_obs, preset_forward

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_golden.npz")
TOL = 1e-4
WORST = {}  # measured worst relative error per preset (printed with -s)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def nets(golden):
    from occlusionenv_amd.encoder import FrozenEncoder

    out = {}
    for preset in ("ppo", "predictor"):
        sd = golden_state_dict(golden, preset)
        out[preset] = (sd, FrozenEncoder.from_state_dict(sd, preset=preset))
    return out


def _err(got, want):
    scale = max(1.0, float(want.abs().max()))
    return float((got.double().cpu() - want).abs().max()) / scale


def _check(preset, key, f, g, f64, g64):
    ef, eg = _err(f, f64), _err(g, g64)
    WORST[preset] = max(WORST.get(preset, 0.0), ef, eg)
    print(f"{preset} {key}: features {ef:.3g}, grad {eg:.3g} (worst so far {WORST[preset]:.3g})")
    assert ef <= TOL and eg <= TOL, (preset, key, ef, eg)


CASES = [(64, 1), (64, 5), (64, 64), (100, 5), (128, 1), (128, 5), (256, 1), (256, 5), (512, 1)]


@pytest.mark.parametrize("preset", ["ppo", "predictor"])
@pytest.mark.parametrize("img,n", CASES)
def test_against_f64_host_model(nets, preset, img, n):
    sd, enc = nets[preset]
    obs64 = make_obs(1000 + img + n, n, img)
    f64, g64 = preset_forward(sd, obs64, preset)
    obs = obs64.float().cuda()
    f, g = enc(obs), enc.predict_grad(obs)
    assert f.shape == (n, 256) and f.dtype == torch.float32 and g.shape == (n, 2)
    _check(preset, f"S={img} N={n}", f, g, f64, g64)


@pytest.mark.parametrize("preset", ["ppo", "predictor"])
def test_against_reference_fixture(golden, nets, preset):
    _sd, enc = nets[preset]
    for n, img, seed in golden["inputs"]:
        obs = make_obs(int(seed), int(n), int(img)).float().cuda()
        f64 = torch.from_numpy(golden[f"{preset}_feat_{img}"])
        g64 = torch.from_numpy(golden[f"{preset}_grad_{img}"])
        _check(preset, f"fixture S={img}", enc(obs), enc.predict_grad(obs), f64, g64)


@pytest.mark.parametrize("residual,dilation", [(False, 2), (True, 1)])
def test_explicit_configurations(nets, residual, dilation):
    """Any dilation / residual combination given explicitly (a state dict stores neither)."""
    from occlusionenv_amd.encoder import FrozenEncoder

    for preset, (sd, _) in nets.items():
        enc = FrozenEncoder.from_state_dict(sd, preset=preset, dilation=dilation, residual=residual)
        p = {"ppo": ("encoder.", True), "predictor": ("features.", False)}[preset]
        obs64 = make_obs(7, 3, 96)
        f64 = encode(sd, obs64, p[0], p[1], dilation, residual)
        err = _err(enc(obs64.float().cuda()), f64)
        assert err <= TOL, (preset, residual, dilation, err)


def test_bitwise_reproducible(nets):
    _sd, enc = nets["ppo"]
    g = torch.Generator().manual_seed(3)
    base = make_obs(11, 8, 128).float()
    batch = base[torch.randint(0, 8, (64,), generator=g)] * (0.5 + torch.rand(64, 1, 1, 1, generator=g))
    batch[:, 3] = base[torch.randint(0, 8, (64,), generator=g)][:, 3]
    batch = batch.cuda()
    a, b = enc(batch), enc(batch)
    assert torch.equal(a, b)
    # env i alone == env i at any position of a batch of 64
    for i in (0, 17, 63):
        assert torch.equal(enc(batch[i:i + 1])[0], a[i])
        perm = torch.roll(torch.arange(64), 29 + i)
        assert torch.equal(enc(batch[perm]), a[perm])
    # chunking changes no bit
    for chunk in (1, 7, 64):
        enc.max_chunk = chunk
        try:
            assert torch.equal(enc(batch), a), chunk
        finally:
            enc.max_chunk = 256
    # non-contiguous input
    nc = batch.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not nc.is_contiguous() and torch.equal(enc(nc), a)


def test_graph_capture_matches_eager(nets):
    _sd, enc = nets["ppo"]
    obs = make_obs(21, 16, 128).float().cuda()
    eager = enc(obs)  # also creates the workspace of this size
    static = obs.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enc(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = enc(static)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    other = make_obs(22, 16, 128).float().cuda()
    static.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, enc(other))


def test_cpu_tensor_raises(nets):
    from occlusionenv_amd._native import NativeError

    with pytest.raises(NativeError):
        nets["ppo"][1](torch.zeros(1, 4, 64, 64))


@pytest.fixture(scope="module")
def ds():
    from occlusionenv_amd.meshes import SyntheticShapeNet

    return SyntheticShapeNet(n_models=8, seed=1234)


def _venv(ds, N, S, seed=77):
    from environment import OcclusionEnv
    from occlusionenv_amd import environment
    from SubProcVecEnv import SimpleVecEnv

    environment.seed_scene_rng(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    return SimpleVecEnv([lambda: OcclusionEnv(ds, img_size=S) for _ in range(N)])


def test_real_observations(nets, ds):
    """obs of a SimpleVecEnv step at 256^2 (depth -1 on the background) against the host model."""
    sd, enc = nets["ppo"]
    venv = _venv(ds, 4, 256)
    venv.reset()
    obs, _r, _d, _i = venv.step(torch.zeros(4, 2, device="cuda"))
    obs = obs[:, 0] if obs.dim() == 5 else obs
    assert obs.shape == (4, 4, 256, 256) and float(obs[:, 3].min()) == -1.0
    f64, g64 = preset_forward(sd, obs.double().cpu(), "ppo")
    _check("ppo", "real obs", enc(obs), enc.predict_grad(obs), f64, g64)
    venv.engine.check_status()


def test_ppo_from_fullnetwork(golden, ds):
    from occlusionenv_amd import ppo

    sd = golden_state_dict(golden, "ppo")
    agent = ppo.BatchedPPO.from_fullnetwork(sd, seed=0, K_epochs=2)
    for pol in (agent.policy, agent.policy_old):
        for name in ("action_head", "value_head"):
            h = getattr(pol, name)
            assert torch.equal(h.weight.cpu(), sd[name + ".weight"].float()) and torch.equal(h.bias.cpu(), sd[name + ".bias"].float())
    enc = agent.encoder
    seen = []
    orig_enc = agent.encoder
    agent.encoder = lambda o: (seen.append(o.clone()), orig_enc(o))[1]
    recs = []
    orig_store = agent.store
    agent.store = lambda r: (recs.append(r.clone()), orig_store(r))[1]
    N, S, T = 16, 128, 4
    venv = _venv(ds, N, S)
    stats = ppo.train_rollouts(venv, agent, n_updates=1, T=T)
    assert len(seen) == T and len(recs) == T and stats[0]["samples"] == N * T and np.isfinite(stats[0]["loss_last"])
    for obs, rec in zip(seen, recs):
        assert torch.equal(rec[:, :256], enc(obs))
    venv._drain()
    venv.engine.check_status()
