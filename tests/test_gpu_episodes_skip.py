"""GPU tests of the skip mask in the batched controller evaluation (occlusionenv_amd/episodes.py): the network of
``PredictedGradient`` and ``Agent`` runs under the mask the engine step of the same iteration took, and the results do not
change by a bit: not between poll intervals, and not against the host-synchronous single-env oracle.

The venv, the seeded evaluation, the oracle (``_oracle``: the reference's loop one env at a time on a single-env engine,
whose kernel model is tests/episode_model.py) and the bitwise comparison are those of tests/test_gpu_episodes.py: N = 6
envs at 64^2, at most MAX_STEP = 12 steps."""
import pytest
import torch

from tests.test_gpu_episodes import MAX_STEP, N, _against_oracle, _children, _evaluate, _oracle, _same
from tests.test_gpu_episodes import ds, nets, venv  # noqa: F401  (module-scoped fixtures, instantiated for this module)

pytestmark = pytest.mark.gpu

KEYS = ("iterations", "finished", "nan_steps", "final_action", "rewards", "full_rewards", "initial_loss")


class Recorder:
    """Stands in for a controller's ``enc`` / ``agent``: records the rows, ``skip`` and ``out`` of every network call."""

    def __init__(self, inner, log):
        self._inner, self._log = inner, log

    def _record(self, obs, skip, out):
        self._log.append(dict(rows=int(obs.shape[0]), skip=None if skip is None else skip.clone(), dtype=getattr(skip, "dtype", None),
                              out_rows=None if out is None else int(out.shape[0])))

    def __call__(self, obs, skip=None, out=None):  # FrozenEncoder
        self._record(obs, skip, out)
        return self._inner(obs, skip=skip, out=out)

    def features(self, obs, skip=None, out=None):  # BatchedPPO
        self._record(obs, skip, out)
        return self._inner.features(obs, skip=skip, out=out)

    def __getattr__(self, name):
        return getattr(self._inner, name)


@pytest.fixture(scope="module")
def runs(venv, nets):  # noqa: F811
    """poll_every -> (results, network calls per controller, the masks the engine steps took per controller)."""
    from occlusionenv_amd import harness

    enc, agent = nets
    eng = venv.engine
    out = {}
    for p in (1, 16, MAX_STEP):
        net_calls, eng_calls = {"model": [], "rl": []}, []
        ctrls = [harness.PredictedGradient(Recorder(enc, net_calls["model"]), step_lr=0.01), harness.Agent(Recorder(agent, net_calls["rl"]))]
        step = eng.step

        def recording_step(a, *args, _step=step, **kw):
            if kw.get("skip") is not None:  # (the loop's steps; nothing else steps the engine with a mask)
                eng_calls.append(dict(rows=int(a.shape[0]), skip=kw["skip"].clone()))
            return _step(a, *args, **kw)

        eng.step = recording_step
        try:
            res, _state = _evaluate(venv, ctrls, gen_device="cuda", trace=True, poll_every=p)
        finally:
            del eng.step  # the instance attribute: the class's method is back
        k = res["model"]["steps"]
        assert len(eng_calls) == k + res["rl"]["steps"]
        out[p] = (res, net_calls, {"model": eng_calls[:k], "rl": eng_calls[k:]})
    return out


@pytest.mark.parametrize("poll_every", [1, 16, MAX_STEP])
@pytest.mark.parametrize("name", ["model", "rl"])
def test_network_takes_the_mask_of_the_engine_step(runs, name, poll_every):
    res, net_calls, eng_calls = runs[poll_every]
    net, eng = net_calls[name], eng_calls[name]
    assert len(net) == len(eng) == res[name]["steps"] >= 1
    skipped = 0
    for i, (c, e) in enumerate(zip(net, eng)):
        assert c["skip"] is not None and c["dtype"] == torch.int32, i
        assert c["rows"] == e["rows"] == c["skip"].shape[0], f"step {i}: the mask is not of the working set's length"
        assert torch.equal(c["skip"], e["skip"]), f"step {i}: the network's mask is not the engine step's"
        assert c["out_rows"] in (None, c["rows"])
        skipped += int((c["skip"] != 0).sum())
    print(name, "poll_every", poll_every, "rows per step", [c["rows"] for c in net], "skipped row steps", skipped,
          "compactions", res[name]["compactions"])
    assert net[0]["rows"] == N and not bool(net[0]["skip"].any())
    # the frozen rows the loop counts are the rows the network skipped (the last step's new ones come after its call)
    assert skipped == res[name]["frozen_row_steps"]
    # these scenes end some episodes at the first step (a property of the seeded setup): the masks are not all zero
    assert skipped > 0 and bool((~res[name]["finished"]).any())


def test_every_poll_interval_gives_the_same_bits(runs):
    base = runs[MAX_STEP][0]
    assert all(v["polls"] == 0 and v["compactions"] == 0 for v in base.values())
    for p in (1, 16):
        for name in base:
            for k in KEYS:
                _same(f"poll_every {p} {name} {k}", runs[p][0][name][k].cpu().numpy(), base[name][k].cpu().numpy())


def test_results_equal_the_host_synchronous_oracle(venv, nets, runs):  # noqa: F811
    enc, agent = nets
    g_model, g_rl = _children(2, "cuda")
    want = dict(model=_oracle(venv, "model", 0.01, g_model, enc=enc), rl=_oracle(venv, "rl", 0.0, g_rl, agent=agent))
    for p, (res, _n, _e) in runs.items():
        for name in ("model", "rl"):
            _against_oracle(f"poll_every {p} {name}", res[name], want[name])


def test_agent_with_a_plain_callable_encoder(venv, nets, runs):  # noqa: F811
    """``BatchedPPO(encoder=...)`` takes any callable obs -> features: the loop must run with one that knows no ``skip`` /
    ``out`` (it is called on every row of the working set, as before the mask) and give the same bits."""
    import copy

    from occlusionenv_amd import harness

    enc, agent = nets
    seen = []
    plain = copy.copy(agent)
    plain.encoder = lambda o: (seen.append(int(o.shape[0])), agent.encoder(o))[1]
    for p in (1, MAX_STEP):
        del seen[:]
        res, _state = _evaluate(venv, [harness.PredictedGradient(enc, step_lr=0.01), harness.Agent(plain)], gen_device="cuda",
                                trace=True, poll_every=p)
        assert len(seen) == res["rl"]["steps"] >= 1 and seen[0] == N
        for k in KEYS:
            _same(f"plain encoder, poll_every {p}, {k}", res["rl"][k].cpu().numpy(), runs[p][0]["rl"][k].cpu().numpy())
