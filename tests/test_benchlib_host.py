"""Host-side checks of scripts/benchlib.py, the measuring method the bench scripts share.  The committed profiles were
written by the scripts as they were before the method became one piece of code, and they keep the samples next to what was
derived from them: ``compare`` and the naming rules have to give back every recorded median, spread, margin, speedup, ratio
and flag exactly, under exactly the recorded keys.  The kernel table is checked against a CSV worked out by hand, the
training inputs against the expressions the scripts used to spell out.  No GPU."""
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import benchlib as bl  # noqa: E402
from tests.encoder_model import make_obs  # noqa: E402

# what an entry holds besides the comparison: the shape, and what only a device can give
SHAPE = {"n_env", "img"}
NET = {"preset", "dilation", "residual"}
CHECKS = {"loss_native", "loss_torch_f32", "grad_rel_to_max_vs_torch_f32"}
SIZES = {"workspace_bytes", "scratch_bytes", "workspace_mib_per_env", "workspace_gib", "scratch_mib"}
BN = {"batch_stats", "parent_running_stats_ms", "ratio_to_parent_running_stats", "workspace_bytes", "scratch_bytes",
      "workspace_mib_per_env"}
PRETRAIN = {"form", "dilation", "first_loss"} | {f"{p}_{k}" for p in ("per_key", "packed") for k in ("kernel_launches", "copies_and_memsets")}
CRITERION = {"device", "warmup", "iters", "calls_per_sample", "native_bytes_per_step", "least_bytes_per_step", "native_frac_hbm_peak",
             "diff_vs_torch_f32"}

# profile -> (the list of entries in it, or None where the file is one entry; the other keys of an entry;
#             [(rule, native name, rival name)])
TRAIN_PROFILES = {
    "encoder_train_bench": ("shapes", SHAPE | CHECKS, [(bl.ONE_RIVAL, "native", "torch")]),
    "sep_encoder_train_bench": ("shapes", SHAPE | NET | CHECKS, [(bl.ONE_RIVAL, "native", "torch")]),
    "decoder_train_bench": ("shapes", SHAPE | CHECKS, [(bl.ONE_RIVAL_NOT_SLOWER, "native", "torch")]),
    "sep_fullnet_train_bench": ("shapes", SHAPE | NET | CHECKS | SIZES, [(bl.VS_RIVAL, "native", "torch"), (bl.VS_RIVAL, "native", "split")]),
    "fullnet_bn_train_bench": ("shapes", SHAPE | NET | CHECKS | BN, [(bl.BN_VS_TORCH, "native", "torch"), (bl.BN_VS_RUNNING, "native", "running_stats")]),
    "sep_fullnet_bn_train_bench": ("shapes", SHAPE | NET | CHECKS | BN, [(bl.BN_VS_TORCH, "native", "torch"), (bl.BN_VS_RUNNING, "native", "running_stats")]),
    "pretrain_step_bench": ("cases", SHAPE | PRETRAIN, [(bl.OPTIMIZERS, "packed", "per_key")]),
    "criterion_bench": (None, SHAPE | CRITERION, [(bl.ONE_RIVAL_NOT_SLOWER, "native", "torch")]),
}
NO_SAMPLES = {"sep_encoder_train_bench"}  # of three of its four entries only the printed summaries were kept (the file's own note)


def _profile(name):
    with open(os.path.join(ROOT, "profiles", name + ".json")) as f:
        return json.load(f)


def _samples(entry, rule, n, r):
    """The two sample lists a rule's comparison was made from: the keys it writes its ``*_ms_all`` fields under."""
    keys = {field: key.format(n=n, r=r) for key, field in rule.items()}
    rival = entry[keys["rival_ms_all"]]
    return entry[keys["native_ms_all"]] if "native_ms_all" in keys else entry["native_ms_all"], rival


def _entries(name):
    doc = _profile(name)
    return doc[TRAIN_PROFILES[name][0]] if TRAIN_PROFILES[name][0] else [doc]


ENTRIES = [(name, i) for name in TRAIN_PROFILES for i in range(len(_entries(name)))]
assert all(any(n == name for n, _i in ENTRIES) for name in TRAIN_PROFILES)


@pytest.mark.parametrize("name,index", ENTRIES, ids=[f"{name}-{i}" for name, i in ENTRIES])
def test_compare_reproduces_the_committed_profile(name, index):
    _key, other, rules = TRAIN_PROFILES[name]
    entry = _entries(name)[index]
    written = set()
    for rule, n, r in rules:
        written |= {key.format(n=n, r=r) for key in rule}
    sampled = any(k.endswith("_ms_all") for k in entry)
    assert sampled or name in NO_SAMPLES
    if not sampled:
        written = {k for k in written if not k.endswith("_all")}
    assert written | other == set(entry), (name, written ^ set(entry) ^ other)
    assert not written & other
    if not sampled:
        pytest.skip(f"profiles/{name}.json keeps no per-sample lists for {entry.get('preset')} {entry['n_env']}x{entry['img']}: "
                    "only its key set is checked")
    for rule, n, r in rules:
        got = bl.named(bl.compare(*_samples(entry, rule, n, r)), rule, n=n, r=r)
        for key, value in got.items():
            assert type(value) is type(entry[key]) and value == entry[key], (name, entry["n_env"], entry["img"], key)


RESIDENT = {"resident_gen_bench": None, "resident_resize_bench": None, "resident_jpeg_bench": "shapes"}


@pytest.mark.parametrize("name", list(RESIDENT))
def test_medians_reproduce_the_resident_profiles(name):
    doc = _profile(name)
    for entry in (doc[RESIDENT[name]] if RESIDENT[name] else [doc]):
        stems = [k[:-len("_ms_all")] for k in entry if k.endswith("_ms_all")]
        assert "a_bare_iteration" in stems and len(stems) >= 4  # (a) and the device passes timed next to it
        got = bl.medians({s: entry[s + "_ms_all"] for s in stems})
        assert all(got[k] == entry[k] for k in got) and set(got) == {s + e for s in stems for e in ("_ms", "_ms_all")}
        runs = [k[:-len("_s_all")] for k in entry if k.endswith("_s_all")]
        assert runs
        for key in runs:  # the whole-call sections: the median-low run; its step count is the only one the file keeps
            secs = entry[key + "_s_all"]
            got = bl.median_low_run(key, secs, [entry[key + "_engine_steps"]] * len(secs), entry["frames"])
            assert {k: entry[k] for k in got} == got


def test_kernel_stats_against_totals_by_hand(tmp_path):
    rows = [("void occ::occ_conv_kernel<3, true>(float const*, int)", 4, 1000000),  # two signatures of one kernel:
            ("occ::occ_conv_kernel<3, true>(float*, int)", 2, 500000),            # they collapse to one name
            ("void at::native::vectorized_elementwise_kernel<4, Add>(int, Add)", 8, 123456),
            ("void occ::occ_pool_kernel(float*)", 4, 1250000),
            ("void occ::occ_conv_kernel<1, false>(float const*, int)", 4, 250000)]  # another instance stays apart
    path = tmp_path / "trace_kernel_stats.csv"
    path.write_text('"Name","Calls","TotalDurationNs"\n' + "".join(f'"{n}",{c},{ns}\n' for n, c, ns in rows))
    got = bl.kernel_stats(str(path), 4, "by hand")
    assert got == dict(
        note="by hand", native_steps_traced_per_config=4,
        total_kernel_us_per_step_of_every_config=780.9,  # (1000 + 500 + 123.456 + 1250 + 250) / 4 = 780.864
        torch_ops_us_per_step_of_every_config=30.9,      # 123.456 rounds to 123.5 in the table; / 4 = 30.875
        kernels={"occ_pool_kernel": dict(calls=4, total_us=1250.0, us_per_step_of_every_config=312.5),
                 "occ_conv_kernel<3, true>": dict(calls=6, total_us=1500.0, us_per_step_of_every_config=375.0),
                 "occ_conv_kernel<1, false>": dict(calls=4, total_us=250.0, us_per_step_of_every_config=62.5)})
    assert list(got["kernels"]) == ["occ_conv_kernel<3, true>", "occ_pool_kernel", "occ_conv_kernel<1, false>"]  # by time


def test_train_inputs_are_the_scripts_expressions():
    n, img = 2, 32
    obs, occl, grad, target = bl.train_inputs(n, img)
    base = make_obs(31, 8, img).float()
    assert torch.equal(obs, base[torch.arange(n) % 8])
    gen = torch.Generator().manual_seed(7)
    want_occl = (torch.rand(n, 1, img // 8, img // 8, generator=gen) > 0.5).float().repeat_interleave(8, 2).repeat_interleave(8, 3)
    want_grad = F.normalize(torch.randn(n, 2, generator=gen), dim=1)
    assert torch.equal(occl, want_occl) and torch.equal(grad, want_grad)
    assert torch.equal(target, F.normalize(torch.randn(n, 2, generator=torch.Generator().manual_seed(7)), dim=1))
    assert occl.shape == (n, 1, img, img) and set(occl.unique().tolist()) <= {0.0, 1.0}
    # more envs than the eight observations: they repeat
    assert torch.equal(bl.train_inputs(10, img)[0][8:], base[:2])


def test_parse_shapes_round_trips():
    for shapes in ([(128, 256), (64, 512)], [(8, 64)]):
        text = ",".join(f"{n}x{img}" for n, img in shapes)
        assert bl.parse_shapes(text) == shapes
    assert bl.parse_shapes("128x256,64x512") == [(128, 256), (64, 512)]


def test_dice_is_the_formula():
    p, t = torch.tensor([[0.5, 1.0], [0.0, 0.25]]), torch.tensor([[1.0, 1.0], [0.0, 1.0]])
    want = ((1 - (1.5 + 1) / (1.25 + 2 + 1)) + (1 - (0.25 + 1) / (0.0625 + 1 + 1))) / 2
    assert abs(float(bl.dice(p.view(2, 1, 1, 2), t.view(2, 1, 1, 2))) - want) < 1e-6
