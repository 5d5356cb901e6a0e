"""Known answers of tests/episode_model.py, the numpy statement of occ_episode_advance, and the host-side pieces of the
batched controller evaluation that need no GPU: the symbol in the header and the binding, the iterations files, the summary."""
import ast
import os
import re
from fractions import Fraction

import numpy as np

from tests import episode_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAN = f32("nan")


def _bits(a):
    return np.asarray(a, f32).view(np.uint32)


def test_nan_step_only_counts():
    st = em.new_state(2, max_step=5, action=[[1, 2], [3, 4]])
    grad = np.array([[0.5, NAN], [0.25, 0.5]], f32)
    left = em.advance(st, em.GRADIENT, 2.0, 1, 5, done=[1, 0], reward=[7, 8], full_reward=[9, 10], grad=grad)
    # env 0: `continue` - no update, no trace row, and its done flag is not looked at; env 1 steps
    assert left == 2 and st["nan_steps"].tolist() == [1, 0] and st["active"].tolist() == [1, 1] and st["skip"].tolist() == [0, 0]
    assert st["action"].tolist() == [[1, 2], [3.5, 5]] and st["finished"].tolist() == [0, 0] and st["iterations"].tolist() == [0, 0]
    assert np.isnan(st["rewards"][:, 0]).all() and np.isnan(st["full_rewards"][:, 0]).all()
    assert st["rewards"][1, 1] == 8 and st["full_rewards"][1, 1] == 10 and np.isnan(st["rewards"][[0, 2, 3, 4], 1]).all()


def test_done_on_the_last_step_is_finished_not_capped():
    st = em.new_state(2, max_step=3)
    left = em.advance(st, em.AGENT, 0.0, 2, 3, done=[1, 0], reward=[1, 2], full_reward=[3, 4], pred=np.array([[5, 6], [7, 8]], f32))
    assert left == 0 and st["finished"].tolist() == [1, 0] and st["iterations"].tolist() == [3, 3]
    assert st["active"].tolist() == [0, 0] and st["skip"].tolist() == [1, 1] and st["action"].tolist() == [[5, 6], [7, 8]]
    assert st["rewards"][2].tolist() == [1, 2]


def test_done_before_the_cap():
    st = em.new_state(3, max_step=9)
    left = em.advance(st, em.RANDOM, 0.5, 4, 9, done=[0, 1, 0], reward=[0] * 3, full_reward=[0] * 3, noise=np.full((3, 2), 2, f32))
    assert left == 2 and st["iterations"].tolist() == [0, 5, 0] and st["finished"].tolist() == [0, 1, 0]
    assert st["active"].tolist() == [1, 0, 1] and st["skip"].tolist() == [0, 1, 0] and (st["action"] == 1).all()


def test_cap_on_a_nan_step():
    st = em.new_state(1, max_step=4, action=[[1, 1]])
    left = em.advance(st, em.GRADIENT, 1.0, 3, 4, done=[1], reward=[5], full_reward=[6], grad=np.array([[NAN, 0]], f32))
    assert left == 0 and st["nan_steps"].tolist() == [1] and st["iterations"].tolist() == [4] and st["finished"].tolist() == [0]
    assert st["active"].tolist() == [0] and st["skip"].tolist() == [1] and st["action"].tolist() == [[1, 1]]
    assert np.isnan(st["rewards"]).all()


def test_frozen_row_is_untouched():
    st = em.new_state(2, max_step=4, action=[[1, 2], [3, 4]])
    st["active"][0], st["skip"][0], st["iterations"][0], st["finished"][0], st["nan_steps"][0] = 0, 1, 2, 1, 7
    before = {k: v.copy() for k, v in st.items()}
    # env 0's inputs are garbage (its rows of a skipped step are undefined): they must not matter
    left = em.advance(st, em.GRADIENT, 1.0, 3, 4, done=[1, 0], reward=[NAN, 1], full_reward=[NAN, 2], grad=np.array([[NAN, NAN], [1, 1]], f32))
    assert left == 0
    for k in st:
        sel = (slice(None), 0) if k in ("rewards", "full_rewards") else 0
        assert np.array_equal(_bits(st[k][sel]) if st[k].dtype == f32 else st[k][sel],
                              _bits(before[k][sel]) if st[k].dtype == f32 else before[k][sel]), k
    assert st["action"][1].tolist() == [4, 5] and st["iterations"].tolist() == [2, 4]


def test_model_rule_negates_the_rate():
    st = em.new_state(1, action=[[9, 9]])
    em.advance(st, em.MODEL, 0.01, 0, 5, done=[0], pred=np.array([[0.3, -0.7]], f32))
    assert np.array_equal(_bits(st["action"][0]), _bits([f32(-0.01) * f32(0.3), f32(-0.01) * f32(-0.7)]))


def test_update_rounds_the_product_then_the_sum():
    """lr = g = 1 + 2^-12: the exact product 1 + 2^-11 + 2^-24 is a tie in f32 and rounds to 1 + 2^-11.  With action = -1
    the two-rounding update gives 2^-11; a fused multiply-add, which rounds the exact sum once, gives 2^-11 + 2^-24."""
    lr = g = f32(1 + 2.0 ** -12)
    exact = Fraction(float(lr)) * Fraction(float(g)) - 1
    fused = f32(float(exact))  # exactly representable: the one rounding of the fused form changes nothing
    assert Fraction(float(fused)) == exact == Fraction(1, 2 ** 11) + Fraction(1, 2 ** 24)
    for rule, kw in ((em.GRADIENT, "grad"), (em.RANDOM, "noise")):
        st = em.new_state(1, action=[[-1, -1]])
        em.advance(st, rule, lr, 0, 5, done=[0], **{kw: np.array([[g, g]], f32)})
        assert st["action"][0, 0] == f32(2.0 ** -11) and st["action"][0, 0] != fused


def test_symbol_in_header_and_binding():
    from occlusionenv_amd import _native as nat

    src = open(os.path.join(ROOT, "include", "occlusionenv_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+occ_episode_advance\s*\(", code)
    assert "occ_episode_advance" in nat.SYMBOLS and len(nat.SYMBOLS["occ_episode_advance"][1]) == 21
    assert int(re.search(r"#define\s+OCC_ABI_VERSION\s+(\d+)", src).group(1)) == 12 == nat.ABI_VERSION
    rules = [int(re.search(rf"#define\s+OCC_EPISODE_{n}\s+(\d+)", src).group(1)) for n in ("GRADIENT", "RANDOM", "MODEL", "AGENT")]
    assert rules == [nat.EPISODE_GRADIENT, nat.EPISODE_RANDOM, nat.EPISODE_MODEL, nat.EPISODE_AGENT]
    assert rules == [em.GRADIENT, em.RANDOM, em.MODEL, em.AGENT]
    lib = nat.load()
    assert hasattr(lib, "occ_episode_advance")
    # bad arguments are turned away before any launch: no pointers, a step at max_step, an unknown rule
    assert lib.occ_episode_advance(*([None] * 6), 0, 1.0, 0, 5, 4, *([None] * 10)) == 1
    import ctypes

    p = ctypes.c_void_p(16)
    assert lib.occ_episode_advance(p, p, p, p, p, p, 0, 1.0, 5, 5, 4, p, p, p, p, p, p, p, p, p, None) == 1
    assert lib.occ_episode_advance(p, p, p, p, p, p, 4, 1.0, 0, 5, 4, p, p, p, p, p, p, p, p, p, None) == 1
    assert lib.occ_episode_advance(p, p, p, None, p, p, 0, 1.0, 0, 5, 4, p, p, p, p, p, p, None, None, p, None) == 1  # GRADIENT without grad


def test_write_iterations_round_trip(tmp_path):
    import torch

    from occlusionenv_amd import harness

    path = tmp_path / "iterations_raw_3.txt"
    d = harness.write_iterations(path, torch.tensor([3, 50, 1]))
    assert d == {0: 3, 1: 50, 2: 1}
    back = ast.literal_eval(open(path).read())
    assert back == d and np.array(list(back.values())).tolist() == [3, 50, 1]  # BayesianTTest.py:62
    az = [-310 / 3200, 0.0, 310 / 3200]  # iterator.py keys its dict by the azimuth
    harness.write_iterations(path, np.array([7, 8, 9]), keys=az)
    assert ast.literal_eval(open(path).read()) == dict(zip(az, [7, 8, 9]))
    for bad in ([0, 1], [0, 0, 1]):
        try:
            harness.write_iterations(path, [1, 2, 3], keys=bad)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_summarise_iterations_by_hand():
    from occlusionenv_amd import harness

    res = dict(raw=dict(iterations=np.array([2, 4, 6, 8]), finished=np.array([1, 1, 1, 0], bool)),
               random=dict(iterations=np.array([8, 4, 8, 8]), finished=np.array([0, 1, 0, 0], bool)),
               rl=dict(iterations=np.array([1, 1, 1, 1]), finished=np.ones(4, bool)))
    s = harness.summarise_iterations(res)
    assert s["controllers"]["raw"] == dict(mean=5.0, median=5.0, finished=0.75)
    assert s["controllers"]["random"] == dict(mean=7.0, median=8.0, finished=0.25)
    assert list(s["pairs"]) == [("raw", "random"), ("raw", "rl"), ("random", "rl")]
    p = s["pairs"][("raw", "random")]  # differences -6, 0, -2, 0: mean -2, sample variance (16 + 4 + 0 + 4) / 3 = 8
    assert p["mean"] == -2.0 and abs(p["std"] - 8 ** 0.5) < 1e-12 and p["faster"] == 0.5
    assert s["pairs"][("raw", "rl")]["faster"] == 0.0 and s["pairs"][("random", "rl")]["mean"] == 6.0
