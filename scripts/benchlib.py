"""The measuring method of the bench scripts, written once.

A sample is ``calls`` calls of a path between two device events, in ms per call.  The paths of one comparison run in one
process: ``warmup`` rounds, then ``iters`` timed rounds, every round visiting the paths in the same order, so that drift of
the device reaches all of them alike.  All samples are kept.  Medians are compared; the margin of a comparison is the larger
of the two paths' min-max spreads.  ``compare`` is that arithmetic as a pure function of two sample lists and ``named`` gives
its fields the key names a script writes, so the committed profiles can be checked against it without a device
(tests/test_benchlib_host.py).
"""
import contextlib
import csv
import ctypes as C
import json
import statistics
import time

import torch
import torch.nn.functional as F

PEAK_F32, PEAK_HBM = 157.3e12, 8.0e12


# ---- timing ---------------------------------------------------------------------------------------------------------------------
def sample(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def interleaved(paths, warmup, iters, calls):
    """``paths``: name -> fn, in the order every round visits them.  -> name -> the ``iters`` timed samples."""
    for _ in range(warmup):
        for fn in paths.values():
            sample(fn, calls)
    ms = {k: [] for k in paths}
    for _ in range(iters):
        for k, fn in paths.items():
            ms[k].append(sample(fn, calls))
    return ms


def timed(fn, warmup, iters):
    """(median, samples) of single calls, each between its own two events: the forward benches' method."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


# ---- the comparison and its key names -------------------------------------------------------------------------------------------
def compare(native, rival):
    """Two sample lists -> the medians, the spreads, the margin (the larger spread) and what follows from them."""
    med, rmed = statistics.median(native), statistics.median(rival)
    spread, rspread = max(native) - min(native), max(rival) - min(rival)
    margin = max(spread, rspread)
    return dict(native_ms=med, native_ms_all=native, native_spread_ms=spread, rival_ms=rmed, rival_ms_all=rival,
                rival_spread_ms=rspread, margin_ms=margin, speedup=rmed / med, ratio=med / rmed,
                faster=bool(med + margin < rmed), slower=bool(rmed + margin < med), not_slower=bool(med <= rmed + margin))


# key written -> field of ``compare``; {n} and {r} are the names of the native path and of its rival
_PAIR = {"{n}_ms": "native_ms", "{n}_ms_all": "native_ms_all", "{r}_ms": "rival_ms", "{r}_ms_all": "rival_ms_all",
         "{n}_spread_ms": "native_spread_ms", "{r}_spread_ms": "rival_spread_ms"}
ONE_RIVAL = {**_PAIR, "margin_ms": "margin_ms", "speedup": "speedup", "faster_by_more_than_margin": "faster"}
ONE_RIVAL_NOT_SLOWER = {**_PAIR, "margin_ms": "margin_ms", "speedup": "speedup", "not_slower": "not_slower"}
VS_RIVAL = {**_PAIR, "margin_vs_{r}_ms": "margin_ms", "speedup_vs_{r}": "speedup", "faster_than_{r}_by_more_than_margin": "faster"}
OPTIMIZERS = {**_PAIR, "margin_ms": "margin_ms", "speedup": "speedup", "{n}_faster_by_more_than_margin": "faster",
              "{n}_slower_by_more_than_margin": "slower"}
# batch-statistics mode: against torch in train mode, and against the running-statistics step of the same build
BN_VS_TORCH = {"{n}_ms": "native_ms", "{n}_ms_all": "native_ms_all", "{n}_spread_ms": "native_spread_ms",
               "torch_train_mode_ms": "rival_ms", "torch_train_mode_ms_all": "rival_ms_all", "torch_spread_ms": "rival_spread_ms",
               "speedup_vs_torch": "speedup", "faster_than_torch_by_more_than_margin": "faster"}
BN_VS_RUNNING = {"running_stats_ms": "rival_ms", "running_stats_ms_all": "rival_ms_all", "running_stats_spread_ms": "rival_spread_ms",
                 "ratio_to_running_stats": "ratio"}


def named(cmp, rule, n="native", r="torch"):
    """The fields of ``compare`` under the keys of a rule above."""
    return {key.format(n=n, r=r): cmp[field] for key, field in rule.items()}


def medians(ms, prefix=""):
    """name -> samples as ``{prefix}{name}_ms`` (the median) and ``{prefix}{name}_ms_all``."""
    out = {}
    for k, v in ms.items():
        out[f"{prefix}{k}_ms"], out[f"{prefix}{k}_ms_all"] = statistics.median(v), v
    return out


def median_low_run(key, secs, steps, frames):
    """Whole timed runs of a generator (seconds and engine steps of each) -> the median-low run under ``{key}_*``."""
    k = secs.index(statistics.median_low(secs))
    return {f"{key}_s": secs[k], f"{key}_s_all": secs, f"{key}_engine_steps": steps[k], f"{key}_ms_per_step": secs[k] / steps[k] * 1e3,
            f"{key}_frames_per_s": frames / secs[k]}


# ---- the training benches' inputs -----------------------------------------------------------------------------------------------
def dice(p, t):
    p, t = p.reshape(p.shape[0], -1), t.reshape(t.shape[0], -1)
    return (1.0 - ((p * t).sum(1) + 1.0) / ((p * p).sum(1) + (t * t).sum(1) + 1.0)).mean()


def train_inputs(n, img):
    """(obs, occl, grad, target) on the host: eight seeded observations repeated to ``n``; from seed 7 a blocky 0/1
    occlusion map and then a unit gradient (the joint benches), or from seed 7 a unit target alone (the encoder benches)."""
    from tests.encoder_model import make_obs

    obs = make_obs(31, 8, img).float()[torch.arange(n) % 8]
    gen = torch.Generator().manual_seed(7)
    occl = (torch.rand(n, 1, img // 8, img // 8, generator=gen) > 0.5).float().repeat_interleave(8, 2).repeat_interleave(8, 3)
    grad = F.normalize(torch.randn(n, 2, generator=gen), dim=1)
    target = F.normalize(torch.randn(n, 2, generator=torch.Generator().manual_seed(7)), dim=1)
    return obs, occl, grad, target


def workspace_sizes(query_symbol, enc, n, img):
    """What a joint step's workspace query answers for ``n`` envs at ``img``, in bytes and in the units the tables use."""
    from occlusionenv_amd import _native as nat

    wsb, scb = C.c_size_t(), C.c_size_t()
    nat.check(getattr(nat.load(), query_symbol)(C.byref(enc._cfg(img)), n, C.byref(wsb), C.byref(scb)), "workspace query")
    return dict(workspace_bytes=wsb.value, scratch_bytes=scb.value, workspace_mib_per_env=wsb.value / n / 2 ** 20,
                workspace_gib=wsb.value / 2 ** 30, scratch_mib=scb.value / 2 ** 20)


def encoder_work(img, separable, residual):
    """(MACs, least bytes) per env of the frozen encoder's forward."""
    from occlusionenv_amd.encoder import layer_plan

    macs, nbytes, h = 0, 4 * 4 * img * img, img
    for _stem, cin, cout, sep, stride in layer_plan(separable):
        ho = h if stride == 1 else (h + 1) // 2
        macs += ho * ho * ((6 * cin + cin * cout) if sep else 9 * cin * cout)
        nbytes += 4 * cout * ho * ho + (4 * cin * h * h if _stem != "initial." else 0)
        if residual and "Layer 2" in _stem:
            nbytes += 4 * cout * ho * ho
        h = ho
    return macs, nbytes


# ---- kernel tables and launch counts --------------------------------------------------------------------------------------------
def kernel_stats(path, steps, note):
    """The per-kernel table of a ``rocprofv3 --kernel-trace --stats`` CSV (*_kernel_stats.csv), template arguments kept,
    the signature dropped; ``steps``: the native steps of every traced (preset, shape) pair."""
    kernels, total = {}, 0.0
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Name"].split("(")[0].replace("void ", "").replace("occ::", "")
            us = float(row["TotalDurationNs"]) / 1e3
            k = kernels.setdefault(name, dict(calls=0, total_us=0.0))
            k["calls"] += int(row["Calls"])
            k["total_us"] = round(k["total_us"] + us, 1)
            total += us
    for k in kernels.values():
        k["us_per_step_of_every_config"] = round(k["total_us"] / steps, 1)
    native = {n: k for n, k in kernels.items() if n.startswith("occ_")}
    other = round(sum(k["total_us"] for n, k in kernels.items() if n not in native) / steps, 1)
    ordered = dict(sorted(native.items(), key=lambda kv: -kv[1]["total_us"]))
    return dict(note=note, native_steps_traced_per_config=steps, total_kernel_us_per_step_of_every_config=round(total / steps, 1),
                torch_ops_us_per_step_of_every_config=other, kernels=ordered)


def count_launches(step):
    """(kernels, copies and memsets) of one step, from torch.profiler's device events."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    device = [e for e in prof.events() if e.device_type == DeviceType.CUDA]
    other = [e for e in device if e.name.lower().startswith(("memcpy", "memset", "copybuffer", "fillbuffer"))]
    return len(device) - len(other), len(other)


def launch_counts(paths, prefix=""):
    """``count_launches`` of every path under ``{prefix}{name}_*``.  The trace is evidence, not the product: where it fails,
    say what went wrong and keep the timings."""
    out = {}
    for k, fn in paths.items():
        try:
            out[f"{prefix}{k}_kernel_launches"], out[f"{prefix}{k}_copies_and_memsets"] = count_launches(fn)
        except Exception as e:
            out[f"{prefix}{k}_kernel_launches"], out[f"{prefix}{k}_launch_count_error"] = None, repr(e)
    return out


# ---- the resident generation benches --------------------------------------------------------------------------------------------
@contextlib.contextmanager
def counted_steps(eng):
    """Counts the calls of ``eng.step`` while active (``["n"]`` of what it yields); restores ``eng.step`` on exit."""
    count, real = dict(n=0), eng.step

    def counted(*a, **kw):
        count["n"] += 1
        return real(*a, **kw)

    eng.step = counted
    try:
        yield count
    finally:
        eng.step = real


def generation_loop(eng, lr, gen):
    """The bare loop the dataset generators share: ``eng.step`` with its backward and the action draws, nothing stored.
    -> (one iteration as a fn, the dict it leaves the last step's ``obs`` and ``fs`` in)."""
    N, dev = eng.N, eng.device
    state = dict(action=lr * torch.randn(N, 2, device=dev, generator=gen))

    def bare():
        a = state["action"].clone().requires_grad_(True)
        obs, rewards, dones, full_state, loss = eng.step(a)
        rewards.sum().backward()
        good = ~torch.isnan(a.grad).any(1)
        fresh = lr * torch.randn(N, 2, device=dev, generator=gen)
        state["action"] = torch.where(good[:, None], fresh, state["action"])
        state["obs"], state["fs"] = obs.detach(), full_state.detach()

    return bare, state


def timed_generation(eng, key, generate, iters, frames):
    """``1 + iters // 2`` whole calls of ``generate()`` (it returns the dataset) on the host clock, each ending in a device
    synchronise; the first warms up, the median-low of the rest is reported under ``{key}_*``."""
    secs, steps = [], []
    for it in range(1 + iters // 2):
        with counted_steps(eng) as count:
            torch.cuda.synchronize()
            t = time.perf_counter()
            ds = generate()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
        assert len(ds) == frames
        del ds
        if it:
            secs.append(dt)
            steps.append(count["n"])
    return median_low_run(key, secs, steps, frames)


# ---- arguments and output -------------------------------------------------------------------------------------------------------
def parse_shapes(text):
    """"128x256,64x512" -> [(128, 256), (64, 512)]"""
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",")]


def emit(result):
    print(json.dumps({k: v for k, v in result.items() if not k.endswith("_all")}), flush=True)


def write(out, path):
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
