"""The ``--batch-stats`` mode of scripts/fullnet_train_bench.py and scripts/sep_fullnet_train_bench.py: one step of the
pretrainer below its optimizer with BatchNorm in train mode, native (``from_encoder(enc, batch_stats=True)``: ``net(obs)`` ->
Dice + MSE -> ``backward``; csrc/occ_bn_train.hpp) against (a) the same network as PyTorch-ROCm ops in f32 with torch autograd
and ``F.batch_norm(training=True)`` (tests/train_model.forward_gated) and (b) the native running-statistics step of the
same build.  One process, interleaved samples, medians compared with the larger min-max spread as the margin.  The
running-statistics step the parent commit recorded for the shape (``profile``, the script's committed output) is reported next
to them when it is there.
"""
import ctypes as C
import json
import os
import statistics

import torch
import torch.nn.functional as F


def sample(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def dice(p, t):
    p, t = p.reshape(p.shape[0], -1), t.reshape(t.shape[0], -1)
    return (1.0 - ((p * t).sum(1) + 1.0) / ((p * p).sum(1) + (t * t).sum(1) + 1.0)).mean()


def recorded_native_ms(profile, n, img):
    """native_ms of the shape in a committed profile of the running-statistics bench, or None."""
    if not profile or not os.path.exists(profile):
        return None
    with open(profile) as f:
        shapes = json.load(f).get("shapes", [])
    return next((s["native_ms"] for s in shapes if s.get("n_env") == n and s.get("img") == img), None)


def run_shape(net_class, form, kind, sd32, enc, obs, occl, grad, warmup, iters, calls, profile=None):
    from occlusionenv_amd import _native as nat
    from occlusionenv_amd import segmentation
    from tests import train_model as tm

    n, img = int(obs.shape[0]), int(obs.shape[2])

    def native_step_fn(net):
        def step():
            net.zero_grad(set_to_none=True)
            _pooled, segm, pred = net(obs)
            loss = segmentation.binary_dice_loss(segm, occl) + F.mse_loss(pred, grad)
            loss.backward()
            return loss

        return step

    net = net_class.from_encoder(enc, batch_stats=True)
    train = native_step_fn(net)
    running = native_step_fn(net_class.from_encoder(enc))
    sd = {k: v.cuda() for k, v in sd32.items()}
    params = {k: sd[k].clone().requires_grad_() for k, _p in net.named_parameters()}
    sdp = dict(sd)
    sdp.update(params)
    model = tm.Net("ppo", form == "separable", enc.dilation, enc.residual, True, True)
    buffers = {st + leaf: sd[st + leaf].clone() for st in tm.bn_stems(model) for leaf in tm.STATS}

    def ref():
        for v in params.values():
            v.grad = None
        pooled, logit = tm.forward_gated(sdp, obs, model, running=buffers)
        pred = F.linear(pooled, sdp["gradPredictor.weight"], sdp["gradPredictor.bias"])
        loss = dice(torch.sigmoid(logit), occl) + F.mse_loss(pred, grad)
        loss.backward()
        return loss

    lw, lg = float(ref().detach()), float(train().detach())
    rel = {}
    for k, p in net.named_parameters():
        err = float((p.grad - params[k].grad).abs().max() / params[k].grad.abs().max())
        rel[kind(k)] = max(rel.get(kind(k), 0.0), err)
    for _ in range(warmup):
        sample(train, calls), sample(ref, calls), sample(running, calls)
    nms, tms, rms = [], [], []
    for _ in range(iters):
        nms.append(sample(train, calls))
        tms.append(sample(ref, calls))
        rms.append(sample(running, calls))
    med, tmed, rmed = statistics.median(nms), statistics.median(tms), statistics.median(rms)
    spread = lambda v: max(v) - min(v)  # noqa: E731
    wsb, scb = C.c_size_t(), C.c_size_t()
    nat.check(nat.load().occ_fullnet_bn_train_workspace_query(C.byref(enc._cfg(img)), n, C.byref(wsb), C.byref(scb)),
              "workspace query")
    parent = recorded_native_ms(profile, n, img)
    return dict(preset="ppo", batch_stats=True, dilation=enc.dilation, residual=enc.residual, n_env=n, img=img,
                native_ms=med, native_ms_all=nms, torch_train_mode_ms=tmed, torch_train_mode_ms_all=tms,
                running_stats_ms=rmed, running_stats_ms_all=rms, native_spread_ms=spread(nms), torch_spread_ms=spread(tms),
                running_stats_spread_ms=spread(rms), speedup_vs_torch=tmed / med,
                faster_than_torch_by_more_than_margin=bool(med + max(spread(nms), spread(tms)) < tmed),
                ratio_to_running_stats=med / rmed, parent_running_stats_ms=parent,
                ratio_to_parent_running_stats=(med / parent if parent else None), loss_native=lg, loss_torch_f32=lw,
                grad_rel_to_max_vs_torch_f32=rel, workspace_bytes=wsb.value, scratch_bytes=scb.value,
                workspace_mib_per_env=wsb.value / n / 2 ** 20)
