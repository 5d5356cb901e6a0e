"""One step of the pretrainer below its optimizer, native (occlusionenv_amd/fullnet.py: ``net(obs)`` -> Dice + MSE ->
``backward``; csrc/occ_fullnet_bwd.hpp) against the same expressions of tests/train_model.py as PyTorch-ROCm ops in
f32 with torch autograd, and against what reaches the same parameters without the joint backward: one
``seghead.SegmentationHead`` step (Dice) plus one ``enctrain.TrainableEncoder`` step (MSE on the head), which runs the encoder
twice and still misses the join.  One process, interleaved samples.

    python scripts/fullnet_train_bench.py --out profiles/fullnet_train_bench.json

Shapes: 128 x 256^2 and 64 x 512^2, preset "ppo" at dilation 1 with the residual.  No path runs an optimizer.  The torch path
runs BatchNorm with its running statistics, as the native ones do.  Each sample is ``--calls`` steps between two HIP events;
after ``--warmup`` samples of each path, ``--iters`` samples alternate between the three.  All samples are kept; medians are
compared, with the larger of the min-max spreads of the two paths compared as the margin.  ``--native-only``: the native joint
step alone, for a kernel trace.  ``--batch-stats``: BatchNorm in train mode instead (scripts/bn_step_bench.py): the native
``batch_stats=True`` step against torch autograd in train mode and against the running-statistics step:

    python scripts/fullnet_train_bench.py --batch-stats --out profiles/fullnet_bn_train_bench.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from occlusionenv_amd import _native as nat  # noqa: E402
from occlusionenv_amd import segmentation  # noqa: E402
from occlusionenv_amd.encoder import FrozenEncoder  # noqa: E402
from occlusionenv_amd.enctrain import TrainableEncoder  # noqa: E402
from occlusionenv_amd.fullnet import TrainableFullNetwork  # noqa: E402
from occlusionenv_amd.seghead import SegmentationHead  # noqa: E402
from tests import train_model as m  # noqa: E402
from tests.encoder_model import make_obs  # noqa: E402

NET = m.Net("ppo", False, 1, True, True)  # the dense joint network


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


def torch_step_fn(sd, params, obs, occl, grad):
    sdp = dict(sd)
    sdp.update(params)

    def step():
        for v in params.values():
            v.grad = None
        pooled, logit = m.forward_gated(sdp, obs, NET)
        pred = F.linear(pooled, sdp["gradPredictor.weight"], sdp["gradPredictor.bias"])
        loss = dice(torch.sigmoid(logit), occl) + F.mse_loss(pred, grad)
        loss.backward()
        return loss

    return step


def native_step_fn(net, obs, occl, grad):
    def step():
        net.zero_grad(set_to_none=True)
        _pooled, segm, pred = net(obs)
        loss = segmentation.binary_dice_loss(segm, occl) + F.mse_loss(pred, grad)
        loss.backward()
        return loss

    return step


def split_step_fn(head, tenc, obs, occl, grad):
    def step():
        head.zero_grad(set_to_none=True)
        tenc.zero_grad(set_to_none=True)
        segmentation.binary_dice_loss(head(obs), occl).backward()
        loss = F.mse_loss(tenc.predict_grad(obs), grad)
        loss.backward()
        return loss

    return step


def run_shape(sd32, enc, n, img, warmup, iters, calls, native_only, batch_stats=False):
    base = make_obs(31, 8, img).float()
    obs = base[torch.arange(n) % 8].cuda()
    gen = torch.Generator().manual_seed(7)
    occl = (torch.rand(n, 1, img // 8, img // 8, generator=gen) > 0.5).float().repeat_interleave(8, 2).repeat_interleave(8, 3).cuda()
    grad = F.normalize(torch.randn(n, 2, generator=gen), dim=1).cuda()
    if batch_stats:
        import bn_step_bench

        return bn_step_bench.run_shape(TrainableFullNetwork, "dense", lambda k: m.kind(NET, k), sd32, enc, obs, occl, grad, warmup,
                                       iters, calls, os.path.join(ROOT, "profiles", "fullnet_train_bench.json"))
    net = TrainableFullNetwork.from_encoder(enc)
    joint = native_step_fn(net, obs, occl, grad)
    wsb, scb = C.c_size_t(), C.c_size_t()
    nat.check(nat.load().occ_fullnet_train_workspace_query(C.byref(enc._cfg(img)), n, C.byref(wsb), C.byref(scb)), "workspace query")
    sizes = dict(workspace_mib_per_env=wsb.value / n / 2 ** 20, workspace_gib=wsb.value / 2 ** 30, scratch_mib=scb.value / 2 ** 20)
    if native_only:
        for _ in range(warmup):
            sample(joint, calls)
        nms = [sample(joint, calls) for _ in range(iters)]
        return dict(n_env=n, img=img, native_ms=statistics.median(nms), native_ms_all=nms, **sizes)
    sd = {k: v.cuda() for k, v in sd32.items()}
    params = {k: sd[k].clone().requires_grad_() for k, _p in net.named_parameters()}
    ref = torch_step_fn(sd, params, obs, occl, grad)
    split = split_step_fn(SegmentationHead.from_encoder(enc), TrainableEncoder.from_encoder(enc), obs, occl, grad)
    lw, lg = float(ref().detach()), float(joint().detach())
    rel = {}
    for k, p in net.named_parameters():
        err = float((p.grad - params[k].grad).abs().max() / params[k].grad.abs().max())
        rel[m.kind(NET, k)] = max(rel.get(m.kind(NET, k), 0.0), err)
    for _ in range(warmup):
        sample(joint, calls), sample(ref, calls), sample(split, calls)
    nms, tms, sms = [], [], []
    for _ in range(iters):
        nms.append(sample(joint, calls))
        tms.append(sample(ref, calls))
        sms.append(sample(split, calls))
    med, tmed, smed = statistics.median(nms), statistics.median(tms), statistics.median(sms)
    spread = lambda v: max(v) - min(v)  # noqa: E731
    margin_t, margin_s = max(spread(nms), spread(tms)), max(spread(nms), spread(sms))
    return dict(n_env=n, img=img, native_ms=med, native_ms_all=nms, torch_ms=tmed, torch_ms_all=tms, split_ms=smed, split_ms_all=sms,
                native_spread_ms=spread(nms), torch_spread_ms=spread(tms), split_spread_ms=spread(sms), margin_vs_torch_ms=margin_t,
                margin_vs_split_ms=margin_s, speedup_vs_torch=tmed / med, speedup_vs_split=smed / med,
                faster_than_torch_by_more_than_margin=bool(med + margin_t < tmed),
                faster_than_split_by_more_than_margin=bool(med + margin_s < smed), loss_native=lg, loss_torch_f32=lw,
                grad_rel_to_max_vs_torch_f32=rel, **sizes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x256,64x512")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--calls", type=int, default=3, help="steps per timed sample")
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--batch-stats", action="store_true", help="time the train-mode BatchNorm step (scripts/bn_step_bench.py)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "fullnet_train_bench needs a GPU"
    sd32 = {k: v.float() for k, v in m.state_dict("ppo").items()}
    enc = FrozenEncoder.from_state_dict(sd32, preset="ppo", dilation=1, residual=True)
    shapes = []
    for s in args.shapes.split(","):
        n, img = (int(v) for v in s.split("x"))
        r = run_shape(sd32, enc, n, img, args.warmup, args.iters, args.calls, args.native_only, args.batch_stats)
        print(json.dumps({k: v for k, v in r.items() if not k.endswith("_all")}), flush=True)
        shapes.append(r)
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, iters=args.iters, calls_per_sample=args.calls, shapes=shapes)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
