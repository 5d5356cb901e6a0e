"""One training step of a native training path below its optimizer (forward, loss, ``backward``; gradients to every
trainable parameter, no optimizer) against the same expressions as PyTorch-ROCm ops in f32 with torch autograd.  ``--path``:

  encoder      ``enctrain.TrainableEncoder``: ``net.predict_grad(obs)`` -> ``F.mse_loss`` (csrc/occ_encoder_bwd.hpp), preset
               "predictor", against tests/encoder_model.preset_forward;
  sep-encoder  ``septrain.TrainableSeparableEncoder``, the same step (csrc/occ_sepenc_bwd.hpp).  Presets: "ppo" = the fixture
               tests/golden/encoder_golden.npz (dilation 2, residual, gradPredictor head), "predictor" =
               tests/train_model.sep_state_dict("predictor", 32, gain 1.25) (dilation 1, no residual, tanh head);
  decoder      ``seghead.SegmentationHead``: ``head(obs)`` -> ``binary_dice_loss`` (csrc/occ_decoder_bwd.hpp) on the object's
               footprint, against the frozen-encoder / trainable-decoder expressions of tests/segmenter_model.py with loss.py's
               Dice formula; both run the frozen encoder without a graph;
  fullnet      ``fullnet.TrainableFullNetwork``: ``net(obs)`` -> Dice + MSE (csrc/occ_fullnet_bwd.hpp), "ppo" at dilation 1
               with the residual, against tests/train_model.forward_gated;
  sep-fullnet  ``sepfullnet.TrainableSeparableFullNetwork``, the same step on the network the agent runs (the fixture
               tests/golden/segmenter_golden.npz, dilation 2), against tests/segmenter_model.full_forward.

The two joint paths have a second rival, "split": what reaches the same parameters without the joint backward, one
``SegmentationHead`` step (Dice) plus one step of the path's trainable encoder (MSE on the head), which runs the encoder
twice and still misses the join.  The torch paths run BatchNorm with its running statistics, as the native ones do.
``--batch-stats`` (joint paths): BatchNorm in train mode instead (csrc/occ_bn_train.hpp): the native
``from_encoder(enc, batch_stats=True)`` step against ``forward_gated`` with ``F.batch_norm(training=True)`` and against the
native running-statistics step of the same build; the running-statistics step recorded in the path's committed profile is
reported next to them when it is there.

Method (scripts/benchlib.py): one process; each sample is ``--calls`` steps between two device events; ``--warmup`` rounds
of every path, then ``--iters`` rounds, each visiting the native path and its rivals in turn.  All samples are kept; medians
are compared, with the larger of the min-max spreads of the two paths compared as the margin.  Before the timing, the loss
of a first call of each side and the gradients' largest difference relative to the largest torch gradient, per parameter
kind.  ``--native-only``: the native step alone, for a kernel trace; ``--stats-from``: the per-kernel table of that trace.

The profiles (committed, but for the one marked; shapes 128 x 256^2 and 64 x 512^2 unless said otherwise):

    python scripts/train_step_bench.py --path encoder --out profiles/encoder_train_bench.json
    python scripts/train_step_bench.py --path sep-encoder --out profiles/sep_encoder_train_bench.json
    python scripts/train_step_bench.py --path decoder --out profiles/decoder_train_bench.json
    python scripts/train_step_bench.py --path fullnet --out profiles/fullnet_train_bench.json    # not recorded yet
    python scripts/train_step_bench.py --path sep-fullnet --out profiles/sep_fullnet_train_bench.json
    python scripts/train_step_bench.py --path fullnet --batch-stats --iters 6 --calls 2 --out profiles/fullnet_bn_train_bench.json
    python scripts/train_step_bench.py --path sep-fullnet --batch-stats --iters 6 --calls 2 --out profiles/sep_fullnet_bn_train_bench.json

and their kernel tables, each trace a run of its own with no other tracing (PATH as above):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o trace -- \\
        python scripts/train_step_bench.py --path PATH --native-only --warmup 1 --iters 3 --calls 1
    python scripts/train_step_bench.py --path PATH --stats-from DIR/.../trace_kernel_stats.csv --stats-steps 4 \\
        --out profiles/sep_encoder_train_kernel_stats.json   # or sep_fullnet_train_kernel_stats.json

(profiles/encoder_train_kernel_stats.json and profiles/decoder_train_kernel_stats.json were grouped by hand from the same kind
of trace; the decoder's ran ``--path decoder --shapes 128x256 --warmup 1 --iters 2 --calls 3``.)
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import benchlib as bl  # noqa: E402
from occlusionenv_amd.segmentation import binary_dice_loss as native_dice  # noqa: E402
from tests import segmenter_model as sm  # noqa: E402
from tests import train_model as m  # noqa: E402
from tests.encoder_model import golden_state_dict, preset_forward  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


# ---- the three step expressions: (outputs of the forward, segmentation target, unit target) -> loss ---------------------------
def file_dice(prob, target):
    """loss.py's Dice formula, as the decoder's torch side has always written it."""
    pf, tf = prob.reshape(prob.shape[0], -1), target.reshape(target.shape[0], -1)
    return (1 - (torch.sum(pf * tf, dim=1) + 1) / (torch.sum(pf.pow(2) + tf.pow(2), dim=1) + 1)).mean()


def joint_expr(net, obs, seg, unit):
    _pooled, segm, pred = net(obs)
    return native_dice(segm, seg) + F.mse_loss(pred, unit)


def split_expr(head, tenc, obs, seg, unit):
    """The joint paths' second rival: one head step, then the trainable encoder's."""
    native_dice(head(obs), seg).backward()
    return F.mse_loss(tenc.predict_grad(obs), unit)


NATIVE_STEP = dict(predict=lambda net, obs, seg, unit: F.mse_loss(net.predict_grad(obs), unit),
                   head=lambda net, obs, seg, unit: native_dice(net(obs), seg), joint=joint_expr)
TORCH_LOSS = dict(predict=lambda out, seg, unit: F.mse_loss(out, unit),
                  head=lambda out, seg, unit: file_dice(out, seg),
                  joint=lambda out, seg, unit: bl.dice(out[0], seg) + F.mse_loss(out[1], unit))


# ---- the torch f32 forwards: (frozen state dict, the same with the trainable tensors, obs, preset) -> outputs ------------------
def decoder_forward(sd, sdp, obs, preset):
    p = sm.PRESETS[preset]
    with torch.no_grad():
        x, skips = sm.encode_full(sd, obs, p["prefix"], True, p["dilation"], p["residual"])
    feats = sm.decode(sdp, x, skips, p["decoder"])
    return torch.sigmoid(F.conv2d(feats, sdp[p["classifier"] + "weight"], sdp[p["classifier"] + "bias"]))


def gated_forward(net, running=None):
    def forward(sd, sdp, obs, preset):
        pooled, logit = m.forward_gated(sdp, obs, net, running=running)
        return torch.sigmoid(logit), F.linear(pooled, sdp["gradPredictor.weight"], sdp["gradPredictor.bias"])

    return forward


def full_forward(sd, sdp, obs, preset):
    out = sm.full_forward(sdp, obs, "ppo", 2, True)
    return out["prob"], out["grad"]


# ---- the weights: preset -> the f32 state dict the frozen encoder is built from -------------------------------------------------
def sep_encoder_weights(preset):
    if preset == "ppo":
        g = np.load(os.path.join(GOLDEN, "encoder_golden.npz"))
        return {k: v.float() for k, v in golden_state_dict(g, "ppo").items() if v.is_floating_point()}
    return {k: v.float() for k, v in m.sep_state_dict("predictor", 32, gain=1.25).items()}


def decoder_weights(preset):
    sd = sm.golden_seg_state_dict(np.load(os.path.join(GOLDEN, "segmenter_golden.npz")), preset)
    return {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}


def tail_kind(key):
    return key[key.index(".conv.") + 1:] if ".conv." in key else ".".join(key.split(".")[-2:])


DENSE_JOINT, SEP_JOINT = m.Net("ppo", False, 1, True, True), m.Net("ppo", True, 2, True, True)
SIZES = ("workspace_bytes", "scratch_bytes", "workspace_mib_per_env", "workspace_gib", "scratch_mib")

def path_row(net, presets, step, weights, forward, kind, enc=None, calls=3, rule=bl.ONE_RIVAL, describe=False, split=None,
             model=None, query=None, sizes=()):
    """One row of PATHS, every field present.  net, split: the trainable class and the split rival's trainable encoder, as
    module.Class under occlusionenv_amd (imported when a run needs them).  presets, weights, enc: the checkpoints and how
    the frozen encoder is built from one.  step: the key of the native expression and of the torch loss.  forward: the
    torch f32 forward.  kind: parameter key -> the kind its gradient error is reported under.  calls, rule: steps per
    sample and the key names of a comparison.  describe: the result names its preset, dilation and residual.  model,
    query, sizes (joint paths): the tests' description of the network, the workspace query and the size keys reported."""
    return dict(net=net, presets=presets, step=step, weights=weights, forward=forward, kind=kind, enc=enc or {}, calls=calls, rule=rule,
                describe=describe, split=split, model=model, query=query, sizes=sizes)


def predictor_forward(sd, sdp, obs, preset):
    return preset_forward(sdp, obs, preset)[1]


PATHS = {
    "encoder": path_row(
        "enctrain.TrainableEncoder", ("predictor",), "predict",
        lambda preset: {k: v.float() for k, v in m.dense_state_dict(preset, 32).items()}, predictor_forward, tail_kind),
    "sep-encoder": path_row(
        "septrain.TrainableSeparableEncoder", ("ppo", "predictor"), "predict", sep_encoder_weights, predictor_forward, tail_kind,
        describe=True),
    "decoder": path_row(
        "seghead.SegmentationHead", ("ppo",), "head", decoder_weights, decoder_forward, tail_kind, calls=5,
        rule=bl.ONE_RIVAL_NOT_SLOWER),
    "fullnet": path_row(
        "fullnet.TrainableFullNetwork", ("ppo",), "joint", lambda preset: {k: v.float() for k, v in m.state_dict(preset).items()},
        gated_forward(DENSE_JOINT), lambda k: m.kind(DENSE_JOINT, k), enc=dict(dilation=1, residual=True), rule=bl.VS_RIVAL,
        split="enctrain.TrainableEncoder", model=DENSE_JOINT, query="occ_fullnet_train_workspace_query", sizes=SIZES[2:]),
    "sep-fullnet": path_row(
        "sepfullnet.TrainableSeparableFullNetwork", ("ppo",), "joint", lambda preset: m.golden_state_dict(), full_forward,
        lambda k: m.kind(SEP_JOINT, k), enc=dict(dilation=2, residual=True), rule=bl.VS_RIVAL, describe=True,
        split="septrain.TrainableSeparableEncoder", model=SEP_JOINT, query="occ_sep_fullnet_train_workspace_query", sizes=SIZES),
}
BN_QUERY = "occ_fullnet_bn_train_workspace_query"


def trainable(name):
    module, cls = name.split(".")
    return getattr(importlib.import_module("occlusionenv_amd." + module), cls)


def native_step_fn(nets, expr, obs, seg, unit):
    def step():
        for net in nets:
            net.zero_grad(set_to_none=True)
        loss = expr(*nets, obs, seg, unit)
        loss.backward()
        return loss

    return step


def torch_step_fn(row, sd, params, preset, obs, seg, unit, forward):
    sdp = dict(sd)
    sdp.update(params)

    def step():
        for v in params.values():
            v.grad = None
        loss = TORCH_LOSS[row["step"]](forward(sd, sdp, obs, preset), seg, unit)
        loss.backward()
        return loss

    return step


def recorded_native_ms(profile, n, img):
    """native_ms of the shape in a committed profile of the running-statistics bench, or None."""
    if not os.path.exists(profile):
        return None
    with open(profile) as f:
        shapes = json.load(f).get("shapes", [])
    return next((s["native_ms"] for s in shapes if s.get("n_env") == n and s.get("img") == img), None)


def run_shape(path, preset, sd32, enc, n, img, warmup, iters, calls, native_only, batch_stats):
    from occlusionenv_amd.seghead import SegmentationHead

    row = PATHS[path]
    obs, occl, grad, target = (t.cuda() for t in bl.train_inputs(n, img))
    seg = (obs[:, 3:4] > 0).float() if row["step"] == "head" else occl  # the object's footprint: a 0/1 map with structure
    unit = target if row["step"] == "predict" else grad
    cls, expr = trainable(row["net"]), NATIVE_STEP[row["step"]]
    net = cls.from_encoder(enc, batch_stats=True) if batch_stats else cls.from_encoder(enc)
    nat = native_step_fn([net], expr, obs, seg, unit)
    out = {}
    if batch_stats or row["describe"]:
        out = dict(preset=preset, batch_stats=True, dilation=enc.dilation, residual=enc.residual)
        if not batch_stats:
            del out["batch_stats"]
    out.update(n_env=n, img=img)
    sizes = {}
    if row["query"]:
        every = bl.workspace_sizes(BN_QUERY if batch_stats else row["query"], enc, n, img)
        sizes = {k: every[k] for k in (SIZES[:3] if batch_stats else row["sizes"])}
    if native_only and not batch_stats:  # the train-mode run has no native-only form: the switch is ignored there
        nms = bl.interleaved(dict(native=nat), warmup, iters, calls)["native"]
        return dict(out, native_ms=statistics.median(nms), native_ms_all=nms, **sizes)
    sd = {k: v.cuda() for k, v in sd32.items() if v.is_floating_point()}
    params = {k: sd[k].clone().requires_grad_() for k, _p in net.named_parameters()}
    forward = row["forward"]
    if batch_stats:
        model = row["model"]._replace(dilation=enc.dilation, residual=enc.residual, batch_stats=True)
        forward = gated_forward(model, running={st + leaf: sd[st + leaf].clone() for st in m.bn_stems(model) for leaf in m.STATS})
    paths = dict(native=nat, torch=torch_step_fn(row, sd, params, preset, obs, seg, unit, forward))
    if batch_stats:
        paths["running_stats"] = native_step_fn([cls.from_encoder(enc)], expr, obs, seg, unit)
    elif row["split"]:
        paths["split"] = native_step_fn([SegmentationHead.from_encoder(enc), trainable(row["split"]).from_encoder(enc)], split_expr,
                                        obs, seg, unit)
    lw, lg = float(paths["torch"]().detach()), float(nat().detach())
    rel = {}
    for k, p in net.named_parameters():
        err = float((p.grad - params[k].grad).abs().max() / params[k].grad.abs().max())
        rel[row["kind"](k)] = max(rel.get(row["kind"](k), 0.0), err)
    ms = bl.interleaved(paths, warmup, iters, calls)
    if batch_stats:
        out.update(bl.named(bl.compare(ms["native"], ms["torch"]), bl.BN_VS_TORCH))
        out.update(bl.named(bl.compare(ms["native"], ms["running_stats"]), bl.BN_VS_RUNNING))
        parent = recorded_native_ms(os.path.join(ROOT, "profiles", path.replace("-", "_") + "_train_bench.json"), n, img)
        out.update(parent_running_stats_ms=parent, ratio_to_parent_running_stats=(out["native_ms"] / parent if parent else None))
    else:
        for rival in list(paths)[1:]:
            out.update(bl.named(bl.compare(ms["native"], ms[rival]), row["rule"], r=rival))
    return dict(out, loss_native=lg, loss_torch_f32=lw, grad_rel_to_max_vs_torch_f32=rel, **sizes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", required=True, choices=list(PATHS))
    ap.add_argument("--shapes", default="128x256,64x512")
    ap.add_argument("--presets", default=None, help="comma separated, of the path's presets (default: all of them)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--calls", type=int, default=None, help="steps per timed sample (default: 3, the decoder's 5)")
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--batch-stats", action="store_true", help="the joint paths' train-mode BatchNorm step")
    ap.add_argument("--stats-from", default=None, help="summarise a rocprofv3 *_kernel_stats.csv instead of timing")
    ap.add_argument("--stats-steps", type=int, default=4, help="native steps traced per (preset, shape)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    row = PATHS[args.path]
    presets = args.presets.split(",") if args.presets else row["presets"]
    if args.batch_stats and not row["model"]:
        ap.error("--batch-stats: only the joint paths have a train-mode BatchNorm step")
    if not set(presets) <= set(row["presets"]):
        ap.error(f"--presets: {args.path} has {', '.join(row['presets'])}")
    if args.stats_from:
        share = "the presets and shapes share one trace, so times are per one step of every (preset, shape) pair" \
            if len(row["presets"]) > 1 else "the shapes share one trace, so times are per one step of every shape"
        return bl.write(bl.kernel_stats(args.stats_from, args.stats_steps, f"rocprofv3 --kernel-trace --stats of scripts/"
                                        f"train_step_bench.py --path {args.path} --native-only, a run of its own; {share}"), args.out)
    from occlusionenv_amd.encoder import FrozenEncoder

    assert torch.cuda.is_available(), "train_step_bench needs a GPU"
    calls = args.calls or row["calls"]
    shapes = []
    for preset in presets:
        sd32 = row["weights"](preset)
        enc = FrozenEncoder.from_state_dict(sd32, preset=preset, **row["enc"])
        assert enc.separable or not args.path.startswith("sep-")
        assert enc.has_decoder or not row["model"]
        for n, img in bl.parse_shapes(args.shapes):
            r = run_shape(args.path, preset, sd32, enc, n, img, args.warmup, args.iters, calls, args.native_only, args.batch_stats)
            bl.emit(r)
            shapes.append(r)
            if row["model"]:  # the joint paths' workspaces are GiB: give them back between shapes, as those benches always did
                torch.cuda.empty_cache()
    bl.write(dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, iters=args.iters, calls_per_sample=calls, shapes=shapes),
             args.out)


if __name__ == "__main__":
    main()
