"""The workspaces, the scratch and the K splits of the native training paths restated in plain integers from
include/occlusionenv_amd.h and the comments of csrc/occ_encoder_bwd.hpp, csrc/occ_sepenc_bwd.hpp, csrc/occ_fullnet_bwd.hpp
and csrc/occ_bn_train.hpp: what the host tests hold to the library's workspace queries, what the split cases of the GPU tests
are chosen from, and where the workspace keeps every layer's relu output.  The decoder's own part is
tests/decoder_split_model.py, on which this builds.  ``net`` is a tests/train_model.Net throughout.

One workspace layout serves every path: the encoder-only workspace (dense and separable keep the same tensors) is a prefix
of the joint one, the joint one a prefix of the batch-statistics one.
"""
from __future__ import annotations

import torch

from tests import decoder_split_model as dsm
from tests.train_model import LEVELS, layers

DW_BLOCKS = 512    # blocks of a dense layer's weight gradient: K slices x (ci, co) tiles
DPW_BLOCKS = 1024  # blocks of a separable layer's pointwise weight gradient
ACT_CHUNK = 4096   # pixels of one (env, channel) plane per block of an activation step
CHANNELS = 1248    # of the 21 BatchNorm layers: 1000 encoder + 248 decoder


def sides(img):
    """[H_0 .. H_5]: the sides halve with ceiling."""
    out = [img]
    for _ in range(LEVELS):
        out.append((out[-1] + 1) // 2)
    return out


def chunks(plane):
    return -(-plane // ACT_CHUNK)


def layer_shapes(img):
    """[(channels, side)] of the 21 layers' outputs in packed order."""
    out, h = [(8, img)], img
    for lv in range(LEVELS):
        out += [(8 << lv, h), (8 << lv, h), (16 << lv, (h + 1) // 2)]
        h = (h + 1) // 2
    return out + [(128 >> j, (img // 16) << j) for j in range(LEVELS)]


# ---- the K split of the weight gradients ---------------------------------------------------------------------------------------
def dw_plans(img, n):
    """The dense encoder.  One dict per layer in packed order: the (ci, co) tile, the pixel tile, tiles per slice, slices,
    partial rows."""
    hs = sides(img)
    plans = []
    for i, (_stem, cin, cout, _sep, stride) in enumerate(layers(False)):
        lv = 0 if i == 0 else (i - 1) // 3
        ho = hs[lv + 1] if stride == 2 else hs[lv]
        cib, cob = min(cin, 64), min(cout, 32)
        t = 4 if cib == 64 else 8
        q = cib * (cob // 8)
        pb = 256 // max(q, 64)
        grid_y = (cin // cib) * (cout // cob)
        tiles_x = -(-ho // t)
        total = n * tiles_x * tiles_x
        want = DW_BLOCKS // grid_y
        tps = -(-total // want)
        slices = -(-total // tps)
        te = tiles_x * tiles_x
        plans.append(dict(sep=False, cin=cin, cout=cout, stride=stride, ho=ho, T=t, cib=cib, cob=cob, pb=pb, grid_y=grid_y,
                          tiles_env=te, total_tiles=total, tps=tps, slices=slices, short_last=total % tps != 0,
                          straddles=any((s * tps) // te != (min(s * tps + tps, total) - 1) // te for s in range(slices)),
                          part_bytes=slices * pb * cin * 9 * cout * 4))
    return plans


def dpw_plans(img, n):
    """The separable encoder.  One dict per layer in packed order.  Separable layers: the (ci, co) tile, the pixel tile, tiles
    per slice, slices and partial rows of the pointwise weight gradient; downs: dw_plans' entry (the dense kernels run)."""
    hs = sides(img)
    dense = dw_plans(img, n)
    plans = []
    for i, (_stem, cin, cout, sep, _stride) in enumerate(layers(True)):
        if not sep:
            plans.append(dense[i])
            continue
        h = hs[0 if i == 0 else (i - 1) // 3]
        cib, cob = min(cin, 64), min(cout, 32)
        t = 16 if cib <= 8 else 4 if cib == 64 else 8
        q = cib * (cob // 8)
        pb = 256 // max(q, 64)
        grid_y = (cin // cib) * (cout // cob)
        tiles_x = -(-h // t)
        total = n * tiles_x * tiles_x
        want = DPW_BLOCKS // grid_y
        tps = -(-total // want)
        slices = -(-total // tps)
        te = tiles_x * tiles_x
        plans.append(dict(sep=True, cin=cin, cout=cout, ho=h, T=t, cib=cib, cob=cob, pb=pb, grid_y=grid_y, tiles_env=te,
                          total_tiles=total, tps=tps, slices=slices, short_last=total % tps != 0,
                          straddles=any((s * tps) // te != (min(s * tps + tps, total) - 1) // te for s in range(slices)),
                          part_bytes=slices * pb * cin * cout * 4))
    return plans


def scratch_bytes(net, img, n):
    """max over the encoder's layers of (activation partials, weight-gradient partials, a separable layer's G partials: nine
    f64 sums per (input channel, env, chunk), not split further: one block per chunk), rounded up to 256; a joint net: the
    larger of that and the decoder's.  Batch statistics need no more."""
    if net.frozen_encoder:  # the decoder's alone
        return dsm.scratch_bytes(img, n)
    need = 0
    for p in (dpw_plans if net.separable else dw_plans)(img, n):
        ch = chunks(p["ho"] * p["ho"])
        need = max(need, p["cout"] * n * ch * 3 * 8, p["part_bytes"])
        if p["sep"]:
            need = max(need, p["cin"] * n * ch * 9 * 8)
    need = (need + 255) & ~255
    return max(need, dsm.scratch_bytes(img, n)) if net.joint else need


# ---- the workspace ---------------------------------------------------------------------------------------------------------------
def kept_bytes(img, n):
    """obs, every encoder layer's input and every layer's r, as f32 (a lower bound of the workspace: no alignment, no
    gradients)."""
    hs = sides(img)
    floats = n * 4 * img * img + n * 8 * img * img  # obs, r_init
    for lv in range(LEVELS):
        c, h, ho = 8 << lv, hs[lv], hs[lv + 1]
        floats += 5 * n * c * h * h + n * 2 * c * ho * ho  # a, r1, b, r2, cc; rd
    return 4 * floats


def _tiles(h):
    t = 16 if h >= 16 else 8
    return (-(-h // t)) ** 2


def encoder_ws_bytes(img, n):
    """The workspace of occ_encoder_train_forward: obs | r_init | per level a, r1, b, r2, cc, rd | pool partials | g0..g2."""
    a = dsm.align
    hs = sides(img)
    total = a(4 * n * 4 * img * img) + a(4 * n * 8 * img * img)
    for lv in range(LEVELS):
        c = 8 << lv
        total += 5 * a(4 * n * c * hs[lv] ** 2) + a(4 * n * 2 * c * hs[lv + 1] ** 2)
    return total + a(4 * n * _tiles(hs[LEVELS]) * 256) + 3 * a(4 * n * 8 * img * img)


def extra_ws_bytes(img, n):
    """What batch statistics add: coef (per channel s, t f32 and mu, rstd f64) | abc (A | B | C, 256 f32 each) | the
    forward's partials (the largest layer's c n chunks 2 doubles), every part 256-byte aligned."""
    a = dsm.align
    part = max(c * n * chunks(side * side) * 2 * 8 for c, side in layer_shapes(img))
    return a(24 * CHANNELS) + a(3 * 256 * 4) + a(part)


def segment_ws_bytes(img, n):
    """The workspace of the inference decoder, what occ_segment_workspace_query reports: two level-0 activation buffers |
    pool partials | the five skips | last."""
    a = dsm.align
    skips = sum(a(4 * n * (8 << lv) * (img >> lv) ** 2) for lv in range(LEVELS))
    return 2 * a(4 * n * 8 * img * img) + a(4 * n * _tiles(img >> LEVELS) * 256) + skips + a(4 * n * 256 * (img >> LEVELS) ** 2)


def ws_bytes(net, img, n):
    """The encoder's; a joint net: + last | y_j, r_j per decoder level | prob | dlast | dskip of levels 1..4 (the sizes of
    y_3 .. y_0); with batch statistics: + extra_ws_bytes.  The decoder over a frozen encoder: the inference decoder's, then
    y_j, r_j per level | prob | g0 | g1 (the sizes of y_4 and y_3)."""
    a = dsm.align
    lvl = dsm.level_bytes(img, n)
    if net.frozen_encoder:
        return segment_ws_bytes(img, n) + 2 * sum(lvl) + a(4 * n * img * img) + lvl[4] + lvl[3]
    total = encoder_ws_bytes(img, n)
    if net.joint:
        last = a(4 * n * 256 * (img // 32) ** 2)
        total += last + 2 * sum(lvl) + a(4 * n * img * img) + last + sum(lvl[:4])
    return total + (extra_ws_bytes(img, n) if net.batch_stats else 0)


def only_written(net, img, n):
    """[(from, to)]: the bytes of the workspace that the backward writes before it reads them, so that whatever they held
    must not matter: g0 | g1 | g2 at the end of the encoder's workspace and, behind a joint net's, dlast | dskip at the end
    of the whole; over a frozen encoder g0 | g1 at the end."""
    lvl, end = dsm.level_bytes(img, n), ws_bytes(net, img, n)
    if net.frozen_encoder:
        return [(end - lvl[4] - lvl[3], end)]
    e_end = encoder_ws_bytes(img, n)
    out = [(e_end - 3 * dsm.align(4 * n * 8 * img * img), e_end)]
    if net.joint:
        out.append((end - dsm.align(4 * n * 256 * (img // 32) ** 2) - sum(lvl[:4]), end))
    return out


def relu_views(img, n, frozen_encoder=False):
    """[(byte offset, channels, side)] x 21: where the workspace keeps r = relu(u) of the 16 encoder layers in packed order
    and, in a joint workspace, of the decoder's five levels (the layout of include/occlusionenv_amd.h).  ``frozen_encoder``:
    the five levels of the decoder-only workspace, which keeps them behind the inference decoder's part."""
    a = dsm.align
    if frozen_encoder:
        out, off = [], segment_ws_bytes(img, n)
    else:
        hs = sides(img)
        off = a(4 * n * 4 * img * img)  # obs
        out = [(off, 8, img)]
        off += a(4 * n * 8 * img * img)
        for lv in range(LEVELS):
            c, act = 8 << lv, a(4 * n * (8 << lv) * hs[lv] ** 2)
            out += [(off + act, c, hs[lv]), (off + 3 * act, c, hs[lv]), (off + 5 * act, 2 * c, hs[lv + 1])]  # a r1 b r2 cc rd
            off += 5 * act + a(4 * n * 2 * c * hs[lv + 1] ** 2)
        off = encoder_ws_bytes(img, n) + a(4 * n * 256 * (img // 32) ** 2)  # past the encoder's part and last
    for j, size in enumerate(dsm.level_bytes(img, n)):
        out.append((off + size, 128 >> j, (img // 16) << j))  # y_j | r_j
        off += 2 * size
    return out


def kept_relu(net, i):
    """The kept r of layer i of the latest forward of a trainable net (any of the native training classes), a view of its
    workspace.  Call it while the net is in the mode (``train()`` / ``eval()``) of that forward: the batch-statistics step
    has a workspace of its own, and which one is viewed goes by the mode the net is in now."""
    n, img = net._latest
    ws, _scratch = net._train_buffers(n, img, net._bn_mode())
    frozen_encoder = "feats" in net.RETURNS and "feats" not in net.DIFFERENTIABLE  # it returns the feature and trains nothing behind it
    off, c, side = relu_views(img, n, frozen_encoder)[i]
    return ws[off:off + 4 * n * c * side * side].view(torch.float32).view(n, c, side, side)
