"""Host model of how the decoder backward splits its work (csrc/occ_decoder_bwd.hpp, include/occlusionenv_amd.h), restated
in plain Python from the comments there; nothing native is imported.

Decoder level j = 0..4 has cout = 128 >> j output and cin = 2 cout input channels; its input is H x H with
H = (S / 32) << j and its output 2H x 2H.

Weight gradient (occ_dec_bwd_dw_kernel): a block owns a cib x cob tile of (ci, co) and one slice of K = N H^2.  K is cut
into T x T pixel tiles, tiles_x^2 per env, numbered with the envs in order; a slice is ``tps`` consecutive tiles, where
tps = ceil(total_tiles / (512 / grid_y)) and grid_y is the number of (ci, co) tiles.  Every block writes ``pb`` partial
dW (one per wave, or per pixel lane when the (ci, co) tile fills more than a wave) of cin x 9 x cout f32.

Activation step (occ_dec_bwd_act_kernel): per (chunk of 4096 pixels, channel, env) up to five f64 partial sums.

Scratch: one buffer serves both, so its size is the maximum over the levels of the two.
"""
from __future__ import annotations

CH = 8           # channels of the last decoder level
LEVELS = 5
DW_BLOCKS = 512  # blocks of the weight gradient per level: K slices x (ci, co) tiles
ACT_CHUNK = 4096  # pixels of one (env, channel) plane per block of the activation step
ACT_SUMS = 5     # f64 sums per block of the activation step (the last level's count, reserved for every level)


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def align(b: int) -> int:
    """Every part of the workspace is 256-byte aligned."""
    return (b + 255) & ~255


def level_channels(j: int) -> int:
    return CH << (LEVELS - 1 - j)


def level_side(img: int, j: int) -> int:
    """H, the side of level j's input; its output is 2H."""
    return (img >> LEVELS) << j


def dw_plan(j: int, H: int, n: int) -> dict:
    """The (ci, co) tile, pixel tile and K split of the weight gradient of level j."""
    cout = level_channels(j)
    cin = 2 * cout
    if cout >= 64:
        T, cib, cob = 4, 64, 64
    elif cout == 32:
        T, cib, cob = 4, 64, 32
    elif cout == 16:
        T, cib, cob = 8, 32, 16
    else:
        T, cib, cob = 8, 16, 8
    q = (cib // 16) * cob  # threads of one (ci, co) tile: 16 ci per thread
    pb = 256 // max(q, 64)
    grid_y = (cin // cib) * (cout // cob)
    tiles_x = ceil_div(H, T)
    tiles_env = tiles_x * tiles_x
    total_tiles = n * tiles_env
    tps = ceil_div(total_tiles, DW_BLOCKS // grid_y)
    slices = ceil_div(total_tiles, tps)
    return dict(T=T, cib=cib, cob=cob, pb=pb, grid_y=grid_y, tiles_x=tiles_x, tiles_env=tiles_env, total_tiles=total_tiles,
                tps=tps, slices=slices, part_bytes=slices * pb * cin * 9 * cout * 4,
                short_last=total_tiles % tps != 0,              # the last slice has fewer than tps tiles
                straddles=tiles_env > 1 and tiles_env % tps != 0)  # some slice starts in one env and ends in the next


def dw_plans(img: int, n: int) -> list:
    return [dw_plan(j, level_side(img, j), n) for j in range(LEVELS)]


def act_chunks(plane: int) -> int:
    return ceil_div(plane, ACT_CHUNK)


def act_bytes(j: int, H: int, n: int) -> int:
    return level_channels(j) * n * act_chunks(4 * H * H) * ACT_SUMS * 8


def scratch_bytes(img: int, n: int) -> int:
    return max(max(act_bytes(j, level_side(img, j), n), dw_plan(j, level_side(img, j), n)["part_bytes"]) for j in range(LEVELS))


def level_bytes(img: int, n: int) -> list:
    """Bytes of y_j (and of r_j) per level in the training workspace; the two gradient buffers g0 and g1 at its end have
    the sizes of levels 4 and 3."""
    return [align(n * level_channels(j) * (2 * level_side(img, j)) ** 2 * 4) for j in range(LEVELS)]


# The GPU cases of tests/test_gpu_decoder_train.py whose weight gradient runs several tiles per block.
SPLIT_CASES = [("ppo", 96, 65), ("segmenter", 64, 130)]
