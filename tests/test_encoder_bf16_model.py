"""CPU tests of the bf16 encoder mode's host side: the host model (tests/encoder_bf16_model.py) against torch.bfloat16 and
against ``encode``; ``occ_encoder_bf16_pack`` (host only) against the model's rounding and the layout the header documents;
the documented sizes; the rejections of a dense configuration.  No device call is made here."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.encoder_bf16_model import encode_bf16, round_bf16
from tests.encoder_model import encode, golden_state_dict, make_obs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_golden.npz")
CH, LEVELS = 8, 5


@pytest.fixture(scope="module")
def sd():
    return golden_state_dict(np.load(GOLDEN), "ppo")


# ---- the model ------------------------------------------------------------------------------------------------------------
def _tie_values():
    """f32 values halfway between two bf16 neighbours (low 16 bits 0x8000) with an even and an odd upper half, both signs,
    several exponents; plus values one f32 ulp either side of a tie."""
    out = []
    for hi in (0x3F80, 0x3F81, 0x3FFF, 0x4000, 0x4049, 0x3E00, 0x3DCD, 0x4780, 0x0100 + 0x3000):
        for sign in (0, 0x8000):
            for lo in (0x8000, 0x7FFF, 0x8001, 0x0000, 0x0001, 0xFFFF):
                out.append(((hi | sign) << 16) | lo)
    return torch.from_numpy(np.array(out, dtype=np.uint32).view(np.float32).copy())


def test_model_rounding_is_torch_bfloat16():
    g = torch.Generator().manual_seed(5)
    x = torch.cat([_tie_values(), torch.randn(4096, generator=g), torch.randn(512, generator=g) * 1e-3,
                   torch.randn(512, generator=g) * 1e3, torch.zeros(1)])
    want = x.to(torch.bfloat16).to(torch.float32)
    got = round_bf16(x, "rne")
    assert got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # the same from f64 directly: an f64 just above an f32-representable tie must round up, which a detour through f32 loses
    tie = 1.0 + 2.0 ** -8
    above = torch.tensor([tie + 2.0 ** -40, -(tie + 2.0 ** -40), tie, -tie], dtype=torch.float64)
    assert round_bf16(above, "rne").tolist() == [1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7), 1.0, -1.0]
    # truncation is the bit mask, and the tests can tell it from RNE
    trunc = round_bf16(x, "trunc")
    assert torch.equal(trunc.view(torch.int32), x.view(torch.int32) & -65536)
    assert not torch.equal(trunc, got)


def test_model_without_rounding_is_encode(sd):
    obs = make_obs(3, 2, 32).float().double()
    for dilation, residual in ((2, True), (1, False)):
        want = encode(sd, obs, "encoder.", True, dilation, residual)
        got = encode_bf16(sd, obs, "encoder.", dilation, residual, rounding=None)
        assert torch.equal(got, want)
    # and with it, it is not
    assert not torch.equal(encode_bf16(sd, obs), encode(sd, obs))
    assert not torch.equal(encode_bf16(sd, obs), encode_bf16(sd, obs, rounding="trunc"))


# ---- occ_encoder_bf16_pack ---------------------------------------------------------------------------------------------------
def _cfg(separable=1, img=64, dilation=2, residual=1):
    from occlusionenv_amd import _native as nat

    cfg = nat.OccEncoderConfig()
    cfg.img, cfg.dilation, cfg.residual, cfg.separable = img, dilation, residual, separable
    return cfg


def _plan():
    plan = [(4, CH, True)]
    for lv in range(LEVELS):
        c = CH << lv
        plan += [(c, c, True), (c, c, True), (c, 2 * c, False)]
    return plan


def _layer_floats(cin, cout, sep):
    return 6 * cin + cin * cout + 3 * cout if sep else 9 * cin * cout + 3 * cout


def _layer_bytes(cin, cout, sep):
    """The header's layout: cin <= 8 as f32; else (dw f32) | fragments bf16 | bias, scale, shift f32."""
    if cin <= 8:
        return 4 * _layer_floats(cin, cout, sep)
    return (24 * cin if sep else 0) + 2 * (cin if sep else 9 * cin) * max(cout, 32) + 12 * cout


def _bf16_bits(w_f32: np.ndarray) -> np.ndarray:
    """The model's RNE rounding of f32 weights, as bf16 bit patterns."""
    r = round_bf16(torch.from_numpy(w_f32.astype(np.float64)), "rne").to(torch.float32).numpy()
    bits = r.view(np.uint32)
    assert not (bits & 0xFFFF).any()
    return (bits >> 16).astype(np.uint16)


def _pack(packed_f32: np.ndarray) -> np.ndarray:
    from occlusionenv_amd import _native as nat

    lib, cfg = nat.load(), _cfg()
    nbytes = lib.occ_encoder_bf16_packed_bytes(C.byref(cfg))
    assert nbytes == sum(_layer_bytes(*l) for l in _plan())
    out = np.full(nbytes + 64, 0xAB, dtype=np.uint8)
    src = np.ascontiguousarray(packed_f32, dtype=np.float32)
    assert lib.occ_encoder_bf16_pack(C.byref(cfg), src.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
    assert (out[nbytes:] == 0xAB).all()  # nothing written past the documented size
    return out[:nbytes]


def _check_pack(packed_f32: np.ndarray):
    out = _pack(packed_f32)
    src_off = dst_off = 0
    for cin, cout, sep in _plan():
        src = packed_f32[src_off:src_off + _layer_floats(cin, cout, sep)]
        dst = out[dst_off:dst_off + _layer_bytes(cin, cout, sep)]
        nw = cin * cout if sep else 9 * cin * cout
        w0 = 6 * cin if sep else 0
        w, tail = src[w0:w0 + nw], src[w0 + nw:]
        want_bits = _bf16_bits(w)
        if cin <= 8:
            d32 = dst.view(np.uint32)
            assert np.array_equal(d32[:w0], src[:w0].view(np.uint32))
            assert np.array_equal(d32[w0:w0 + nw], want_bits.astype(np.uint32) << 16)
            assert np.array_equal(d32[w0 + nw:], tail.view(np.uint32))
        else:
            o = 0
            if sep:  # dw[c / 8][v0 v1 v2 h0 h1 h2][8]
                dw = dst[:24 * cin].view(np.uint32).reshape(cin // 8, 6, 8)
                taps = src[:6 * cin].view(np.uint32).reshape(2, cin // 8, 8, 3)  # [v | h][group][channel][tap]
                want = taps.transpose(1, 0, 3, 2).reshape(cin // 8, 6, 8)
                assert np.array_equal(dw, want)
                o = 24 * cin
            K, CP = (cin if sep else 9 * cin), max(cout, 32)
            frag = dst[o:o + 2 * K * CP].view(np.uint16).reshape(K // 16, CP // 32, 64, 8)
            kb, ct, lane, j = np.meshgrid(np.arange(K // 16), np.arange(CP // 32), np.arange(64), np.arange(8), indexing="ij")
            k = 16 * kb + 8 * (lane >> 5) + j
            m = lane & 31
            co = 32 * ct + 16 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3)
            if sep:
                table = want_bits.reshape(cin, cout)  # pw[k][co]
                idx = (k, np.minimum(co, cout - 1))
            else:
                table = want_bits.reshape(cin, 9, cout)  # w[ci][tap][co], k = tap * cin + ci
                idx = (k % cin, k // cin, np.minimum(co, cout - 1))
            want = np.where(co < cout, table[idx], 0).astype(np.uint16)
            assert np.array_equal(frag, want), (cin, cout, sep)
            assert np.array_equal(dst[o + 2 * K * CP:].view(np.uint32), tail.view(np.uint32))
        src_off += src.size
        dst_off += dst.size
    assert src_off == packed_f32.size and dst_off == out.size


def test_pack_rounds_the_golden_weights_as_the_model(sd):
    from occlusionenv_amd.encoder import pack_state_dict

    separable, packed, _ = pack_state_dict(sd, "encoder.")
    assert separable
    _check_pack(packed)


def test_pack_rounds_ties_to_even():
    from occlusionenv_amd.encoder import packed_floats

    rng = np.random.default_rng(9)
    n = packed_floats(True)
    hi = rng.integers(0x3C00, 0x4100, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 15)
    lo = rng.choice(np.array([0x8000, 0x7FFF, 0x8001, 0x0000, 0xFFFF], dtype=np.uint32), n)
    _check_pack(((hi << 16) | lo).view(np.float32))


def test_documented_sizes():
    from occlusionenv_amd import _native as nat

    lib = nat.load()

    def align(b):
        return (b + 255) & ~255

    for img, n, side5 in ((32, 1, 1), (100, 3, 4), (256, 256, 8), (512, 64, 16), (1024, 2, 32)):
        nbytes, f32bytes = C.c_size_t(), C.c_size_t()
        assert lib.occ_encoder_bf16_workspace_query(C.byref(_cfg(img=img)), n, C.byref(nbytes)) == 0
        tiles = ((side5 + 7) // 8) ** 2
        assert nbytes.value == 3 * align(n * 8 * img * img * 2) + align(n * tiles * 256 * 4)
        assert lib.occ_encoder_workspace_query(C.byref(_cfg(img=img)), n, C.byref(f32bytes)) == 0
        assert nbytes.value < 0.51 * f32bytes.value + 64 * 1024  # about half of the f32 workspace
    assert lib.occ_encoder_bf16_workspace_query(C.byref(_cfg(img=16)), 1, C.byref(nbytes)) == 1
    assert lib.occ_encoder_bf16_workspace_query(C.byref(_cfg()), 0, C.byref(nbytes)) == 1


def test_dense_configuration_is_rejected():
    from occlusionenv_amd import _native as nat

    lib, dense = nat.load(), _cfg(separable=0)
    nbytes, p = C.c_size_t(), C.c_void_p(4096)
    assert lib.occ_encoder_bf16_packed_bytes(C.byref(dense)) == -1
    assert lib.occ_encoder_bf16_workspace_query(C.byref(dense), 4, C.byref(nbytes)) == 1
    buf = np.zeros(16, dtype=np.float32)
    assert lib.occ_encoder_bf16_pack(C.byref(dense), buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)) == 1
    # before any launch: no device is touched (this host has none)
    assert lib.occ_encoder_forward_bf16(C.byref(dense), p, p, 4, p, 1 << 40, p, None, None) == 1
    assert lib.occ_encoder_forward_bf16(C.byref(_cfg()), None, p, 4, p, 1 << 40, p, None, None) == 1
    assert lib.occ_encoder_forward_bf16(C.byref(_cfg()), p, p, 4, p, 16, p, None, None) == 1  # workspace too small
