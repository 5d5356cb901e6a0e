"""Host-side checks of the generic pack / unpack pair of occlusionenv_amd/nettrain.py, which the encoder's and the decoder's
packed layouts are thin calls to: for both weight permutations it round-trips, and on the state dicts of
tests/test_encoder_train_host.py and tests/test_decoder_train_host.py it gives the buffers of ``encoder.pack_state_dict`` and
``encoder.pack_decoder``.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import train_model as tm
from tests.segmenter_model import golden_seg_state_dict


def _plans():
    from occlusionenv_amd.encoder import decoder_plan, layer_plan
    from occlusionenv_amd.nettrain import DECODER_PERM, ENCODER_PERM

    enc = [(cin, cout) for _stem, cin, cout, _sep, _stride in layer_plan(False)]
    dec = [(cin, cout) for _j, cin, cout in decoder_plan()]
    # perm, plan, the shape of a layer's weight as the checkpoint holds it, floats after the layers
    return {"encoder": (ENCODER_PERM, enc, lambda cin, cout: (cout, cin, 3, 3), 0),
            "decoder": (DECODER_PERM, dec, lambda cin, cout: (cin, cout, 3, 3), 9)}


def _folded(sd, stems):
    from occlusionenv_amd.nettrain import fold_bn_vectors

    layers = []
    for st in stems:
        scale, shift, _ = fold_bn_vectors(sd[st + "bn.weight"], sd[st + "bn.bias"], sd[st + "bn.running_mean"], sd[st + "bn.running_var"])
        layers.append((sd[st + "conv.weight"], sd[st + "conv.bias"], scale, shift))
    return layers


@pytest.mark.parametrize("which", ["encoder", "decoder"])
def test_generic_pair_round_trips(which):
    from occlusionenv_amd.nettrain import pack_layers, unpack_layers

    perm, plan, wshape, ntail = _plans()[which]
    floats = sum(9 * cin * cout + 3 * cout for cin, cout in plan) + ntail
    buf = torch.randn(floats, generator=torch.Generator().manual_seed(5))
    layers, off = unpack_layers(buf, plan, perm)
    assert off == floats - ntail
    assert [tuple(l[0].shape) for l in layers] == [wshape(cin, cout) for cin, cout in plan]
    assert all(tuple(x.shape) == (cout,) for l, (_cin, cout) in zip(layers, plan) for x in l[1:])
    tail = (buf[off:off + ntail - 1], buf[off + ntail - 1:]) if ntail else ()
    assert torch.equal(pack_layers(layers, perm, tail), buf)
    # the layout: w[ci][ky * 3 + kx][co] whichever way the checkpoint holds the weight
    cin, cout = plan[1]
    lo = 9 * plan[0][0] * plan[0][1] + 3 * plan[0][1]
    ci, co, ky, kx = cin - 1, cout - 3, 2, 1
    idx = (co, ci, ky, kx) if which == "encoder" else (ci, co, ky, kx)
    assert float(layers[1][0][idx]) == float(buf[lo + (ci * 9 + ky * 3 + kx) * cout + co])
    # and from tensors to buffer and back: the views are the tensors
    g = torch.Generator().manual_seed(6)
    made = [(torch.randn(*wshape(cin, cout), generator=g), *(torch.randn(cout, generator=g) for _ in range(3))) for cin, cout in plan]
    back, _off = unpack_layers(pack_layers(made, perm), plan, perm)
    assert all(torch.equal(x, y) for b, f in zip(back, made) for x, y in zip(b, f))


def test_generic_pack_equals_pack_state_dict():
    from occlusionenv_amd.encoder import pack_state_dict
    from occlusionenv_amd.enctrain import pack_encoder_buffer
    from occlusionenv_amd.nettrain import ENCODER_PERM, encoder_part, pack_layers

    for preset in ("predictor", "ppo"):
        sd = {k: v.float() for k, v in tm.dense_state_dict(preset, 11).items()}
        separable, want, _offsets = pack_state_dict(sd, tm.preset_keys(preset)["prefix"])
        assert not separable
        layers = _folded(sd, encoder_part(preset).stems)
        got = pack_layers(layers, ENCODER_PERM)
        assert np.array_equal(got.numpy(), want)
        assert torch.equal(pack_encoder_buffer(layers), got)


def test_generic_pack_equals_pack_decoder():
    from occlusionenv_amd.encoder import DECODER_KEYS, pack_decoder
    from occlusionenv_amd.nettrain import DECODER_PERM, decoder_part, pack_layers
    from occlusionenv_amd.seghead import pack_decoder_buffer

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segmenter_golden.npz"))
    for preset in ("ppo", "segmenter"):
        sd = {k: v.float() for k, v in golden_seg_state_dict(g, preset).items()}
        part = decoder_part(preset)
        levels = _folded(sd, part.stems)
        tail = [sd[k] for k in part.tail]
        got = pack_layers(levels, DECODER_PERM, tail)
        assert np.array_equal(got.numpy(), pack_decoder(sd, *DECODER_KEYS[preset]))
        assert torch.equal(pack_decoder_buffer(levels, *tail), got)


def test_wrong_sized_buffers_raise():
    from occlusionenv_amd.encoder import decoder_packed_floats, packed_floats
    from occlusionenv_amd.enctrain import unpack_encoder_buffer
    from occlusionenv_amd.seghead import unpack_decoder_buffer

    with pytest.raises(ValueError, match="packed dense encoder buffer"):
        unpack_encoder_buffer(torch.zeros(packed_floats(False) + 1))
    with pytest.raises(ValueError, match="packed decoder buffer"):
        unpack_decoder_buffer(torch.zeros(decoder_packed_floats() - 1))
