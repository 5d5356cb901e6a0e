"""Generates tests/golden/packed_digests.json: a SHA-256 of every packed weight buffer and key list the package derives
from the checkpoints of the tests.  It was run on the commit before the packed layout got its one module
(occlusionenv_amd/netlayout.py) and calls only functions that exist on both sides of that change, so
tests/test_packed_layout_host.py, which recomputes the digests, holds the layout to the bytes it had.  No GPU.

    python tests/golden/make_packed_digests.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "packed_digests.json")
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def _sha(data) -> str:
    return hashlib.sha256(data).hexdigest()


def _keys(tensors) -> str:
    return _sha("\n".join(tensors).encode())


def _f32(sd):
    return {k: v.float() for k, v in sd.items()}


def _part_pack(sd, part) -> str:
    """``part.pack`` of the layers of ``sd`` folded as the training step folds them."""
    from occlusionenv_amd.nettrain import fold_bn_vectors

    layers = []
    for stem, leaves in zip(part.stems, part.layer_leaves()):
        scale, shift, _rstd = fold_bn_vectors(*(sd[stem + k] for k in leaves[-2:] + ("bn.running_mean", "bn.running_var")))
        layers.append(tuple(sd[stem + leaf] for leaf in leaves[:-2]) + (scale, shift))
    buf = part.pack(layers, [sd[k] for k in part.tail])
    assert buf.numel() == part.floats
    return _sha(buf.contiguous().numpy().tobytes())


def compute() -> dict:
    from occlusionenv_amd.encoder import DECODER_KEYS, PRESETS, decoder_tensors, encoder_tensors, pack_decoder, pack_state_dict
    from occlusionenv_amd.nettrain import decoder_part, encoder_part, sep_encoder_part
    from tests import train_model as tm
    from tests.encoder_model import golden_state_dict
    from tests.segmenter_model import golden_seg_state_dict

    enc_golden = np.load(os.path.join(HERE, "encoder_golden.npz"))
    seg_golden = np.load(os.path.join(HERE, "segmenter_golden.npz"))
    # name -> (state dict, preset); "/f32": the same rounded to f32 first
    encoders = {f"encoder_golden/{p}": (golden_state_dict(enc_golden, p), p) for p in ("ppo", "predictor")}
    encoders.update({f"segmenter_golden/{p}": (golden_seg_state_dict(seg_golden, p), p) for p in ("ppo", "segmenter")})
    for p in ("ppo", "predictor"):
        for name, sd in ((f"dense11/{p}", tm.dense_state_dict(p, 11)), (f"sep32/{p}", tm.sep_state_dict(p, 32))):
            encoders[name] = (sd, p)
            encoders[name + "/f32"] = (_f32(sd), p)
    out = {}
    for name, (sd, preset) in encoders.items():
        prefix, ghead = PRESETS[preset][0], PRESETS[preset][1]
        separable, packed, offsets = pack_state_dict(sd, prefix)
        assert packed.dtype == np.float32
        out[f"pack_state_dict/{name}"] = _sha(packed.tobytes())
        out[f"layer_offsets/{name}"] = _sha(json.dumps([int(o) for o in offsets]).encode())
        out[f"encoder_tensors/{name}"] = _keys(encoder_tensors(sd, prefix, separable, ghead))
        if name.endswith("/f32"):
            part = (sep_encoder_part if separable else encoder_part)(preset)
            out[f"part_pack/{name}"] = _part_pack(sd, part)
    for preset in ("ppo", "segmenter"):
        sd = golden_seg_state_dict(seg_golden, preset)
        packed = pack_decoder(sd, *DECODER_KEYS[preset])
        assert packed.dtype == np.float32
        out[f"pack_decoder/segmenter_golden/{preset}"] = _sha(packed.tobytes())
        out[f"decoder_tensors/segmenter_golden/{preset}"] = _keys(decoder_tensors(sd, *DECODER_KEYS[preset]))
        out[f"part_pack/segmenter_golden/{preset}/decoder/f32"] = _part_pack(_f32(sd), decoder_part(preset))
        # the encoder under the decoder, rounded to f32, through its part as well
        separable = preset == "ppo"
        out[f"part_pack/segmenter_golden/{preset}/encoder/f32"] = _part_pack(_f32(sd), (sep_encoder_part if separable else encoder_part)(preset))
    return out


if __name__ == "__main__":
    digests = compute()
    with open(PATH, "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print(PATH, len(digests), "digests")
