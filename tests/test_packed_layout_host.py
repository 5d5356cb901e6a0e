"""The packed weight layout, held to the bytes it had before it got its one module (occlusionenv_amd/netlayout.py):
tests/golden/packed_digests.json was written by tests/golden/make_packed_digests.py on the commit before that change, when
the checkpoint loader (``encoder.pack_state_dict`` / ``pack_decoder``) and the training wrappers' ``Part.pack`` were two
independent descriptions of the layout; here the digests are recomputed from today's code.  The tests that compare the two
paths with each other (tests/test_nettrain_host.py and the ``*_train_host.py`` files) now compare one piece of code with
itself; this one is what keeps either from moving.  No GPU."""
import json

from tests.golden import make_packed_digests as mpd


def test_packed_bytes_and_key_lists_are_the_recorded_ones():
    with open(mpd.PATH) as f:
        want = json.load(f)
    got = mpd.compute()
    assert sorted(got) == sorted(want)
    assert len(want) == 48 and {k.split("/")[0] for k in want} == {
        "pack_state_dict", "layer_offsets", "encoder_tensors", "pack_decoder", "decoder_tensors", "part_pack"}
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, differ


def test_layout_module_stands_alone():
    """netlayout is the bottom of the package: it imports nothing of it, and the names that moved stay where they were."""
    import ast
    import inspect

    from occlusionenv_amd import encoder, enctrain, netlayout, nettrain, seghead, septrain

    tree = ast.parse(inspect.getsource(netlayout))
    imported = {a.name.split(".")[0] for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    imported |= {n.module.split(".")[0] if n.level == 0 else "." for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert imported <= {"__future__", "re", "typing", "numpy", "torch"}, imported
    for module, names in ((encoder, "layer_plan packed_floats decoder_plan decoder_packed_floats pack_state_dict pack_decoder "
                                    "DECODER_KEYS PRESETS LEVELS FEATURES CH BN_EPS encoder_tensors decoder_tensors"),
                          (nettrain, "fold_bn_vectors bn_param_grads bn_layer_shapes pack_layers unpack_layers ENCODER_PERM "
                                     "DECODER_PERM LEAVES SEP_LEAVES Part encoder_part sep_encoder_part decoder_part "
                                     "pack_encoder_buffer unpack_encoder_buffer pack_decoder_buffer unpack_decoder_buffer"),
                          (enctrain, "pack_encoder_buffer unpack_encoder_buffer"),
                          (septrain, "pack_sep_encoder_buffer unpack_sep_encoder_buffer"),
                          (seghead, "fold_bn_vectors bn_param_grads pack_decoder_buffer unpack_decoder_buffer")):
        for name in names.split():
            assert getattr(module, name) is getattr(netlayout, name), (module.__name__, name)
