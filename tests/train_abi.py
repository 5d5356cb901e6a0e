"""The argument contract of the native training entry points (include/occlusionenv_amd.h), as data: six triples of a workspace
query, a train forward and a backward.  tests/test_train_abi_host.py makes the same family of refused calls for every row.
The rows restate the header; nothing here is read from the library."""

# ---- argument roles ----------------------------------------------------------------------------------------------------------
CFG = ("cfg", "cfg")
N_ENV = ("n_env", "n_env")
STREAM = ("stream", "stream")


def ptr(name, align=None):
    """A required pointer; ``align``: the byte alignment the library checks, None where it checks none."""
    return ("ptr", name, align)


def out(name):
    """A required out-parameter of a query."""
    return ("out", name)


def nbytes(name, answer):
    """The byte size of the buffer in front of it; its minimum is the query's ``answer`` (0: ws_bytes, 1: scratch_bytes)."""
    return ("bytes", name, answer)


WS, WS_BYTES = ptr("ws", 16), nbytes("ws_bytes", 0)
SCRATCH, SCRATCH_BYTES = ptr("scratch", 16), nbytes("scratch_bytes", 1)

QUERY = (CFG, N_ENV, out("ws_bytes"), out("scratch_bytes"))
ENC_FORWARD = (CFG, ptr("packed", 4), ptr("obs", 4), N_ENV, WS, WS_BYTES, ptr("feats", 4), STREAM)
ENC_BACKWARD = (CFG, ptr("packed", 4), N_ENV, WS, WS_BYTES, ptr("grad_feats", 4), SCRATCH, SCRATCH_BYTES,
                ptr("grad_packed", 4), STREAM)
FULL_FORWARD = (CFG, ptr("enc_packed", 4), ptr("dec_packed", 4), ptr("obs", 4), N_ENV, WS, WS_BYTES, ptr("feats", 4),
                ptr("prob", 8), STREAM)
FULL_BACKWARD = (CFG, ptr("enc_packed", 4), ptr("dec_packed", 4), N_ENV, WS, WS_BYTES, ptr("grad_feats", 4), ptr("grad_prob", 16),
                 SCRATCH, SCRATCH_BYTES, ptr("grad_enc_packed", 4), ptr("grad_dec_packed", 4), STREAM)
# with batch statistics prob is read back as float4, and bn_stats sits in front of the stream
BN_FORWARD = FULL_FORWARD[:8] + (ptr("prob", 16), ptr("bn_stats", 4), STREAM)


# ---- configs: (img, dilation, residual, separable) -------------------------------------------------------------------------
def dense(img=64, dilation=1, residual=1, separable=0):
    return (img, dilation, residual, separable)


def sep(img=64, dilation=2, residual=1, separable=1):
    return (img, dilation, residual, separable)


def triple(stem, backward, forward_args, backward_args, accepts, refuses, query_refuses=(), query_accepts=()):
    """``accepts``: configs every entry point takes at n_env = 2 (each gets the whole family of refused calls around it).
    ``refuses``: configs, or (config, n_env), that all three refuse.  ``query_refuses`` / ``query_accepts``: tried on the query
    alone, as (config, n_env)."""
    return dict(query=(stem + "_workspace_query", QUERY), forward=(stem + "_forward", forward_args),
                backward=(backward, backward_args), accepts=tuple(accepts), refuses=tuple(refuses),
                query_refuses=tuple(query_refuses), query_accepts=tuple(query_accepts))


TRIPLES = {
    # the decoder with the encoder frozen runs on either encoder form; the float pointers other than the float4 / float2
    # planes are not checked for alignment here
    "segment": triple(
        "occ_segment_train", "occ_segment_backward",
        (CFG, ptr("enc_packed"), ptr("dec_packed"), ptr("obs"), N_ENV, WS, WS_BYTES, ptr("feats"), ptr("prob", 8), STREAM),
        (CFG, ptr("dec_packed"), N_ENV, WS, WS_BYTES, ptr("grad_prob", 16), SCRATCH, SCRATCH_BYTES, ptr("grad_packed"), STREAM),
        accepts=(sep(), dense()), refuses=(sep(100),), query_accepts=((sep(32), 65535),)),
    "encoder": triple(
        "occ_encoder_train", "occ_encoder_backward", ENC_FORWARD, ENC_BACKWARD,
        accepts=(dense(residual=0), dense()),
        refuses=(dense(residual=0, separable=1), dense(dilation=2, residual=0), dense(31, residual=0), dense(1025, residual=0),
                 dense(residual=2)),
        query_accepts=((dense(32), 65535),)),
    "sep_encoder": triple(
        "occ_sep_encoder_train", "occ_sep_encoder_backward", ENC_FORWARD, ENC_BACKWARD,
        accepts=(sep(), sep(dilation=1, residual=0)),
        refuses=(sep(separable=0), sep(dilation=3), sep(residual=2), sep(31), sep(1025)),
        query_accepts=((sep(32), 65535),)),
    # the dense entry points keep refusing a separable config, and the separable ones a dense config
    "fullnet": triple(
        "occ_fullnet_train", "occ_fullnet_backward", FULL_FORWARD, FULL_BACKWARD,
        accepts=(dense(), dense(residual=0)),
        refuses=(dense(separable=1), dense(dilation=2), dense(48), dense(residual=2), sep()),
        query_refuses=((dense(0), 2), (dense(1056), 2)), query_accepts=((dense(32), 65535),)),
    "sep_fullnet": triple(
        "occ_sep_fullnet_train", "occ_sep_fullnet_backward", FULL_FORWARD, FULL_BACKWARD,
        accepts=(sep(), sep(dilation=1, residual=0)),
        refuses=(sep(separable=0), dense(), sep(dilation=3), sep(dilation=0), sep(48), sep(16), sep(residual=2)),
        query_refuses=((sep(separable=2), 2), (sep(0), 2), (sep(1056), 2), (sep(), -1)),
        query_accepts=((sep(32), 1), (sep(32), 65535))),
    # one triple for both encoder forms; every BatchNorm needs two values per channel: n_env (img / 32)^2 >= 2
    "fullnet_bn": triple(
        "occ_fullnet_bn_train", "occ_fullnet_bn_backward", BN_FORWARD, FULL_BACKWARD,
        accepts=(dense(), sep()),
        refuses=(dense(48), dense(16), dense(residual=2), dense(dilation=3), dense(dilation=2), dense(separable=2),
                 sep(48), sep(16), sep(residual=2), sep(dilation=3), (dense(32), 1), (sep(32), 1)),
        query_refuses=((dense(16), 8), (sep(16), 8)),
        query_accepts=((dense(32), 2), (sep(32), 2), (dense(), 1), (sep(), 1), (dense(32), 65535), (sep(32), 65535))),
}
ROLES = ("query", "forward", "backward")
ENTRY_POINTS = [(name, role) for name in TRIPLES for role in ROLES]
