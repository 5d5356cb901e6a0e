// occ_fullnet_bwd.hpp -- joint training of the encoder (dense at dilation 1, or separable at dilation 1 or 2: the network
// the agent runs is FullNetwork(8, dilation=2, separable=True)), the segmentation decoder and the classifier (one step of
// pretrainer.py below its losses): a forward that keeps what the backward needs, and the backward with respect to every
// encoder and decoder parameter for two upstream gradients at once, d loss / d feats and d loss / d prob.  Part of the single
// translation unit occ_kernels.hip (included inside namespace occ, after occ_decoder_bwd.hpp, occ_encoder_bwd.hpp and
// occ_sepenc_bwd.hpp, whose kernels it launches; it has no kernel and no launcher of its own: both passes go through
// dec_backward and enc_backward, and one host path serves both encoder forms).
//
// Forward: enc_train_forward with the last down also storing its output (18 launches), then dec_train_forward on that
// output and on the encoder's level tensors cc[lv] as the skips, which are not copied (5 launches): 23 launches.  The FMA
// order and the grids are those of the two training forwards, so feats and prob are the same to the bit.
//
// Backward: the decoder first, from the full-resolution level down (dec_backward with a DecJoin, 25 launches), then the
// encoder from the deepest level up (enc_backward with an EncJoin, 79 launches dense, 112 separable): 104 or 137 launches.
// The decoder does not depend on the encoder's form and the downs of both forms are the dense stride-2 layers, so the two
// passes meet in the same places:
//   * every decoder level's dY is the d skip of encoder level lv = 4 - j.  For lv >= 1 the decoder's activation step is out of
//     place (dU goes to one buffer of the size of y_4, dY stays where the level above's input gradient wrote it), and
//     occ_enc_bwd_dx2_kernel<T, 1> adds it to the stride-2 input gradient in its epilogue.  For lv = 0 dY is never stored:
//     occ_enc_bwd_dx2_kernel<16, 2> rebuilds gp p (1 - p) cls_w[ci] from grad_prob and the kept prob, as
//     occ_dec_bwd_act_kernel<true> formed it.  Kept: 0.94 buffers of (n,8,S,S) instead of 1.94.
//   * the deepest decoder level's input gradient d(last down output) is computed (occ_dec_bwd_dx_kernel on a 256-channel
//     input; a 1 x 1 plane at S = 32) and occ_enc_bwd_act_kernel<true> adds it to grad_feats / (H H).
// No join is a launch of its own.  The decoder's dU buffer is the encoder's first gradient buffer g[0], which is free when
// the encoder pass starts: enc_backward's first access to any of its three gradient buffers is the last down's activation
// step writing gA = g[0], after the decoder's last launch on the same stream, and neither form reads a buffer of the
// rotation before the pass itself has written it.
//
// Workspace (occ_fullnet_train_workspace_query, occ_sep_fullnet_train_workspace_query: the same for both forms), every part
// 256-byte aligned, f32:
//   the workspace of occ_encoder_train_forward (obs .. pool partials | g0 | g1 | g2) |
//   last (n,256,S/32,S/32) | per decoder level j = 0..4: y_j | r_j (n, 128 >> j, S/16 << j, S/16 << j) | p (n,S,S) |
//   dlast (n,256,S/32,S/32) | dskip[lv], lv = 1..4 (n, 8 << lv, S >> lv, S >> lv)
// g0 holds the decoder's dU.  Scratch: the larger of the two backward passes' scratch (the encoder's depends on its form).
//
// Both passes take an optional BnTrain (occ_bn_train.hpp): BatchNorm on the batch's statistics instead of the folded running
// ones, on a workspace with three more parts; null leaves every launch as it is.

struct FullTrainWs {
    EncTrainWs enc;
    TrainWs dec;  // lvl_bytes, p_bytes and scratch are used; its offsets are not
    size_t last, y[kEncLevels], r[kEncLevels], p, dlast, dskip[kEncLevels], total, scratch;
};

inline FullTrainWs full_train_ws_layout(int img, int n, bool separable) {
    FullTrainWs l;
    l.enc = enc_train_ws_layout(img, n, separable);
    l.dec = train_ws_layout(img, n);
    size_t at = l.enc.total;
    auto take = [&](size_t bytes) {
        const size_t o = at;
        at += enc_align(bytes);
        return o;
    };
    l.last = take(l.dec.seg.last_bytes);
    for (int j = 0; j < kEncLevels; ++j) {
        l.y[j] = take(l.dec.lvl_bytes[j]);
        l.r[j] = take(l.dec.lvl_bytes[j]);
    }
    l.p = take(l.dec.p_bytes);
    l.dlast = take(l.dec.seg.last_bytes);
    l.dskip[0] = 0;  // rebuilt where it is read
    for (int lv = 1; lv < kEncLevels; ++lv) l.dskip[lv] = take(l.dec.lvl_bytes[kEncLevels - 1 - lv]);
    l.total = at;
    l.scratch = l.enc.scratch > l.dec.scratch ? l.enc.scratch : l.dec.scratch;
    return l;
}

inline TrainPtrs full_train_ptrs(const FullTrainWs& l, char* ws) {
    TrainPtrs t;
    t.last = (float*)(ws + l.last);
    for (int lv = 0; lv < kEncLevels; ++lv) t.skip[lv] = (float*)(ws + l.enc.cc[lv]);
    for (int j = 0; j < kEncLevels; ++j) {
        t.y[j] = (float*)(ws + l.y[j]);
        t.r[j] = (float*)(ws + l.r[j]);
    }
    t.p = (float*)(ws + l.p);
    t.g[0] = t.g[1] = nullptr;  // the joint backward keeps its gradients in DecJoin
    return t;
}

// 23 launches.  bn: batch-statistics BatchNorm (occ_bn_train.hpp), which both passes take.
static void full_train_forward(int img, int dil, bool residual, bool separable, const float* enc_packed, const float* dec_packed,
                               const float* obs, int n, char* ws, float* feats, float* prob, hipStream_t st,
                               const BnTrain* bn = nullptr) {
    const FullTrainWs l = full_train_ws_layout(img, n, separable);
    const TrainPtrs t = full_train_ptrs(l, ws);
    enc_train_forward(img, dil, residual, separable, enc_packed, obs, n, ws, feats, st, t.last, bn);
    dec_train_forward(img, dec_packed, n, t, prob, st, bn);
}

// The backward of the latest full_train_forward of the same form on this workspace: 104 launches (dense), 137
// (separable).  Both gradient buffers are overwritten.
static void full_backward(int img, int dil, bool residual, bool separable, const float* enc_packed, const float* dec_packed, int n,
                          char* ws, const float* grad_feats, const float* grad_prob, char* scratch, float* grad_enc,
                          float* grad_dec, hipStream_t st, const BnTrain* bn = nullptr) {
    const FullTrainWs l = full_train_ws_layout(img, n, separable);
    const TrainPtrs t = full_train_ptrs(l, ws);
    DecJoin dj;
    dj.dlast = (float*)(ws + l.dlast);
    dj.dskip[0] = nullptr;
    for (int lv = 1; lv < kEncLevels; ++lv) dj.dskip[lv] = (float*)(ws + l.dskip[lv]);
    dj.du = (float*)(ws + l.enc.g[0]);
    dec_backward(img, dec_packed, n, t, grad_prob, scratch, grad_dec, st, &dj, bn);

    EncJoin ej;
    ej.dlast = dj.dlast;
    ej.skip[0] = {nullptr, grad_prob, t.p, dec_packed + dec_packed_floats() - (kEncCh + 1)};
    for (int lv = 1; lv < kEncLevels; ++lv) ej.skip[lv] = {dj.dskip[lv], nullptr, nullptr, nullptr};
    enc_backward(img, dil, residual, separable, enc_packed, n, ws, grad_feats, scratch, grad_enc, st, &ej, bn);
}
