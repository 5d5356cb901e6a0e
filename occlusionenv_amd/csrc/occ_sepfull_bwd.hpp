// occ_sepfull_bwd.hpp -- joint training of the separable encoder (dilation 1 or 2, with or without the residual), the
// segmentation decoder and the classifier: the separable counterpart of occ_fullnet_bwd.hpp and the step that pretrains
// the network the agent runs, FullNetwork(8, dilation=2, separable=True).  Part of the single translation unit
// occ_kernels.hip (included inside namespace occ, after occ_sepenc_bwd.hpp and occ_fullnet_bwd.hpp; it has no kernel and no
// launcher of its own: both passes go through dec_backward and sep_backward).
//
// Forward: the separable enc_train_forward with the last down also storing its output (18 launches), then dec_train_forward on that
// output and on the encoder's level tensors cc[lv] as the skips, which are not copied (5 launches): 23 launches.  The FMA
// order and the grids are those of the two training forwards, so feats and prob are the same to the bit.
//
// Backward: the decoder first (dec_backward with a DecJoin, 25 launches), then the separable encoder from the deepest
// level up (sep_backward with an EncJoin, 112 launches): 137 launches.  The decoder does not depend on the encoder's form
// and the separable encoder's downs are the dense stride-2 layers, so the joins are those of occ_fullnet_bwd.hpp: dlast
// is the dY of the last down's activation step (occ_enc_bwd_act_kernel<true>), dskip[lv] is added in the epilogue of
// the level's stride-2 input gradient (occ_enc_bwd_dx2_kernel<T, 1>; <16, 2> rebuilds it from grad_prob at level 0).
// The decoder's dU buffer is g[0]: sep_backward's first access to any of its three gradient buffers is the last down's
// activation step writing gA = g[0], after the decoder's last launch on the same stream, and no buffer of the rotation
// is read before the pass itself has written it.
//
// Workspace: FullTrainWs as it is (the separable training workspace is the dense one).  Scratch: the larger of the
// separable backward's and the decoder's.

inline FullTrainWs sep_full_train_ws_layout(int img, int n) {
    FullTrainWs l = full_train_ws_layout(img, n);
    const size_t sep = sep_train_ws_layout(img, n).scratch;
    l.scratch = sep > l.dec.scratch ? sep : l.dec.scratch;
    return l;
}

// 23 launches.
static void sep_full_train_forward(int img, int dil, bool residual, const float* enc_packed, const float* dec_packed,
                                   const float* obs, int n, char* ws, float* feats, float* prob, hipStream_t st) {
    const FullTrainWs l = full_train_ws_layout(img, n);
    const TrainPtrs t = full_train_ptrs(l, ws);
    enc_train_forward(img, dil, residual, true, enc_packed, obs, n, ws, feats, st, t.last);
    dec_train_forward(img, dec_packed, n, t, prob, st);
}

// The backward of the latest sep_full_train_forward on this workspace: 137 launches.  Both gradient buffers are
// overwritten.
static void sep_full_backward(int img, int dil, bool residual, const float* enc_packed, const float* dec_packed, int n, char* ws,
                              const float* grad_feats, const float* grad_prob, char* scratch, float* grad_enc, float* grad_dec,
                              hipStream_t st) {
    const FullTrainWs l = full_train_ws_layout(img, n);
    const TrainPtrs t = full_train_ptrs(l, ws);
    DecJoin dj;
    dj.dlast = (float*)(ws + l.dlast);
    dj.dskip[0] = nullptr;
    for (int lv = 1; lv < kEncLevels; ++lv) dj.dskip[lv] = (float*)(ws + l.dskip[lv]);
    dj.du = (float*)(ws + l.enc.g[0]);
    dec_backward(img, dec_packed, n, t, grad_prob, scratch, grad_dec, st, &dj);

    EncJoin ej;
    ej.dlast = dj.dlast;
    ej.skip[0] = {nullptr, grad_prob, t.p, dec_packed + dec_packed_floats() - (kEncCh + 1)};
    for (int lv = 1; lv < kEncLevels; ++lv) ej.skip[lv] = {dj.dskip[lv], nullptr, nullptr, nullptr};
    sep_backward(img, dil, residual, enc_packed, n, ws, grad_feats, scratch, grad_enc, st, &ej);
}
