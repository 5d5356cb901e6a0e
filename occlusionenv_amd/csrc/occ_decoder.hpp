// occ_decoder.hpp -- inference of the segmentation decoder of FullNetwork / Segmenter (model.py:25-33,52-67,109-166): the
// predicted occlusion map the reference's pretrained checkpoint is judged by (pretrainer.py:127-141), and the counts of
// that judgement.  Part of the single translation unit occ_kernels.hip (included inside namespace occ, after
// occ_encoder.hpp, whose LDS staging and launch conventions it follows).
//
// The network: x = the encoder's last down output (N,256,S/32,S/32); five times x = up_j(x) + skip, with up_j =
// TrConv(2c -> c), c = 128, 64, 32, 16, 8 = bn(relu(ConvTranspose2d(2c, c, 3, stride 2, padding 1, output_padding 1)))
// and skip the encoder's per-level feature, deepest first; then Conv2d(8, 1, 1) and a sigmoid.
// TrConvBlock.forward returns self.up(x) (model.py:63-67): the two `net` layers of every decoder block are computed and
// thrown away by the reference, so they have no effect in eval mode.  They are NOT run here and their weights are not part
// of the packed decoder; no layer is missing.
//
//   occ_dec_up_kernel       one whole TrConv + skip add.  A thread owns one INPUT pixel (iy, ix), hence the 2 x 2 output
//                           quad (2 iy .. 2 iy + 1, 2 ix .. 2 ix + 1), for COG output channels.  With k = 3, stride 2,
//                           padding 1 an output (oy, ox) collects x[iy'][ix'] * w[ky][kx] with oy = 2 iy' - 1 + ky, so the
//                           quad reads a = x[iy][ix], b = x[iy][ix+1], c = x[iy+1][ix], d = x[iy+1][ix+1] (zero beyond the
//                           edge: the output_padding row / column) and uses each of the nine taps exactly once:
//                               o00 = a w11            o01 = a w12 + b w10
//                               o10 = a w21 + c w01    o11 = a w22 + b w20 + c w02 + d w00
//                           No zero-stuffed taps, no parity branches.  The (T + 1) x (T + 1) input tile is staged in LDS
//                           kEncCC channels at a time (row pitch T + 1 = 17 words at T = 16: the four rows a wave reads
//                           span 67 consecutive words, so all but three lanes hit distinct banks); weights are
//                           wave-uniform scalar loads.
//                           FUSE = true (the last level, 16 -> 8 at full resolution, bandwidth-bound): the thread holds
//                           all 8 channels of its quad, so the 1 x 1 classifier and the sigmoid run in the epilogue; the
//                           (N,8,S,S) decoder feature and the logit are stored only when asked for.
//                           TRAIN = true (the training forwards, occ_decoder_bwd.hpp) only adds stores to the epilogue: r =
//                           relu(.) and y always and, FUSE, a kept copy of prob; prob is that of inference to the bit.
//   occ_seg_metrics_kernel  per env the three integer counts of pretrainer.py:133-139 (agree, intersection, union of the
//                           two maps thresholded > 0.5): wave reductions, one block sum, then integer atomic adds,
//                           which commute exactly.
//
// f32 with f32 accumulation in a fixed order, no floating-point atomics: maps are bitwise independent of the batch size and
// of an env's position in the batch.

// logit: inference: where the logit is stored, or null.  TRAIN: where the kept copy of prob is stored (no logit is).
// rkeep (TRAIN): (n, cout, 2H, 2H), where r is stored; not read otherwise.
// env_skip: the env mask of the inference forwards (enc_env_skipped; `skip` here is the encoder's per-level feature).
template <int T, int COG, bool FUSE, bool TRAIN = false>
__global__ __launch_bounds__(256) void occ_dec_up_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                         const float* __restrict__ skip, const float* __restrict__ w, int cin,
                                                         int cout, int H, int tiles_x, const float* __restrict__ cls,
                                                         float* __restrict__ prob, float* __restrict__ logit,
                                                         float* __restrict__ rkeep, const int32_t* __restrict__ env_skip) {
    constexpr int TT = T * T, R = T + 1, RR = R * R;
    __shared__ float s[kEncCC * RR];
    if (enc_env_skipped<TRAIN>(env_skip, blockIdx.z)) return;
    const int tid = threadIdx.x;
    const int p = tid % TT;
    const int ng = blockDim.x / TT;
    const int g = __builtin_amdgcn_readfirstlane(tid / TT);
    const int co0 = (blockIdx.y * ng + g) * COG;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const int iy0 = ty * T, ix0 = tx * T;
    const int py = p / T, px = p % T;
    const size_t plane = (size_t)H * H;
    const float* xe = x + (size_t)blockIdx.z * cin * plane;
    const float* bias = w + (size_t)cin * 9 * cout;
    const float* bns = bias + cout;
    const float* bnt = bns + cout;

    float acc[4][COG];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < COG; ++j) acc[q][j] = 0.f;

    for (int ci0 = 0; ci0 < cin; ci0 += kEncCC) {
        const int cc = min(kEncCC, cin - ci0);
        __syncthreads();
        for (int i = tid; i < cc * RR; i += blockDim.x) {
            const int c = i / RR, r = i - c * RR;
            const int ry = r / R, rx = r - ry * R;
            const int gy = iy0 + ry, gx = ix0 + rx;
            float v = 0.f;
            if (gy < H && gx < H) v = xe[(ci0 + c) * plane + (size_t)gy * H + gx];
            s[i] = v;
        }
        __syncthreads();
        for (int c = 0; c < cc; ++c) {
            const float* sc = s + c * RR + py * R + px;
            const float a = sc[0], b = sc[1], cv = sc[R], dv = sc[R + 1];
            const float* wr = w + (size_t)(ci0 + c) * 9 * cout + co0;  // w[ci][ky * 3 + kx][co]
#pragma unroll
            for (int j = 0; j < COG; ++j) {
                acc[0][j] = fmaf(wr[4 * cout + j], a, acc[0][j]);
                acc[1][j] = fmaf(wr[3 * cout + j], b, fmaf(wr[5 * cout + j], a, acc[1][j]));
                acc[2][j] = fmaf(wr[1 * cout + j], cv, fmaf(wr[7 * cout + j], a, acc[2][j]));
                acc[3][j] = fmaf(wr[0 * cout + j], dv,
                                 fmaf(wr[2 * cout + j], cv, fmaf(wr[6 * cout + j], b, fmaf(wr[8 * cout + j], a, acc[3][j]))));
            }
        }
    }
    const int iy = iy0 + py, ix = ix0 + px;
    if (iy >= H || ix >= H) return;
    const int W2 = 2 * H;
    const size_t oplane = 4 * plane;
    const size_t off = (size_t)(2 * iy) * W2 + 2 * ix;  // even: the two pixels of a quad row are one aligned float2
    const size_t ebase = (size_t)blockIdx.z * cout * oplane;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < COG; ++j) {
        const int co = co0 + j;
        const float2 s0 = *reinterpret_cast<const float2*>(skip + ebase + co * oplane + off);
        const float2 s1 = *reinterpret_cast<const float2*>(skip + ebase + co * oplane + off + W2);
        float r[4], v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            r[q] = fmaxf(acc[q][j] + bias[co], 0.f);
            v[q] = fmaf(r[q], bns[co], bnt[co]);
        }
        v[0] += s0.x;
        v[1] += s0.y;
        v[2] += s1.x;
        v[3] += s1.y;
        if constexpr (TRAIN) {
            *reinterpret_cast<float2*>(rkeep + ebase + co * oplane + off) = make_float2(r[0], r[1]);
            *reinterpret_cast<float2*>(rkeep + ebase + co * oplane + off + W2) = make_float2(r[2], r[3]);
        }
        if (TRAIN || !FUSE || y) {
            *reinterpret_cast<float2*>(y + ebase + co * oplane + off) = make_float2(v[0], v[1]);
            *reinterpret_cast<float2*>(y + ebase + co * oplane + off + W2) = make_float2(v[2], v[3]);
        }
        if constexpr (FUSE) {
#pragma unroll
            for (int q = 0; q < 4; ++q) z[q] = fmaf(cls[j], v[q], z[q]);
        }
    }
    if constexpr (FUSE) {
        // classifier Conv2d(8, 1, 1) and the sigmoid (model.py:149,159); COG = cout = 8: cls = w[8] | bias
        float pr[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            z[q] += cls[COG];
            pr[q] = 1.f / (1.f + expf(-z[q]));
        }
        const size_t o = (size_t)blockIdx.z * oplane + off;
        *reinterpret_cast<float2*>(prob + o) = make_float2(pr[0], pr[1]);
        *reinterpret_cast<float2*>(prob + o + W2) = make_float2(pr[2], pr[3]);
        if constexpr (TRAIN) {
            *reinterpret_cast<float2*>(logit + o) = make_float2(pr[0], pr[1]);
            *reinterpret_cast<float2*>(logit + o + W2) = make_float2(pr[2], pr[3]);
        } else if (logit) {
            *reinterpret_cast<float2*>(logit + o) = make_float2(z[0], z[1]);
            *reinterpret_cast<float2*>(logit + o + W2) = make_float2(z[2], z[3]);
        }
    }
}

// counts[env] = {pixels where (pred > 0.5) == (target > 0.5), where both hold, where either holds}.  target is read with a
// pixel stride (the alpha channel of an (N,S,S,4) image: stride 4).  counts must be zero on entry (the entry point clears
// them on the same stream).
constexpr int kSegMetricsBlock = 256;
constexpr int kSegMetricsPerBlock = 256 * 16;

__global__ __launch_bounds__(kSegMetricsBlock) void occ_seg_metrics_kernel(const float* __restrict__ pred,
                                                                           const float* __restrict__ target, int tstride,
                                                                           int npix, unsigned long long* __restrict__ counts) {
    __shared__ int part[kSegMetricsBlock / 64][3];
    const float* pe = pred + (size_t)blockIdx.y * npix;
    const float* te = target + (size_t)blockIdx.y * npix * tstride;
    const int lo = blockIdx.x * kSegMetricsPerBlock;
    const int hi = min(npix, lo + kSegMetricsPerBlock);
    int agree = 0, inter = 0, uni = 0;
    for (int i = lo + threadIdx.x; i < hi; i += kSegMetricsBlock) {
        const bool a = pe[i] > 0.5f, b = te[(size_t)i * tstride] > 0.5f;
        agree += a == b;
        inter += a && b;
        uni += a || b;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        agree += __shfl_down(agree, d);
        inter += __shfl_down(inter, d);
        uni += __shfl_down(uni, d);
    }
    const int wave = threadIdx.x / 64;
    if (threadIdx.x % 64 == 0) {
        part[wave][0] = agree;
        part[wave][1] = inter;
        part[wave][2] = uni;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        int sum = 0;
        for (int k = 0; k < kSegMetricsBlock / 64; ++k) sum += part[k][threadIdx.x];
        atomicAdd(counts + (size_t)blockIdx.y * 3 + threadIdx.x, (unsigned long long)sum);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------

// floats of the packed decoder (header: occ_decoder_packed_floats): five up layers, then the classifier
inline long long dec_packed_floats() {
    long long n = 0;
    for (int j = 0; j < kEncLevels; ++j) {
        const int c = kEncCh << (kEncLevels - 1 - j);
        n += 9LL * 2 * c * c + 3LL * c;
    }
    return n + kEncCh + 1;
}

// workspace of occ_segment_forward: b0 | b1 (level-0 size each; the decoder's intermediate outputs ping-pong in them once
// the encoder is through) | skip[0..5) | last | partials
struct SegWs {
    size_t buf_bytes, part_bytes, skip_bytes[kEncLevels], last_bytes, total;
};

inline SegWs seg_ws_layout(int img, int n) {
    SegWs l;
    enc_ws_layout(img, n, &l.buf_bytes, &l.part_bytes);
    l.total = 2 * l.buf_bytes + l.part_bytes;
    for (int lv = 0; lv < kEncLevels; ++lv) {
        const size_t side = (size_t)(img >> lv);
        l.skip_bytes[lv] = enc_align((size_t)n * (kEncCh << lv) * side * side * sizeof(float));
        l.total += l.skip_bytes[lv];
    }
    const size_t side = (size_t)(img >> kEncLevels);
    l.last_bytes = enc_align((size_t)n * kEncFeat * side * side * sizeof(float));
    l.total += l.last_bytes;
    return l;
}

// cls = null: a level below the last; prob and logit are not used.  rkeep = null: inference.  rkeep given (the training
// forwards, occ_decoder_bwd.hpp): the TRAIN instantiation on the same grid; `logit` is then where the kept prob goes.
template <bool TRAIN>
static void dec_launch_up_t(const float* x, float* y, const float* skip, const float* w, int cin, int cout, int H, int n,
                            const float* cls, float* prob, float* logit, hipStream_t st, float* rkeep, const int32_t* env_skip) {
    constexpr int COG = 16;  // 64 accumulators per thread; cout = 128, 64, 32, 16 below the last level
    const int T = enc_tile(H);
    const TileLaunch l = tile_launch(T, H, cls ? 1 : cout / COG, n);
#define OCC_DEC_UP(TT, CG, FUSE)                                                                                               \
    hipLaunchKernelGGL((occ_dec_up_kernel<TT, CG, FUSE, TRAIN>), l.grid, l.block, 0, st, x, y, skip, w, cin, cout, H, l.tiles_x, cls, \
                       prob, logit, rkeep, env_skip)
    if (cls) OCC_DEC_UP(16, 8, true);  // the last level: cout = 8, H = S / 2 >= 16
    else if (T == 16) OCC_DEC_UP(16, COG, false);
    else OCC_DEC_UP(8, COG, false);
#undef OCC_DEC_UP
}

static void dec_launch_up(const float* x, float* y, const float* skip, const float* w, int cin, int cout, int H, int n,
                          const float* cls, float* prob, float* logit, hipStream_t st, float* rkeep = nullptr,
                          const int32_t* env_skip = nullptr) {
    if (rkeep) dec_launch_up_t<true>(x, y, skip, w, cin, cout, H, n, cls, prob, logit, st, rkeep, nullptr);
    else dec_launch_up_t<false>(x, y, skip, w, cin, cout, H, n, cls, prob, logit, st, nullptr, env_skip);
}

// Encoder (17 launches, keeping the skips) + decoder (5 launches): 22 launches.  img % 32 == 0.  env_skip = null, or the env
// mask: a skipped env's rows of feats, prob, logit and dec_feat keep what they held.
static void seg_forward(int img, int dil, bool residual, bool separable, const float* enc_packed, const float* dec_packed,
                        const float* obs, int n, char* ws, float* feats, float* prob, float* logit, float* dec_feat,
                        hipStream_t st, const int32_t* env_skip = nullptr) {
    const SegWs l = seg_ws_layout(img, n);
    float* b0 = (float*)ws;
    float* b1 = (float*)(ws + l.buf_bytes);
    char* at = ws + 2 * l.buf_bytes + l.part_bytes;
    EncKeep keep;
    for (int lv = 0; lv < kEncLevels; ++lv) {
        keep.skip[lv] = (float*)at;
        at += l.skip_bytes[lv];
    }
    keep.last = (float*)at;
    enc_forward(img, dil, residual, separable, enc_packed, obs, n, ws, feats, st, &keep, env_skip);

    const float* w = dec_packed;
    const float* cls = dec_packed + dec_packed_floats() - (kEncCh + 1);
    const float* x = keep.last;
    int H = img >> kEncLevels;
    for (int j = 0; j < kEncLevels; ++j) {
        const int lv = kEncLevels - 1 - j;
        const int c = kEncCh << lv;
        const bool last = j == kEncLevels - 1;
        float* y = last ? dec_feat : (j % 2 == 0 ? b0 : b1);
        dec_launch_up(x, y, keep.skip[lv], w, 2 * c, c, H, n, last ? cls : nullptr, prob, logit, st, nullptr, env_skip);
        w += 9LL * 2 * c * c + 3LL * c;
        x = y;
        H *= 2;
    }
}
