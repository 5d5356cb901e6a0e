// occ_encoder_bwd.hpp -- training of the encoder through its pooled 256-d feature: a forward that keeps what the backward
// needs, and the backward with respect to every encoder parameter.  The kernels here are those of the dense (non-separable,
// dilation 1) layers; the host side -- the layer table (enc_train_layers), the workspace and scratch sizes
// (enc_train_ws_layout), the training forward walk (enc_train_forward) and the backward walk (enc_backward) -- exists once
// for the dense and the separable encoder, whose stride-1 layers go through sep_bwd_layer (occ_sepenc_bwd.hpp) and whose
// downs are the dense stride-2 layers of this file.  Part of the single translation unit occ_kernels.hip (included inside
// namespace occ, after occ_encoder.hpp, whose forward kernels it launches and whose tiling and packed layout its backward
// mirrors, and after occ_decoder_bwd.hpp, whose reduction helpers and two of whose kernels it reuses).
//
// Forward per layer (16 of them: initial, then Layer 1, Layer 2, down per level): u = conv(x) + b, r = relu(u),
// y = s r + t (+ the block input, Layer 2 of a residual block); feats = mean of the last down's y.  BatchNorm runs with
// its running statistics (s, t folded by the host).  No d obs is computed.
//
//   occ_enc_copy_kernel           obs -> ws (the backward has no obs argument; the initial layer's dW reads the copy).
//   occ_enc_dense_kernel<.., TRAIN>  (occ_encoder.hpp) the inference kernel itself at dilation 1, one loop nest for both
//                                 (feats are the same to the bit), whose epilogue also stores r; POOL (the last down)
//                                 stores r and the pool partials, and y only for the joint training (occ_fullnet_bwd.hpp),
//                                 whose decoder reads it.
//   occ_enc_bwd_act_kernel        per (chunk of 4096 pixels, channel, env): dU = dY s [r > 0], written to a buffer of its
//                                 own (the dY of a residual block's Layer 2 is needed again); POOL: dY = grad_feats[n][c] /
//                                 (H H), never stored.  f64 block partials of dS = sum dY r, dT = sum dY, dB = sum dU in
//                                 the layout of occ_dec_bwd_act_kernel (bwd_block_partials); occ_dec_bwd_act_final_kernel
//                                 adds them in block order.  The gate is the forward's own r > 0.
//   occ_enc_bwd_dx1_kernel        stride 1: dX[ci][y][x] = sum_co sum_k w[ci][k][co] dU[co][y + 1 - ky][x + 1 - kx] (+ add).
//                                 A thread owns one pixel for CIG input channels; the (T + 2)^2 dU tile (one-pixel halo,
//                                 zero outside the image) is staged in LDS 8 output channels at a time; weights are
//                                 wave-uniform scalar loads of 8 consecutive co.  `add`: the residual's second path.
//   occ_enc_bwd_dx2_kernel        stride 2: a thread owns the 2 x 2 input quad (2 qy + {0,1}, 2 qx + {0,1}) for 8 input
//                                 channels and reads dU at (qy + {0,1}, qx + {0,1}): the quad mapping of occ_dec_up_kernel
//                                 (1, 2, 2 and 4 taps per quad pixel, no zero-stuffed taps, no parity branches).  dU rows /
//                                 columns >= Ho read as zero; quad pixels >= H are not stored.
//                                 JOIN (the joint training): the decoder's d skip of the level is added in the epilogue,
//                                 read from a kept tensor or, at level 0, rebuilt as gp p (1 - p) cls_w[ci].
//   occ_enc_bwd_dw_kernel         dW[ci][k][co] = sum_{n,oy,ox} x[ci][s oy - 1 + ky][s ox - 1 + kx] dU[co][oy][ox], a
//                                 (9 cin) x cout contraction over K = N Ho^2.  A thread owns 1 ci x 9 taps x 8 co (72 f32
//                                 accumulators); a block owns a CIB x COB tile of (ci, co) and one slice of K (consecutive
//                                 T x T output-pixel tiles, envs in order); when the tile needs fewer than 256 threads the
//                                 others take other pixels (P pixel lanes), added inside the wave by __shfl_xor steps in
//                                 a fixed order (bwd_dw_fold).  Every block writes its partial dW (one per wave or pixel
//                                 lane) to caller scratch; occ_dec_bwd_sum_kernel adds the partials in f64 in a fixed order.
//
// Launches: train forward 18 (copy, 16 layers, pool); dense backward 79 (per layer act, act-final, dW, sum = 64, and the
// input gradient of the 15 layers above the initial one); separable backward 112 (occ_sepenc_bwd.hpp).  No floating-point
// atomics; the split of K is a function of (S, N) alone: every gradient is bitwise the same from call to call.  Nothing is
// allocated or synchronised.
// Host side: the K split (DwPlan, dw_split) and the per-layer tail (bwd_layer_tail) are those of occ_decoder_bwd.hpp, the
// grids of the two input gradients come from tile_launch (occ_encoder.hpp).
//
// Workspace (occ_encoder_train_workspace_query, occ_sep_encoder_train_workspace_query: the same tensors are kept for both
// forms; only the scratch differs), every part 256-byte aligned, f32, H_0 = S, H_{lv+1} = ceil(H_lv / 2), c = 8 << lv:
//   obs (n,4,S,S) | r_init (n,8,S,S) |
//   per level lv: a (n,c,H,H) block input | r1 | b = Layer 1 output | r2 | cc = Layer 2 output (+ a) | rd (n,2c,H',H')
//                 (a of level lv + 1 is the down's y; the last down stores no y)
//   | pool partials (n, tiles, 256) | g0 | g1 | g2: three gradient buffers of (n,8,S,S)
// At 256^2 that is 30.31 MiB per env (1 obs, 23.31 kept activations, 6 gradient): 128 envs take 3.79 GiB.

constexpr int kEncDwBlocks = 512;  // blocks of the weight gradient per layer (K slices x (ci, co) tiles)
constexpr int kEncDwCot = 8;       // output channels per thread of the weight gradient

__global__ __launch_bounds__(256) void occ_enc_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

// Activation step of one layer.  dy: (n, c, plane); du: (n, c, plane), may be dy itself.  POOL: dY = gf[env][ch] / count, plus
// dy when dy is not null (the decoder's gradient of the last down's output, occ_fullnet_bwd.hpp).
// partials[((ch * n + env) * chunks + chunk) * 3 + k]: k = 0 dS, 1 dT, 2 dB.
template <bool POOL>
__global__ __launch_bounds__(256) void occ_enc_bwd_act_kernel(const float* dy, float* du, const float* __restrict__ r,
                                                              const float* __restrict__ bns, int c, int plane,
                                                              const float* __restrict__ gf, float count,
                                                              double* __restrict__ partials) {
    const int ch = blockIdx.y, env = blockIdx.z;
    const size_t base = ((size_t)env * c + ch) * plane;
    const float sc = bns[ch];
    float pooled = 0.f;
    if constexpr (POOL) pooled = gf[(size_t)env * c + ch] / count;
    double sum[3] = {0.0, 0.0, 0.0};
    const int lo = blockIdx.x * kBwdChunk;
    for (int j = 0; j < kBwdChunk / 256; ++j) {
        const int i = lo + (int)threadIdx.x + 256 * j;
        if (i >= plane) break;
        const float rv = r[base + i];
        float d;
        if constexpr (POOL) d = dy ? pooled + dy[base + i] : pooled;
        else d = dy[base + i];
        const float u = rv > 0.f ? d * sc : 0.f;
        sum[0] = fma((double)d, (double)rv, sum[0]);
        sum[1] += (double)d;
        sum[2] += (double)u;
        du[base + i] = u;
    }
    bwd_block_partials(sum, partials + ((((size_t)ch * gridDim.z + env) * gridDim.x) + blockIdx.x) * 3);
}

// du: (n, cout, H, H); dx, add: (n, cin, H, H); w: the layer's packed w[ci][k][co].  cin % CIG == 0, cout % 8 == 0.
template <int T, int CIG>
__global__ __launch_bounds__(256) void occ_enc_bwd_dx1_kernel(const float* __restrict__ du, float* __restrict__ dx,
                                                              const float* __restrict__ add, const float* __restrict__ w,
                                                              int cin, int cout, int H, int tiles_x) {
    constexpr int TT = T * T, R = T + 2, RR = R * R, CC = kBwdDxCC;
    __shared__ float s[CC * RR];
    const int tid = threadIdx.x;
    const int p = tid % TT;
    const int ng = blockDim.x / TT;
    const int g = __builtin_amdgcn_readfirstlane(tid / TT);
    const int ci0 = (blockIdx.y * ng + g) * CIG;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const int iy0 = ty * T, ix0 = tx * T;
    const int py = p / T, px = p % T;
    const size_t plane = (size_t)H * H;
    const float* de = du + (size_t)blockIdx.z * cout * plane;

    float acc[CIG];
#pragma unroll
    for (int j = 0; j < CIG; ++j) acc[j] = 0.f;

    for (int co0 = 0; co0 < cout; co0 += CC) {
        __syncthreads();
        for (int i = tid; i < CC * RR; i += blockDim.x) {
            const int c = i / RR, r = i - c * RR;
            const int ry = r / R, rx = r - ry * R;
            const int gy = iy0 - 1 + ry, gx = ix0 - 1 + rx;
            float v = 0.f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < H) v = de[(co0 + c) * plane + (size_t)gy * H + gx];
            s[i] = v;
        }
        __syncthreads();
        float d[CC][9];
#pragma unroll
        for (int c = 0; c < CC; ++c) {
            const float* sp = s + c * RR + py * R + px;  // staged (y - 1, x - 1); tap k reads dU at (y + 1 - ky, x + 1 - kx)
#pragma unroll
            for (int k = 0; k < 9; ++k) d[c][k] = sp[(2 - k / 3) * R + 2 - k % 3];
        }
        const float* wr = w + (size_t)ci0 * 9 * cout + co0;
#pragma unroll
        for (int j = 0; j < CIG; ++j)
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float* wk = wr + (size_t)(j * 9 + k) * cout;
#pragma unroll
                for (int c = 0; c < CC; ++c) acc[j] = fmaf(wk[c], d[c][k], acc[j]);
            }
    }
    const int iy = iy0 + py, ix = ix0 + px;
    if (iy >= H || ix >= H) return;
    const size_t o = ((size_t)blockIdx.z * cin + ci0) * plane + (size_t)iy * H + ix;
#pragma unroll
    for (int j = 0; j < CIG; ++j) {
        float v = acc[j];
        if (add) v += add[o + j * plane];
        dx[o + j * plane] = v;
    }
}

// What the joint training (occ_fullnet_bwd.hpp) adds to the stride-2 input gradient: the decoder's d skip of the level.
struct EncSkipGrad {
    const float* add;   // JOIN 1: (n, cin, H, H), the kept dY of the decoder level that read this skip
    const float* gp;    // JOIN 2 (level 0): d loss / d prob (n, H, H); d skip[ci] = gp p (1 - p) clsw[ci] is rebuilt here
    const float* prob;  //         the forward's kept prob (n, H, H)
    const float* clsw;  //         cls_w[cin]
};

// du: (n, cout, Ho, Ho), Ho = ceil(H / 2); dx: (n, cin, H, H).  cin % 8 == 0, cout % 8 == 0.  A T x T tile of quads.
// JOIN 0: dx = the input gradient; 1 and 2: plus the d skip of EncSkipGrad, added in the epilogue.
template <int T, int JOIN = 0>
__global__ __launch_bounds__(256) void occ_enc_bwd_dx2_kernel(const float* __restrict__ du, float* __restrict__ dx,
                                                              const float* __restrict__ w, int cin, int cout, int H, int Ho,
                                                              int tiles_x, EncSkipGrad sk) {
    constexpr int TT = T * T, R = T + 1, RR = R * R, CC = kBwdDxCC, CIG = 8;
    __shared__ float s[CC * RR];
    const int tid = threadIdx.x;
    const int p = tid % TT;
    const int ng = blockDim.x / TT;
    const int g = __builtin_amdgcn_readfirstlane(tid / TT);
    const int ci0 = (blockIdx.y * ng + g) * CIG;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const int qy0 = ty * T, qx0 = tx * T;
    const int py = p / T, px = p % T;
    const size_t oplane = (size_t)Ho * Ho;
    const float* de = du + (size_t)blockIdx.z * cout * oplane;

    float acc[4][CIG];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < CIG; ++j) acc[q][j] = 0.f;

    for (int co0 = 0; co0 < cout; co0 += CC) {
        __syncthreads();
        for (int i = tid; i < CC * RR; i += blockDim.x) {
            const int c = i / RR, r = i - c * RR;
            const int ry = r / R, rx = r - ry * R;
            const int gy = qy0 + ry, gx = qx0 + rx;
            float v = 0.f;
            if (gy < Ho && gx < Ho) v = de[(co0 + c) * oplane + (size_t)gy * Ho + gx];
            s[i] = v;
        }
        __syncthreads();
        float d[CC][4];
#pragma unroll
        for (int c = 0; c < CC; ++c) {
            const float* sp = s + c * RR + py * R + px;
            d[c][0] = sp[0], d[c][1] = sp[1], d[c][2] = sp[R], d[c][3] = sp[R + 1];
        }
        const float* wr = w + (size_t)ci0 * 9 * cout + co0;
#pragma unroll
        for (int j = 0; j < CIG; ++j) {
            const float* wj = wr + (size_t)j * 9 * cout;  // wj[k * cout + c] = w[ci][k][co0 + c]
#pragma unroll
            for (int c = 0; c < CC; ++c) {
                const float a = d[c][0], b = d[c][1], cv = d[c][2], dv = d[c][3];
                // input (2qy + ey, 2qx + ex) meets output (qy + (ey + 1 - ky) / 2, ..) for the taps of matching parity
                acc[0][j] = fmaf(wj[4 * cout + c], a, acc[0][j]);
                acc[1][j] = fmaf(wj[3 * cout + c], b, fmaf(wj[5 * cout + c], a, acc[1][j]));
                acc[2][j] = fmaf(wj[1 * cout + c], cv, fmaf(wj[7 * cout + c], a, acc[2][j]));
                acc[3][j] = fmaf(wj[0 * cout + c], dv,
                                 fmaf(wj[2 * cout + c], cv, fmaf(wj[6 * cout + c], b, fmaf(wj[8 * cout + c], a, acc[3][j]))));
            }
        }
    }
    const int qy = qy0 + py, qx = qx0 + px;
    const int iy = 2 * qy, ix = 2 * qx;
    if (iy >= H || ix >= H) return;
    const size_t plane = (size_t)H * H;
    const size_t xo = ((size_t)blockIdx.z * cin + ci0) * plane + (size_t)iy * H + ix;
    float* xe = dx + xo;
    const bool right = ix + 1 < H, below = iy + 1 < H;
    const bool in[4] = {true, right, below, right && below};
    const size_t qoff[4] = {0, 1, (size_t)H, (size_t)H + 1};
    float dz[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (JOIN == 2) {  // dz as occ_dec_bwd_act_kernel<true> forms it
        const size_t po = (size_t)blockIdx.z * plane + (size_t)iy * H + ix;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (in[q]) {
                const float pv = sk.prob[po + qoff[q]];
                dz[q] = sk.gp[po + qoff[q]] * (pv * (1.f - pv));
            }
    }
#pragma unroll
    for (int j = 0; j < CIG; ++j) {
        float cw = 0.f;
        if constexpr (JOIN == 2) cw = sk.clsw[ci0 + j];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!in[q]) continue;
            float v = acc[q][j];
            if constexpr (JOIN == 1) v += sk.add[xo + j * plane + qoff[q]];
            if constexpr (JOIN == 2) v += dz[q] * cw;
            xe[j * plane + qoff[q]] = v;
        }
    }
}

// x: (n, cin, H, H); du: (n, cout, Ho, Ho); part: [slice * PB + wave or pixel lane][cin * 9 * cout], PB = 256 / max(Q, 64).
// A slice is the tiles [blockIdx.x * tps, .. + tps) of the n * tiles_x^2 output-pixel tiles, envs in order.
template <int T, int CIB, int COB, int STRIDE>
__global__ __launch_bounds__(256) void occ_enc_bwd_dw_kernel(const float* __restrict__ x, const float* __restrict__ du,
                                                             float* __restrict__ part, int cin, int cout, int H, int Ho,
                                                             int tiles_x, int total_tiles, int tps) {
    constexpr int TT = T * T, R = (T - 1) * STRIDE + 3, RR = R * R, XP = RR | 1, COT = kEncDwCot, Q = CIB * (COB / COT),
                  P = 256 / Q;
    static_assert(Q <= 256 && 256 % Q == 0 && (Q >= 64 || 64 % Q == 0) && COB % COT == 0, "thread layout");
    __shared__ float xs[CIB * XP];
    __shared__ float ds[COB * TT];
    const int tid = threadIdx.x;
    const int q = tid % Q, pl = tid / Q;
    const int cil = q % CIB, cog = q / CIB;
    const int nco = cout / COB;
    const int ci0 = (blockIdx.y / nco) * CIB, co0 = (blockIdx.y % nco) * COB;
    const size_t plane = (size_t)H * H, oplane = (size_t)Ho * Ho;
    const int tiles_env = tiles_x * tiles_x;

    float acc[9][COT];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int j = 0; j < COT; ++j) acc[k][j] = 0.f;

    const int t0 = blockIdx.x * tps, t1 = min(t0 + tps, total_tiles);
    for (int t = t0; t < t1; ++t) {
        const int env = t / tiles_env, rem = t - env * tiles_env;
        const int oy0 = (rem / tiles_x) * T, ox0 = (rem % tiles_x) * T;
        const float* xe = x + ((size_t)env * cin + ci0) * plane;
        const float* de = du + ((size_t)env * cout + co0) * oplane;
        __syncthreads();
        for (int i = tid; i < CIB * RR; i += 256) {
            const int c = i / RR, r = i - c * RR;
            const int ry = r / R, rx = r - ry * R;
            const int gy = oy0 * STRIDE - 1 + ry, gx = ox0 * STRIDE - 1 + rx;
            float v = 0.f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < H) v = xe[c * plane + (size_t)gy * H + gx];
            xs[c * XP + r] = v;
        }
        for (int i = tid; i < COB * TT; i += 256) {
            const int c = i / TT, p = i - c * TT;
            const int gy = oy0 + p / T, gx = ox0 + p % T;
            float v = 0.f;
            if (gy < Ho && gx < Ho) v = de[c * oplane + (size_t)gy * Ho + gx];
            ds[i] = v;
        }
        __syncthreads();
        for (int p = pl; p < TT; p += P) {
            const float* xp = xs + cil * XP + (p / T) * STRIDE * R + (p % T) * STRIDE;
            float xv[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) xv[k] = xp[(k / 3) * R + k % 3];
            const float* dp = ds + cog * COT * TT + p;
#pragma unroll
            for (int j = 0; j < COT; ++j) {
                const float d = dp[j * TT];
#pragma unroll
                for (int k = 0; k < 9; ++k) acc[k][j] = fmaf(xv[k], d, acc[k][j]);
            }
        }
    }
    constexpr int PB = dw_partials(Q);
    int pb;
    if (!bwd_dw_fold<Q>(reinterpret_cast<float(&)[9 * COT]>(acc), pl, pb)) return;
    const size_t nout = (size_t)cin * 9 * cout;
    float* dst = part + ((size_t)blockIdx.x * PB + pb) * nout + (size_t)(ci0 + cil) * 9 * cout + co0 + cog * COT;
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int j = 0; j < COT; ++j) dst[(size_t)k * cout + j] = acc[k][j];
}

// ---- host side -----------------------------------------------------------------------------------------------------

// The 16 layers in packed order.  separable: the stride-1 layers are separable ones (the downs are dense either way).
struct EncLayer {
    int cin, cout, stride, H, Ho;  // input side, output side
    long long woff;                // floats into the packed buffer
};

inline void enc_train_layers(int img, bool separable, EncLayer* L) {
    long long off = 0;
    int H = img, i = 0;
    auto put = [&](int cin, int cout, int stride) {
        L[i++] = {cin, cout, stride, H, enc_out_size(H, stride), off};
        off += enc_layer_floats(cin, cout, separable && stride == 1);
    };
    put(4, kEncCh, 1);
    for (int lv = 0; lv < kEncLevels; ++lv) {
        const int c = kEncCh << lv;
        put(c, c, 1);
        put(c, c, 1);
        put(c, 2 * c, 2);
        H = enc_out_size(H, 2);
    }
}

// The (ci, co) tile, pixel tile and K split (dw_split, occ_decoder_bwd.hpp) of the weight gradient of one layer: a thread
// owns 1 ci x 8 co.
inline DwPlan enc_dw_plan(int cin, int cout, int Ho, int n) {
    const int cib = cin < 64 ? cin : 64, cob = cout < 32 ? cout : 32;
    return dw_split(cib, cob, cib == 64 ? 4 : 8, cib * (cob / kEncDwCot), cin, cout, Ho, n, kEncDwBlocks);
}

struct EncTrainWs {
    size_t obs, r_init, a[kEncLevels], r1[kEncLevels], b[kEncLevels], r2[kEncLevels], cc[kEncLevels], rd[kEncLevels], part, g[3];
    size_t total, scratch;
};

// The separable stride-1 layer's backward (occ_sepenc_bwd.hpp, included after this file).
inline DwPlan sep_dpw_plan(int cin, int cout, int H, int n);
static void sep_bwd_layer(const EncLayer& L, int d, const float* packed, float* grad_packed, int n, const float* x, const float* r,
                          const float* dy, float* du, float* dh, float* dx, const float* add, char* scratch, hipStream_t st,
                          const BnTrain* bn = nullptr, int index = 0);

// The workspace is the same for both forms (the same tensors are kept); the scratch is the largest of every layer's
// activation partials, weight gradient partials (dense or, a separable layer, pointwise) and, a separable layer, G partials.
inline EncTrainWs enc_train_ws_layout(int img, int n, bool separable) {
    EncTrainWs l;
    size_t at = 0;
    auto take = [&](size_t floats) {
        const size_t o = at;
        at += enc_align(floats * sizeof(float));
        return o;
    };
    const size_t S2 = (size_t)img * img;
    l.obs = take((size_t)n * 4 * S2);
    l.r_init = take((size_t)n * kEncCh * S2);
    int H = img;
    for (int lv = 0; lv < kEncLevels; ++lv) {
        const size_t act = (size_t)n * (kEncCh << lv) * H * H;
        const int Ho = enc_out_size(H, 2);
        l.a[lv] = take(act);
        l.r1[lv] = take(act);
        l.b[lv] = take(act);
        l.r2[lv] = take(act);
        l.cc[lv] = take(act);
        l.rd[lv] = take((size_t)n * (2 * kEncCh << lv) * Ho * Ho);
        H = Ho;
    }
    l.part = take((size_t)n * enc_tiles(H) * kEncFeat);
    for (int i = 0; i < 3; ++i) l.g[i] = take((size_t)n * kEncCh * S2);
    l.total = at;
    l.scratch = 0;
    EncLayer L[16];
    enc_train_layers(img, separable, L);
    for (int i = 0; i < 16; ++i) {
        const bool sep = separable && L[i].stride == 1;
        const size_t chunks = bwd_chunks(L[i].Ho * L[i].Ho);
        const size_t act = (size_t)L[i].cout * n * chunks * 3 * sizeof(double);
        const size_t dw = sep ? sep_dpw_plan(L[i].cin, L[i].cout, L[i].H, n).part_bytes
                              : enc_dw_plan(L[i].cin, L[i].cout, L[i].Ho, n).part_bytes;
        const size_t gp = sep ? (size_t)L[i].cin * n * chunks * 9 * sizeof(double) : 0;
        l.scratch = act > l.scratch ? act : l.scratch;
        l.scratch = dw > l.scratch ? dw : l.scratch;
        l.scratch = gp > l.scratch ? gp : l.scratch;
    }
    l.scratch = enc_align(l.scratch);
    return l;
}

// The encoder, dense (dil = 1) or separable, on n envs with everything kept: 18 launches (copy, 16 layers through the
// launchers of occ_encoder.hpp with a place for r, pool).
// last_y: where the last down also stores its output (n, 256, H_5, H_5), or null.
// bn (with last_y): batch statistics (occ_bn_train.hpp): every layer's y and feats come from bn_fwd_layer (3 launches per
// layer more, no pool launch); the scale / shift slots of `packed` carry gamma / beta.
static void enc_train_forward(int img, int dil, bool residual, bool separable, const float* packed, const float* obs, int n,
                              char* ws, float* feats, hipStream_t st, float* last_y = nullptr, const BnTrain* bn = nullptr) {
    const EncTrainWs l = enc_train_ws_layout(img, n, separable);
    EncLayer L[16];
    enc_train_layers(img, separable, L);
    auto F = [&](size_t off) { return (float*)(ws + off); };
    const size_t nobs = (size_t)n * 4 * img * img;
    const size_t cblocks = (nobs + 1023) / 1024;
    hipLaunchKernelGGL(occ_enc_copy_kernel, dim3((unsigned)(cblocks < 65535 ? cblocks : 65535)), dim3(256), 0, st, obs, F(l.obs),
                       nobs);
    auto layer = [&](const EncLayer& Li, int d, const float* x, float* y, float* r, const float* resid, float* partials) {
        const float* w = packed + Li.woff;
        if (separable && Li.stride == 1) enc_launch_sep(x, y, resid, w, Li.cin, Li.cout, Li.H, d, n, st, r);
        else enc_launch_dense(x, y, resid, w, Li.cin, Li.cout, Li.H, Li.stride, d, n, partials, st, false, r);
        if (bn) {
            const float* gamma = w + enc_layer_floats(Li.cin, Li.cout, separable && Li.stride == 1) - 2 * Li.cout;
            bn_fwd_layer(*bn, (int)(&Li - L), Li.cout, Li.Ho * Li.Ho, n, gamma, gamma + Li.cout, r, y, resid,
                         partials ? feats : nullptr, nullptr, nullptr, nullptr, st);
        }
    };
    layer(L[0], 1, F(l.obs), F(l.a[0]), F(l.r_init), nullptr, nullptr);
    for (int lv = 0; lv < kEncLevels; ++lv) {
        const EncLayer* Ll = L + 1 + 3 * lv;
        const bool last = lv == kEncLevels - 1;
        layer(Ll[0], dil, F(l.a[lv]), F(l.b[lv]), F(l.r1[lv]), nullptr, nullptr);
        layer(Ll[1], dil, F(l.b[lv]), F(l.cc[lv]), F(l.r2[lv]), residual ? F(l.a[lv]) : nullptr, nullptr);
        layer(Ll[2], 1, F(l.cc[lv]), last ? last_y : F(l.a[lv + 1]), F(l.rd[lv]), nullptr, last ? F(l.part) : nullptr);
    }
    if (bn) return;
    const int Hl = L[15].Ho;
    hipLaunchKernelGGL(occ_enc_pool_kernel, dim3(n), dim3(kEncFeat), 0, st, F(l.part), enc_tiles(Hl), (float)(Hl * Hl), feats, nullptr);
}

template <int T, int CIB, int COB, int STRIDE>
static void enc_launch_dw_t(const DwPlan& p, const float* x, const float* du, float* part, const EncLayer& L, hipStream_t st) {
    hipLaunchKernelGGL((occ_enc_bwd_dw_kernel<T, CIB, COB, STRIDE>), dim3(p.slices, p.grid_y), dim3(256), 0, st, x, du, part, L.cin,
                       L.cout, L.H, L.Ho, p.tiles_x, p.total_tiles, p.tps);
}

// The nine (ci, co) tiles of enc_dw_plan: stride 1 has cout = cin (4 -> 8 for the initial layer), stride 2 cout = 2 cin.
static void enc_launch_dw(const DwPlan& p, const float* x, const float* du, float* part, const EncLayer& L, hipStream_t st) {
    if (L.stride == 1) {
        if (p.cib == 4) enc_launch_dw_t<8, 4, 8, 1>(p, x, du, part, L, st);
        else if (p.cib == 8) enc_launch_dw_t<8, 8, 8, 1>(p, x, du, part, L, st);
        else if (p.cib == 16) enc_launch_dw_t<8, 16, 16, 1>(p, x, du, part, L, st);
        else if (p.cib == 32) enc_launch_dw_t<8, 32, 32, 1>(p, x, du, part, L, st);
        else enc_launch_dw_t<4, 64, 32, 1>(p, x, du, part, L, st);
    } else {
        if (p.cib == 8) enc_launch_dw_t<8, 8, 16, 2>(p, x, du, part, L, st);
        else if (p.cib == 16) enc_launch_dw_t<8, 16, 32, 2>(p, x, du, part, L, st);
        else if (p.cib == 32) enc_launch_dw_t<8, 32, 32, 2>(p, x, du, part, L, st);
        else enc_launch_dw_t<4, 64, 32, 2>(p, x, du, part, L, st);
    }
}

static void enc_launch_dx1(const float* du, float* dx, const float* add, const float* w, const EncLayer& L, int n, hipStream_t st) {
    const int T = enc_tile(L.H);
    const TileLaunch l = tile_launch(T, L.H, L.cin == 8 ? 1 : L.cin / kBwdDxCIG, n);
#define OCC_ENC_DX1(TT, CIG) \
    hipLaunchKernelGGL((occ_enc_bwd_dx1_kernel<TT, CIG>), l.grid, l.block, 0, st, du, dx, add, w, L.cin, L.cout, L.H, l.tiles_x)
    if (L.cin == 8 && T == 16) OCC_ENC_DX1(16, 8);
    else if (L.cin == 8) OCC_ENC_DX1(8, 8);
    else if (T == 16) OCC_ENC_DX1(16, kBwdDxCIG);
    else OCC_ENC_DX1(8, kBwdDxCIG);
#undef OCC_ENC_DX1
}

// sk: null, or the d skip to add (sk->add, or sk->gp at level 0, where Ho = S / 2 >= 16).
static void enc_launch_dx2(const float* du, float* dx, const float* w, const EncLayer& L, int n, hipStream_t st,
                           const EncSkipGrad* sk = nullptr) {
    const int T = enc_tile(L.Ho);
    const TileLaunch l = tile_launch(T, L.Ho, L.cin / 8, n);
    const EncSkipGrad s = sk ? *sk : EncSkipGrad{nullptr, nullptr, nullptr, nullptr};
#define OCC_ENC_DX2(TT, JOIN) \
    hipLaunchKernelGGL((occ_enc_bwd_dx2_kernel<TT, JOIN>), l.grid, l.block, 0, st, du, dx, w, L.cin, L.cout, L.H, L.Ho, l.tiles_x, s)
    if (s.gp) OCC_ENC_DX2(16, 2);
    else if (s.add && T == 16) OCC_ENC_DX2(16, 1);
    else if (s.add) OCC_ENC_DX2(8, 1);
    else if (T == 16) OCC_ENC_DX2(16, 0);
    else OCC_ENC_DX2(8, 0);
#undef OCC_ENC_DX2
}

// One layer's parameter gradients from its dY (or, pool, from grad_feats and, when not null, dy): dU is left in `du`.
// 4 launches.  bn: the forward ran with batch statistics; the activation step is bn_bwd_act for layer `index` (6 launches).
static void enc_bwd_layer(const EncLayer& L, const float* packed, float* grad_packed, int n, const float* x, const float* r,
                          const float* dy, float* du, const float* gf, char* scratch, hipStream_t st, const BnTrain* bn = nullptr,
                          int index = 0) {
    const int plane = L.Ho * L.Ho, chunks = bwd_chunks(plane);
    const float* w = packed + L.woff;
    float* gw = grad_packed + L.woff;
    float* gbias = gw + 9LL * L.cin * L.cout;
    const float* bns = w + 9LL * L.cin * L.cout + L.cout;
    const dim3 agrid(chunks, L.cout, n);
    if (bn)
        bn_bwd_act(*bn, index, L.cout, plane, n, BnDy{dy, gf, nullptr, nullptr, nullptr, nullptr}, du, r, bns, gbias + L.cout,
                   gbias + 2 * L.cout, nullptr, scratch, st);
    else if (gf)
        hipLaunchKernelGGL((occ_enc_bwd_act_kernel<true>), agrid, dim3(256), 0, st, dy, du, r, bns, L.cout, plane, gf,
                           (float)plane, (double*)scratch);
    else
        hipLaunchKernelGGL((occ_enc_bwd_act_kernel<false>), agrid, dim3(256), 0, st, dy, du, r, bns, L.cout, plane, nullptr, 1.f,
                           (double*)scratch);
    const BwdActDst dst = bn ? BwdActDst{{gbias, nullptr, nullptr, nullptr, nullptr}}
                             : BwdActDst{{gbias + L.cout, gbias + 2 * L.cout, gbias, nullptr, nullptr}};
    const DwPlan p = enc_dw_plan(L.cin, L.cout, L.Ho, n);
    bwd_layer_tail(p, 9 * L.cin * L.cout, L.cout, n * chunks, bn ? 1 : 3, dst, scratch, gw, st, [&](float* part) { enc_launch_dw(p, x, du, part, L, st); });
}

// join (occ_fullnet_bwd.hpp): the decoder's gradients that meet the encoder's, in the dense downs of either form: dlast
// joins the pool backward in the last down's activation step, skip[lv] joins the dY of cc[lv] in the epilogue of the
// down's input gradient.
struct EncJoin {
    const float* dlast;             // (n, 256, H_5, H_5)
    EncSkipGrad skip[kEncLevels];
};

// Where a stride-1 layer of the walk reads its dY and leaves dU, dH (separable only) and its input gradient (null: none).
// Per level gA holds the down's dY / dU and gB the dY of Layer 2's output (kept for the residual); the block input's
// gradient ends in gC, which is the gA of the level above.  In between the two forms differ:
//   dense      gC = Layer 2's dU, gA = Layer 1's dY, turned into its dU in place;
//   separable  gA = dH of both layers, gC = Layer 2's dU, Layer 1's dY and dU in place (the initial layer's dH goes to gC).
struct EncBwdBufs {
    const float* dy;
    float *du, *dh, *dx;
};
enum EncBwdRole { kBwdLayer2, kBwdLayer1, kBwdInitial };

inline EncBwdBufs enc_bwd_bufs(bool separable, EncBwdRole role, float* gA, float* gB, float* gC) {
    if (separable) {
        if (role == kBwdLayer2) return {gB, gC, gA, gC};
        if (role == kBwdLayer1) return {gC, gC, gA, gC};
        return {gA, gA, gC, nullptr};
    }
    if (role == kBwdLayer2) return {gB, gC, nullptr, gA};
    if (role == kBwdLayer1) return {gA, gA, nullptr, gC};
    return {gA, gA, nullptr, nullptr};
}

// The backward of the latest enc_train_forward of the same form on this workspace, the deepest layer first: 79 launches
// (dense), 112 (separable).  grad_packed is overwritten.
static void enc_backward(int img, int dil, bool residual, bool separable, const float* packed, int n, char* ws,
                         const float* grad_feats, char* scratch, float* grad_packed, hipStream_t st, const EncJoin* join = nullptr,
                         const BnTrain* bn = nullptr) {
    const EncTrainWs l = enc_train_ws_layout(img, n, separable);
    EncLayer L[16];
    enc_train_layers(img, separable, L);
    auto F = [&](size_t off) { return (float*)(ws + off); };
    float *gA = F(l.g[0]), *gB = F(l.g[1]), *gC = F(l.g[2]);
    // one stride-1 layer: its parameter gradients and, when b.dx is not null, its input gradient (+ add)
    auto layer = [&](const EncLayer& Li, int d, EncBwdRole role, const float* x, const float* r, const float* add) {
        const EncBwdBufs b = enc_bwd_bufs(separable, role, gA, gB, gC);
        if (separable) {
            sep_bwd_layer(Li, d, packed, grad_packed, n, x, r, b.dy, b.du, b.dh, b.dx, add, scratch, st, bn, (int)(&Li - L));
        } else {
            enc_bwd_layer(Li, packed, grad_packed, n, x, r, b.dy, b.du, nullptr, scratch, st, bn, (int)(&Li - L));
            if (b.dx) enc_launch_dx1(b.du, b.dx, add, packed + Li.woff, Li, n, st);
        }
    };
    for (int lv = kEncLevels - 1; lv >= 0; --lv) {
        const EncLayer* Ll = L + 1 + 3 * lv;
        const bool last = lv == kEncLevels - 1;
        enc_bwd_layer(Ll[2], packed, grad_packed, n, F(l.cc[lv]), F(l.rd[lv]), last ? (join ? join->dlast : nullptr) : gA, gA,
                      last ? grad_feats : nullptr, scratch, st, bn, 3 + 3 * lv);
        enc_launch_dx2(gA, gB, packed + Ll[2].woff, Ll[2], n, st, join ? &join->skip[lv] : nullptr);
        layer(Ll[1], dil, kBwdLayer2, F(l.b[lv]), F(l.r2[lv]), nullptr);
        layer(Ll[0], dil, kBwdLayer1, F(l.a[lv]), F(l.r1[lv]), residual ? gB : nullptr);
        float* t = gA;
        gA = gC;
        gC = t;
    }
    layer(L[0], 1, kBwdInitial, F(l.obs), F(l.r_init), nullptr);
}
