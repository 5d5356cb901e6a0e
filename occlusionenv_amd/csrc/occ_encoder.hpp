// occ_encoder.hpp -- inference of the frozen FullNetwork / PredictorNet encoder (model.py:8-101) whose pooled 256-d feature
// the reference's PPO agent stores every step (PPO.py:47,152-162) and its gradient predictors read (model.py:81-85,164).
// Part of the single translation unit occ_kernels.hip (included inside namespace occ; not a stand-alone header).
//
// The network: initial Conv(4 -> 8), then five ConvBlocks at c = 8 * 2^i (two Conv(c -> c), optional residual, then
// down = dense 3x3 stride-2 Conv(c -> 2c)); the feature is the spatial mean of the last down output.  Every Conv is
// bn(relu(conv(x))): the BatchNorm sits after the ReLU, so it stays a per-channel affine epilogue y = relu(.) * s + t.
// All arithmetic is f32 with f32 accumulation (VALU FMAs; weights are wave-uniform scalar loads).
//
//   occ_enc_sep_kernel    one separable Conv: depthwise (3,1) with dilation (d,1), depthwise (1,3) with dilation (1,d),
//                         pointwise + bias, ReLU, BN affine, + residual.  The input tile and its dilation halo are staged
//                         in LDS (8 channels at a time); each thread forms both depthwise results of its pixel in
//                         registers, so neither depthwise intermediate exists outside the thread.  TRAIN = true (the
//                         training forwards, occ_encoder_bwd.hpp) also stores r = relu(.), which the backward reads.
//   occ_enc_dense_kernel  dense 3x3 Conv, stride 1 or 2, dilation 1 or 2, + bias, ReLU, BN affine (+ residual): the
//                         down convs and the dense layers of the "predictor" preset.  POOL = true (the last down): the
//                         output is not stored; each block writes the per-channel sum over its tile's pixels (a fixed
//                         sequential order) to a partials row instead.  KEEP = true (occ_segment_forward) stores the
//                         output as well, from the same registers: the partials do not change by a bit.  TRAIN = true
//                         also stores r and, POOL, the output where the caller gives a place for it.
//   occ_enc_pool_kernel   per (env, channel) one fixed-order sum of the tile partials / (Ho * Wo).
//
// A thread owns one output pixel and COG output channels; a block is a T x T pixel tile times NG channel groups (one
// wave-uniform group per wave when T = 8).  Nothing depends on the batch size or on an env's position in the batch, and
// there are no atomics: features are bitwise reproducible.  TRAIN only adds stores to the epilogue: the training forwards
// run these very loop nests, so their features are those of inference to the bit.

constexpr int kEncCh = 8;       // channels after the initial layer
constexpr int kEncLevels = 5;   // ConvBlocks
constexpr int kEncFeat = 256;   // kEncCh << kEncLevels
constexpr int kEncCC = 8;       // input channels staged in LDS per step
constexpr int kEncMaxR = 35;    // staged rows / columns: (16 - 1) * stride 2 + 2 * dilation 2 + 1

// The LDS stages, padded to the largest staged region: dense (any stride / dilation) and separable (T + 2 d <= 20).
constexpr int kEncLds = kEncCC * kEncMaxR * kEncMaxR;
constexpr int kEncSepLds = kEncCC * 20 * 20;

// The skip mask of the inference forwards (occ_encoder_forward_masked, occ_segment_forward_masked): skip = null, or one
// int32 per env; a block whose env has a non-zero entry returns at once, before any LDS access, barrier or memory access
// other than this one load, so a skipped env costs one block dispatch and one scalar load per block and writes nothing.
// The env index comes from the grid and the address is the same for the whole block: a scalar load and a uniform branch.
// TRAIN instantiations take no mask (their launchers pass null) and compile the test away.
template <bool TRAIN>
__device__ __forceinline__ bool enc_env_skipped(const int32_t* __restrict__ skip, unsigned env) {
    if constexpr (TRAIN) return false;
    else return skip != nullptr && skip[env] != 0;
}

// rkeep (TRAIN): (n, cout, H, W), where r is stored; not read otherwise.
template <int T, int COG, bool TRAIN = false>
__global__ __launch_bounds__(256) void occ_enc_sep_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          const float* __restrict__ resid, const float* __restrict__ w,
                                                          int cin, int cout, int H, int W, int d, int tiles_x,
                                                          float* __restrict__ rkeep, const int32_t* __restrict__ skip) {
    __shared__ float s[kEncSepLds];
    if (enc_env_skipped<TRAIN>(skip, blockIdx.z)) return;
    constexpr int TT = T * T;
    const int tid = threadIdx.x;
    const int p = tid % TT;
    const int ng = blockDim.x / TT;
    const int g = __builtin_amdgcn_readfirstlane(tid / TT);
    const int co0 = (blockIdx.y * ng + g) * COG;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const int oy0 = ty * T, ox0 = tx * T;
    const int py = p / T, px = p % T;
    const size_t plane = (size_t)H * W;
    const float* xe = x + (size_t)blockIdx.z * cin * plane;
    const float* wv = w;
    const float* wh = wv + 3 * cin;
    const float* pw = wh + 3 * cin;
    const float* bias = pw + (size_t)cin * cout;
    const float* bns = bias + cout;
    const float* bnt = bns + cout;
    const int R = T + 2 * d;
    const int RR = R * R;

    float acc[COG];
#pragma unroll
    for (int j = 0; j < COG; ++j) acc[j] = 0.f;

    for (int ci0 = 0; ci0 < cin; ci0 += kEncCC) {
        const int cc = min(kEncCC, cin - ci0);
        __syncthreads();
        for (int i = tid; i < cc * RR; i += blockDim.x) {
            const int c = i / RR, r = i - c * RR;
            const int ry = r / R, rx = r - ry * R;
            const int gy = oy0 - d + ry, gx = ox0 - d + rx;
            float v = 0.f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xe[(ci0 + c) * plane + (size_t)gy * W + gx];
            s[i] = v;
        }
        __syncthreads();
        for (int c = 0; c < cc; ++c) {
            const int ci = ci0 + c;
            const float* sc = s + c * RR + py * R + px;  // staged (py - d, px - d)
            float u = 0.f;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                // depthwise (3,1): the column px + (kh - 1) d of the vertical result (zero outside the image, as the
                // staged input is); then the (1,3) tap kh on it
                float t = 0.f;
#pragma unroll
                for (int kv = 0; kv < 3; ++kv) t = fmaf(wv[ci * 3 + kv], sc[(kv * d) * R + kh * d], t);
                u = fmaf(wh[ci * 3 + kh], t, u);
            }
            const float* pr = pw + (size_t)ci * cout + co0;
#pragma unroll
            for (int j = 0; j < COG; ++j) acc[j] = fmaf(pr[j], u, acc[j]);
        }
    }
    const int oy = oy0 + py, ox = ox0 + px;
    if (oy >= H || ox >= W) return;
    float* ye = y + (size_t)blockIdx.z * cout * plane + (size_t)oy * W + ox;
    const float* re = resid ? resid + (size_t)blockIdx.z * cout * plane + (size_t)oy * W + ox : nullptr;
    float* rk = TRAIN ? rkeep + (size_t)blockIdx.z * cout * plane + (size_t)oy * W + ox : nullptr;
#pragma unroll
    for (int j = 0; j < COG; ++j) {
        const int co = co0 + j;
        const float r = fmaxf(acc[j] + bias[co], 0.f);
        float v = fmaf(r, bns[co], bnt[co]);
        if (re) v += re[co * plane];
        if constexpr (TRAIN) rk[co * plane] = r;
        ye[co * plane] = v;
    }
}

// rkeep (TRAIN): (n, cout, Ho, Wo), where r is stored; not read otherwise.  TRAIN && POOL: y may be null (no output kept).
template <int T, int COG, bool POOL, bool KEEP = false, bool TRAIN = false>
__global__ __launch_bounds__(256) void occ_enc_dense_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            const float* __restrict__ resid, const float* __restrict__ w,
                                                            int cin, int cout, int H, int W, int Ho, int Wo, int stride,
                                                            int d, int tiles_x, float* __restrict__ partials,
                                                            float* __restrict__ rkeep, const int32_t* __restrict__ skip) {
    __shared__ float s[kEncLds];
    if (enc_env_skipped<TRAIN>(skip, blockIdx.z)) return;
    constexpr int TT = T * T;
    const int tid = threadIdx.x;
    const int p = tid % TT;
    const int ng = blockDim.x / TT;
    const int g = __builtin_amdgcn_readfirstlane(tid / TT);
    const int co0 = (blockIdx.y * ng + g) * COG;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const int oy0 = ty * T, ox0 = tx * T;
    const int py = p / T, px = p % T;
    const size_t plane = (size_t)H * W;
    const float* xe = x + (size_t)blockIdx.z * cin * plane;
    const float* bias = w + (size_t)cin * 9 * cout;
    const float* bns = bias + cout;
    const float* bnt = bns + cout;
    const int R = (T - 1) * stride + 2 * d + 1;
    const int RR = R * R;
    const int iy0 = oy0 * stride - d, ix0 = ox0 * stride - d;  // padding = dilation for k = 3

    float acc[COG];
#pragma unroll
    for (int j = 0; j < COG; ++j) acc[j] = 0.f;

    for (int ci0 = 0; ci0 < cin; ci0 += kEncCC) {
        const int cc = min(kEncCC, cin - ci0);
        __syncthreads();
        for (int i = tid; i < cc * RR; i += blockDim.x) {
            const int c = i / RR, r = i - c * RR;
            const int ry = r / R, rx = r - ry * R;
            const int gy = iy0 + ry, gx = ix0 + rx;
            float v = 0.f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xe[(ci0 + c) * plane + (size_t)gy * W + gx];
            s[i] = v;
        }
        __syncthreads();
        for (int c = 0; c < cc; ++c) {
            const int ci = ci0 + c;
            const float* sc = s + c * RR + (py * stride) * R + px * stride;
            float in[9];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) in[ky * 3 + kx] = sc[(ky * d) * R + kx * d];
            const float* wr = w + (size_t)ci * 9 * cout + co0;
#pragma unroll
            for (int k = 0; k < 9; ++k)
#pragma unroll
                for (int j = 0; j < COG; ++j) acc[j] = fmaf(wr[k * cout + j], in[k], acc[j]);
        }
    }
    const int oy = oy0 + py, ox = ox0 + px;
    const bool valid = oy < Ho && ox < Wo;
    const size_t oplane = (size_t)Ho * Wo;
    if constexpr (!POOL) {
        if (!valid) return;
        float* ye = y + (size_t)blockIdx.z * cout * oplane + (size_t)oy * Wo + ox;
        const float* re = resid ? resid + (size_t)blockIdx.z * cout * oplane + (size_t)oy * Wo + ox : nullptr;
        float* rk = TRAIN ? rkeep + (size_t)blockIdx.z * cout * oplane + (size_t)oy * Wo + ox : nullptr;
#pragma unroll
        for (int j = 0; j < COG; ++j) {
            const int co = co0 + j;
            const float r = fmaxf(acc[j] + bias[co], 0.f);
            float v = fmaf(r, bns[co], bnt[co]);
            if (re) v += re[co * oplane];
            if constexpr (TRAIN) rk[co * oplane] = r;
            ye[co * oplane] = v;
        }
    } else {
        // per-tile channel sums in a fixed order: every value goes to LDS, then one thread per channel adds the tile's
        // pixels in pixel order (pixels outside the output contribute exact zeros)
        static_assert(256 * COG <= kEncLds, "the pool stage reuses the LDS stage");
        __syncthreads();
#pragma unroll
        for (int j = 0; j < COG; ++j) {
            const int co = co0 + j;
            const float r = fmaxf(acc[j] + bias[co], 0.f);
            const float v = fmaf(r, bns[co], bnt[co]);
            s[(g * COG + j) * TT + p] = valid ? v : 0.f;
            if constexpr (KEEP) {
                if (valid) y[((size_t)blockIdx.z * cout + co) * oplane + (size_t)oy * Wo + ox] = v;
            }
            if constexpr (TRAIN) {
                if (valid) {
                    const size_t o = ((size_t)blockIdx.z * cout + co) * oplane + (size_t)oy * Wo + ox;
                    rkeep[o] = r;
                    if (y) y[o] = v;  // the joint training's decoder reads the last down's output
                }
            }
        }
        __syncthreads();
        if (tid < ng * COG) {
            const float* row = s + tid * TT;
            float sum = 0.f;
            for (int q = 0; q < TT; ++q) sum += row[q];
            const int gg = tid / COG, j = tid % COG;
            const int ntiles = gridDim.x;
            partials[((size_t)blockIdx.z * ntiles + blockIdx.x) * cout + (blockIdx.y * ng + gg) * COG + j] = sum;
        }
    }
}

// feats[n][c] = (sum over tiles t in order of partials[n][t][c]) / count
__global__ __launch_bounds__(kEncFeat) void occ_enc_pool_kernel(const float* __restrict__ partials, int ntiles, float count,
                                                                float* __restrict__ feats, const int32_t* __restrict__ skip) {
    if (enc_env_skipped<false>(skip, blockIdx.x)) return;
    const int c = threadIdx.x;
    const float* pe = partials + (size_t)blockIdx.x * ntiles * kEncFeat + c;
    float sum = 0.f;
    for (int t = 0; t < ntiles; ++t) sum += pe[(size_t)t * kEncFeat];
    feats[(size_t)blockIdx.x * kEncFeat + c] = sum / count;
}

// ---- host side: layer walk, packed sizes, launches -----------------------------------------------------------------

inline int enc_out_size(int h, int stride) { return stride == 1 ? h : (h + 1) / 2; }

// floats of one packed layer (header: occ_encoder_packed_floats)
inline long long enc_layer_floats(int cin, int cout, bool separable) {
    return separable ? 6LL * cin + (long long)cin * cout + 3LL * cout : 9LL * cin * cout + 3LL * cout;
}

inline long long enc_packed_floats(bool separable) {
    long long n = enc_layer_floats(4, kEncCh, separable);
    for (int lv = 0; lv < kEncLevels; ++lv) {
        const int c = kEncCh << lv;
        n += 2 * enc_layer_floats(c, c, separable) + enc_layer_floats(c, 2 * c, false);
    }
    return n;
}

inline int enc_tile(int ho) { return ho >= 16 ? 16 : 8; }
inline int enc_cog(int cout) { return cout >= 32 ? 32 : cout; }
inline int enc_groups(int T, int cout) {  // channel groups per block: 256 threads at most
    if (T == 16) return 1;
    const int ng = cout / enc_cog(cout);
    return ng < 4 ? ng : 4;
}
// Grid and block of the kernels whose thread owns one pixel (or quad) of a T x T tile for one of `groups` channel groups
// (the decoder's up layers and every input gradient): T == 16: one group per block, 256 threads; T == 8: up to 4 groups,
// 64 ng threads.  The conv forwards differ (enc_groups: the groups depend on COG).
struct TileLaunch {
    int tiles_x;
    dim3 grid, block;
};
inline TileLaunch tile_launch(int T, int side, int groups, int n) {
    const int tiles_x = (side + T - 1) / T;
    const int ng = T == 16 ? 1 : groups < 4 ? groups : 4;
    return {tiles_x, dim3(tiles_x * tiles_x, groups / ng, n), dim3(T == 16 ? 256 : 64 * ng)};
}
inline int enc_tiles(int ho) {
    const int T = enc_tile(ho);
    const int t = (ho + T - 1) / T;
    return t * t;
}

inline size_t enc_align(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace: three activation buffers of the level-0 size (n, 8, S, S) and the partials (n, tiles of the last down, 256)
inline void enc_ws_layout(int img, int n, size_t* buf_bytes, size_t* part_bytes) {
    *buf_bytes = enc_align((size_t)n * kEncCh * img * img * sizeof(float));
    int h = img;
    for (int lv = 0; lv < kEncLevels; ++lv) h = enc_out_size(h, 2);
    *part_bytes = enc_align((size_t)n * enc_tiles(h) * kEncFeat * sizeof(float));
}

// The launchers of one layer.  rkeep = null: inference.  rkeep given (the training forwards, occ_encoder_bwd.hpp): the TRAIN
// instantiation on the same grid, which also stores r there.
template <int T, bool TRAIN>
static void enc_launch_sep_t(const float* x, float* y, const float* resid, const float* w, int cin, int cout, int H, int d,
                             int n, hipStream_t st, float* rkeep, const int32_t* skip) {
    const int cog = enc_cog(cout), ng = enc_groups(T, cout);
    const int tiles_x = (H + T - 1) / T;
    const dim3 grid(tiles_x * tiles_x, cout / (cog * ng), n), block(T * T * ng);
#define OCC_ENC_SEP(COG) \
    hipLaunchKernelGGL((occ_enc_sep_kernel<T, COG, TRAIN>), grid, block, 0, st, x, y, resid, w, cin, cout, H, H, d, tiles_x, rkeep, skip)
    if (cog == 8) OCC_ENC_SEP(8);
    else if (cog == 16) OCC_ENC_SEP(16);
    else OCC_ENC_SEP(32);
#undef OCC_ENC_SEP
}

static void enc_launch_sep(const float* x, float* y, const float* resid, const float* w, int cin, int cout, int H, int d, int n,
                           hipStream_t st, float* rkeep = nullptr, const int32_t* skip = nullptr) {
    const bool t16 = enc_tile(H) == 16;
    if (rkeep) t16 ? enc_launch_sep_t<16, true>(x, y, resid, w, cin, cout, H, d, n, st, rkeep, nullptr)
                   : enc_launch_sep_t<8, true>(x, y, resid, w, cin, cout, H, d, n, st, rkeep, nullptr);
    else t16 ? enc_launch_sep_t<16, false>(x, y, resid, w, cin, cout, H, d, n, st, nullptr, skip)
             : enc_launch_sep_t<8, false>(x, y, resid, w, cin, cout, H, d, n, st, nullptr, skip);
}

// keep (inference, with partials): the last down also stores its output.  With rkeep it does so where y is not null.
template <int T, bool TRAIN>
static void enc_launch_dense_t(const float* x, float* y, const float* resid, const float* w, int cin, int cout, int H, int stride,
                               int d, int n, float* partials, bool keep, hipStream_t st, float* rkeep, const int32_t* skip) {
    const int Ho = enc_out_size(H, stride);
    const int cog = enc_cog(cout), ng = enc_groups(T, cout);
    const int tiles_x = (Ho + T - 1) / T;
    const dim3 grid(tiles_x * tiles_x, cout / (cog * ng), n), block(T * T * ng);
#define OCC_ENC_DENSE(COG, POOL, KEEP)                                                                                          \
    hipLaunchKernelGGL((occ_enc_dense_kernel<T, COG, POOL, KEEP, TRAIN>), grid, block, 0, st, x, y, resid, w, cin, cout, H, H, Ho, Ho, \
                       stride, d, tiles_x, partials, rkeep, skip)
    if (partials) {  // the last down: cout = 256
        if constexpr (TRAIN) OCC_ENC_DENSE(32, true, false);
        else if (keep) OCC_ENC_DENSE(32, true, true);
        else OCC_ENC_DENSE(32, true, false);
    } else if (cog == 8) OCC_ENC_DENSE(8, false, false);
    else if (cog == 16) OCC_ENC_DENSE(16, false, false);
    else OCC_ENC_DENSE(32, false, false);
#undef OCC_ENC_DENSE
}

static void enc_launch_dense(const float* x, float* y, const float* resid, const float* w, int cin, int cout, int H, int stride,
                             int d, int n, float* partials, hipStream_t st, bool keep = false, float* rkeep = nullptr,
                             const int32_t* skip = nullptr) {
    const bool t16 = enc_tile(enc_out_size(H, stride)) == 16;
    if (rkeep) t16 ? enc_launch_dense_t<16, true>(x, y, resid, w, cin, cout, H, stride, d, n, partials, keep, st, rkeep, nullptr)
                   : enc_launch_dense_t<8, true>(x, y, resid, w, cin, cout, H, stride, d, n, partials, keep, st, rkeep, nullptr);
    else t16 ? enc_launch_dense_t<16, false>(x, y, resid, w, cin, cout, H, stride, d, n, partials, keep, st, nullptr, skip)
             : enc_launch_dense_t<8, false>(x, y, resid, w, cin, cout, H, stride, d, n, partials, keep, st, nullptr, skip);
}

// The whole encoder on n envs: 17 launches (the initial layer, two layers and a down per level, the pool).
// keep = null (occ_encoder_forward): ws holds b0, b1, b2 and the partials.  keep = the five skip tensors and the last
// down output (occ_segment_forward, occ_decoder.hpp): ws holds b0, b1 and the partials; every level's Layer 2 writes its
// skip tensor instead of b2 and the last down also stores its output.  The same kernels run on the same values in the
// same order either way, so the pooled feature is the same to the bit.
// skip = null, or the env mask (enc_env_skipped): the same 17 launches on the same grids; the blocks of a skipped env return
// at once, so its feats row and its part of every buffer keep what they held.
struct EncKeep {
    float* skip[kEncLevels];  // (n, 8 << lv, S >> lv, S >> lv): Layer 2 (+ residual), what the down conv reads
    float* last;              // (n, 256, S / 32, S / 32)
};

static void enc_forward(int img, int dil, bool residual, bool separable, const float* packed, const float* obs, int n, char* ws,
                        float* feats, hipStream_t st, const EncKeep* keep = nullptr, const int32_t* skip = nullptr) {
    size_t buf_bytes, part_bytes;
    enc_ws_layout(img, n, &buf_bytes, &part_bytes);
    float* b0 = (float*)ws;
    float* b1 = (float*)(ws + buf_bytes);
    float* b2 = keep ? nullptr : (float*)(ws + 2 * buf_bytes);
    float* part = (float*)(ws + (keep ? 2 : 3) * buf_bytes);
    const float* w = packed;
    int H = img;
    // initial: Conv(4 -> 8) with dilation 1 (model.py:92)
    if (separable) enc_launch_sep(obs, b0, nullptr, w, 4, kEncCh, H, 1, n, st, nullptr, skip);
    else enc_launch_dense(obs, b0, nullptr, w, 4, kEncCh, H, 1, 1, n, nullptr, st, false, nullptr, skip);
    w += enc_layer_floats(4, kEncCh, separable);
    for (int lv = 0; lv < kEncLevels; ++lv) {
        const int c = kEncCh << lv;
        if (keep) b2 = keep->skip[lv];
        // Layer 1: b0 -> b1; Layer 2: b1 (+ b0) -> b2; down: b2 -> b0 (or the partials of the pooled feature)
        if (separable) enc_launch_sep(b0, b1, nullptr, w, c, c, H, dil, n, st, nullptr, skip);
        else enc_launch_dense(b0, b1, nullptr, w, c, c, H, 1, dil, n, nullptr, st, false, nullptr, skip);
        w += enc_layer_floats(c, c, separable);
        if (separable) enc_launch_sep(b1, b2, residual ? b0 : nullptr, w, c, c, H, dil, n, st, nullptr, skip);
        else enc_launch_dense(b1, b2, residual ? b0 : nullptr, w, c, c, H, 1, dil, n, nullptr, st, false, nullptr, skip);
        w += enc_layer_floats(c, c, separable);
        const bool last = lv == kEncLevels - 1;
        enc_launch_dense(b2, last && keep ? keep->last : b0, nullptr, w, c, 2 * c, H, 2, 1, n, last ? part : nullptr, st,
                         last && keep, nullptr, skip);
        w += enc_layer_floats(c, 2 * c, false);
        H = enc_out_size(H, 2);
    }
    hipLaunchKernelGGL(occ_enc_pool_kernel, dim3(n), dim3(kEncFeat), 0, st, part, enc_tiles(H), (float)(H * H), feats, skip);
}
