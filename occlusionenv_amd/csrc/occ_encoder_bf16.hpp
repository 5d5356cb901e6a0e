// occ_encoder_bf16.hpp -- bf16 inference of the frozen SEPARABLE encoder (occ_encoder.hpp is the f32 path and the contract of
// the network; this file adds a mode and changes nothing there).  Part of the single translation unit occ_kernels.hip.
//
// Where values are rounded (round = to nearest even, to bfloat16); everything else is f32:
//   * contraction operands: the depthwise pair's result h (formed in f32 in the thread, as in occ_enc_sep_kernel, then
//     rounded), the pointwise weights and the dense down weights (rounded on the host, occ_encoder_bf16_pack);
//   * stored activations: relu(u) * s + t (+ the residual, read back as bf16 and added in f32), rounded once at the store.
// The observation, the depthwise taps, biases, BN scale / shift, accumulators, epilogues, pool partials and feats are f32.
// The last down stores nothing: its partials are fixed-order sums of the unrounded epilogue values; occ_enc_pool_kernel
// finishes them.  No atomics; nothing depends on the batch size or on an env's position; 17 launches, as the f32 path.
//
// Activations are channel-last: (n, H, W, c) bf16, so a pixel's 8 consecutive channels are one 16-byte access and, in LDS,
// one ds_read_b128 that is already an MFMA operand fragment.
//
//   occ_enc16_init_kernel   initial separable Conv(4 -> 8) on the f32 planar observation          VALU (cin = 4)
//   occ_enc16_sep8_kernel   level 0's separable Conv(8 -> 8)                                      VALU (bandwidth-bound)
//   occ_enc16_down8_kernel  level 0's down Conv(8 -> 16), K = 72                                  VALU (bandwidth-bound)
//   occ_enc16_sep_kernel    separable Conv(c -> c), c = 16..128: the whole halo tile (all channels) staged in LDS once; lane
//                           (r, h) of a wave forms h for pixel r and the 8 channels 16 kb + 8 h.. in registers, packs them
//                           (v_cvt_pk_bf16_f32) as the B fragment of v_mfma_f32_32x32x16_bf16; A = the weight fragment,
//                           one 16-byte load in the packed order.  D: lane (r, h) holds pixel r, channels 32 ct + 16 h + reg
//                           (the pack permutes the weight rows so), i.e. two 16-byte stores per pixel and ct.
//   occ_enc16_down_kernel   down Conv(c -> 2c), c = 16..128, K = 9 c ordered (tap, channel): the B fragment is a staged
//                           pixel's 16 bytes as they lie in LDS, no VALU work.  POOL (c = 128): partials instead of a store.
//
// MFMA lane maps (32x32x16 bf16): lane l, r = l & 31, h = l >> 5: A[row r][k = 8 h + j], B[k = 8 h + j][col r], j = 0..7;
// D[row (reg & 3) + 8 (reg >> 2) + 4 h][col r], reg = 0..15.  Weight row m of a 32-row tile ct is output channel
// 32 ct + 16 ((m >> 2) & 1) + 4 (m >> 3) + (m & 3), which makes D's reg the channel offset inside the lane's 16.

typedef __bf16 enc16_frag __attribute__((ext_vector_type(8)));
typedef __bf16 enc16_bf2 __attribute__((ext_vector_type(2)));
typedef float enc16_f2 __attribute__((ext_vector_type(2)));
typedef float enc16_acc __attribute__((ext_vector_type(16)));

// two f32 -> two bf16 (RNE) in one word, low half first
__device__ __forceinline__ uint32_t enc16_pack2(float a, float b) {
    enc16_f2 f = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, enc16_bf2));
}
__device__ __forceinline__ float enc16_round(float a) { return __uint_as_float(enc16_pack2(a, 0.f) << 16); }
__device__ __forceinline__ uint4 enc16_pack8(const float* v) {
    return make_uint4(enc16_pack2(v[0], v[1]), enc16_pack2(v[2], v[3]), enc16_pack2(v[4], v[5]), enc16_pack2(v[6], v[7]));
}
__device__ __forceinline__ void enc16_unpack8(uint4 q, float* v) {
    v[0] = __uint_as_float(q.x << 16), v[1] = __uint_as_float(q.x & 0xffff0000u);
    v[2] = __uint_as_float(q.y << 16), v[3] = __uint_as_float(q.y & 0xffff0000u);
    v[4] = __uint_as_float(q.z << 16), v[5] = __uint_as_float(q.z & 0xffff0000u);
    v[6] = __uint_as_float(q.w << 16), v[7] = __uint_as_float(q.w & 0xffff0000u);
}

// ---- level 0 on the VALU ---------------------------------------------------------------------------------------------------
// These three read their layer in the f32 layout of occ_encoder.hpp (the contraction weights hold bf16 values widened to f32).

// y (n, H, W, 8) bf16 = initial layer of x (n, 4, H, W) f32; 16 x 16 pixels per block, dilation 1
__global__ __launch_bounds__(256) void occ_enc16_init_kernel(const float* __restrict__ x, uint4* __restrict__ y,
                                                             const float* __restrict__ w, int H, int W, int tiles_x,
                                                             const int32_t* __restrict__ skip) {
    constexpr int T = 16, R = T + 2, RR = R * R, CIN = 4, CO = 8;
    __shared__ float s[CIN * RR];
    if (enc_env_skipped<false>(skip, blockIdx.z)) return;
    const int tid = threadIdx.x;
    const int oy0 = (blockIdx.x / tiles_x) * T, ox0 = (blockIdx.x % tiles_x) * T;
    const int py = tid / T, px = tid % T;
    const size_t plane = (size_t)H * W;
    const float* xe = x + (size_t)blockIdx.z * CIN * plane;
    const float* wv = w;
    const float* wh = wv + 3 * CIN;
    const float* pw = wh + 3 * CIN;
    const float* bias = pw + CIN * CO;
    const float* bns = bias + CO;
    const float* bnt = bns + CO;
    for (int i = tid; i < CIN * RR; i += 256) {
        const int c = i / RR, r = i - c * RR;
        const int ry = r / R, rx = r - ry * R;
        const int gy = oy0 - 1 + ry, gx = ox0 - 1 + rx;
        float v = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xe[c * plane + (size_t)gy * W + gx];
        s[i] = v;
    }
    __syncthreads();
    float acc[CO];
#pragma unroll
    for (int j = 0; j < CO; ++j) acc[j] = 0.f;
#pragma unroll
    for (int c = 0; c < CIN; ++c) {
        const float* sc = s + c * RR + py * R + px;
        float u = 0.f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            float t = 0.f;
#pragma unroll
            for (int kv = 0; kv < 3; ++kv) t = fmaf(wv[c * 3 + kv], sc[kv * R + kh], t);
            u = fmaf(wh[c * 3 + kh], t, u);
        }
        u = enc16_round(u);
#pragma unroll
        for (int j = 0; j < CO; ++j) acc[j] = fmaf(pw[c * CO + j], u, acc[j]);
    }
    const int oy = oy0 + py, ox = ox0 + px;
    if (oy >= H || ox >= W) return;
    float v[CO];
#pragma unroll
    for (int j = 0; j < CO; ++j) v[j] = fmaf(fmaxf(acc[j] + bias[j], 0.f), bns[j], bnt[j]);
    y[(size_t)blockIdx.z * plane + (size_t)oy * W + ox] = enc16_pack8(v);
}

// y = separable Conv(8 -> 8) of x, both (n, H, W, 8) bf16; resid: null or (n, H, W, 8) bf16
__global__ __launch_bounds__(256) void occ_enc16_sep8_kernel(const uint4* __restrict__ x, uint4* __restrict__ y,
                                                             const uint4* __restrict__ resid, const float* __restrict__ w, int H,
                                                             int W, int d, int tiles_x, const int32_t* __restrict__ skip) {
    constexpr int T = 16, C = 8;
    __shared__ uint4 s[(T + 4) * (T + 4)];
    if (enc_env_skipped<false>(skip, blockIdx.z)) return;
    const int tid = threadIdx.x;
    const int oy0 = (blockIdx.x / tiles_x) * T, ox0 = (blockIdx.x % tiles_x) * T;
    const int py = tid / T, px = tid % T;
    const size_t plane = (size_t)H * W;
    const uint4* xe = x + (size_t)blockIdx.z * plane;
    const float* wv = w;
    const float* wh = wv + 3 * C;
    const float* pw = wh + 3 * C;
    const float* bias = pw + C * C;
    const float* bns = bias + C;
    const float* bnt = bns + C;
    const int R = T + 2 * d;
    for (int i = tid; i < R * R; i += 256) {
        const int ry = i / R, rx = i - ry * R;
        const int gy = oy0 - d + ry, gx = ox0 - d + rx;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xe[(size_t)gy * W + gx];
        s[i] = v;
    }
    __syncthreads();
    const uint4* sc = s + py * R + px;  // staged (py - d, px - d)
    float u[C];
#pragma unroll
    for (int c = 0; c < C; ++c) u[c] = 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        float t[C];
#pragma unroll
        for (int c = 0; c < C; ++c) t[c] = 0.f;
#pragma unroll
        for (int kv = 0; kv < 3; ++kv) {
            float in[C];
            enc16_unpack8(sc[(kv * d) * R + kh * d], in);
#pragma unroll
            for (int c = 0; c < C; ++c) t[c] = fmaf(wv[c * 3 + kv], in[c], t[c]);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) u[c] = fmaf(wh[c * 3 + kh], t[c], u[c]);
    }
    float acc[C];
#pragma unroll
    for (int j = 0; j < C; ++j) acc[j] = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float ub = enc16_round(u[c]);
#pragma unroll
        for (int j = 0; j < C; ++j) acc[j] = fmaf(pw[c * C + j], ub, acc[j]);
    }
    const int oy = oy0 + py, ox = ox0 + px;
    if (oy >= H || ox >= W) return;
    const size_t o = (size_t)blockIdx.z * plane + (size_t)oy * W + ox;
    float v[C];
#pragma unroll
    for (int j = 0; j < C; ++j) v[j] = fmaf(fmaxf(acc[j] + bias[j], 0.f), bns[j], bnt[j]);
    if (resid) {
        float r[C];
        enc16_unpack8(resid[o], r);
#pragma unroll
        for (int j = 0; j < C; ++j) v[j] += r[j];
    }
    y[o] = enc16_pack8(v);
}

// y (n, Ho, Wo, 16) bf16 = dense 3x3 stride-2 Conv(8 -> 16) of x (n, H, W, 8) bf16
__global__ __launch_bounds__(256) void occ_enc16_down8_kernel(const uint4* __restrict__ x, uint4* __restrict__ y,
                                                              const float* __restrict__ w, int H, int W, int Ho, int Wo,
                                                              int tiles_x, const int32_t* __restrict__ skip) {
    constexpr int T = 16, R = 2 * T + 1, C = 8, CO = 16;
    __shared__ uint4 s[R * R];
    if (enc_env_skipped<false>(skip, blockIdx.z)) return;
    const int tid = threadIdx.x;
    const int oy0 = (blockIdx.x / tiles_x) * T, ox0 = (blockIdx.x % tiles_x) * T;
    const int py = tid / T, px = tid % T;
    const uint4* xe = x + (size_t)blockIdx.z * H * W;
    const float* bias = w + C * 9 * CO;
    const float* bns = bias + CO;
    const float* bnt = bns + CO;
    const int iy0 = oy0 * 2 - 1, ix0 = ox0 * 2 - 1;
    for (int i = tid; i < R * R; i += 256) {
        const int ry = i / R, rx = i - ry * R;
        const int gy = iy0 + ry, gx = ix0 + rx;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xe[(size_t)gy * W + gx];
        s[i] = v;
    }
    __syncthreads();
    const uint4* sc = s + (py * 2) * R + px * 2;
    float acc[CO];
#pragma unroll
    for (int j = 0; j < CO; ++j) acc[j] = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        float in[C];
        enc16_unpack8(sc[(k / 3) * R + k % 3], in);
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int j = 0; j < CO; ++j) acc[j] = fmaf(w[(c * 9 + k) * CO + j], in[c], acc[j]);
    }
    const int oy = oy0 + py, ox = ox0 + px;
    if (oy >= Ho || ox >= Wo) return;
    float v[CO];
#pragma unroll
    for (int j = 0; j < CO; ++j) v[j] = fmaf(fmaxf(acc[j] + bias[j], 0.f), bns[j], bnt[j]);
    uint4* ye = y + (((size_t)blockIdx.z * Ho + oy) * Wo + ox) * 2;
    ye[0] = enc16_pack8(v);
    ye[1] = enc16_pack8(v + 8);
}

// ---- levels 1-4 on the matrix cores ------------------------------------------------------------------------------------------

constexpr int enc16_cpad(int c) { return c < 32 ? 32 : c; }  // output channels padded to whole 32-row weight tiles

// The epilogue of one D tile: the lane's pixel, its 16 channels co.. of a (.., cout) bf16 tensor at pixel offset `pix`.
__device__ __forceinline__ void enc16_epilogue(const enc16_acc& acc, const float* __restrict__ bias, int cout, int co, float* v) {
    const float4* b4 = (const float4*)(bias + co);
    const float4* s4 = (const float4*)(bias + cout + co);
    const float4* t4 = (const float4*)(bias + 2 * cout + co);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 b = b4[q], sc = s4[q], sh = t4[q];
        v[4 * q + 0] = fmaf(fmaxf(acc[4 * q + 0] + b.x, 0.f), sc.x, sh.x);
        v[4 * q + 1] = fmaf(fmaxf(acc[4 * q + 1] + b.y, 0.f), sc.y, sh.y);
        v[4 * q + 2] = fmaf(fmaxf(acc[4 * q + 2] + b.z, 0.f), sc.z, sh.z);
        v[4 * q + 3] = fmaf(fmaxf(acc[4 * q + 3] + b.w, 0.f), sc.w, sh.w);
    }
}

// y = separable Conv(C -> C) of x, both (n, H, W, C) bf16; resid: null or (n, H, W, C) bf16.  T x T pixels per block,
// 32 pixels (2 rows of 16, or 4 of 8) per wave and pass.  w: dw[C/16][2][6][8] f32 (per 8-channel group the taps
// v0 v1 v2 h0 h1 h2) | weight fragments [C/16][CP/32][64 lanes][8] bf16 | bias | bn_scale | bn_shift [C] f32.
template <int C, int T>
__global__ __launch_bounds__(T == 16 ? 256 : 128) void occ_enc16_sep_kernel(const uint4* __restrict__ x, uint4* __restrict__ y,
                                                                            const uint4* __restrict__ resid,
                                                                            const char* __restrict__ w, int H, int W, int d,
                                                                            int tiles_x, const int32_t* __restrict__ skip) {
    constexpr int C8 = C / 8, PS = C8 + 1;  // 16-byte words per pixel; LDS pixel stride (one word of padding: no bank conflicts)
    constexpr int NCT = enc16_cpad(C) / 32, NKB = C / 16;
    constexpr int NT = T == 16 ? 256 : 128;
    __shared__ uint4 s[(T + 4) * (T + 4) * PS];
    if (enc_env_skipped<false>(skip, blockIdx.z)) return;
    const int tid = threadIdx.x;
    const int oy0 = (blockIdx.x / tiles_x) * T, ox0 = (blockIdx.x % tiles_x) * T;
    const size_t plane = (size_t)H * W;
    const uint4* xe = x + (size_t)blockIdx.z * plane * C8;
    const int R = T + 2 * d;
    for (int i = tid; i < R * R * C8; i += NT) {
        const int pix = i / C8, c8 = i - pix * C8;
        const int ry = pix / R, rx = pix - ry * R;
        const int gy = oy0 - d + ry, gx = ox0 - d + rx;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xe[((size_t)gy * W + gx) * C8 + c8];
        s[pix * PS + c8] = v;
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const float4* dw = (const float4*)w;
    const uint4* frag = (const uint4*)(w + 6 * C * sizeof(float));
    const float* bias = (const float*)(w + 6 * C * sizeof(float) + (size_t)C * enc16_cpad(C) * 2);
#pragma unroll 1
    for (int pg = wave; pg < T * T / 32; pg += NT / 64) {
        const int p = pg * 32 + r;
        const int py = p / T, px = p % T;
        enc16_acc acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[ct][i] = 0.f;
#pragma unroll 1
        for (int kb = 0; kb < NKB; ++kb) {
            // the depthwise pair for the channels 16 kb + 8 h .. + 7 of this lane's pixel
            float tw[6][8];
            const float4* dwl = dw + (kb * 2 + h) * 12;
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const float4 a = dwl[2 * q], b = dwl[2 * q + 1];
                tw[q][0] = a.x, tw[q][1] = a.y, tw[q][2] = a.z, tw[q][3] = a.w;
                tw[q][4] = b.x, tw[q][5] = b.y, tw[q][6] = b.z, tw[q][7] = b.w;
            }
            const uint4* sc = s + (py * R + px) * PS + kb * 2 + h;
            float u[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) u[c] = 0.f;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                float t[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) t[c] = 0.f;
#pragma unroll
                for (int kv = 0; kv < 3; ++kv) {
                    float in[8];
                    enc16_unpack8(sc[((kv * d) * R + kh * d) * PS], in);
#pragma unroll
                    for (int c = 0; c < 8; ++c) t[c] = fmaf(tw[kv][c], in[c], t[c]);
                }
#pragma unroll
                for (int c = 0; c < 8; ++c) u[c] = fmaf(tw[3 + kh][c], t[c], u[c]);
            }
            const enc16_frag b = __builtin_bit_cast(enc16_frag, enc16_pack8(u));
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const enc16_frag a = __builtin_bit_cast(enc16_frag, frag[(kb * NCT + ct) * 64 + lane]);
                acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[ct], 0, 0, 0);
            }
        }
        const int oy = oy0 + py, ox = ox0 + px;
        if (oy >= H || ox >= W) continue;
        if (C < 32 && h != 0) continue;  // the padded half of the only weight tile
        const size_t o = ((size_t)blockIdx.z * plane + (size_t)oy * W + ox) * C8;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const int co = ct * 32 + 16 * h;
            float v[16];
            enc16_epilogue(acc[ct], bias, C, co, v);
            if (resid) {
                float rr[16];
                enc16_unpack8(resid[o + co / 8], rr);
                enc16_unpack8(resid[o + co / 8 + 1], rr + 8);
#pragma unroll
                for (int i = 0; i < 16; ++i) v[i] += rr[i];
            }
            y[o + co / 8] = enc16_pack8(v);
            y[o + co / 8 + 1] = enc16_pack8(v + 8);
        }
    }
}

// y (n, Ho, Wo, 2C) bf16 = dense 3x3 stride-2 Conv(C -> 2C) of x (n, H, W, C) bf16; 8 x 8 output pixels (two 32-pixel
// groups) per block of four waves.  From 128 output channels up a wave owns every fourth weight tile for both pixel groups
// (each weight fragment feeds two MFMAs); below, a wave owns one (group, tile) pair.  The input tile is staged min(C, 64)
// channels at a time.  w: weight fragments [9 C / 16][2C / 32][64 lanes][8] bf16, k = tap * C + channel | bias | bn_scale |
// bn_shift [2C] f32.  POOL (C = 128): nothing is stored; partials (n, tiles, 256) receives per channel the sum over the
// tile's 64 pixels in pixel order (pixels outside the output are exact zeros).
template <int C, bool POOL>
__global__ __launch_bounds__(256) void occ_enc16_down_kernel(const uint4* __restrict__ x, uint4* __restrict__ y,
                                                             const char* __restrict__ w, int H, int W, int Ho, int Wo,
                                                             int tiles_x, float* __restrict__ partials,
                                                             const int32_t* __restrict__ skip) {
    constexpr int T = 8, R = 2 * T + 1, CO = 2 * C, C8 = C / 8;
    constexpr int CC = C < 64 ? C : 64, PS = CC / 8 + 1;  // staged channels; LDS pixel stride in 16-byte words
    constexpr int NCT = CO / 32, NKC = C / 16;
    constexpr bool WIDE = NCT >= 4;
    constexpr int NPW = WIDE ? NCT / 4 : 1, GP = WIDE ? 2 : 1;  // weight tiles and pixel groups per wave
    constexpr int kPoolRow = 65;                                   // 64 pixels + 1: the channel sums read conflict-free
    constexpr int kStage = R * R * PS, kPool = POOL ? 4 * 32 * kPoolRow / 4 : 0;
    __shared__ uint4 s[kStage > kPool ? kStage : kPool];
    if (enc_env_skipped<false>(skip, blockIdx.z)) return;
    const int tid = threadIdx.x;
    const int oy0 = (blockIdx.x / tiles_x) * T, ox0 = (blockIdx.x % tiles_x) * T;
    const uint4* xe = x + (size_t)blockIdx.z * H * W * C8;
    const int iy0 = oy0 * 2 - 1, ix0 = ox0 * 2 - 1;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const uint4* frag = (const uint4*)w;
    const float* bias = (const float*)(w + (size_t)9 * C * CO * 2);
    const int ct0 = WIDE ? wave : wave >> 1;
    const bool active = ct0 < NCT;
    int spix[GP];  // the staged pixel of tap (0, 0) of each of this wave's output pixels
#pragma unroll
    for (int g = 0; g < GP; ++g) {
        const int p = (WIDE ? g : wave & 1) * 32 + r;
        spix[g] = ((p / T) * 2) * R + (p % T) * 2;
    }
    enc16_acc acc[NPW][GP];
#pragma unroll
    for (int j = 0; j < NPW; ++j)
#pragma unroll
        for (int g = 0; g < GP; ++g)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][g][i] = 0.f;

    for (int c0 = 0; c0 < C; c0 += CC) {
        if (c0) __syncthreads();
        for (int i = tid; i < R * R * (CC / 8); i += 256) {
            const int pix = i / (CC / 8), c8 = i - pix * (CC / 8);
            const int ry = pix / R, rx = pix - ry * R;
            const int gy = iy0 + ry, gx = ix0 + rx;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xe[((size_t)gy * W + gx) * C8 + c0 / 8 + c8];
            s[pix * PS + c8] = v;
        }
        __syncthreads();
        if (active) {
            for (int tap = 0; tap < 9; ++tap) {
                const int toff = (tap / 3) * R + tap % 3;
#pragma unroll
                for (int cb = 0; cb < CC / 16; ++cb) {
                    const int kb = tap * NKC + c0 / 16 + cb;
                    enc16_frag b[GP];
#pragma unroll
                    for (int g = 0; g < GP; ++g) b[g] = __builtin_bit_cast(enc16_frag, s[(spix[g] + toff) * PS + cb * 2 + h]);
#pragma unroll
                    for (int j = 0; j < NPW; ++j) {
                        const enc16_frag a = __builtin_bit_cast(enc16_frag, frag[((size_t)kb * NCT + ct0 + 4 * j) * 64 + lane]);
#pragma unroll
                        for (int g = 0; g < GP; ++g) acc[j][g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[g], acc[j][g], 0, 0, 0);
                    }
                }
            }
        }
    }
    if constexpr (!POOL) {
        if (!active) return;
#pragma unroll
        for (int g = 0; g < GP; ++g) {
            const int p = (WIDE ? g : wave & 1) * 32 + r;
            const int oy = oy0 + p / T, ox = ox0 + p % T;
            if (oy >= Ho || ox >= Wo) continue;
            uint4* ye = y + (((size_t)blockIdx.z * Ho + oy) * Wo + ox) * (CO / 8);
#pragma unroll
            for (int j = 0; j < NPW; ++j) {
                const int co = (ct0 + 4 * j) * 32 + 16 * h;
                float v[16];
                enc16_epilogue(acc[j][g], bias, CO, co, v);
                ye[co / 8] = enc16_pack8(v);
                ye[co / 8 + 1] = enc16_pack8(v + 8);
            }
        }
    } else {
        static_assert(!POOL || (WIDE && GP == 2), "the pooled down is the wide form");
        float* sp = (float*)s + wave * 32 * kPoolRow;  // this wave's [32 channels][64 pixels (+1)]
#pragma unroll
        for (int j = 0; j < NPW; ++j) {
            const int ct = ct0 + 4 * j;
            __syncthreads();  // the stage (j = 0) or the previous tile's sums have been read
#pragma unroll
            for (int g = 0; g < GP; ++g) {
                const int p = g * 32 + r;
                const bool valid = oy0 + p / T < Ho && ox0 + p % T < Wo;
                float v[16];
                enc16_epilogue(acc[j][g], bias, CO, ct * 32 + 16 * h, v);
#pragma unroll
                for (int i = 0; i < 16; ++i) sp[(16 * h + i) * kPoolRow + p] = valid ? v[i] : 0.f;
            }
            __syncthreads();
            if (lane < 32) {
                const float* row = sp + lane * kPoolRow;
                float sum = 0.f;
                for (int q = 0; q < 64; ++q) sum += row[q];
                partials[((size_t)blockIdx.z * gridDim.x + blockIdx.x) * CO + ct * 32 + lane] = sum;
            }
        }
    }
}

// ---- host side: packed layout, workspace, launches -------------------------------------------------------------------------------

// bytes of one packed layer (header: occ_encoder_bf16_packed_bytes).  cin <= 8: the f32 layout.
inline long long enc16_layer_bytes(int cin, int cout, bool sep) {
    if (cin <= 8) return 4 * enc_layer_floats(cin, cout, sep);
    return sep ? 24LL * cin + 2LL * cin * enc16_cpad(cout) + 12LL * cout : 18LL * cin * cout + 12LL * cout;
}

inline long long enc16_packed_bytes() {
    long long n = enc16_layer_bytes(4, kEncCh, true);
    for (int lv = 0; lv < kEncLevels; ++lv) {
        const int c = kEncCh << lv;
        n += 2 * enc16_layer_bytes(c, c, true) + enc16_layer_bytes(c, 2 * c, false);
    }
    return n;
}

// f32 -> bf16 bits, round to nearest even, in integer arithmetic (a NaN stays a quiet NaN)
inline uint16_t enc16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float enc16_widen(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// output channel of weight row m of tile ct (see the lane maps above)
inline int enc16_row_channel(int ct, int m) { return ct * 32 + 16 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3); }

// One layer: src in the f32 layout of occ_encoder.hpp -> dst.  Host only.
inline void enc16_pack_layer(const float* src, char* dst, int cin, int cout, bool sep) {
    const long long nw = sep ? (long long)cin * cout : 9LL * cin * cout;  // contraction weights
    const float* wsrc = sep ? src + 6 * cin : src;
    if (cin <= 8) {
        float* o = (float*)dst;
        const long long total = enc_layer_floats(cin, cout, sep);
        memcpy(o, src, (size_t)total * 4);
        float* wdst = sep ? o + 6 * cin : o;
        for (long long i = 0; i < nw; ++i) wdst[i] = enc16_widen(enc16_rne(wsrc[i]));
        return;
    }
    const int nct = enc16_cpad(cout) / 32;
    uint16_t* fr;
    int nkb;
    if (sep) {
        float* dwo = (float*)dst;  // [kb][half][v0 v1 v2 h0 h1 h2][8]
        for (int ci = 0; ci < cin; ++ci)
            for (int q = 0; q < 6; ++q) dwo[(ci / 8) * 48 + q * 8 + ci % 8] = src[(q / 3) * 3 * cin + ci * 3 + q % 3];
        fr = (uint16_t*)(dst + 24LL * cin);
        nkb = cin / 16;
    } else {
        fr = (uint16_t*)dst;
        nkb = 9 * cin / 16;
    }
    for (int kb = 0; kb < nkb; ++kb)
        for (int ct = 0; ct < nct; ++ct)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int k = kb * 16 + 8 * (lane >> 5) + j, co = enc16_row_channel(ct, lane & 31);
                    float v = 0.f;
                    if (co < cout) v = sep ? wsrc[(long long)k * cout + co] : wsrc[((long long)(k % cin) * 9 + k / cin) * cout + co];
                    fr[(((long long)kb * nct + ct) * 64 + lane) * 8 + j] = enc16_rne(v);
                }
    memcpy((char*)fr + 2LL * nkb * 16 * nct * 32, wsrc + nw, (size_t)cout * 12);
}

inline void enc16_pack(const float* src, char* dst) {
    auto one = [&](int cin, int cout, bool sep) {
        enc16_pack_layer(src, dst, cin, cout, sep);
        src += enc_layer_floats(cin, cout, sep);
        dst += enc16_layer_bytes(cin, cout, sep);
    };
    one(4, kEncCh, true);
    for (int lv = 0; lv < kEncLevels; ++lv) {
        const int c = kEncCh << lv;
        one(c, c, true);
        one(c, c, true);
        one(c, 2 * c, false);
    }
}

inline int enc16_pool_tiles(int img) {  // 8 x 8 tiles of the last down's output
    int h = img;
    for (int lv = 0; lv < kEncLevels; ++lv) h = enc_out_size(h, 2);
    const int t = (h + 7) / 8;
    return t * t;
}

// workspace: three (n, S, S, 8) bf16 activation buffers and the f32 partials (n, tiles of the last down, 256)
inline void enc16_ws_layout(int img, int n, size_t* buf_bytes, size_t* part_bytes) {
    *buf_bytes = enc_align((size_t)n * kEncCh * img * img * 2);
    *part_bytes = enc_align((size_t)n * enc16_pool_tiles(img) * kEncFeat * sizeof(float));
}

static void enc16_launch_sep(const uint4* x, uint4* y, const uint4* resid, const char* w, int c, int H, int d, int n, hipStream_t st,
                             const int32_t* skip) {
    const int T = c <= 64 && H >= 16 ? 16 : 8;
    const int tiles_x = (H + T - 1) / T;
    const dim3 grid(tiles_x * tiles_x, 1, n);
#define OCC_ENC16_SEP(C, TT) \
    hipLaunchKernelGGL((occ_enc16_sep_kernel<C, TT>), grid, dim3(TT == 16 ? 256 : 128), 0, st, x, y, resid, w, H, H, d, tiles_x, skip)
    if (c == 8) hipLaunchKernelGGL(occ_enc16_sep8_kernel, grid, dim3(256), 0, st, x, y, resid, (const float*)w, H, H, d, tiles_x, skip);
    else if (c == 16) { if (T == 16) OCC_ENC16_SEP(16, 16); else OCC_ENC16_SEP(16, 8); }
    else if (c == 32) { if (T == 16) OCC_ENC16_SEP(32, 16); else OCC_ENC16_SEP(32, 8); }
    else if (c == 64) { if (T == 16) OCC_ENC16_SEP(64, 16); else OCC_ENC16_SEP(64, 8); }
    else OCC_ENC16_SEP(128, 8);
#undef OCC_ENC16_SEP
}

static void enc16_launch_down(const uint4* x, uint4* y, const char* w, int c, int H, int n, float* partials, hipStream_t st,
                              const int32_t* skip) {
    const int Ho = enc_out_size(H, 2);
    const int T = c == 8 ? 16 : 8;
    const int tiles_x = (Ho + T - 1) / T;
    const dim3 grid(tiles_x * tiles_x, 1, n);
#define OCC_ENC16_DOWN(C, POOL) \
    hipLaunchKernelGGL((occ_enc16_down_kernel<C, POOL>), grid, dim3(256), 0, st, x, y, w, H, H, Ho, Ho, tiles_x, partials, skip)
    if (c == 8) hipLaunchKernelGGL(occ_enc16_down8_kernel, grid, dim3(256), 0, st, x, y, (const float*)w, H, H, Ho, Ho, tiles_x, skip);
    else if (c == 16) OCC_ENC16_DOWN(16, false);
    else if (c == 32) OCC_ENC16_DOWN(32, false);
    else if (c == 64) OCC_ENC16_DOWN(64, false);
    else OCC_ENC16_DOWN(128, true);
#undef OCC_ENC16_DOWN
}

// The whole encoder on n envs in the bf16 mode: the 17 launches of enc_forward, on grids sized by n.
static void enc16_forward(int img, int dil, bool residual, const char* packed, const float* obs, int n, char* ws, float* feats,
                          hipStream_t st, const int32_t* skip) {
    size_t buf_bytes, part_bytes;
    enc16_ws_layout(img, n, &buf_bytes, &part_bytes);
    uint4* b0 = (uint4*)ws;
    uint4* b1 = (uint4*)(ws + buf_bytes);
    uint4* b2 = (uint4*)(ws + 2 * buf_bytes);
    float* part = (float*)(ws + 3 * buf_bytes);
    const char* w = packed;
    int H = img;
    {
        const int tiles_x = (H + 15) / 16;
        hipLaunchKernelGGL(occ_enc16_init_kernel, dim3(tiles_x * tiles_x, 1, n), dim3(256), 0, st, obs, b0, (const float*)w, H, H,
                           tiles_x, skip);
        w += enc16_layer_bytes(4, kEncCh, true);
    }
    for (int lv = 0; lv < kEncLevels; ++lv) {
        const int c = kEncCh << lv;
        enc16_launch_sep(b0, b1, nullptr, w, c, H, dil, n, st, skip);
        w += enc16_layer_bytes(c, c, true);
        enc16_launch_sep(b1, b2, residual ? b0 : nullptr, w, c, H, dil, n, st, skip);
        w += enc16_layer_bytes(c, c, true);
        enc16_launch_down(b2, b0, w, c, H, n, lv == kEncLevels - 1 ? part : nullptr, st, skip);
        w += enc16_layer_bytes(c, 2 * c, false);
        H = enc_out_size(H, 2);
    }
    hipLaunchKernelGGL(occ_enc_pool_kernel, dim3(n), dim3(kEncFeat), 0, st, part, enc16_pool_tiles(img), (float)(H * H), feats, skip);
}
