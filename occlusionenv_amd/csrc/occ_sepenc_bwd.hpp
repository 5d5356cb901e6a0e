// occ_sepenc_bwd.hpp -- the backward of one separable layer (dilation 1 or 2): its kernels, the K split of its pointwise
// weight gradient (sep_dpw_plan) and sep_bwd_layer, which the one backward walk of occ_encoder_bwd.hpp (enc_backward with
// `separable`) calls for the initial layer and for Layer 1 and Layer 2 of every level.  The training forward, the workspace,
// the gradient-buffer rotation and the dense stride-2 downs are those of occ_encoder_bwd.hpp.  Part of the single
// translation unit occ_kernels.hip (included inside namespace occ, after occ_encoder_bwd.hpp).
//
// A separable layer (initial at dilation 1, Layer 1 and Layer 2 of every level at dilation d): h = dw_h(dw_v(x)), both
// depthwise convs without bias and with zero padding d, so h[ci] is the 9-tap stencil wv[ci][kv] wh[ci][kh] on zero-padded
// x at offsets ((kv - 1) d, (kh - 1) d); u = pw h + bias, r = relu(u), y = s r + t (+ the block input, Layer 2 of a
// residual block).  Packed: wv[ci][3] | wh[ci][3] | pw[ci][co] | bias | scale | shift.  The downs are dense (packed and
// trained as in occ_encoder_bwd.hpp).
//
//   occ_enc_sep_kernel<.., TRAIN>  (occ_encoder.hpp) the inference kernel itself, one loop nest for both (feats are the
//                              same to the bit), whose epilogue also stores r.  h is not kept: the backward rebuilds it
//                              from the kept x.
//   occ_enc_bwd_act_kernel     (occ_encoder_bwd.hpp, as it is) dU = dY s [r > 0] and the f64 partials of ds, dt, dbias.
//   occ_sep_bwd_dpw_kernel     dPW[ci][co] = sum_{n,p} h[ci][p] dU[co][p], a cin x cout contraction over K = N H^2 with the
//                              thread layout, K split and lane fold (bwd_dw_fold) of occ_enc_bwd_dw_kernel: a thread owns
//                              1 ci x 8 co, keeps its channel's six depthwise taps in registers and forms h of each pixel
//                              from the LDS-staged x tile (halo d) in the forward's FMA order.  Partials to caller scratch,
//                              added by occ_dec_bwd_sum_kernel (bwd_layer_tail with cin cout elements).
//   occ_sep_bwd_dh_kernel      dH[ci][p] = sum_co pw[ci][co] dU[co][p]: a thread owns one pixel for CIG input channels,
//                              weights are wave-uniform scalar loads.
//   occ_sep_bwd_g_kernel       per (chunk of 4096 pixels, channel, env) the nine correlation sums
//                              G[kv][kh] = sum_p dH[p] x[p + ((kv - 1) d, (kh - 1) d)] (x zero outside), in f64, as block
//                              partials in the layout of occ_enc_bwd_act_kernel with nine sums (bwd_block_partials).
//   occ_sep_bwd_g_final_kernel one wave per channel: the partials of G in block order (bwd_wave_strided_sum), then in f64
//                              dwv[kv] = sum_kh wh[kh] G[kv][kh], dwh[kh] = sum_kv wv[kv] G[kv][kh].
//   occ_sep_bwd_dx_kernel      dX[ci][p] = sum_{kv,kh} wv[kv] wh[kh] dH[ci][p - ((kv - 1) d, (kh - 1) d)] (+ add, the
//                              residual's second path): the forward's depthwise pair with the stencil flipped, two 3-tap
//                              passes in registers on an LDS tile of side T + 2 d.  Not run for the initial layer.
//
// Launches: a separable layer takes 8 (act, act-final, dPW, sum, dH, G, G-final, dX; 7 for the initial layer), a down 5 as
// in occ_encoder_bwd.hpp: 112 for the backward.  No floating-point atomics; every reduction over pixels or envs goes through
// block partials in caller scratch added in f64 in a fixed order, and the K split is a function of (S, N) alone: every
// gradient is bitwise the same from call to call.  Nothing is allocated or synchronised.

constexpr int kSepDwBlocks = 1024;  // blocks of the pointwise weight gradient per layer (K slices x (ci, co) tiles)

// x: (n, cin, H, H); du: (n, cout, H, H); w: the layer's packed wv[ci][3] | wh[ci][3];
// part: [slice * PB + wave or pixel lane][cin * cout], PB = 256 / max(Q, 64).
// A slice is the tiles [blockIdx.x * tps, .. + tps) of the n * tiles_x^2 pixel tiles, envs in order.
template <int T, int CIB, int COB>
__global__ __launch_bounds__(256) void occ_sep_bwd_dpw_kernel(const float* __restrict__ x, const float* __restrict__ du,
                                                              const float* __restrict__ w, float* __restrict__ part, int cin,
                                                              int cout, int H, int d, int tiles_x, int total_tiles, int tps) {
    constexpr int TT = T * T, RM = T + 4, XP = (RM * RM) | 1, COT = kEncDwCot, Q = CIB * (COB / COT), P = 256 / Q;
    static_assert(Q <= 256 && 256 % Q == 0 && (Q >= 64 || 64 % Q == 0) && COB % COT == 0, "thread layout");
    __shared__ float xs[CIB * XP];
    __shared__ float ds[COB * TT];
    const int tid = threadIdx.x;
    const int q = tid % Q, pl = tid / Q;
    const int cil = q % CIB, cog = q / CIB;
    const int nco = cout / COB;
    const int ci0 = (blockIdx.y / nco) * CIB, co0 = (blockIdx.y % nco) * COB;
    const size_t plane = (size_t)H * H;
    const int tiles_env = tiles_x * tiles_x;
    const int R = T + 2 * d, RR = R * R;
    float wv[3], wh[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) wv[k] = w[(ci0 + cil) * 3 + k], wh[k] = w[3 * cin + (ci0 + cil) * 3 + k];

    float acc[COT];
#pragma unroll
    for (int j = 0; j < COT; ++j) acc[j] = 0.f;

    const int t0 = blockIdx.x * tps, t1 = min(t0 + tps, total_tiles);
    for (int t = t0; t < t1; ++t) {
        const int env = t / tiles_env, rem = t - env * tiles_env;
        const int oy0 = (rem / tiles_x) * T, ox0 = (rem % tiles_x) * T;
        const float* xe = x + ((size_t)env * cin + ci0) * plane;
        const float* de = du + ((size_t)env * cout + co0) * plane;
        __syncthreads();
        for (int i = tid; i < CIB * RR; i += 256) {
            const int c = i / RR, r = i - c * RR;
            const int ry = r / R, rx = r - ry * R;
            const int gy = oy0 - d + ry, gx = ox0 - d + rx;
            float v = 0.f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < H) v = xe[c * plane + (size_t)gy * H + gx];
            xs[c * XP + r] = v;
        }
        for (int i = tid; i < COB * TT; i += 256) {
            const int c = i / TT, p = i - c * TT;
            const int gy = oy0 + p / T, gx = ox0 + p % T;
            float v = 0.f;
            if (gy < H && gx < H) v = de[c * plane + (size_t)gy * H + gx];
            ds[i] = v;
        }
        __syncthreads();
        for (int p = pl; p < TT; p += P) {
            const float* xp = xs + cil * XP + (p / T) * R + p % T;  // staged (py - d, px - d)
            float h = 0.f;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {  // h as the forward forms it
                float tv = 0.f;
#pragma unroll
                for (int kv = 0; kv < 3; ++kv) tv = fmaf(wv[kv], xp[(kv * d) * R + kh * d], tv);
                h = fmaf(wh[kh], tv, h);
            }
            const float* dp = ds + cog * COT * TT + p;
#pragma unroll
            for (int j = 0; j < COT; ++j) acc[j] = fmaf(h, dp[j * TT], acc[j]);
        }
    }
    constexpr int PB = dw_partials(Q);
    int pb;
    if (!bwd_dw_fold<Q>(acc, pl, pb)) return;
    const size_t nout = (size_t)cin * cout;
    float* dst = part + ((size_t)blockIdx.x * PB + pb) * nout + (size_t)(ci0 + cil) * cout + co0 + cog * COT;
#pragma unroll
    for (int j = 0; j < COT; ++j) dst[j] = acc[j];
}

// du: (n, cout, plane); dh: (n, cin, plane); pw: the layer's packed pw[ci][co].  cin % CIG == 0, cout % 8 == 0.
template <int CIG>
__global__ __launch_bounds__(256) void occ_sep_bwd_dh_kernel(const float* __restrict__ du, float* __restrict__ dh,
                                                             const float* __restrict__ pw, int cin, int cout, int plane) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= plane) return;
    const int ci0 = blockIdx.y * CIG;
    const float* de = du + (size_t)blockIdx.z * cout * plane + i;
    float acc[CIG];
#pragma unroll
    for (int j = 0; j < CIG; ++j) acc[j] = 0.f;
    for (int co0 = 0; co0 < cout; co0 += 8) {
        float dv[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) dv[c] = de[(size_t)(co0 + c) * plane];
        const float* wr = pw + (size_t)ci0 * cout + co0;
#pragma unroll
        for (int j = 0; j < CIG; ++j)
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[j] = fmaf(wr[j * cout + c], dv[c], acc[j]);
    }
    float* he = dh + ((size_t)blockIdx.z * cin + ci0) * plane + i;
#pragma unroll
    for (int j = 0; j < CIG; ++j) he[(size_t)j * plane] = acc[j];
}

// x, dh: (n, c, H, H).  partials[((ch * n + env) * chunks + chunk) * 9 + kv * 3 + kh].
__global__ __launch_bounds__(256) void occ_sep_bwd_g_kernel(const float* __restrict__ x, const float* __restrict__ dh, int c,
                                                            int H, int d, double* __restrict__ partials) {
    const int ch = blockIdx.y, env = blockIdx.z;
    const int plane = H * H;
    const size_t base = ((size_t)env * c + ch) * plane;
    double sum[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) sum[k] = 0.0;
    const int lo = blockIdx.x * kBwdChunk;
    for (int j = 0; j < kBwdChunk / 256; ++j) {
        const int i = lo + (int)threadIdx.x + 256 * j;
        if (i >= plane) break;
        const int py = i / H, px = i - py * H;
        const double g = (double)dh[base + i];
#pragma unroll
        for (int kv = 0; kv < 3; ++kv)
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int gy = py + (kv - 1) * d, gx = px + (kh - 1) * d;
                float v = 0.f;
                if (gy >= 0 && gy < H && gx >= 0 && gx < H) v = x[base + (size_t)gy * H + gx];
                sum[kv * 3 + kh] = fma(g, (double)v, sum[kv * 3 + kh]);
            }
    }
    bwd_block_partials(sum, partials + ((((size_t)ch * gridDim.z + env) * gridDim.x) + blockIdx.x) * 9);
}

// One wave per channel: G = the channel's nparts partials (bwd_wave_strided_sum), then the two depthwise gradients.  w, gw: the layer's packed wv[ci][3] | wh[ci][3] and its gradient.
__global__ __launch_bounds__(64) void occ_sep_bwd_g_final_kernel(const double* __restrict__ partials, int nparts,
                                                                 const float* __restrict__ w, float* __restrict__ gw, int cin) {
    const int ch = blockIdx.x;
    const double* pe = partials + (size_t)ch * nparts * 9;
    double G[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) G[k] = bwd_wave_strided_sum(pe + k, nparts, 9);
    if (threadIdx.x != 0) return;
    const float* wv = w + ch * 3;
    const float* wh = w + 3 * cin + ch * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double dv = 0.0, dhz = 0.0;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            dv = fma((double)wh[m], G[k * 3 + m], dv);   // dwv[k] = sum_kh wh[kh] G[k][kh]
            dhz = fma((double)wv[m], G[m * 3 + k], dhz);  // dwh[k] = sum_kv wv[kv] G[kv][k]
        }
        gw[ch * 3 + k] = (float)dv;
        gw[3 * cin + ch * 3 + k] = (float)dhz;
    }
}

// dh, dx, add: (n, cin, H, H); w: the layer's packed wv | wh.  cin % 8 == 0.  A thread owns one pixel for the 8 channels
// of its group; the (T + 2 d)^2 dH tiles of the block's 8 ng channels are staged in LDS.
template <int T>
__global__ __launch_bounds__(256) void occ_sep_bwd_dx_kernel(const float* __restrict__ dh, float* __restrict__ dx,
                                                             const float* __restrict__ add, const float* __restrict__ w, int cin,
                                                             int H, int d, int tiles_x) {
    constexpr int TT = T * T, NGM = T == 16 ? 1 : 4, CIG = 8;
    __shared__ float s[NGM * CIG * (T + 4) * (T + 4)];
    const int tid = threadIdx.x;
    const int p = tid % TT;
    const int ng = blockDim.x / TT;
    const int g = __builtin_amdgcn_readfirstlane(tid / TT);
    const int cb0 = blockIdx.y * ng * CIG;  // the block's first channel
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const int iy0 = ty * T, ix0 = tx * T;
    const int py = p / T, px = p % T;
    const size_t plane = (size_t)H * H;
    const float* he = dh + ((size_t)blockIdx.z * cin + cb0) * plane;
    const int R = T + 2 * d, RR = R * R;
    for (int i = tid; i < ng * CIG * RR; i += blockDim.x) {
        const int c = i / RR, r = i - c * RR;
        const int ry = r / R, rx = r - ry * R;
        const int gy = iy0 - d + ry, gx = ix0 - d + rx;
        float v = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < H) v = he[c * plane + (size_t)gy * H + gx];
        s[i] = v;
    }
    __syncthreads();
    const int iy = iy0 + py, ix = ix0 + px;
    if (iy >= H || ix >= H) return;
    const int ci0 = cb0 + g * CIG;
    const float* wv = w;
    const float* wh = w + 3 * cin;
    const size_t o = ((size_t)blockIdx.z * cin + ci0) * plane + (size_t)iy * H + ix;
#pragma unroll
    for (int j = 0; j < CIG; ++j) {
        const int ci = ci0 + j;
        const float* sc = s + (g * CIG + j) * RR + py * R + px;  // staged (py - d, px - d)
        float v = 0.f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            // tap (kv, kh) reads dH at (y - (kv - 1) d, x - (kh - 1) d): the forward's stencil flipped
            float t = 0.f;
#pragma unroll
            for (int kv = 0; kv < 3; ++kv) t = fmaf(wv[ci * 3 + kv], sc[((2 - kv) * d) * R + (2 - kh) * d], t);
            v = fmaf(wh[ci * 3 + kh], t, v);
        }
        if (add) v += add[o + j * plane];
        dx[o + j * plane] = v;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------

// The (ci, co) tile, pixel tile and K split (dw_split, occ_decoder_bwd.hpp) of the pointwise weight gradient: a thread
// owns 1 ci x 8 co; 16-pixel tiles where a block owns at most 8 input channels (the smaller halo share).
inline DwPlan sep_dpw_plan(int cin, int cout, int H, int n) {
    const int cib = cin < 64 ? cin : 64, cob = cout < 32 ? cout : 32;
    DwPlan p = dw_split(cib, cob, cib <= 8 ? 16 : cib == 64 ? 4 : 8, cib * (cob / kEncDwCot), cin, cout, H, n, kSepDwBlocks);
    p.part_bytes = (size_t)p.slices * p.pb * cin * cout * sizeof(float);
    return p;
}

template <int T, int CIB, int COB>
static void sep_launch_dpw_t(const DwPlan& p, const float* x, const float* du, const float* w, float* part, const EncLayer& L, int d,
                             hipStream_t st) {
    hipLaunchKernelGGL((occ_sep_bwd_dpw_kernel<T, CIB, COB>), dim3(p.slices, p.grid_y), dim3(256), 0, st, x, du, w, part, L.cin,
                       L.cout, L.H, d, p.tiles_x, p.total_tiles, p.tps);
}

// The five (ci, co) tiles of sep_dpw_plan: cout = cin, or 4 -> 8 for the initial layer.
static void sep_launch_dpw(const DwPlan& p, const float* x, const float* du, const float* w, float* part, const EncLayer& L, int d,
                           hipStream_t st) {
    if (p.cib == 4) sep_launch_dpw_t<16, 4, 8>(p, x, du, w, part, L, d, st);
    else if (p.cib == 8) sep_launch_dpw_t<16, 8, 8>(p, x, du, w, part, L, d, st);
    else if (p.cib == 16) sep_launch_dpw_t<8, 16, 16>(p, x, du, w, part, L, d, st);
    else if (p.cib == 32) sep_launch_dpw_t<8, 32, 32>(p, x, du, w, part, L, d, st);
    else sep_launch_dpw_t<4, 64, 32>(p, x, du, w, part, L, d, st);
}

// One separable layer's parameter gradients and, when dx is not null, its input gradient (+ add) from its dY: dU goes to
// `du` (may be dy itself), dH to `dh`; dx may be du.  8 launches (7 without dx).  bn: the forward ran with batch
// statistics; the activation step is bn_bwd_act for layer `index` (2 launches more).
static void sep_bwd_layer(const EncLayer& L, int d, const float* packed, float* grad_packed, int n, const float* x, const float* r,
                          const float* dy, float* du, float* dh, float* dx, const float* add, char* scratch, hipStream_t st,
                          const BnTrain* bn, int index) {
    const int plane = L.H * L.H, chunks = bwd_chunks(plane);
    const float* w = packed + L.woff;
    float* gw = grad_packed + L.woff;
    const float* pw = w + 6 * L.cin;
    float* gpw = gw + 6 * L.cin;
    float* gbias = gpw + (long long)L.cin * L.cout;
    const float* bns = pw + (long long)L.cin * L.cout + L.cout;
    if (bn)
        bn_bwd_act(*bn, index, L.cout, plane, n, BnDy{dy, nullptr, nullptr, nullptr, nullptr, nullptr}, du, r, bns, gbias + L.cout,
                   gbias + 2 * L.cout, nullptr, scratch, st);
    else
        hipLaunchKernelGGL((occ_enc_bwd_act_kernel<false>), dim3(chunks, L.cout, n), dim3(256), 0, st, dy, du, r, bns, L.cout,
                           plane, nullptr, 1.f, (double*)scratch);
    const BwdActDst dst = bn ? BwdActDst{{gbias, nullptr, nullptr, nullptr, nullptr}}
                             : BwdActDst{{gbias + L.cout, gbias + 2 * L.cout, gbias, nullptr, nullptr}};
    const DwPlan p = sep_dpw_plan(L.cin, L.cout, L.H, n);
    bwd_layer_tail(p, L.cin * L.cout, L.cout, n * chunks, bn ? 1 : 3, dst, scratch, gpw, st,
                   [&](float* part) { sep_launch_dpw(p, x, du, w, part, L, d, st); });
    const int pblocks = (plane + 255) / 256;
    if (L.cin == 4)
        hipLaunchKernelGGL((occ_sep_bwd_dh_kernel<4>), dim3(pblocks, 1, n), dim3(256), 0, st, du, dh, pw, L.cin, L.cout, plane);
    else if (L.cin == 8)
        hipLaunchKernelGGL((occ_sep_bwd_dh_kernel<8>), dim3(pblocks, 1, n), dim3(256), 0, st, du, dh, pw, L.cin, L.cout, plane);
    else
        hipLaunchKernelGGL((occ_sep_bwd_dh_kernel<16>), dim3(pblocks, L.cin / 16, n), dim3(256), 0, st, du, dh, pw, L.cin, L.cout,
                           plane);
    hipLaunchKernelGGL(occ_sep_bwd_g_kernel, dim3(chunks, L.cin, n), dim3(256), 0, st, x, dh, L.cin, L.H, d, (double*)scratch);
    hipLaunchKernelGGL(occ_sep_bwd_g_final_kernel, dim3(L.cin), dim3(64), 0, st, (const double*)scratch, n * chunks, w, gw, L.cin);
    if (!dx) return;
    const int T = enc_tile(L.H);
    const TileLaunch tl = tile_launch(T, L.H, L.cin / 8, n);
    if (T == 16) hipLaunchKernelGGL((occ_sep_bwd_dx_kernel<16>), tl.grid, tl.block, 0, st, dh, dx, add, w, L.cin, L.H, d, tl.tiles_x);
    else hipLaunchKernelGGL((occ_sep_bwd_dx_kernel<8>), tl.grid, tl.block, 0, st, dh, dx, add, w, L.cin, L.H, d, tl.tiles_x);
}
