// occ_bn_train.hpp -- batch-statistics ("train-mode") BatchNorm for the joint training step of occ_fullnet_bwd.hpp, both
// encoder forms and all 21 layers (16 encoder layers, 5 decoder levels): nn.BatchNorm2d as pretrainer.py runs it after
// model.train().  Part of the single translation unit occ_kernels.hip (included inside namespace occ, after
// occ_fullnet_bwd.hpp).  The conv / up kernels, the weight and input gradients, the joins and the reduction tails are those of
// the running-statistics step; this file replaces what touches the BatchNorm itself: the epilogue's y in the forward and the
// activation step in the backward.  The walks (enc_train_forward, dec_train_forward, enc_backward, dec_backward) take a
// BnTrain and call bn_fwd_layer / bn_bwd_act below where they otherwise rely on the folded scale and shift.
//
// Per layer, channel c, M = N H W values of r = relu(u); the packed scale / shift slots carry gamma / beta:
//   forward   mu = mean r, v = mean r^2 - mu^2 (biased), rstd = 1 / sqrt(v + 1e-5), s = gamma rstd, t = beta - mu s,
//             y = s r + t (+ the residual or the skip, as the conv kernel's epilogue adds them)
//   backward  dbeta = sum dY, dgamma = rstd (sum dY r - mu sum dY),
//             dR = A dY + C r + B with A = s, C = -s rstd dgamma / M, B = -s dbeta / M - C mu (f64, rounded once),
//             dU = [r > 0] dR (the forward's kept r is the gate)
// The residual, the skip joins and d last enter after the BatchNorm and are untouched.
//
//   occ_bn_stats_kernel       per (chunk of 4096 pixels, channel, env): f64 block partials of sum r, sum r^2
//                             (bwd_block_partials), after the conv / up kernel has stored r (and a y that is overwritten).
//   occ_bn_fwd_final_kernel   one wave per channel (bwd_wave_strided_sum): s, t (f32) and mu, rstd (f64) to the layer's
//                             region of the workspace, mean | biased var to the caller's bn_stats.
//   occ_bn_apply_kernel       y = fma(r, s, t) (+ residual / skip).
//   occ_bn_apply_pool_kernel  the last down: one block per (channel, env) writes y (`last`) and feats = the spatial mean of
//                             y, summed in f64 in a fixed order.
//   occ_bn_apply_cls_kernel   the last decoder level: a thread owns a pixel's 8 channels, writes y_4 and runs the classifier
//                             and the sigmoid on it (prob and the kept p; what the up kernel's fused classifier wrote from
//                             the unnormalised y is overwritten).
//   occ_bn_bwd_sums_kernel    forms dY as the layer kind's activation step does (plain: the dY buffer; pool: gf / count +
//                             dlast; last decoder level: gp p (1 - p) cls_w[c]) and writes f64 partials of sum dY, sum dY r
//                             (and sum dz y_4[c], sum dz).  It stores nothing else: dU may be written over dY afterwards.
//   occ_bn_bwd_final_kernel   one wave per channel: dgamma, dbeta into the dbn_scale / dbn_shift slots, dcls_w / dcls_b at
//                             the last level, and A | B | C of the layer.
//   occ_bn_bwd_act_kernel     dU and the f64 partials of sum dU = dbias, which bwd_layer_tail adds (one sum per channel).
// Planes with a multiple of 4 pixels are read and written 16 bytes per lane (V = 4); the others (S = 96: 3 x 3, 9 x 9 ..)
// one pixel per lane (V = 1); a chunk's ragged end is cut at the plane.  No floating-point atomics, every sum in a fixed
// order in f64: bitwise the same from call to call.
//
// Forward: 3 launches per layer more, one fewer for the pool: 23 + 62 = 85.  Backward: 2 per layer more: 146 dense, 179
// separable.
//
// Workspace (occ_fullnet_bn_train_workspace_query): the joint workspace of occ_fullnet_bwd.hpp, then, 256-byte aligned,
//   coef: per layer in packed order, c channels: s[c] | t[c] (f32) | mu[c] | rstd[c] (f64); 24 x 1248 bytes |
//   abc: A[256] | B[256] | C[256] (f32) of the layer in flight |
//   forward partials: the largest layer's c n chunks 2 doubles
// Scratch: that of the joint step (the sums take 2 or 4 doubles where its activation step takes 3 or 5).

constexpr int kBnLayers = 21;
constexpr int kBnChannels = 1248;  // 1000 encoder + 248 decoder
constexpr double kBnEps = 1e-5;

struct BnTrain {
    char* coef;
    float* abc;
    double* part;  // forward partials
    float* stats;  // the caller's bn_stats (forward only)
};

// channels of the layers before `layer` (0..15 the encoder's in packed order, 16 + j decoder level j)
inline int bn_ch_off(int layer) {
    int off = 0;
    for (int i = 0; i < layer; ++i) {
        int c;
        if (i == 0) c = kEncCh;
        else if (i < 16) c = (kEncCh << ((i - 1) / 3)) * ((i - 1) % 3 == 2 ? 2 : 1);
        else c = kEncCh << (kEncLevels - 1 - (i - 16));
        off += c;
    }
    return off;
}

struct BnCoef {
    float *s, *t;
    double *mu, *rstd;
};
inline BnCoef bn_coef(const BnTrain& bn, int layer, int c) {
    char* at = bn.coef + (size_t)24 * bn_ch_off(layer);
    return {(float*)at, (float*)at + c, (double*)(at + 8 * (size_t)c), (double*)(at + 8 * (size_t)c) + c};
}

template <int V>
__device__ __forceinline__ void bn_load(const float* p, float (&v)[V]) {
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        v[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void bn_store(float* p, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}

// r: (n, c, plane).  partials[((ch * n + env) * chunks + chunk) * 2 + k]: k = 0 sum r, 1 sum r^2.  V = 4: plane % 4 == 0.
template <int V>
__global__ __launch_bounds__(256) void occ_bn_stats_kernel(const float* __restrict__ r, int c, int plane,
                                                           double* __restrict__ partials) {
    const int ch = blockIdx.y, env = blockIdx.z;
    const size_t base = ((size_t)env * c + ch) * plane;
    double sum[2] = {0.0, 0.0};
    const int lo = blockIdx.x * kBwdChunk, hi = min(lo + kBwdChunk, plane);
    for (int i = lo + V * (int)threadIdx.x; i < hi; i += 256 * V) {
        float rv[V];
        bn_load<V>(r + base + i, rv);
#pragma unroll
        for (int q = 0; q < V; ++q) {
            sum[0] += (double)rv[q];
            sum[1] = fma((double)rv[q], (double)rv[q], sum[1]);
        }
    }
    bwd_block_partials(sum, partials + ((((size_t)ch * gridDim.z + env) * gridDim.x) + blockIdx.x) * 2);
}

// One wave per channel.  gamma, beta: the layer's packed scale / shift slots; stats: mean[c] | var_biased[c]; m = n plane.
__global__ __launch_bounds__(64) void occ_bn_fwd_final_kernel(const double* __restrict__ partials, int nparts, int c, double m,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              BnCoef co, float* __restrict__ stats) {
    const int ch = blockIdx.x;
    const double* pe = partials + (size_t)ch * nparts * 2;
    const double s1 = bwd_wave_strided_sum(pe, nparts, 2);
    const double s2 = bwd_wave_strided_sum(pe + 1, nparts, 2);
    if (threadIdx.x != 0) return;
    const double mu = s1 / m;
    const double v = fmax(s2 / m - mu * mu, 0.0);
    const double rstd = 1.0 / sqrt(v + kBnEps);
    const double s = (double)gamma[ch] * rstd;
    co.s[ch] = (float)s;
    co.t[ch] = (float)((double)beta[ch] - mu * s);
    co.mu[ch] = mu;
    co.rstd[ch] = rstd;
    stats[ch] = (float)mu;
    stats[c + ch] = (float)v;
}

// y = fma(r, s, t) (+ add): r, y, add (n, c, plane); add is the residual or the skip, or null.
template <int V>
__global__ __launch_bounds__(256) void occ_bn_apply_kernel(const float* __restrict__ r, float* __restrict__ y,
                                                           const float* __restrict__ add, const float* __restrict__ s,
                                                           const float* __restrict__ t, int c, int plane) {
    const int ch = blockIdx.y, env = blockIdx.z;
    const size_t base = ((size_t)env * c + ch) * plane;
    const float sc = s[ch], sh = t[ch];
    const int lo = blockIdx.x * kBwdChunk, hi = min(lo + kBwdChunk, plane);
    for (int i = lo + V * (int)threadIdx.x; i < hi; i += 256 * V) {
        float rv[V], av[V], yv[V];
        bn_load<V>(r + base + i, rv);
        if (add) bn_load<V>(add + base + i, av);
#pragma unroll
        for (int q = 0; q < V; ++q) {
            yv[q] = fmaf(rv[q], sc, sh);
            if (add) yv[q] += av[q];
        }
        bn_store<V>(y + base + i, yv);
    }
}

// The last down: one block per (channel, env).  y: `last` (n, c, plane); feats[env][ch] = mean of y.
__global__ __launch_bounds__(256) void occ_bn_apply_pool_kernel(const float* __restrict__ r, float* __restrict__ y,
                                                                const float* __restrict__ s, const float* __restrict__ t, int c,
                                                                int plane, float* __restrict__ feats) {
    __shared__ double total[1];
    const int ch = blockIdx.x, env = blockIdx.y;
    const size_t base = ((size_t)env * c + ch) * plane;
    const float sc = s[ch], sh = t[ch];
    double sum[1] = {0.0};
    for (int i = threadIdx.x; i < plane; i += 256) {
        const float v = fmaf(r[base + i], sc, sh);
        y[base + i] = v;
        sum[0] += (double)v;
    }
    bwd_block_partials(sum, total);
    __syncthreads();
    if (threadIdx.x == 0) feats[(size_t)env * c + ch] = (float)(total[0] / (double)plane);
}

// The last decoder level (c = 8): r, y, skip (n, 8, plane); cls = w[8] | bias; prob, pkeep (n, plane).
template <int V>
__global__ __launch_bounds__(256) void occ_bn_apply_cls_kernel(const float* __restrict__ r, float* __restrict__ y,
                                                               const float* __restrict__ skip, const float* __restrict__ s,
                                                               const float* __restrict__ t, const float* __restrict__ cls,
                                                               int plane, float* __restrict__ prob, float* __restrict__ pkeep) {
    const int env = blockIdx.z;
    const size_t base = (size_t)env * kEncCh * plane;
    const int lo = blockIdx.x * kBwdChunk, hi = min(lo + kBwdChunk, plane);
    for (int i = lo + V * (int)threadIdx.x; i < hi; i += 256 * V) {
        float z[V];
#pragma unroll
        for (int q = 0; q < V; ++q) z[q] = 0.f;
#pragma unroll
        for (int ch = 0; ch < kEncCh; ++ch) {
            float rv[V], kv[V], yv[V];
            bn_load<V>(r + base + (size_t)ch * plane + i, rv);
            bn_load<V>(skip + base + (size_t)ch * plane + i, kv);
#pragma unroll
            for (int q = 0; q < V; ++q) {
                yv[q] = fmaf(rv[q], s[ch], t[ch]) + kv[q];
                z[q] = fmaf(cls[ch], yv[q], z[q]);
            }
            bn_store<V>(y + base + (size_t)ch * plane + i, yv);
        }
        float pr[V];
#pragma unroll
        for (int q = 0; q < V; ++q) pr[q] = 1.f / (1.f + expf(-(z[q] + cls[kEncCh])));
        bn_store<V>(prob + (size_t)env * plane + i, pr);
        bn_store<V>(pkeep + (size_t)env * plane + i, pr);
    }
}

// Where a layer's dY comes from (declared in occ_decoder_bwd.hpp: BnDy).  KIND 0: dy; 1 (pool): gf[env][ch] / count (+ dy
// when not null); 2 (last decoder level): dz cls_w[ch], dz = gp p (1 - p).
enum { kBnPlain = 0, kBnPool = 1, kBnLast = 2 };

template <int KIND, int V>
__device__ __forceinline__ void bn_form_dy(const BnDy& src, size_t at, size_t pix, float pooled, float cw, float (&dy)[V],
                                           float (&dz)[V]) {
    if constexpr (KIND == kBnLast) {
        float gv[V], pv[V];
        bn_load<V>(src.gp + pix, gv);
        bn_load<V>(src.prob + pix, pv);
#pragma unroll
        for (int q = 0; q < V; ++q) {
            dz[q] = gv[q] * (pv[q] * (1.f - pv[q]));
            dy[q] = dz[q] * cw;
        }
    } else if constexpr (KIND == kBnPool) {
        if (src.dy) {
            bn_load<V>(src.dy + at, dy);
#pragma unroll
            for (int q = 0; q < V; ++q) dy[q] += pooled;
        } else {
#pragma unroll
            for (int q = 0; q < V; ++q) dy[q] = pooled;
        }
    } else {
        bn_load<V>(src.dy + at, dy);
    }
}

// partials[((ch * n + env) * chunks + chunk) * NS + k], NS = KIND == 2 ? 4 : 2: k = 0 sum dY, 1 sum dY r, 2 sum dz y4[ch],
// 3 sum dz.  Nothing else is written.
template <int KIND, int V>
__global__ __launch_bounds__(256) void occ_bn_bwd_sums_kernel(BnDy src, const float* __restrict__ r, int c, int plane,
                                                              float count, double* __restrict__ partials) {
    constexpr int NS = KIND == kBnLast ? 4 : 2;
    const int ch = blockIdx.y, env = blockIdx.z;
    const size_t base = ((size_t)env * c + ch) * plane;
    float pooled = 0.f, cw = 0.f;
    if constexpr (KIND == kBnPool) pooled = src.gf[(size_t)env * c + ch] / count;
    if constexpr (KIND == kBnLast) cw = src.clsw[ch];
    double sum[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) sum[k] = 0.0;
    const int lo = blockIdx.x * kBwdChunk, hi = min(lo + kBwdChunk, plane);
    for (int i = lo + V * (int)threadIdx.x; i < hi; i += 256 * V) {
        float rv[V], dy[V], dz[V];
        bn_load<V>(r + base + i, rv);
        bn_form_dy<KIND, V>(src, base + i, (size_t)env * plane + i, pooled, cw, dy, dz);
        if constexpr (KIND == kBnLast) {
            float yv[V];
            bn_load<V>(src.y4 + base + i, yv);
#pragma unroll
            for (int q = 0; q < V; ++q) {
                sum[2] = fma((double)dz[q], (double)yv[q], sum[2]);
                sum[3] += (double)dz[q];
            }
        }
#pragma unroll
        for (int q = 0; q < V; ++q) {
            sum[0] += (double)dy[q];
            sum[1] = fma((double)dy[q], (double)rv[q], sum[1]);
        }
    }
    bwd_block_partials(sum, partials + ((((size_t)ch * gridDim.z + env) * gridDim.x) + blockIdx.x) * NS);
}

// One wave per channel.  gamma: the layer's packed scale slot; gscale, gshift: the dbn_scale / dbn_shift slots of the packed
// gradient; gcls (ns == 4): dcls_w[8] | dcls_b, dcls_b from channel 0 (every channel's blocks form the same dz);
// abc: A[256] | B[256] | C[256]; m = n plane.
__global__ __launch_bounds__(64) void occ_bn_bwd_final_kernel(const double* __restrict__ partials, int nparts, int ns, double m,
                                                              const float* __restrict__ gamma, BnCoef co,
                                                              float* __restrict__ gscale, float* __restrict__ gshift,
                                                              float* __restrict__ gcls, float* __restrict__ abc) {
    const int ch = blockIdx.x;
    const double* pe = partials + (size_t)ch * nparts * ns;
    const double sdy = bwd_wave_strided_sum(pe, nparts, ns);
    const double sdyr = bwd_wave_strided_sum(pe + 1, nparts, ns);
    double szy = 0.0, sz = 0.0;
    if (ns == 4) {
        szy = bwd_wave_strided_sum(pe + 2, nparts, ns);
        sz = bwd_wave_strided_sum(pe + 3, nparts, ns);
    }
    if (threadIdx.x != 0) return;
    const double mu = co.mu[ch], rstd = co.rstd[ch];
    const double dgamma = rstd * (sdyr - mu * sdy);
    const double s = (double)gamma[ch] * rstd;
    const double C = -s * rstd * dgamma / m;
    gscale[ch] = (float)dgamma;
    gshift[ch] = (float)sdy;
    abc[ch] = (float)s;
    abc[256 + ch] = (float)(-s * sdy / m - C * mu);
    abc[512 + ch] = (float)C;
    if (ns == 4) {
        gcls[ch] = (float)szy;
        if (ch == 0) gcls[kEncCh] = (float)sz;
    }
}

// dU = [r > 0] (A dY + C r + B) to du (n, c, plane), which may be the dY buffer itself (every lane reads its pixels before
// it writes them).  partials[(ch * n + env) * chunks + chunk] = sum dU.
template <int KIND, int V>
__global__ __launch_bounds__(256) void occ_bn_bwd_act_kernel(BnDy src, float* du, const float* __restrict__ r,
                                                             const float* __restrict__ abc, int c, int plane, float count,
                                                             double* __restrict__ partials) {
    const int ch = blockIdx.y, env = blockIdx.z;
    const size_t base = ((size_t)env * c + ch) * plane;
    const float A = abc[ch], B = abc[256 + ch], C = abc[512 + ch];
    float pooled = 0.f, cw = 0.f;
    if constexpr (KIND == kBnPool) pooled = src.gf[(size_t)env * c + ch] / count;
    if constexpr (KIND == kBnLast) cw = src.clsw[ch];
    double sum[1] = {0.0};
    const int lo = blockIdx.x * kBwdChunk, hi = min(lo + kBwdChunk, plane);
    for (int i = lo + V * (int)threadIdx.x; i < hi; i += 256 * V) {
        float rv[V], dy[V], dz[V], uv[V];
        bn_load<V>(r + base + i, rv);
        bn_form_dy<KIND, V>(src, base + i, (size_t)env * plane + i, pooled, cw, dy, dz);
#pragma unroll
        for (int q = 0; q < V; ++q) {
            uv[q] = rv[q] > 0.f ? fmaf(A, dy[q], fmaf(C, rv[q], B)) : 0.f;
            sum[0] += (double)uv[q];
        }
        bn_store<V>(du + base + i, uv);
    }
    bwd_block_partials(sum, partials + (((size_t)ch * gridDim.z + env) * gridDim.x) + blockIdx.x);
}

// ---- host side -----------------------------------------------------------------------------------------------------

// One layer's batch statistics and its y from the kept r: 3 launches.  gamma / beta: the layer's packed scale / shift
// slots.  feats: the last down (y is `last`); cls: the last decoder level (add is its skip).
static void bn_fwd_layer(const BnTrain& bn, int layer, int c, int plane, int n, const float* gamma, const float* beta,
                         const float* r, float* y, const float* add, float* feats, const float* cls, float* prob, float* pkeep,
                         hipStream_t st) {
    const int chunks = bwd_chunks(plane);
    const dim3 grid(chunks, c, n);
    const bool v4 = plane % 4 == 0;
    const BnCoef co = bn_coef(bn, layer, c);
    if (v4) hipLaunchKernelGGL((occ_bn_stats_kernel<4>), grid, dim3(256), 0, st, r, c, plane, bn.part);
    else hipLaunchKernelGGL((occ_bn_stats_kernel<1>), grid, dim3(256), 0, st, r, c, plane, bn.part);
    hipLaunchKernelGGL(occ_bn_fwd_final_kernel, dim3(c), dim3(64), 0, st, (const double*)bn.part, n * chunks, c,
                       (double)n * plane, gamma, beta, co, bn.stats + 2 * bn_ch_off(layer));
    if (feats) {
        hipLaunchKernelGGL(occ_bn_apply_pool_kernel, dim3(c, n), dim3(256), 0, st, r, y, (const float*)co.s, (const float*)co.t, c,
                           plane, feats);
    } else if (cls) {
        const dim3 cgrid(chunks, 1, n);
        if (v4)
            hipLaunchKernelGGL((occ_bn_apply_cls_kernel<4>), cgrid, dim3(256), 0, st, r, y, add, (const float*)co.s,
                               (const float*)co.t, cls, plane, prob, pkeep);
        else
            hipLaunchKernelGGL((occ_bn_apply_cls_kernel<1>), cgrid, dim3(256), 0, st, r, y, add, (const float*)co.s,
                               (const float*)co.t, cls, plane, prob, pkeep);
    } else if (v4) {
        hipLaunchKernelGGL((occ_bn_apply_kernel<4>), grid, dim3(256), 0, st, r, y, add, (const float*)co.s, (const float*)co.t, c,
                           plane);
    } else {
        hipLaunchKernelGGL((occ_bn_apply_kernel<1>), grid, dim3(256), 0, st, r, y, add, (const float*)co.s, (const float*)co.t, c,
                           plane);
    }
}

template <int KIND, int V>
static void bn_bwd_act_t(const BnTrain& bn, const BnCoef& co, int c, int plane, int n, const BnDy& src, float* du, const float* r,
                         const float* gamma, float* gscale, float* gshift, float* gcls, char* scratch, hipStream_t st) {
    const int chunks = bwd_chunks(plane);
    const dim3 grid(chunks, c, n);
    hipLaunchKernelGGL((occ_bn_bwd_sums_kernel<KIND, V>), grid, dim3(256), 0, st, src, r, c, plane, (float)plane, (double*)scratch);
    hipLaunchKernelGGL(occ_bn_bwd_final_kernel, dim3(c), dim3(64), 0, st, (const double*)scratch, n * chunks,
                       KIND == kBnLast ? 4 : 2, (double)n * plane, gamma, co, gscale, gshift, gcls, bn.abc);
    hipLaunchKernelGGL((occ_bn_bwd_act_kernel<KIND, V>), grid, dim3(256), 0, st, src, du, r, (const float*)bn.abc, c, plane,
                       (float)plane, (double*)scratch);
}

// The activation step of one layer in train mode: dgamma, dbeta (and the classifier's gradient) are final, dU is in `du`
// and the n chunks partials of sum dU per channel are in scratch for bwd_layer_tail (one sum).  3 launches.
static void bn_bwd_act(const BnTrain& bn, int layer, int c, int plane, int n, const BnDy& src, float* du, const float* r,
                       const float* gamma, float* gscale, float* gshift, float* gcls, char* scratch, hipStream_t st) {
    const BnCoef co = bn_coef(bn, layer, c);
    const bool v4 = plane % 4 == 0;
#define OCC_BN_BWD(KIND)                                                                                          \
    if (v4) bn_bwd_act_t<KIND, 4>(bn, co, c, plane, n, src, du, r, gamma, gscale, gshift, gcls, scratch, st);    \
    else bn_bwd_act_t<KIND, 1>(bn, co, c, plane, n, src, du, r, gamma, gscale, gshift, gcls, scratch, st)
    if (src.gp) {
        OCC_BN_BWD(kBnLast);
    } else if (src.gf) {
        OCC_BN_BWD(kBnPool);
    } else {
        OCC_BN_BWD(kBnPlain);
    }
#undef OCC_BN_BWD
}

struct FullBnTrainWs {
    FullTrainWs full;
    size_t coef, abc, part, total;
};

inline FullBnTrainWs full_bn_train_ws_layout(int img, int n, bool separable) {
    FullBnTrainWs l;
    l.full = full_train_ws_layout(img, n, separable);
    size_t at = l.full.total;
    auto take = [&](size_t bytes) {
        const size_t o = at;
        at += enc_align(bytes);
        return o;
    };
    l.coef = take((size_t)24 * kBnChannels);
    l.abc = take((size_t)3 * 256 * sizeof(float));
    size_t part = 0;
    EncLayer L[16];
    enc_train_layers(img, separable, L);
    for (int i = 0; i < 16; ++i) {
        const size_t b = (size_t)L[i].cout * n * bwd_chunks(L[i].Ho * L[i].Ho) * 2 * sizeof(double);
        part = b > part ? b : part;
    }
    for (int j = 0; j < kEncLevels; ++j) {
        const int H = (img >> kEncLevels) << (j + 1);
        const size_t b = (size_t)(kEncCh << (kEncLevels - 1 - j)) * n * bwd_chunks(H * H) * 2 * sizeof(double);
        part = b > part ? b : part;
    }
    l.part = take(part);
    l.total = at;
    return l;
}

inline BnTrain full_bn_ptrs(const FullBnTrainWs& l, char* ws, float* stats) {
    return {ws + l.coef, (float*)(ws + l.abc), (double*)(ws + l.part), stats};
}

// every BatchNorm of the step sees at least two values per channel: the deepest plane is (S / 32)^2
inline bool bn_train_shape_ok(int img, int n) { return (long long)n * (img / 32) * (img / 32) >= 2; }
