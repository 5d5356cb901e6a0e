// occ_criterion.hpp -- the pretrainer's segmentation criterion on a predicted occlusion map (pretrainer.py:89,127-141,
// 176-189): every sum and count that loss.py's BinaryDiceLoss (p = 2), nn.BCELoss and the accuracy / IoU lines need, from
// ONE read of pred and target, and the criterion's gradient with respect to pred.  Part of the single translation unit
// occ_kernels.hip (included inside namespace occ, after occ_decoder.hpp, whose pixel-stride convention for the target it
// follows).
//
//   occ_seg_criterion_kernel        per (env, block of 4096 pixels): S_pt = sum p t, S_pp = sum p^2, S_tt = sum t^2,
//                                   S_bce = sum -(t max(log p, -100) + (1 - t) max(log(1 - p), -100)) as f64 block
//                                   partials in caller scratch, and the three counts of occ_seg_metrics_kernel (agree,
//                                   intersection, union at > 0.5; int64 atomic adds, which commute exactly).
//   occ_seg_criterion_final_kernel  per env: the block partials summed in block order, f64 -> sums[env][4].
//   occ_seg_criterion_grad_kernel   elementwise grad_pred: Dice a_i t + b_i p, or BCE g (p - t) / max(p (1 - p), 1e-12).
//
// Summation order (the reproducibility rule of DESIGN §4.4: no floating-point atomics, a fixed order at every stage):
//   thread   16 pixels in a fixed order (four groups of four consecutive pixels, group j at 4 (tid + 256 j)); the same
//            assignment whether the group is fetched by one 16-byte load or by four 4-byte loads, so the load width
//            (a function of alignment and stride only) changes no bit
//   wave     six __shfl_down steps (32, 16, 8, 4, 2, 1)
//   block    the four wave sums in wave order -> scratch[(env, block)][4]
//   env      the (S^2 + 4095) / 4096 block partials in block order
// The block grid is a function of S alone and blockIdx.y is the env, so an env's sums do not depend on the batch size, on
// its position in the batch, on how the host chunks the batch or on the run.
//
// Depth of the f32 addition chain: 0.  Every addition, at every stage, is f64.  p t, p^2 and t^2 are formed in f64 from
// the f32 inputs and are exact there (24-bit x 24-bit significands fit in 53 bits).  The only f32 roundings are the two
// logf per pixel (log p and log(1 - p), with 1 - p formed in f32 as nn.BCELoss does): relative error about 1 ulp = 6e-8
// of a term that is at most 100, and for p < 0.5 the rounding of 1 - p adds at most 6e-8 absolute to log(1 - p).  The f64
// chain is at most 16 + 6 + 4 + 256 additions deep (S = 1024), relative error below 282 x 1.1e-16 = 3.2e-14 of the sum of
// magnitudes.  So S_pt, S_pp, S_tt are within 3.2e-14 relative of the exact sums and S_bce / S^2, the per-pixel mean the
// tests compare, is within about 1.3e-7 x max(1, mean) of the f64 host model: three orders below the 1e-4 bar of this
// family (tests/test_gpu_criterion.py).  The gradient is formed in f64 from f64 coefficients and rounded once to f32
// (relative error 6e-8).

constexpr int kCritBlock = 256;
constexpr int kCritGroups = 4;                                 // groups of four consecutive pixels per thread
constexpr int kCritPerBlock = kCritBlock * 4 * kCritGroups;  // 4096, = kSegMetricsPerBlock

inline int crit_blocks(int npix) { return (npix + kCritPerBlock - 1) / kCritPerBlock; }

// The four pixels i .. i + 3 of one env (i % 4 == 0); pixels at or beyond npix read as 0 and are masked by the caller.
// VEC: base 16-byte aligned, npix % 4 == 0 (so the group is whole) and, for the target, stride 1.
template <bool VEC>
__device__ __forceinline__ void crit_load4(const float* __restrict__ base, int stride, int i, int npix, float v[4]) {
    if constexpr (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(base + i);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = i + c < npix ? base[(size_t)(i + c) * stride] : 0.f;
    }
}

template <bool VP, bool VT>
__global__ __launch_bounds__(kCritBlock) void occ_seg_criterion_kernel(const float* __restrict__ pred,
                                                                       const float* __restrict__ target, int tstride, int npix,
                                                                       double* __restrict__ partials,
                                                                       unsigned long long* __restrict__ counts) {
    __shared__ double fpart[kCritBlock / 64][4];
    __shared__ int ipart[kCritBlock / 64][3];
    const float* pe = pred + (size_t)blockIdx.y * npix;
    const float* te = target + (size_t)blockIdx.y * npix * tstride;
    const int lo = blockIdx.x * kCritPerBlock;
    double s_pt = 0.0, s_pp = 0.0, s_tt = 0.0, s_bce = 0.0;
    int agree = 0, inter = 0, uni = 0;
#pragma unroll
    for (int j = 0; j < kCritGroups; ++j) {
        const int i = lo + 4 * (threadIdx.x + kCritBlock * j);
        if (i >= npix) break;  // groups ascend with j
        float p[4], t[4];
        crit_load4<VP>(pe, 1, i, npix, p);
        crit_load4<VT>(te, tstride, i, npix, t);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (i + c >= npix) break;
            const double pd = p[c], td = t[c];
            s_pt = fma(pd, td, s_pt);
            s_pp = fma(pd, pd, s_pp);
            s_tt = fma(td, td, s_tt);
            const double lp = fmaxf(logf(p[c]), -100.f), lq = fmaxf(logf(1.f - p[c]), -100.f);
            s_bce -= fma(td, lp, (1.0 - td) * lq);
            const bool a = p[c] > 0.5f, b = t[c] > 0.5f;
            agree += a == b;
            inter += a && b;
            uni += a || b;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s_pt += __shfl_down(s_pt, d);
        s_pp += __shfl_down(s_pp, d);
        s_tt += __shfl_down(s_tt, d);
        s_bce += __shfl_down(s_bce, d);
        agree += __shfl_down(agree, d);
        inter += __shfl_down(inter, d);
        uni += __shfl_down(uni, d);
    }
    const int wave = threadIdx.x / 64;
    if (threadIdx.x % 64 == 0) {
        fpart[wave][0] = s_pt, fpart[wave][1] = s_pp, fpart[wave][2] = s_tt, fpart[wave][3] = s_bce;
        ipart[wave][0] = agree, ipart[wave][1] = inter, ipart[wave][2] = uni;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double sum = 0.0;
        for (int k = 0; k < kCritBlock / 64; ++k) sum += fpart[k][threadIdx.x];
        partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = sum;
    }
    if (counts && threadIdx.x < 3) {
        int sum = 0;
        for (int k = 0; k < kCritBlock / 64; ++k) sum += ipart[k][threadIdx.x];
        atomicAdd(counts + (size_t)blockIdx.y * 3 + threadIdx.x, (unsigned long long)sum);
    }
}

// sums[env][k] = the env's nblk block partials of sum k in block order.  One thread per (env, k).
__global__ __launch_bounds__(64) void occ_seg_criterion_final_kernel(const double* __restrict__ partials, int nblk, int n_env,
                                                                     double* __restrict__ sums) {
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= n_env * 4) return;
    const int env = idx >> 2, k = idx & 3;
    const double* pe = partials + (size_t)env * nblk * 4 + k;
    double sum = 0.0;
    for (int b = 0; b < nblk; ++b) sum += pe[(size_t)b * 4];
    sums[idx] = sum;
}

// mode OCC_CRITERION_DICE: grad = coef[env][0] t + coef[env][1] p, the derivative of 1 - num / den (num = S_pt + smooth,
// den = S_pp + S_tt + smooth) with the upstream gradient and the reduction folded into the coefficients by the host.
// mode OCC_CRITERION_BCE: grad = coef[env][0] (p - t) / max(p (1 - p), 1e-12), nn.BCELoss's backward rule.
template <bool VP, bool VT, bool BCE>
__global__ __launch_bounds__(kCritBlock) void occ_seg_criterion_grad_kernel(const float* __restrict__ pred,
                                                                            const float* __restrict__ target, int tstride,
                                                                            int npix, const double* __restrict__ coef,
                                                                            float* __restrict__ grad) {
    const float* pe = pred + (size_t)blockIdx.y * npix;
    const float* te = target + (size_t)blockIdx.y * npix * tstride;
    float* ge = grad + (size_t)blockIdx.y * npix;
    const double a = coef[(size_t)blockIdx.y * 2], b = coef[(size_t)blockIdx.y * 2 + 1];
    const int lo = blockIdx.x * kCritPerBlock;
#pragma unroll
    for (int j = 0; j < kCritGroups; ++j) {
        const int i = lo + 4 * (threadIdx.x + kCritBlock * j);
        if (i >= npix) break;
        float p[4], t[4], g[4];
        crit_load4<VP>(pe, 1, i, npix, p);
        crit_load4<VT>(te, tstride, i, npix, t);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double pd = p[c], td = t[c];
            if constexpr (BCE)
                g[c] = (float)(a * (pd - td) / fmax(pd * (1.0 - pd), 1e-12));
            else
                g[c] = (float)fma(a, td, b * pd);
        }
        if constexpr (VP) {  // grad_pred shares pred's shape; its alignment is part of the VP condition
            *reinterpret_cast<float4*>(ge + i) = make_float4(g[0], g[1], g[2], g[3]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (i + c < npix) ge[i + c] = g[c];
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------

inline bool crit_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static void crit_launch(const float* pred, const float* target, int tstride, int n_env, int npix, double* partials,
                        unsigned long long* counts, hipStream_t st) {
    const dim3 grid(crit_blocks(npix), n_env), block(kCritBlock);
    const bool vp = npix % 4 == 0 && crit_aligned16(pred);
    const bool vt = vp && tstride == 1 && crit_aligned16(target);
    if (vt)
        hipLaunchKernelGGL((occ_seg_criterion_kernel<true, true>), grid, block, 0, st, pred, target, tstride, npix, partials, counts);
    else if (vp)
        hipLaunchKernelGGL((occ_seg_criterion_kernel<true, false>), grid, block, 0, st, pred, target, tstride, npix, partials, counts);
    else
        hipLaunchKernelGGL((occ_seg_criterion_kernel<false, false>), grid, block, 0, st, pred, target, tstride, npix, partials, counts);
}

template <bool BCE>
static void crit_grad_launch(const float* pred, const float* target, int tstride, int n_env, int npix, const double* coef,
                             float* grad, hipStream_t st) {
    const dim3 grid(crit_blocks(npix), n_env), block(kCritBlock);
    const bool vp = npix % 4 == 0 && crit_aligned16(pred) && crit_aligned16(grad);
    const bool vt = vp && tstride == 1 && crit_aligned16(target);
    if (vt)
        hipLaunchKernelGGL((occ_seg_criterion_grad_kernel<true, true, BCE>), grid, block, 0, st, pred, target, tstride, npix, coef, grad);
    else if (vp)
        hipLaunchKernelGGL((occ_seg_criterion_grad_kernel<true, false, BCE>), grid, block, 0, st, pred, target, tstride, npix, coef, grad);
    else
        hipLaunchKernelGGL((occ_seg_criterion_grad_kernel<false, false, BCE>), grid, block, 0, st, pred, target, tstride, npix, coef, grad);
}
