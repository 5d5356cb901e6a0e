// occ_adamw.hpp -- AdamW on the packed parameters of the joint training step (occ_net_adamw_*; header: "The optimizer of
// the joint training step").  Part of the single translation unit occ_kernels.hip (included inside namespace occ; not a
// stand-alone header).
//
// The joint backward (occ_fullnet_backward, occ_sep_fullnet_backward, occ_fullnet_bn_backward) writes one packed gradient
// per part, and the next forward reads one packed buffer per part.  Every packed slot is a permutation of a checkpoint
// tensor or one half of a BatchNorm (scale, shift) pair, and AdamW is elementwise, so the step runs in packed order: a
// master buffer `theta` per part holds the raw values (gamma and beta in the scale / shift slots), the moments lie next to
// it in the same order, and ONE launch
//   * applies the chain rule from (d scale, d shift) to (d gamma, d beta) in the BatchNorm slots (running statistics),
//   * takes torch.optim.AdamW's step on every slot of both parts and of an optional plain segment (the grad head),
//   * writes the packed buffer the next forward reads: a copy of theta, the BatchNorm slots folded with the running
//     statistics from the UPDATED gamma and beta (running statistics) or left as they are (batch statistics).
//
// The work is cut into segments from the layer walk of enc_packed_floats / dec_packed_floats: per layer a plain run (conv
// weights and bias) and a pair run (scale[c] | shift[c]), then the decoder's tail and the head.  Every segment starts on a
// 16-byte boundary of its buffer (all channel counts are multiples of 4), so a thread moves 16 bytes at a time; only the
// last four floats of a plain run can be partial (the classifier's 9 floats, the head's 514) and go element by element.
// One thread owns a channel's (gamma, beta) pair, because the new shift needs the new gamma.  The fold and the chain rule
// are f64 with every operation rounded on its own (fp contract off around them: no fused multiply-add), as the unfused
// torch ops of nettrain.fold_bn_vectors and nettrain.bn_param_grads round them, and go to f32 once.  No atomics, no
// reductions, no LDS.

constexpr int kAdamwBlock = 256;
constexpr int kAdamwPerBlock = kAdamwBlock * 4;  // floats (plain run) or channels (pair run) of one block
constexpr int kAdamwMaxSegs = 48;                // 21 layers x 2, the decoder's tail, the head

struct AdamwPart {  // one packed buffer set: the encoder's, the decoder's, the head's (out == nullptr: nothing to write)
    float* theta;
    float* m;
    float* v;
    const float* grad;
    float* out;
};

struct AdamwSeg {
    int part;      // index into AdamwArgs::part
    int pair;      // 0: a plain run of `count` floats; 1: scale[count] | shift[count]
    int off;       // first float of the run in its part
    int count;
    int stat_off;  // pair: mean[count] | var[count] at stats + stat_off
    int block0;    // first block of the run
};

struct AdamwCoef {  // torch.optim.AdamW's scalars, formed in double on the host and rounded to f32 once
    float decay;     // 1 - lr * weight_decay
    float w1;        // 1 - beta1
    float b2;        // beta2
    float w2;        // 1 - beta2
    float neg_step;  // -lr / (1 - beta1^step)
    float bc2_sqrt;  // sqrt(1 - beta2^step)
    float eps;
};

struct AdamwArgs {
    AdamwPart part[3];
    const float* stats;
    AdamwSeg seg[kAdamwMaxSegs];
    int nseg;
    int fold;  // 1: the pair runs hold (d scale, d shift) and write (scale, shift); 0: d gamma, d beta; gamma, beta
    AdamwCoef k;
};

// The segments of both parts (and of a head of `head_count` floats) -> the number of blocks; stat_floats: the size of the
// running-statistics buffer, mean[c] | var[c] per layer.
inline int adamw_plan(bool separable, int head_count, AdamwArgs* a, int* stat_floats = nullptr) {
    int nseg = 0, blocks = 0, stat = 0;
    auto run = [&](int part, int pair, int off, int count) {
        a->seg[nseg++] = AdamwSeg{part, pair, off, count, stat, blocks};
        blocks += (count + kAdamwPerBlock - 1) / kAdamwPerBlock;
        if (pair) stat += 2 * count;
    };
    int off = 0;
    auto layer = [&](int part, int cin, int cout, bool sep) {
        const int plain = (int)enc_layer_floats(cin, cout, sep) - 2 * cout;  // conv weights and bias
        run(part, 0, off, plain);
        run(part, 1, off + plain, cout);
        off += plain + 2 * cout;
    };
    layer(0, 4, kEncCh, separable);
    for (int lv = 0; lv < kEncLevels; ++lv) {
        const int c = kEncCh << lv;
        layer(0, c, c, separable);
        layer(0, c, c, separable);
        layer(0, c, 2 * c, false);
    }
    off = 0;
    for (int j = 0; j < kEncLevels; ++j) {
        const int c = kEncCh << (kEncLevels - 1 - j);
        layer(1, 2 * c, c, false);
    }
    run(1, 0, off, kEncCh + 1);  // the classifier
    if (head_count > 0) run(2, 0, 0, head_count);
    a->nseg = nseg;
    if (stat_floats) *stat_floats = stat;
    return blocks;
}

// No contraction is left to the compiler from here to the kernel: every rounding below is written out.
#pragma clang fp contract(off)

// torch.optim.AdamW's rule in f32 with the roundings of its foreach path on the device, where every torch op rounds to f32
// on its own and a multiply-add inside one op is fused: mul_ (decay); lerp_ = fma(w, g - m, m) for a weight below 0.5;
// mul_ (beta2) and addcmul_ = fma(1 - beta2, g g, v); sqrt, div, add (eps); addcdiv_ = fma(-lr / bc1, m / denom, p).
__device__ __forceinline__ void adamw_update(const AdamwCoef& k, float g, float& p, float& m, float& v) {
    p = p * k.decay;
    const float diff = g - m;
    m = k.w1 < 0.5f ? __builtin_fmaf(k.w1, diff, m) : __builtin_fmaf(-diff, 1.f - k.w1, g);
    v = __builtin_fmaf(k.w2, g * g, v * k.b2);
    const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
    p = __builtin_fmaf(k.neg_step, m / denom, p);
}

// The BatchNorm arithmetic in f64, every operation rounded on its own: a fused multiply-add would differ from torch's
// separate multiply and subtract in the last bit.
__device__ __forceinline__ double bn_rstd(float var) { return 1.0 / sqrt((double)var + kBnEps); }
// d gamma of (d scale, d shift): nettrain.bn_param_grads
__device__ __forceinline__ float bn_dgamma(float dscale, float dshift, double mean, double rstd) {
    return (float)(((double)dscale - mean * (double)dshift) * rstd);
}
// (scale, shift) of (gamma, beta): nettrain.fold_bn_vectors; shift takes the unrounded scale
__device__ __forceinline__ void bn_fold(float gamma, float beta, double mean, double rstd, float& scale, float& shift) {
    const double sc = (double)gamma * rstd;
    scale = (float)sc;
    shift = (float)((double)beta - mean * sc);
}
#pragma clang fp contract(fast)

struct alignas(16) AdamwF4 {  // four consecutive floats of a buffer, moved as one 16-byte access
    float e[4];
};

// UPDATE = false: only the packed output is (re)written from theta, for a change of the BatchNorm mode.
template <bool UPDATE>
__global__ __launch_bounds__(kAdamwBlock) void occ_adamw_kernel(const AdamwArgs a) {
    int s = 0;
    while (s + 1 < a.nseg && a.seg[s + 1].block0 <= (int)blockIdx.x) ++s;  // wave-uniform
    const AdamwSeg sg = a.seg[s];
    const AdamwPart pt = a.part[sg.part];
    const int i = ((int)blockIdx.x - sg.block0) * kAdamwPerBlock + (int)threadIdx.x * 4;
    if (i >= sg.count) return;

    if (!sg.pair || !a.fold) {
        // a plain run; without the fold a pair is a plain run of 2 c floats
        const int count = sg.pair ? 2 * sg.count : sg.count;
        for (int base = i; base < count; base += sg.count) {  // pair: the gamma float4, then the beta float4
            const int at = sg.off + base;
            if (base + 4 <= count) {
                AdamwF4 p = *(const AdamwF4*)(pt.theta + at);
                if (UPDATE) {
                    AdamwF4 m = *(const AdamwF4*)(pt.m + at), v = *(const AdamwF4*)(pt.v + at);
                    const AdamwF4 g = *(const AdamwF4*)(pt.grad + at);
#pragma unroll
                    for (int j = 0; j < 4; ++j) adamw_update(a.k, g.e[j], p.e[j], m.e[j], v.e[j]);
                    *(AdamwF4*)(pt.theta + at) = p;
                    *(AdamwF4*)(pt.m + at) = m;
                    *(AdamwF4*)(pt.v + at) = v;
                }
                if (pt.out) *(AdamwF4*)(pt.out + at) = p;
            } else {
                for (int e = at; e < sg.off + count; ++e) {
                    float p = pt.theta[e];
                    if (UPDATE) {
                        float m = pt.m[e], v = pt.v[e];
                        adamw_update(a.k, pt.grad[e], p, m, v);
                        pt.theta[e] = p;
                        pt.m[e] = m;
                        pt.v[e] = v;
                    }
                    if (pt.out) pt.out[e] = p;
                }
            }
            if (!sg.pair) break;
        }
        return;
    }

    // a pair run with the fold: channels i .. i + 3 (every channel count is a multiple of 4)
    const int ga = sg.off + i, be = ga + sg.count;
    const AdamwF4 mean = *(const AdamwF4*)(a.stats + sg.stat_off + i);
    const AdamwF4 var = *(const AdamwF4*)(a.stats + sg.stat_off + sg.count + i);
    AdamwF4 gamma = *(const AdamwF4*)(pt.theta + ga), beta = *(const AdamwF4*)(pt.theta + be);
    AdamwF4 mg, vg, mb, vb, dscale, dshift;
    if (UPDATE) {
        mg = *(const AdamwF4*)(pt.m + ga), vg = *(const AdamwF4*)(pt.v + ga);
        mb = *(const AdamwF4*)(pt.m + be), vb = *(const AdamwF4*)(pt.v + be);
        dscale = *(const AdamwF4*)(pt.grad + ga), dshift = *(const AdamwF4*)(pt.grad + be);
    }
    AdamwF4 scale, shift;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double mu = (double)mean.e[j];
        const double rstd = bn_rstd(var.e[j]);
        if (UPDATE) {
            adamw_update(a.k, bn_dgamma(dscale.e[j], dshift.e[j], mu, rstd), gamma.e[j], mg.e[j], vg.e[j]);
            adamw_update(a.k, dshift.e[j], beta.e[j], mb.e[j], vb.e[j]);
        }
        bn_fold(gamma.e[j], beta.e[j], mu, rstd, scale.e[j], shift.e[j]);
    }
    if (UPDATE) {
        *(AdamwF4*)(pt.theta + ga) = gamma;
        *(AdamwF4*)(pt.theta + be) = beta;
        *(AdamwF4*)(pt.m + ga) = mg;
        *(AdamwF4*)(pt.v + ga) = vg;
        *(AdamwF4*)(pt.m + be) = mb;
        *(AdamwF4*)(pt.v + be) = vb;
    }
    *(AdamwF4*)(pt.out + ga) = scale;
    *(AdamwF4*)(pt.out + be) = shift;
}

// One launch over the plan of `a` (part, stats, fold and k already set).
template <bool UPDATE>
inline void adamw_launch(bool separable, int head_count, AdamwArgs& a, hipStream_t st) {
    const int blocks = adamw_plan(separable, head_count, &a);
    hipLaunchKernelGGL(occ_adamw_kernel<UPDATE>, dim3(blocks), dim3(kAdamwBlock), 0, st, a);
}
