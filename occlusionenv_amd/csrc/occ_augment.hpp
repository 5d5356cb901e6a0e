// occ_augment.hpp -- the pretraining input pipeline on the device (occ_augment_*; header: "The pretraining input
// pipeline").  Part of the single translation unit occ_kernels.hip (included inside namespace occ; not a stand-alone header).
//
// The dataset is resident: per frame one u32 word per pixel (R | G << 8 | B << 16 | label << 24) and one int16 of depth,
// decoded and resized once.  A batch is a gather by frame index plus what dataset.py draws per sample: torchvision's
// ColorJitter on its PIL path (ImageEnhance.Brightness / Contrast / Color and the hue shift through PIL's HSV mode, in a
// random order), the horizontal flip, the division by 255 and Normalize(0.5, 0.25).  Every rounding of PIL's C code is
// written out below (tests/augment_model.py is the same arithmetic in numpy, checked against PIL), so a batch has the bits
// the reference's loader would hand the network for the same draws.
//
// Three of the four ops are point ops.  Contrast blends with the rounded mean luminance of the WHOLE image as it stands when
// contrast's turn comes, so there are two passes:
//   occ_augment_sum_kernel   per pixel the ops ordered before contrast, the integer luminance, a block sum; each block
//                            stores its partial as u32 with a plain store to workspace[sample][block].  Samples without
//                            jitter exit at once; the launch is skipped when the call has no parameter array.
//   occ_augment_out_kernel   every block adds the partials of its image (integer: order-free, bitwise reproducible),
//                            rounds the mean, runs the whole chain from the source word, reads through the flip and
//                            writes the four planes and the label; block 0 of a sample copies its grad and pos rows.
// Lane = pixel: one coalesced 4-byte and one 2-byte load, five coalesced float stores.  No atomics, no memset, LDS only for
// the block sum, no MFMA.

constexpr int kAugBlock = 256;          // pixels of one block
constexpr uint32_t kAugMaxPixels = 1u << 24;  // 255 * 2^24 < 2^32: the u32 luminance sum cannot overflow

inline int aug_blocks_per_image(int img) { return (img * img + kAugBlock - 1) / kAugBlock; }

// Nothing below may be contracted into a fused multiply-add: PIL rounds the multiply and the add separately, and the
// truncations that follow see the difference.
#pragma clang fp contract(off)

struct AugRgb {
    int r, g, b;
};

// PIL's convert("L")
__device__ __forceinline__ int aug_luminance(const AugRgb& c) {
    return (int)(((uint32_t)c.r * 19595u + (uint32_t)c.g * 38470u + (uint32_t)c.b * 7471u + 0x8000u) >> 16);
}

// PIL's ImagingBlend(deg, x, f) for one channel: f32, the product and the sum rounded separately, truncated; clipped only
// for a factor outside [0, 1] (inside, t lies between the two levels)
__device__ __forceinline__ int aug_blend(int deg, int x, float f, bool inside) {
    const float prod = f * (float)(x - deg);
    const float t = (float)deg + prod;
    if (inside) return (int)t;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}
__device__ __forceinline__ AugRgb aug_blend3(int dr, int dg, int db, const AugRgb& c, float f) {
    const bool inside = f >= 0.f && f <= 1.f;
    return AugRgb{aug_blend(dr, c.r, f, inside), aug_blend(dg, c.g, f, inside), aug_blend(db, c.b, f, inside)};
}

__device__ __forceinline__ int aug_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// PIL's RGB -> HSV -> (h + shift) mod 256 -> RGB (Convert.c: rgb2hsv_row, hsv2rgb_row).  The widths are PIL's: f32 where
// its variables are float, f64 where a double constant promotes the expression.
__device__ __forceinline__ AugRgb aug_hue(const AugRgb& c, int shift) {
    const int mx = max(c.r, max(c.g, c.b)), mn = min(c.r, min(c.g, c.b));
    int uh = 0, us = 0;
    const int v = mx;
    if (mx != mn) {
        const float cr = (float)(mx - mn);
        const float s = cr / (float)mx;
        const float rc = (float)(mx - c.r) / cr, gc = (float)(mx - c.g) / cr, bc = (float)(mx - c.b) / cr;
        float h;
        if (c.r == mx)
            h = bc - gc;
        else if (c.g == mx)
            h = (float)(2.0 + (double)rc - (double)bc);
        else
            h = (float)(4.0 + (double)gc - (double)rc);
        const double x = (double)h / 6.0 + 1.0;  // > 0: fmod(x, 1.0) = x - floor(x)
        h = (float)(x - floor(x));
        uh = aug_clip8((int)((double)h * 255.0));
        us = aug_clip8((int)((double)s * 255.0));
    }
    uh = (uh + shift) & 255;
    if (us == 0) return AugRgb{v, v, v};
    const float fh = (float)uh * 6.0f / 255.0f;
    const float fi = floorf(fh);
    const float f = fh - fi;
    const float fs = (float)us / 255.0f;
    const float vf = (float)v;
    const int p = aug_clip8((int)floorf(vf * (1.0f - fs) + 0.5f));
    const int q = aug_clip8((int)floorf(vf * (1.0f - fs * f) + 0.5f));
    const int t = aug_clip8((int)floorf(vf * (1.0f - fs * (1.0f - f)) + 0.5f));
    switch ((int)fi % 6) {
        case 0: return AugRgb{v, t, p};
        case 1: return AugRgb{q, v, p};
        case 2: return AugRgb{p, v, t};
        case 3: return AugRgb{p, q, v};
        case 4: return AugRgb{t, p, v};
        default: return AugRgb{v, p, q};
    }
}

constexpr int kAugBrightness = 0, kAugContrast = 1, kAugSaturation = 2, kAugHue = 3;

// One point op (not contrast)
__device__ __forceinline__ AugRgb aug_point_op(int op, const AugRgb& c, const OccAugmentParams& p) {
    if (op == kAugBrightness) return aug_blend3(0, 0, 0, c, p.brightness);
    if (op == kAugSaturation) {
        const int l = aug_luminance(c);
        return aug_blend3(l, l, l, c, p.saturation);
    }
    return aug_hue(c, p.hue_shift);
}

// The ops ordered before contrast: the pixel whose luminance contrast's mean is taken over
__device__ __forceinline__ AugRgb aug_before_contrast(AugRgb c, const OccAugmentParams& p) {
    for (int k = 0; k < 4; ++k) {
        const int op = (p.order >> (2 * k)) & 3;
        if (op == kAugContrast) break;
        c = aug_point_op(op, c, p);
    }
    return c;
}

// The whole chain with contrast's mean known
__device__ __forceinline__ AugRgb aug_chain(AugRgb c, const OccAugmentParams& p, int mean) {
    for (int k = 0; k < 4; ++k) {
        const int op = (p.order >> (2 * k)) & 3;
        c = op == kAugContrast ? aug_blend3(mean, mean, mean, c, p.contrast) : aug_point_op(op, c, p);
    }
    return c;
}

// int(sum / count + 0.5) of ImageEnhance.Contrast, in Python's f64
__device__ __forceinline__ int aug_round_mean(uint32_t sum, int pixels) { return (int)((double)sum / (double)pixels + 0.5); }

__device__ __forceinline__ float aug_convert(int level, bool normalize) {
    const float c = (float)level / 255.0f;
    return normalize ? (c - 0.5f) / 0.25f : c;
}

#pragma clang fp contract(fast)

__device__ __forceinline__ AugRgb aug_unpack(uint32_t w) { return AugRgb{(int)(w & 255u), (int)((w >> 8) & 255u), (int)((w >> 16) & 255u)}; }

// The frame a sample reads: the caller keeps idx in [0, m_frames); the clamp only keeps every address inside the store.
__device__ __forceinline__ size_t aug_frame(const int64_t* idx, int i, int m_frames) {
    const int64_t f = idx[i];
    return (size_t)(f < 0 ? 0 : (f >= m_frames ? m_frames - 1 : f));
}

// Sum of v over the block (every thread calls it; every thread gets the sum).
__device__ __forceinline__ uint32_t aug_block_sum(uint32_t v, uint32_t* lds) {
    v = (uint32_t)wave_sum_i((int)v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < kAugBlock / 64; ++w) s += lds[w];
    return s;
}

// grid (blocks_per_image, n)
__global__ __launch_bounds__(kAugBlock) void occ_augment_sum_kernel(const uint32_t* __restrict__ rgbl, int m_frames, int pixels,
                                                                    const int64_t* __restrict__ idx,
                                                                    const OccAugmentParams* __restrict__ params,
                                                                    uint32_t* __restrict__ partial) {
    __shared__ uint32_t lds[kAugBlock / 64];
    const int i = blockIdx.y;
    const OccAugmentParams p = params[i];
    if (!p.jitter) return;  // block-uniform
    const int px = (int)blockIdx.x * kAugBlock + (int)threadIdx.x;
    uint32_t l = 0;
    if (px < pixels) {
        const uint32_t w = rgbl[aug_frame(idx, i, m_frames) * (size_t)pixels + px];
        l = (uint32_t)aug_luminance(aug_before_contrast(aug_unpack(w), p));
    }
    const uint32_t s = aug_block_sum(l, lds);
    if (threadIdx.x == 0) partial[(size_t)i * gridDim.x + blockIdx.x] = s;
}

// grid (blocks_per_image, n); params == nullptr: no jitter, no flip, partial is not read
__global__ __launch_bounds__(kAugBlock) void occ_augment_out_kernel(const uint32_t* __restrict__ rgbl, const int16_t* __restrict__ depth,
                                                                    const float* __restrict__ pos, const float* __restrict__ grad,
                                                                    int m_frames, int img, const int64_t* __restrict__ idx,
                                                                    const OccAugmentParams* __restrict__ params,
                                                                    const uint32_t* __restrict__ partial, int normalize,
                                                                    float* __restrict__ out_img, float* __restrict__ out_label,
                                                                    float* __restrict__ out_grad, float* __restrict__ out_pos) {
    __shared__ uint32_t lds[kAugBlock / 64];
    const int i = blockIdx.y;
    const int pixels = img * img;
    const size_t frame = aug_frame(idx, i, m_frames);
    OccAugmentParams p{};
    if (params) p = params[i];
    int mean = 0;
    if (p.jitter) {  // block-uniform
        uint32_t s = 0;
        for (int b = threadIdx.x; b < (int)gridDim.x; b += kAugBlock) s += partial[(size_t)i * gridDim.x + b];
        mean = aug_round_mean(aug_block_sum(s, lds), pixels);
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) {
        out_grad[(size_t)i * 2 + threadIdx.x] = grad[frame * 2 + threadIdx.x];
        out_pos[(size_t)i * 2 + threadIdx.x] = pos[frame * 2 + threadIdx.x];
    }
    const int px = (int)blockIdx.x * kAugBlock + (int)threadIdx.x;
    if (px >= pixels) return;
    int src = px;
    if (p.flip) {
        const int y = px / img, x = px - y * img;
        src = y * img + (img - 1 - x);
    }
    const uint32_t w = rgbl[frame * (size_t)pixels + src];
    const int d = depth[frame * (size_t)pixels + src];
    AugRgb c = aug_unpack(w);
    if (p.jitter) c = aug_chain(c, p, mean);
    const bool norm = normalize != 0;
    float* o = out_img + (size_t)i * 4 * pixels + px;
    o[0] = aug_convert(c.r, norm);
    o[(size_t)pixels] = aug_convert(c.g, norm);
    o[(size_t)2 * pixels] = aug_convert(c.b, norm);
    o[(size_t)3 * pixels] = aug_convert(d, norm);
    out_label[(size_t)i * pixels + px] = (w >> 24) ? 1.0f : 0.0f;
}
