// occ_resize.hpp -- PIL's Image.resize between two resident stores (occ_dataset_resize; header: "Resizing frames between
// resident stores").  Part of the single translation unit occ_kernels.hip (included inside namespace occ; not a
// stand-alone header).
//
// The reference renders at 512 x 512 and its reader shrinks every item to 256 x 256 with Image.resize(size) and no filter
// argument (dataset.py:65-67): BICUBIC for the "RGB" and the "I" image, NEAREST for the "1" image.  This is that call for
// a frame of the store of occ_augment.hpp: the three colour bytes through Resample.c's 8-bit path (22-bit fixed-point
// coefficients, the horizontal pass clipped to u8 before the vertical one), the depth through its 32-bit path (f64
// accumulation in tap order, each pass rounded to int32), the label byte through Geometry.c's nearest-neighbour scaling.
// tests/resize_model.py is the same arithmetic in numpy, checked against PIL.
//
// Workspace (8-byte aligned device memory; S = dst_img, R = src_img, K = resize_taps(R, S)), the same table for both axes:
//   double  k[S][K]       the normalised bicubic coefficients of output index xx, zero from count on
//   int32   kk[S][K]      their 8-bit form, (int)(k * 2^22 -+ 0.5)
//   int32   bounds[S][2]  xmin and count: output xx reads the inputs xmin .. xmin + count - 1
//   int32   nearest[S]    the input index the nearest-neighbour pass reads, clamped to [0, R - 1]
// in this order without padding: every array starts where the one before it ends.
//
//   occ_resize_table_kernel  lane = output index: precompute_coeffs and normalize_coeffs_8bpc of Resample.c, and the
//                            running sum of ImagingScaleAffine.  f64, no fused multiply-add.
//   occ_resize_kernel        one block per kResizeTile x kResizeTile output tile of one frame.  The tile's input window
//                            (the rows and columns its first and last outputs bound, at most kResizeWin on a side) goes
//                            into LDS as words and int16, the horizontal pass writes window-rows x tile-columns of u8
//                            triples and int32 depths into LDS, the vertical pass reads those and stores one word and one
//                            int16 per output pixel.  Thread = one tile column and every eighth row; the taps are the outer
//                            loop, so a coefficient is loaded once per thread and tap and the f64 sums still add in tap order.
// Supported sizes: min(R, ceil((min(kResizeTile, S) - 1) * R / S + 4 * max(R / S, 1)) + 2) <= kResizeWin: the window of a
// tile fits LDS.  That is every R / S <= 2 (any upscaling, non-integer ratios), and larger ratios where the source is at
// most kResizeWin pixels wide (9 -> 1).
// Frames whose slot is outside [0, m_frames) are skipped by whole blocks before any address is formed from the slot.
// No atomics, no allocation, plain stores, a fixed order of every sum: bitwise the same from call to call.

constexpr int kResizeTile = 32;   // output pixels on a side of one block's tile
constexpr int kResizeWin = 72;    // input pixels on a side of the largest window: (32 - 1) * 2 + 4 * 2 + 2
constexpr int kResizeBlock = 256;
constexpr int kResizeRowsH = (kResizeWin + kResizeBlock / kResizeTile - 1) / (kResizeBlock / kResizeTile);  // 9 window rows per thread
constexpr int kResizeRowsV = kResizeTile / (kResizeBlock / kResizeTile);                                    // 4 tile rows per thread
constexpr uint32_t kResizeMaxPixels = 1u << 24;

// Everything in f64 below rounds operation by operation, as the C of PIL does on the host
#pragma clang fp contract(off)

// Resample.c: ksize = (int)ceil(support) * 2 + 1; no output has more taps than the source has pixels
inline int resize_taps(int R, int S) {
    const double scale = (double)R / (double)S;
    const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
    const double k = ceil(support) * 2.0 + 1.0;
    return k < (double)R ? (int)k : R;
}

// The window bound of the header; both sizes already within [1, 4096]
inline bool resize_ratio_ok(int R, int S) {
    const double scale = (double)R / (double)S;
    const int t = S < kResizeTile ? S : kResizeTile;
    const double need = ceil((double)(t - 1) * scale + 4.0 * (scale < 1.0 ? 1.0 : scale)) + 2.0;
    return need <= (double)kResizeWin || R <= kResizeWin;
}

inline size_t resize_table_bytes(int R, int S) {
    const size_t K = (size_t)resize_taps(R, S);
    return (size_t)S * K * (sizeof(double) + sizeof(int32_t)) + (size_t)S * 3 * sizeof(int32_t);
}

struct ResizeTables {
    double* k;
    int32_t* kk;
    int32_t* bounds;
    int32_t* nearest;
};

inline ResizeTables resize_tables(void* workspace, int R, int S) {
    const size_t K = (size_t)resize_taps(R, S);
    ResizeTables t;
    t.k = (double*)workspace;
    t.kk = (int32_t*)(t.k + (size_t)S * K);
    t.bounds = t.kk + (size_t)S * K;
    t.nearest = t.bounds + (size_t)S * 2;
    return t;
}

// Resample.c bicubic_filter, a = -0.5
__device__ __forceinline__ double resize_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
    return 0.0;
}

// grid (ceil(S / 64)), lane = output index
__global__ __launch_bounds__(64) void occ_resize_table_kernel(int R, int S, int K, ResizeTables t) {
    const int xx = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (xx >= S) return;
    const double scale = (double)R / (double)S;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const double ss = 1.0 / filterscale;
    const double center = ((double)xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > R) xmax = R;
    xmax -= xmin;
    if (xmax > K) xmax = K;  // cannot happen (K is PIL's ksize or R); keeps every index inside the row
    double* k = t.k + (size_t)xx * K;
    int32_t* kk = t.kk + (size_t)xx * K;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
        const double w = resize_bicubic(((double)(x + xmin) - center + 0.5) * ss);
        k[x] = w;
        ww = ww + w;
    }
    for (int x = 0; x < K; ++x) {
        double v = 0.0;
        if (x < xmax) {
            v = k[x];
            if (ww != 0.0) v = v / ww;
        }
        k[x] = v;
        kk[x] = v < 0.0 ? (int)(-0.5 + v * 4194304.0) : (int)(0.5 + v * 4194304.0);
    }
    t.bounds[2 * xx] = xmin;
    t.bounds[2 * xx + 1] = xmax;
    // Geometry.c ImagingScaleAffine: xo = a * 0.5, then xo += a per output -- a running sum, not xx * a
    double xo = scale * 0.5;
    for (int x = 0; x < xx; ++x) xo = xo + scale;
    int src = (int)xo;
    t.nearest[xx] = src < 0 ? 0 : (src > R - 1 ? R - 1 : src);
}

// One 32-bit tap: the product and the sum rounded separately
__device__ __forceinline__ double resize_tap_f64(double acc, int pixel, double k) {
    const double p = (double)pixel * k;
    return acc + p;
}

// Resample.c ROUND_UP
__device__ __forceinline__ int resize_round(double acc) { return (int)(acc < 0.0 ? acc - 0.5 : acc + 0.5); }

#pragma clang fp contract(fast)

__device__ __forceinline__ int resize_clip8(int acc) { return aug_clip8(acc >> 22); }  // arithmetic shift

// grid (tiles_per_side^2, n)
__global__ __launch_bounds__(kResizeBlock) void occ_resize_kernel(const uint32_t* __restrict__ src_rgbl, const int16_t* __restrict__ src_depth,
                                                                 int R, const int64_t* __restrict__ slot, uint32_t* __restrict__ dst_rgbl,
                                                                 int16_t* __restrict__ dst_depth, int m_frames, int S, int K,
                                                                 ResizeTables t) {
    __shared__ uint32_t win_w[kResizeWin * kResizeWin];
    __shared__ uint32_t hor_w[kResizeWin * kResizeTile];
    __shared__ int32_t hor_d[kResizeWin * kResizeTile];
    __shared__ int16_t win_d[kResizeWin * kResizeWin];
    const int i = blockIdx.y;
    const int64_t frame = pack_frame(slot, i, m_frames);  // block-uniform
    if (frame < 0) return;
    const int tiles = (S + kResizeTile - 1) / kResizeTile;
    const int ty = (int)blockIdx.x / tiles, tx = (int)blockIdx.x - ty * tiles;
    const int ox0 = tx * kResizeTile, oy0 = ty * kResizeTile;
    const int tw = min(kResizeTile, S - ox0), th = min(kResizeTile, S - oy0);
    // the window: from the first output's first input to the last output's last input, on each axis
    const int wx0 = max(t.bounds[2 * ox0], 0), wy0 = max(t.bounds[2 * oy0], 0);
    const int wx1 = min(t.bounds[2 * (ox0 + tw - 1)] + t.bounds[2 * (ox0 + tw - 1) + 1], R);
    const int wy1 = min(t.bounds[2 * (oy0 + th - 1)] + t.bounds[2 * (oy0 + th - 1) + 1], R);
    const int ww = wx1 - wx0, wh = wy1 - wy0;
    if (ww < 1 || wh < 1 || ww > kResizeWin || wh > kResizeWin) return;  // block-uniform; the host's size check rules it out

    const size_t src_at = (size_t)i * R * R;
    for (int e = threadIdx.x; e < ww * wh; e += kResizeBlock) {
        const int r = e / ww, c = e - r * ww;
        const size_t at = src_at + (size_t)(wy0 + r) * R + (wx0 + c);
        win_w[r * kResizeWin + c] = src_rgbl[at];
        win_d[r * kResizeWin + c] = src_depth[at];
    }
    const int col = threadIdx.x & (kResizeTile - 1), row0 = threadIdx.x / kResizeTile;
    constexpr int kRowStep = kResizeBlock / kResizeTile;
    const bool col_ok = col < tw;
    __syncthreads();

    // horizontal: window row r, tile column col
    if (col_ok) {
        const int first = t.bounds[2 * (ox0 + col)] - wx0;
        const int count = min(t.bounds[2 * (ox0 + col) + 1], ww - first);
        const double* kf = t.k + (size_t)(ox0 + col) * K;
        const int32_t* ki = t.kk + (size_t)(ox0 + col) * K;
        int a0[kResizeRowsH], a1[kResizeRowsH], a2[kResizeRowsH];
        double ad[kResizeRowsH];
#pragma unroll
        for (int j = 0; j < kResizeRowsH; ++j) {
            a0[j] = a1[j] = a2[j] = 1 << 21;
            ad[j] = 0.0;
        }
        if (first >= 0) {
            for (int x = 0; x < count; ++x) {
                const int c8 = ki[x];
                const double cf = kf[x];
#pragma unroll
                for (int j = 0; j < kResizeRowsH; ++j) {
                    const int r = row0 + j * kRowStep;
                    if (r < wh) {
                        const uint32_t w = win_w[r * kResizeWin + first + x];
                        a0[j] += (int)(w & 255u) * c8;
                        a1[j] += (int)((w >> 8) & 255u) * c8;
                        a2[j] += (int)((w >> 16) & 255u) * c8;
                        ad[j] = resize_tap_f64(ad[j], (int)win_d[r * kResizeWin + first + x], cf);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kResizeRowsH; ++j) {
            const int r = row0 + j * kRowStep;
            if (r < wh) {
                hor_w[r * kResizeTile + col] = (uint32_t)resize_clip8(a0[j]) | (uint32_t)resize_clip8(a1[j]) << 8 | (uint32_t)resize_clip8(a2[j]) << 16;
                hor_d[r * kResizeTile + col] = resize_round(ad[j]);
            }
        }
    }
    __syncthreads();

    // vertical: tile row oy, tile column col
    if (!col_ok) return;
    int first[kResizeRowsV], count[kResizeRowsV], b0[kResizeRowsV], b1[kResizeRowsV], b2[kResizeRowsV];
    double bd[kResizeRowsV];
    int most = 0;
#pragma unroll
    for (int j = 0; j < kResizeRowsV; ++j) {
        const int oy = row0 + j * kRowStep;
        first[j] = count[j] = 0;
        if (oy < th) {
            first[j] = t.bounds[2 * (oy0 + oy)] - wy0;
            count[j] = first[j] >= 0 ? min(t.bounds[2 * (oy0 + oy) + 1], wh - first[j]) : 0;
        }
        most = max(most, count[j]);
        b0[j] = b1[j] = b2[j] = 1 << 21;
        bd[j] = 0.0;
    }
    for (int y = 0; y < most; ++y) {
#pragma unroll
        for (int j = 0; j < kResizeRowsV; ++j) {
            if (y < count[j]) {
                const size_t kat = (size_t)(oy0 + row0 + j * kRowStep) * K + y;
                const int c8 = t.kk[kat];
                const uint32_t w = hor_w[(first[j] + y) * kResizeTile + col];
                b0[j] += (int)(w & 255u) * c8;
                b1[j] += (int)((w >> 8) & 255u) * c8;
                b2[j] += (int)((w >> 16) & 255u) * c8;
                bd[j] = resize_tap_f64(bd[j], hor_d[(first[j] + y) * kResizeTile + col], t.k[kat]);
            }
        }
    }
    const int sx = t.nearest[ox0 + col];
#pragma unroll
    for (int j = 0; j < kResizeRowsV; ++j) {
        const int oy = row0 + j * kRowStep;
        if (oy < th) {
            const int sy = t.nearest[oy0 + oy];
            const uint32_t label = src_rgbl[src_at + (size_t)min(max(sy, 0), R - 1) * R + min(max(sx, 0), R - 1)] & 0xff000000u;
            const int d = resize_round(bd[j]);
            const size_t at = (size_t)frame * S * S + (size_t)(oy0 + oy) * S + (ox0 + col);
            dst_rgbl[at] = (uint32_t)resize_clip8(b0[j]) | (uint32_t)resize_clip8(b1[j]) << 8 | (uint32_t)resize_clip8(b2[j]) << 16 | label;
            dst_depth[at] = (int16_t)(d < -32768 ? -32768 : (d > 32767 ? 32767 : d));
        }
    }
}
