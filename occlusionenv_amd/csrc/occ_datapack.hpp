// occ_datapack.hpp -- rendered frames into the resident dataset (occ_dataset_pack; header: "Packing rendered frames into
// the resident dataset").  Part of the single translation unit occ_kernels.hip (included inside namespace occ; not a
// stand-alone header).
//
// What dataset_io.RunWriter.write_frame and devdata.DeviceDataset.from_directory do to a frame between the engine's step
// and the store of occ_augment.hpp, without the files: img_as_ubyte on the colours (stored B <-> R swapped, as the writer
// saves BGR and the reader opens RGB), depth * 51 truncated, img_as_ubyte on the occlusion alpha and PIL's convert("1"),
// which is Floyd-Steinberg error diffusion over the whole image (Convert.c tobilevel).  tests/datapack_model.py is the same
// arithmetic in numpy, checked against PIL and against the files.
//
//   occ_datapack_point_kernel   lane = pixel: four coalesced plane loads and the strided alpha, one word and one int16
//                               stored.  The label byte of the word gets the label itself (label_mode 1: alpha > 0.5) or
//                               the 8-bit alpha that the dither pass turns into it in place (label_mode 0).
//   occ_datapack_dither_kernel  one wave per frame.  tobilevel carries three values along a row (l, l0, l1) and one int per
//                               column from row to row (errors[x + 1] of row y - 1, final once that row has done column
//                               x + 1).  So row y can run two columns behind row y - 1: lane r is row r of a band of 64
//                               rows, at step t it does column t - 2 r, and hands the errors value it produced to lane
//                               r + 1 with a lane shift; one step past its last column it hands over l0, which is
//                               errors[W].  Lane 0 reads the errors row the previous band's last row left in LDS (zeros
//                               for the first band), the band's last row writes it back in place: it writes errors[x] 2 (R - 1)
//                               steps after lane 0 read errors[x + 1].  (S / 64) (S + 126) dependent steps per frame
//                               instead of S^2.  The label bytes of kDitherChunk steps are loaded one chunk ahead of
//                               the chain (their addresses do not depend on it).
// Envs whose slot is outside [0, m_frames) are skipped by whole blocks before any address is formed from the slot.
// No atomics, no allocation, nothing but plain stores; integer arithmetic in the dither: bitwise the same from call to call.

constexpr int kPackBlock = 256;     // pixels of one block of the point pass
constexpr int kDitherRows = 64;     // rows of one band: one per lane
constexpr int kDitherChunk = 8;     // steps whose label bytes are loaded together
constexpr int kDitherMaxImg = 4096; // img * img <= 2^24
constexpr uint32_t kPackMaxPixels = 1u << 24;

// The product with 255.0 and rint must stay two roundings of their own
#pragma clang fp contract(off)

// dataset_io._ubyte: clip(rint((double)x * 255.0), 0, 255), round-half-even (rint in the default rounding mode), NaN -> 0
__device__ __forceinline__ uint32_t pack_ubyte(float x) {
    const double r = rint((double)x * 255.0);
    if (!(r > 0.0)) return 0u;  // also NaN
    return r >= 255.0 ? 255u : (uint32_t)r;
}

// depth[depth == -1] = 0; (depth * 51).astype(uint8): one f32 product, truncated; outside the cast's range defined as
// t <= 0 or NaN -> 0, t >= 255 -> 255
__device__ __forceinline__ int pack_depth(float d) {
    if (d == -1.0f) d = 0.0f;
    const float t = d * 51.0f;
    if (!(t > 0.0f)) return 0;
    return t >= 255.0f ? 255 : (int)t;
}

#pragma clang fp contract(fast)

// The frame env i writes, or -1: skipped
__device__ __forceinline__ int64_t pack_frame(const int64_t* slot, int i, int m_frames) {
    const int64_t f = slot[i];
    return f >= 0 && f < (int64_t)m_frames ? f : (int64_t)-1;
}

// grid (blocks_per_image, n)
__global__ __launch_bounds__(kPackBlock) void occ_datapack_point_kernel(const float* __restrict__ obs, const float* __restrict__ alpha,
                                                                       int alpha_stride, int pixels, const int64_t* __restrict__ slot,
                                                                       uint32_t* __restrict__ rgbl, int16_t* __restrict__ depth,
                                                                       int m_frames, int label_mode) {
    const int i = blockIdx.y;
    const int64_t frame = pack_frame(slot, i, m_frames);  // block-uniform
    if (frame < 0) return;
    const int px = (int)blockIdx.x * kPackBlock + (int)threadIdx.x;
    if (px >= pixels) return;
    const float* o = obs + (size_t)i * 4 * pixels + px;
    const float c0 = o[0], c1 = o[(size_t)pixels], c2 = o[(size_t)2 * pixels], d = o[(size_t)3 * pixels];
    const float a = alpha[((size_t)i * pixels + px) * (size_t)alpha_stride];
    const uint32_t lab = label_mode ? (a > 0.5f ? 1u : 0u) : pack_ubyte(a);
    const size_t at = (size_t)frame * pixels + px;
    rgbl[at] = pack_ubyte(c2) | pack_ubyte(c1) << 8 | pack_ubyte(c0) << 16 | lab << 24;
    depth[at] = (int16_t)pack_depth(d);
}

// The label bytes of the steps t0 .. t0 + kDitherChunk - 1 of this lane's row (0 where the lane has no column)
__device__ __forceinline__ void dither_load(const uint8_t* row, bool row_ok, int x0, int img, int (&v)[kDitherChunk]) {
#pragma unroll
    for (int k = 0; k < kDitherChunk; ++k) {
        const int x = x0 + k;
        v[k] = row_ok && x >= 0 && x < img ? (int)row[(size_t)x * 4] : 0;
    }
}

// grid (n), block = one wave
__global__ __launch_bounds__(kDitherRows) void occ_datapack_dither_kernel(const int64_t* __restrict__ slot, uint32_t* rgbl, int img,
                                                                         int m_frames) {
    __shared__ int errors[kDitherMaxImg + 1];
    const int64_t frame = pack_frame(slot, blockIdx.x, m_frames);  // block-uniform
    if (frame < 0) return;
    const int lane = threadIdx.x;
    for (int x = lane; x <= img; x += kDitherRows) errors[x] = 0;
    // the label byte (bits 24..31 of the little-endian word) of pixel (0, 0) of the frame
    uint8_t* const label = reinterpret_cast<uint8_t*>(rgbl + (size_t)frame * img * img) + 3;
    for (int y0 = 0; y0 < img; y0 += kDitherRows) {
        __syncthreads();  // the errors row of the band above (or the zeros) is complete
        const int rows = min(kDitherRows, img - y0);
        const bool row_ok = lane < rows, last = lane == rows - 1;
        uint8_t* const row = label + (size_t)(y0 + (row_ok ? lane : 0)) * img * 4;
        const int steps = img + 2 * (rows - 1) + 1;  // the last row's step past its last column included
        int l = 0, l0 = 0, l1 = 0, produced = 0;
        int cur[kDitherChunk], nxt[kDitherChunk];
        dither_load(row, row_ok, -2 * lane, img, cur);
        for (int t0 = 0; t0 < steps; t0 += kDitherChunk) {
            dither_load(row, row_ok, t0 + kDitherChunk - 2 * lane, img, nxt);
            int above[kDitherChunk];  // lane 0: errors[x + 1] of the band above; x = t there
#pragma unroll
            for (int k = 0; k < kDitherChunk; ++k) above[k] = errors[min(t0 + k + 1, img)];
#pragma unroll
            for (int k = 0; k < kDitherChunk; ++k) {
                const int x = t0 + k - 2 * lane;
                const int up = __shfl_up(produced, 1, kDitherRows);  // what the row above produced one step ago
                const int err = lane == 0 ? above[k] : up;
                if (row_ok && x >= 0 && x < img) {
                    l = aug_clip8(cur[k] + (l + err) / 16);  // C division: toward zero
                    const int out = l > 128 ? 1 : 0;
                    const int e = l - 255 * out;
                    produced = 3 * e + l0;  // errors[x]
                    l0 = 5 * e + l1;
                    l1 = e;
                    l = 7 * e;
                    row[(size_t)x * 4] = (uint8_t)out;
                    if (last) errors[x] = produced;
                } else if (row_ok && x == img) {
                    produced = l0;  // errors[W]
                    if (last) errors[img] = l0;
                }
            }
#pragma unroll
            for (int k = 0; k < kDitherChunk; ++k) cur[k] = nxt[k];
        }
    }
}
