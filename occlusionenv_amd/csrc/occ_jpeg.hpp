// occ_jpeg.hpp -- the JPEG round trip in place in the resident store (occ_dataset_jpeg; header: "JPEG round trip in the
// resident store").  Part of the single translation unit occ_kernels.hip (included inside namespace occ; not a
// stand-alone header).
//
// The reference writes every colour image as a baseline 4:2:0 JPEG at the rendering size (datasetGenerator.py:104) and
// trains on what the reader decodes.  Entropy coding is lossless, so writing and reading the file is a function of the
// pixels and the two quantisation tables: libjpeg's colour conversion, 2x2 chroma averaging, slow-integer forward DCT,
// quantisation, dequantisation, slow-integer inverse DCT, triangle-filter ("fancy") chroma upsampling and colour conversion
// back.  This is that function for the three colour bytes of a frame of the store of occ_augment.hpp, in int32 throughout,
// no floating point.  tests/jpeg_model.py is the same arithmetic in numpy, checked against PIL.
//
// Two launches and a workspace of two bytes per chroma sample (Cb | Cr << 8; n planes of cs x cs, cs = 8 ceil(S / 16)):
//   occ_jpeg_block_kernel     one block of 256 threads per 32 x 32 pixel tile (2 x 2 MCUs) of one frame.
//                             Thread = one 2 x 2 pixel quad: four words loaded (edges by clamping, see below), four Y
//                             samples and one Cb / Cr sample each into LDS.  Then lane = one 8-sample 1-D transform of one
//                             of the tile's 24 blocks (16 Y, 4 Cb, 4 Cr; 192 of the 256 lanes): forward rows | forward
//                             columns, quantise, dequantise, inverse columns (the same lane owns the column throughout) |
//                             inverse rows, with a barrier at each |.  Last the quad threads store Y' into the low byte of
//                             their four words (the label byte kept, G and B are dead from here on) and the quad's Cb', Cr'
//                             into the workspace.  In place is safe: a block reads and writes its own tile only, and
//                             every load of a block is complete before its first barrier.
//   occ_jpeg_upsample_kernel  lane = pixel: the four chroma samples around it from the workspace (h2v2 fancy upsampling,
//                             its edge cases at the real last chroma row and column), Y' from the word, the three colour
//                             bytes stored with the label byte.  It reads chroma across block borders, which is why it is
//                             a launch of its own: a fused kernel would redo the chroma blocks of a one-sample halo.
// LDS layout: block b is 8 rows of stride kJpegStride = 9 words, blocks kJpegBlockWords = 72 words apart, so with lane
// l = 8 b + k the row owner reads word 9 l + j at step j and the column owner word 72 b + 9 j + k = l + 64 b + 9 j.
// ds_read_b32 and ds_write_b32 (and the ds_read2_b32 / ds_write2_b32 pairs the compiler forms, each dword on its own) bank
// by word mod 32 within a 32-lane half: 9 l mod 32 and (l + 9 j) mod 32 take 32 different values over 32 consecutive
// lanes, so both passes are conflict-free.  (An unpadded stride 8 would put a column pass on 8 banks, four
// lanes each.)  The quad threads' stores (stride 2 along a row, two rows 18 words apart per half-wave) are two-way; there
// are four per thread.  24 x 72 + 128 words = 7.25 KiB per block: LDS does not bound occupancy.
//
// Edges, as jcsample.c / jcprepct.c leave them: columns past the image replicate the last column; Y rows past the image
// replicate the last Y row; chroma rows past ceil(S / 2) replicate the last CHROMA row (whose second input row, for odd S,
// is the last input row again), which is not the downsampling of replicated input rows.  All of it is clamping of the
// coordinates a thread loads from, and stays inside the block's own tile.
// Frames whose slot is outside [0, m_frames) are skipped by whole blocks before any address is formed from the slot.
// No atomics, no allocation, plain stores, integers only: bitwise the same from call to call.

constexpr int kJpegTile = 32;        // pixels on a side of one block's tile: 2 x 2 MCUs
constexpr int kJpegBlock = 256;      // one 2 x 2 quad per thread
constexpr int kJpegStride = 9;       // words between the rows of an 8 x 8 block in LDS
constexpr int kJpegBlockWords = 8 * kJpegStride;
constexpr int kJpegBlocks = 24;      // 16 Y, 4 Cb, 4 Cr
constexpr int kJpegMaxImg = 4096;

// JPEG specification, Annex K, tables K.1 and K.2, row-major
static const uint8_t kJpegBase[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// The luminance and the chrominance table of one quality, handed to the kernel by value
struct JpegTables {
    uint16_t q[2][64];
};

// jcparam.c jpeg_set_quality with force_baseline
inline JpegTables jpeg_tables(int quality) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    JpegTables t;
    for (int k = 0; k < 2; ++k)
        for (int e = 0; e < 64; ++e) {
            const int v = ((int)kJpegBase[k][e] * scale + 50) / 100;
            t.q[k][e] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
    return t;
}

inline int jpeg_chroma_side(int img) { return (img + 15) / 16 * 8; }

__device__ __forceinline__ int jpeg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }  // arithmetic shift

// The odd part both transforms share (jfdctint.c / jidctint.c): in t4, t5, t6, t7; out the four sums before the descale
__device__ __forceinline__ void jpeg_odd(int& t4, int& t5, int& t6, int& t7) {
    int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446;
    t5 *= 16819;
    t6 *= 25172;
    t7 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    t4 += z1 + z3;
    t5 += z2 + z4;
    t6 += z2 + z3;
    t7 += z1 + z4;
}

// jfdctint.c: the row pass scales up by 4, the column pass takes that and 8 more out
template <bool kRowPass>
__device__ __forceinline__ void jpeg_fdct(int (&d)[8]) {
    const int t0 = d[0] + d[7], t1 = d[1] + d[6], t2 = d[2] + d[5], t3 = d[3] + d[4];
    int t7 = d[0] - d[7], t6 = d[1] - d[6], t5 = d[2] - d[5], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = kRowPass ? 11 : 15;
    d[0] = kRowPass ? (t10 + t11) << 2 : jpeg_descale(t10 + t11, 2);
    d[4] = kRowPass ? (t10 - t11) << 2 : jpeg_descale(t10 - t11, 2);
    const int z = (t12 + t13) * 4433;
    d[2] = jpeg_descale(z + t13 * 6270, n);
    d[6] = jpeg_descale(z - t12 * 15137, n);
    jpeg_odd(t4, t5, t6, t7);
    d[7] = jpeg_descale(t4, n);
    d[5] = jpeg_descale(t5, n);
    d[3] = jpeg_descale(t6, n);
    d[1] = jpeg_descale(t7, n);
}

// jidctint.c, descaled by n bits (11 after the column pass, 18 after the row pass)
__device__ __forceinline__ void jpeg_idct(int (&d)[8], int n) {
    const int z = (d[2] + d[6]) * 4433;
    const int e2 = z - d[6] * 15137, e3 = z + d[2] * 6270;
    const int e0 = (d[0] + d[4]) << 13, e1 = (d[0] - d[4]) << 13;
    const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    int t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
    jpeg_odd(t0, t1, t2, t3);
    d[0] = jpeg_descale(t10 + t3, n);
    d[7] = jpeg_descale(t10 - t3, n);
    d[1] = jpeg_descale(t11 + t2, n);
    d[6] = jpeg_descale(t11 - t2, n);
    d[2] = jpeg_descale(t12 + t1, n);
    d[5] = jpeg_descale(t12 - t1, n);
    d[3] = jpeg_descale(t13 + t0, n);
    d[4] = jpeg_descale(t13 - t0, n);
}

// jccolor.c rgb_ycc_convert
__device__ __forceinline__ int jpeg_y(uint32_t w) {
    const int r = (int)(w & 255u), g = (int)((w >> 8) & 255u), b = (int)((w >> 16) & 255u);
    return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
}
__device__ __forceinline__ int jpeg_cb(uint32_t w) {
    const int r = (int)(w & 255u), g = (int)((w >> 8) & 255u), b = (int)((w >> 16) & 255u);
    return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
}
__device__ __forceinline__ int jpeg_cr(uint32_t w) {
    const int r = (int)(w & 255u), g = (int)((w >> 8) & 255u), b = (int)((w >> 16) & 255u);
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// grid (tiles_per_side^2, n)
__global__ __launch_bounds__(kJpegBlock) void occ_jpeg_block_kernel(uint32_t* rgbl, int m_frames, int S, const int64_t* __restrict__ slot,
                                                                   JpegTables tab, uint16_t* __restrict__ chroma, int cs) {
    __shared__ int blk[kJpegBlocks * kJpegBlockWords];
    __shared__ int qt[128];
    const int i = blockIdx.y;
    const int64_t frame = pack_frame(slot, i, m_frames);  // block-uniform
    if (frame < 0) return;
    const int tiles = (S + kJpegTile - 1) / kJpegTile;
    const int ty = (int)blockIdx.x / tiles, tx = (int)blockIdx.x - ty * tiles;
    const int ox0 = tx * kJpegTile, oy0 = ty * kJpegTile;  // both below S
    const int t = threadIdx.x;
    if (t < 128) qt[t] = (int)tab.q[t >> 6][t & 63];

    // the quad: pixels (y0 .. y0 + 1, x0 .. x0 + 1), chroma sample (gcy, gcx)
    const int qx = t & 15, qy = t >> 4;
    const int x0 = ox0 + 2 * qx, y0 = oy0 + 2 * qy;
    const int gcx = (ox0 >> 1) + qx, gcy = (oy0 >> 1) + qy;
    const int xa = min(x0, S - 1), xb = min(x0 + 1, S - 1), ya = min(y0, S - 1), yb = min(y0 + 1, S - 1);
    uint32_t* const base = rgbl + (size_t)frame * S * S;
    const uint32_t w00 = base[(size_t)ya * S + xa], w01 = base[(size_t)ya * S + xb];
    const uint32_t w10 = base[(size_t)yb * S + xa], w11 = base[(size_t)yb * S + xb];
    uint32_t c00 = w00, c01 = w01, c10 = w10, c11 = w11;
    const int last_c = (S - 1) >> 1;  // the last real chroma row, ceil(S / 2) - 1
    if (gcy > last_c) {               // a padding row of the chroma planes: the last chroma row again
        const int ra = 2 * last_c, rb = min(2 * last_c + 1, S - 1);
        c00 = base[(size_t)ra * S + xa];
        c01 = base[(size_t)ra * S + xb];
        c10 = base[(size_t)rb * S + xa];
        c11 = base[(size_t)rb * S + xb];
    }
    const int bias = 1 + (gcx & 1);
    const int cb = (jpeg_cb(c00) + jpeg_cb(c01) + jpeg_cb(c10) + jpeg_cb(c11) + bias) >> 2;
    const int cr = (jpeg_cr(c00) + jpeg_cr(c01) + jpeg_cr(c10) + jpeg_cr(c11) + bias) >> 2;
    const int px = 2 * qx, py = 2 * qy;
    int* const yq = blk + ((py >> 3) * 4 + (px >> 3)) * kJpegBlockWords + (py & 7) * kJpegStride + (px & 7);
    int* const cq = blk + (16 + (qy >> 3) * 2 + (qx >> 3)) * kJpegBlockWords + (qy & 7) * kJpegStride + (qx & 7);
    yq[0] = jpeg_y(w00) - 128;
    yq[1] = jpeg_y(w01) - 128;
    yq[kJpegStride] = jpeg_y(w10) - 128;
    yq[kJpegStride + 1] = jpeg_y(w11) - 128;
    cq[0] = cb - 128;
    cq[4 * kJpegBlockWords] = cr - 128;
    __syncthreads();

    // lane = one 1-D transform: block t / 8, row or column t % 8
    const bool lane_ok = t < kJpegBlocks * 8;
    int* const p = blk + (t >> 3) * kJpegBlockWords;
    const int k = t & 7;
    int d[8];
    if (lane_ok) {
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = p[k * kJpegStride + j];
        jpeg_fdct<true>(d);
#pragma unroll
        for (int j = 0; j < 8; ++j) p[k * kJpegStride + j] = d[j];
    }
    __syncthreads();
    if (lane_ok) {
        const int* const q = qt + (t >= 16 * 8 ? 64 : 0);
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = p[j * kJpegStride + k];
        jpeg_fdct<false>(d);
#pragma unroll
        for (int j = 0; j < 8; ++j) {  // jcdctmgr.c quantize, then the decoder's multiplication
            const int qv = q[j * 8 + k];
            const uint32_t q8 = (uint32_t)qv << 3;
            const uint32_t a = (uint32_t)(d[j] < 0 ? -d[j] : d[j]);
            const int c = (int)((a + (q8 >> 1)) / q8);
            d[j] = (d[j] < 0 ? -c : c) * qv;
        }
        jpeg_idct(d, 11);
#pragma unroll
        for (int j = 0; j < 8; ++j) p[j * kJpegStride + k] = d[j];
    }
    __syncthreads();
    if (lane_ok) {
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = p[k * kJpegStride + j];
        jpeg_idct(d, 18);
#pragma unroll
        for (int j = 0; j < 8; ++j) p[k * kJpegStride + j] = aug_clip8(d[j] + 128);
    }
    __syncthreads();

    const uint32_t keep = 0xff000000u;
    if (y0 < S) {
        if (x0 < S) base[(size_t)y0 * S + x0] = (w00 & keep) | (uint32_t)yq[0];
        if (x0 + 1 < S) base[(size_t)y0 * S + x0 + 1] = (w01 & keep) | (uint32_t)yq[1];
    }
    if (y0 + 1 < S) {
        if (x0 < S) base[(size_t)(y0 + 1) * S + x0] = (w10 & keep) | (uint32_t)yq[kJpegStride];
        if (x0 + 1 < S) base[(size_t)(y0 + 1) * S + x0 + 1] = (w11 & keep) | (uint32_t)yq[kJpegStride + 1];
    }
    if (gcx < cs && gcy < cs)
        chroma[((size_t)i * cs + gcy) * cs + gcx] = (uint16_t)((uint32_t)cq[0] | (uint32_t)cq[4 * kJpegBlockWords] << 8);
}

// grid (ceil(S * S / kJpegBlock), n)
__global__ __launch_bounds__(kJpegBlock) void occ_jpeg_upsample_kernel(uint32_t* rgbl, int m_frames, int S, const int64_t* __restrict__ slot,
                                                                      const uint16_t* __restrict__ chroma, int cs) {
    const int i = blockIdx.y;
    const int64_t frame = pack_frame(slot, i, m_frames);  // block-uniform
    if (frame < 0) return;
    const int px = (int)blockIdx.x * kJpegBlock + (int)threadIdx.x;
    if (px >= S * S) return;
    const int y = px / S, x = px - y * S;
    const int last_c = (S - 1) >> 1;  // the filter's edges are the real last chroma row and column
    const int r = y >> 1, c = x >> 1;
    const int rn = (y & 1) ? min(r + 1, last_c) : max(r - 1, 0);
    const int cn = (x & 1) ? min(c + 1, last_c) : max(c - 1, 0);
    const uint16_t* const plane = chroma + (size_t)i * cs * cs;
    const uint32_t near_c = plane[r * cs + c], far_c = plane[rn * cs + c];
    const uint32_t near_n = plane[r * cs + cn], far_n = plane[rn * cs + cn];
    const int round = (x & 1) ? 7 : 8;
    // jdsample.c h2v2_fancy_upsample: 3/4 nearer row + 1/4 further row, then the same along the row
    const int sb_c = 3 * (int)(near_c & 255u) + (int)(far_c & 255u), sb_n = 3 * (int)(near_n & 255u) + (int)(far_n & 255u);
    const int sr_c = 3 * (int)(near_c >> 8) + (int)(far_c >> 8), sr_n = 3 * (int)(near_n >> 8) + (int)(far_n >> 8);
    const int u = ((3 * sb_c + sb_n + round) >> 4) - 128, v = ((3 * sr_c + sr_n + round) >> 4) - 128;
    uint32_t* const at = rgbl + (size_t)frame * S * S + px;
    const uint32_t w = *at;
    const int yy = (int)(w & 255u);
    // jdcolor.c ycc_rgb_convert
    const int red = aug_clip8(yy + ((91881 * v + 32768) >> 16));
    const int blue = aug_clip8(yy + ((116130 * u + 32768) >> 16));
    const int green = aug_clip8(yy + ((-22554 * u - 46802 * v + 32768) >> 16));
    *at = (w & 0xff000000u) | (uint32_t)red | (uint32_t)green << 8 | (uint32_t)blue << 16;
}
