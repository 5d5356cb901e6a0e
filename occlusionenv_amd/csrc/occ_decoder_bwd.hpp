// occ_decoder_bwd.hpp -- training of the segmentation decoder and classifier with the encoder frozen: a forward that keeps
// what the backward needs, and the backward with respect to every decoder parameter.  Part of the single translation unit
// occ_kernels.hip (included inside namespace occ, after occ_decoder.hpp, whose forward kernel it launches and whose quad
// mapping, LDS staging and packed layout its backward mirrors, and after occ_criterion.hpp's reduction rule, which it follows).
//
// Forward per level j (c = 128 .. 8): u = convT(x_j) + b, r = relu(u), y_j = s r + t + skip, x_{j+1} = y_j; after the last
// level z = cls_w y_4 + cls_b, p = sigmoid(z).  BatchNorm runs with its running statistics (s, t folded by the host).
//
//   occ_dec_up_kernel<.., TRAIN>  (occ_decoder.hpp) the inference kernel itself, one loop nest for both (prob is the same
//                               to the bit), whose epilogue also stores r_j and, at the last level, y_4 and a second copy of p.
//   occ_dec_bwd_act_kernel      per (chunk of 4096 pixels, channel, env): dU = dY s [r > 0] written over dY (to a buffer of its
//                               own in the joint training of occ_fullnet_bwd.hpp, which reads dY again), with dY = dz
//                               cls_w[c], dz = g p (1 - p) at the last level; f64 block partials of dS = sum dY r, dT = sum
//                               dY, dB = sum dU (and sum dz y_4[c], sum dz at the last level).  The gate is the forward's
//                               own r > 0.
//   occ_dec_bwd_act_final_kernel  one wave per (channel, sum): lane l adds partials l, l + 64, .. in order, then six
//                               __shfl_down steps; all f64, rounded once to f32.
//   occ_dec_bwd_dx_kernel       dX[ci][iy][ix] = sum_co sum_k w[ci][k][co] dU[co][2 iy - 1 + ky][2 ix - 1 + kx]: the mirror
//                               of the forward's quad mapping.  A thread owns one input pixel for 16 input channels; the
//                               (2 T + 1)^2 dU tile is staged in LDS 8 output channels at a time (row / column -1 and 2 H
//                               read as zero); weights are wave-uniform scalar loads of 8 consecutive co.  Not launched for
//                               level 0 while the encoder is frozen; the joint training launches it there too.
//   occ_dec_bwd_dw_kernel       dW[ci][k][co] = sum_{n,iy,ix} x[ci][iy][ix] dU[co][2 iy - 1 + ky][2 ix - 1 + kx], a
//                               (2c) x (9c) contraction over K = N H^2.  A thread owns 16 ci x 9 taps x 1 co (144 f32
//                               accumulators); a block owns a CIB x COB tile of (ci, co) and one slice of K (consecutive
//                               T x T pixel tiles, envs in order); when the (ci, co) tile needs fewer than 256 threads the
//                               others take other pixels of the tile (P pixel lanes), which are added inside the wave by
//                               __shfl_xor steps in a fixed order.  Every block writes its partial dW (one per wave or per
//                               pixel lane) to caller scratch.
//   occ_dec_bwd_sum_kernel      the partials added per element in a fixed order (four interleaved chains in f64, then the
//                               four in order), rounded once to f32.
//
// No floating-point atomics; the split of K is a function of (S, N) alone: every gradient is bitwise the same from call to
// call.  f32 chains: a thread's accumulator sees at most tiles-per-slice x T^2 / P products before the f64 stage.
//
// The tails that make up that contract exist once, as device helpers below, for the kernels of this file, of
// occ_encoder_bwd.hpp and of occ_sepenc_bwd.hpp: bwd_block_partials (the f64 sums of a block), bwd_wave_strided_sum (the
// final sum of block partials) and bwd_dw_fold (the pixel lanes and the partial slot of a K-split weight gradient).
//
// Host side, shared with occ_encoder_bwd.hpp and occ_sepenc_bwd.hpp: DwPlan / dw_split (the K split of a weight gradient)
// and bwd_layer_tail (what follows a layer's activation step); the grids of the up layers and of the input gradient come
// from tile_launch (occ_encoder.hpp).

constexpr int kBwdChunk = 4096;   // pixels of one (env, channel) plane per block of the activation step
constexpr int kBwdDxCC = 8;       // output channels of dU staged per step of the input gradient
constexpr int kBwdDxCIG = 16;     // input channels per thread of the input gradient
constexpr int kBwdDwBlocks = 512;  // blocks of the weight gradient per level (K slices x (ci, co) tiles)

// ---- the fixed-order reductions of every training backward (this file, occ_encoder_bwd.hpp, occ_sepenc_bwd.hpp) --------

// The NS f64 sums of a 256-thread block to dst[NS]: six __shfl_down steps per wave, then thread k < NS adds the four
// waves in order.
template <int NS>
__device__ __forceinline__ void bwd_block_partials(double (&sum)[NS], double* __restrict__ dst) {
    __shared__ double part[4][NS];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
        for (int k = 0; k < NS; ++k) sum[k] += __shfl_down(sum[k], d);
    const int wave = threadIdx.x / 64;
    if (threadIdx.x % 64 == 0)
#pragma unroll
        for (int k = 0; k < NS; ++k) part[wave][k] = sum[k];
    __syncthreads();
    if (threadIdx.x < NS) {
        double t = 0.0;
        for (int k = 0; k < 4; ++k) t += part[k][threadIdx.x];
        dst[threadIdx.x] = t;
    }
}

// One wave's sum of p[0], p[stride], .., p[(n - 1) stride]: lane l adds elements l, l + 64, .. in order, then six
// __shfl_down steps; lane 0 holds the sum.
__device__ __forceinline__ double bwd_wave_strided_sum(const double* __restrict__ p, int n, int stride) {
    double sum = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) sum += p[(size_t)i * stride];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_down(sum, d);
    return sum;
}

// The partials a block of a K-split weight gradient writes when one pixel takes q threads: one per wave (q < 64, the
// wave's pixel lanes are folded first) or one per pixel lane.
constexpr int dw_partials(int q) { return 256 / (q < 64 ? 64 : q); }

// The end of a K-split weight gradient kernel whose pixel takes Q threads (pixel lane pl = tid / Q): the pixel lanes of a
// wave are added into its first Q lanes by __shfl_xor steps from Q upwards, element by element.  False: the thread stores
// nothing; true: it stores acc into partial pb of its block's dw_partials(Q).
template <int Q, int N>
__device__ __forceinline__ bool bwd_dw_fold(float (&acc)[N], int pl, int& pb) {
    if constexpr (Q < 64) {
#pragma unroll
        for (int d = Q; d < 64; d <<= 1)
#pragma unroll
            for (int i = 0; i < N; ++i) acc[i] += __shfl_xor(acc[i], d);
        if (threadIdx.x % 64 >= Q) return false;
        pb = threadIdx.x / 64;
    } else {
        pb = pl;
    }
    return true;
}

// Activation step of one level.  dy: (n, c, plane) (not read when LAST); du: (n, c, plane), may be dy itself (the decoder
// alone; the joint training of occ_fullnet_bwd.hpp keeps dY, the level's d skip).  r: the forward's relu(u).
// LAST: gp = d loss / d prob and prob are (n, plane), y4 (n, c, plane), clsw[c].
// partials[((ch * n + env) * chunks + chunk) * NS + k], NS = LAST ? 5 : 3: k = 0 dS, 1 dT, 2 dB, 3 sum dz y4[ch], 4 sum dz.
template <bool LAST>
__global__ __launch_bounds__(256) void occ_dec_bwd_act_kernel(const float* dyp, float* dup, const float* __restrict__ r,
                                                              const float* __restrict__ bns, int c, int plane,
                                                              const float* __restrict__ gp, const float* __restrict__ prob,
                                                              const float* __restrict__ y4, const float* __restrict__ clsw,
                                                              double* __restrict__ partials) {
    constexpr int NS = LAST ? 5 : 3;
    const int ch = blockIdx.y, env = blockIdx.z;
    const size_t base = ((size_t)env * c + ch) * plane;
    const float sc = bns[ch];
    const float cw = LAST ? clsw[ch] : 0.f;
    double sum[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) sum[k] = 0.0;
    const int lo = blockIdx.x * kBwdChunk;
#pragma unroll
    for (int j = 0; j < kBwdChunk / 1024; ++j) {
        const int i = lo + 4 * ((int)threadIdx.x + 256 * j);  // plane % 4 == 0: the four pixels are inside or outside together
        if (i >= plane) break;
        const float4 r4 = *reinterpret_cast<const float4*>(r + base + i);
        const float rv[4] = {r4.x, r4.y, r4.z, r4.w};
        float dy[4], dz[4] = {0.f, 0.f, 0.f, 0.f}, yv[4] = {0.f, 0.f, 0.f, 0.f}, du[4];
        if constexpr (LAST) {
            const float4 g4 = *reinterpret_cast<const float4*>(gp + (size_t)env * plane + i);
            const float4 p4 = *reinterpret_cast<const float4*>(prob + (size_t)env * plane + i);
            const float4 y = *reinterpret_cast<const float4*>(y4 + base + i);
            const float gv[4] = {g4.x, g4.y, g4.z, g4.w}, pv[4] = {p4.x, p4.y, p4.z, p4.w};
            yv[0] = y.x, yv[1] = y.y, yv[2] = y.z, yv[3] = y.w;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                dz[q] = gv[q] * (pv[q] * (1.f - pv[q]));
                dy[q] = dz[q] * cw;
            }
        } else {
            const float4 d4 = *reinterpret_cast<const float4*>(dyp + base + i);
            dy[0] = d4.x, dy[1] = d4.y, dy[2] = d4.z, dy[3] = d4.w;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            du[q] = rv[q] > 0.f ? dy[q] * sc : 0.f;
            sum[0] = fma((double)dy[q], (double)rv[q], sum[0]);
            sum[1] += (double)dy[q];
            sum[2] += (double)du[q];
            if constexpr (LAST) {
                sum[3] = fma((double)dz[q], (double)yv[q], sum[3]);
                sum[4] += (double)dz[q];
            }
        }
        *reinterpret_cast<float4*>(dup + base + i) = make_float4(du[0], du[1], du[2], du[3]);
    }
    bwd_block_partials(sum, partials + ((((size_t)ch * gridDim.z + env) * gridDim.x) + blockIdx.x) * NS);
}

// One wave per (channel, sum k): dst[k][ch] = the channel's nparts partials.  dst[4] (sum dz) is taken from channel 0 only
// (every channel's block forms the same dz).
struct BwdActDst {
    float* p[5];  // dscale, dshift, dbias, dcls_w, dcls_b
};

__global__ __launch_bounds__(64) void occ_dec_bwd_act_final_kernel(const double* __restrict__ partials, int nparts, int ns,
                                                                   BwdActDst dst) {
    const int ch = blockIdx.x, k = blockIdx.y;
    const double* pe = partials + (size_t)ch * nparts * ns + k;
    const double sum = bwd_wave_strided_sum(pe, nparts, ns);
    if (threadIdx.x != 0) return;
    if (k < 4) dst.p[k][ch] = (float)sum;
    else if (ch == 0) dst.p[4][0] = (float)sum;
}

// du: (n, cout, 2H, 2H); dx: (n, cin, H, H); w: the level's packed w[ci][k][co].  cin % 16 == 0, cout % 8 == 0.
template <int T>
__global__ __launch_bounds__(256) void occ_dec_bwd_dx_kernel(const float* __restrict__ du, float* __restrict__ dx,
                                                             const float* __restrict__ w, int cin, int cout, int H, int tiles_x) {
    constexpr int TT = T * T, R = 2 * T + 1, RR = R * R, CIG = kBwdDxCIG, CC = kBwdDxCC;
    __shared__ float s[CC * RR];
    const int tid = threadIdx.x;
    const int p = tid % TT;
    const int ng = blockDim.x / TT;
    const int g = __builtin_amdgcn_readfirstlane(tid / TT);
    const int ci0 = (blockIdx.y * ng + g) * CIG;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const int iy0 = ty * T, ix0 = tx * T;
    const int py = p / T, px = p % T;
    const int W2 = 2 * H;
    const size_t oplane = (size_t)W2 * W2;
    const float* de = du + (size_t)blockIdx.z * cout * oplane;

    float acc[CIG];
#pragma unroll
    for (int j = 0; j < CIG; ++j) acc[j] = 0.f;

    for (int co0 = 0; co0 < cout; co0 += CC) {
        __syncthreads();
        for (int i = tid; i < CC * RR; i += blockDim.x) {
            const int c = i / RR, r = i - c * RR;
            const int ry = r / R, rx = r - ry * R;
            const int gy = 2 * iy0 - 1 + ry, gx = 2 * ix0 - 1 + rx;
            float v = 0.f;
            if (gy >= 0 && gy < W2 && gx >= 0 && gx < W2) v = de[(co0 + c) * oplane + (size_t)gy * W2 + gx];
            s[i] = v;
        }
        __syncthreads();
        float d[CC][9];
#pragma unroll
        for (int c = 0; c < CC; ++c) {
            const float* sp = s + c * RR + 2 * py * R + 2 * px;
#pragma unroll
            for (int k = 0; k < 9; ++k) d[c][k] = sp[(k / 3) * R + k % 3];
        }
        const float* wr = w + (size_t)ci0 * 9 * cout + co0;
#pragma unroll
        for (int j = 0; j < CIG; ++j)
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float* wk = wr + (size_t)(j * 9 + k) * cout;
#pragma unroll
                for (int c = 0; c < CC; ++c) acc[j] = fmaf(wk[c], d[c][k], acc[j]);
            }
    }
    const int iy = iy0 + py, ix = ix0 + px;
    if (iy >= H || ix >= H) return;
    const size_t plane = (size_t)H * H;
    float* xe = dx + ((size_t)blockIdx.z * cin + ci0) * plane + (size_t)iy * H + ix;
#pragma unroll
    for (int j = 0; j < CIG; ++j) xe[j * plane] = acc[j];
}

// x: (n, cin, H, H); du: (n, cout, 2H, 2H); part: [slice * PB + wave or pixel lane][cin * 9 * cout], PB = 256 / max(Q, 64).
// A slice is the tiles [blockIdx.x * tps, .. + tps) of the n * tiles_x^2 tiles, envs in order.
template <int T, int CIB, int COB>
__global__ __launch_bounds__(256) void occ_dec_bwd_dw_kernel(const float* __restrict__ x, const float* __restrict__ du,
                                                             float* __restrict__ part, int cin, int cout, int H, int tiles_x,
                                                             int total_tiles, int tps) {
    constexpr int TT = T * T, R = 2 * T + 1, RR = R * R, XP = TT + 1, Q = (CIB / 16) * COB, P = 256 / Q;
    static_assert(Q <= 256 && 256 % Q == 0 && (Q >= 64 || 64 % Q == 0), "thread layout");
    __shared__ float xs[CIB * XP];
    __shared__ float ds[COB * RR];
    const int tid = threadIdx.x;
    const int q = tid % Q, pl = tid / Q;
    const int col = q % COB, cig = q / COB;
    const int nco = cout / COB;
    const int ci0 = (blockIdx.y / nco) * CIB, co0 = (blockIdx.y % nco) * COB;
    const int W2 = 2 * H;
    const size_t plane = (size_t)H * H, oplane = 4 * plane;
    const int tiles_env = tiles_x * tiles_x;

    float acc[16][9];
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[i][k] = 0.f;

    const int t0 = blockIdx.x * tps, t1 = min(t0 + tps, total_tiles);
    for (int t = t0; t < t1; ++t) {
        const int env = t / tiles_env, rem = t - env * tiles_env;
        const int iy0 = (rem / tiles_x) * T, ix0 = (rem % tiles_x) * T;
        const float* xe = x + ((size_t)env * cin + ci0) * plane;
        const float* de = du + ((size_t)env * cout + co0) * oplane;
        __syncthreads();
        for (int i = tid; i < CIB * TT; i += 256) {
            const int c = i / TT, p = i - c * TT;
            const int gy = iy0 + p / T, gx = ix0 + p % T;
            float v = 0.f;
            if (gy < H && gx < H) v = xe[c * plane + (size_t)gy * H + gx];
            xs[c * XP + p] = v;
        }
        for (int i = tid; i < COB * RR; i += 256) {
            const int c = i / RR, r = i - c * RR;
            const int ry = r / R, rx = r - ry * R;
            const int gy = 2 * iy0 - 1 + ry, gx = 2 * ix0 - 1 + rx;
            float v = 0.f;
            if (gy >= 0 && gy < W2 && gx >= 0 && gx < W2) v = de[c * oplane + (size_t)gy * W2 + gx];
            ds[i] = v;
        }
        __syncthreads();
        for (int p = pl; p < TT; p += P) {
            const float* dp = ds + col * RR + 2 * (p / T) * R + 2 * (p % T);
            float d[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) d[k] = dp[(k / 3) * R + k % 3];
            const float* xp = xs + cig * 16 * XP + p;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float xv = xp[i * XP];
#pragma unroll
                for (int k = 0; k < 9; ++k) acc[i][k] = fmaf(xv, d[k], acc[i][k]);
            }
        }
    }
    constexpr int PB = dw_partials(Q);
    int pb;
    if (!bwd_dw_fold<Q>(reinterpret_cast<float(&)[16 * 9]>(acc), pl, pb)) return;
    const size_t nout = (size_t)cin * 9 * cout;
    float* dst = part + ((size_t)blockIdx.x * PB + pb) * nout + (size_t)(ci0 + cig * 16) * 9 * cout + co0 + col;
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int k = 0; k < 9; ++k) dst[(size_t)(i * 9 + k) * cout] = acc[i][k];
}

// out[e] = part[0][e] + part[1][e] + ..: four interleaved f64 chains (partials s, s + 4, ..), then the four in order.
__global__ __launch_bounds__(256) void occ_dec_bwd_sum_kernel(const float* __restrict__ part, int nparts, int nout,
                                                              float* __restrict__ out) {
    __shared__ double red[4][64];
    const int lane = threadIdx.x % 64, sub = threadIdx.x / 64;
    const int e = blockIdx.x * 64 + lane;
    double sum = 0.0;
    if (e < nout)
        for (int p = sub; p < nparts; p += 4) sum += (double)part[(size_t)p * nout + e];
    red[sub][lane] = sum;
    __syncthreads();
    if (sub == 0 && e < nout) out[e] = (float)(((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]);
}

// ---- host side -----------------------------------------------------------------------------------------------------

// The (ci, co) tile, pixel tile and K split of one weight gradient, the decoder's (bwd_dw_plan) or the encoder's
// (enc_dw_plan, occ_encoder_bwd.hpp).
struct DwPlan {
    int T, cib, cob, pb, grid_y, tiles_x, total_tiles, tps, slices;
    size_t part_bytes;
};

// The K split for a cib x cob tile of (ci, co) whose one pixel takes q threads, over the T x T tiles of n planes of
// side x side pixels, aiming at `blocks` blocks per launch: a function of the shapes alone.
inline DwPlan dw_split(int cib, int cob, int T, int q, int cin, int cout, int side, int n, int blocks) {
    DwPlan p;
    p.T = T, p.cib = cib, p.cob = cob;
    p.pb = dw_partials(q);
    p.grid_y = (cin / cib) * (cout / cob);
    p.tiles_x = (side + T - 1) / T;
    p.total_tiles = n * p.tiles_x * p.tiles_x;
    const int want = blocks / p.grid_y;
    p.tps = (p.total_tiles + want - 1) / want;
    p.slices = (p.total_tiles + p.tps - 1) / p.tps;
    p.part_bytes = (size_t)p.slices * p.pb * cin * 9 * cout * sizeof(float);
    return p;
}

// Decoder level j (cout = 128 >> j): a thread owns 16 ci x 1 co.
inline DwPlan bwd_dw_plan(int j, int H, int n) {
    const int cout = kEncCh << (kEncLevels - 1 - j);
    int T, cib, cob;
    if (cout >= 64) T = 4, cib = 64, cob = 64;
    else if (cout == 32) T = 4, cib = 64, cob = 32;
    else if (cout == 16) T = 8, cib = 32, cob = 16;
    else T = 8, cib = 16, cob = 8;
    return dw_split(cib, cob, T, (cib / 16) * cob, 2 * cout, cout, H, n, kBwdDwBlocks);
}

inline int bwd_chunks(int plane) { return (plane + kBwdChunk - 1) / kBwdChunk; }

// Batch-statistics BatchNorm of the joint training (occ_bn_train.hpp, included after occ_fullnet_bwd.hpp).  A walk that is
// given a BnTrain runs bn_fwd_layer after each conv / up kernel and bn_bwd_act in place of each activation step.
struct BnTrain;
struct BnDy {
    const float* dy;    // (n, c, plane), or with gf what is added to the pooled gradient (may be null)
    const float* gf;    // the last down: d loss / d feats (n, c)
    const float *gp, *prob, *y4, *clsw;  // the last decoder level: d loss / d prob, the kept prob, y_4 and cls_w
};
static void bn_fwd_layer(const BnTrain& bn, int layer, int c, int plane, int n, const float* gamma, const float* beta,
                         const float* r, float* y, const float* add, float* feats, const float* cls, float* prob, float* pkeep,
                         hipStream_t st);
static void bn_bwd_act(const BnTrain& bn, int layer, int c, int plane, int n, const BnDy& src, float* du, const float* r,
                       const float* gamma, float* gscale, float* gshift, float* gcls, char* scratch, hipStream_t st);

// workspace of occ_segment_train_forward / occ_segment_backward: the workspace of occ_segment_forward (b0 | b1 | partials |
// skips | last; b0 and b1 serve the encoder only), then per level j: y_j | r_j, then p, then the two gradient buffers
// g0 (the size of y_4) and g1 (the size of y_3) that dY / dU of the levels alternate in.
struct TrainWs {
    SegWs seg;
    size_t lvl_bytes[kEncLevels], p_bytes, total, scratch;
};

inline TrainWs train_ws_layout(int img, int n) {
    TrainWs l;
    l.seg = seg_ws_layout(img, n);
    l.total = l.seg.total;
    l.scratch = 0;
    int H = img >> kEncLevels;
    for (int j = 0; j < kEncLevels; ++j) {
        const int c = kEncCh << (kEncLevels - 1 - j);
        l.lvl_bytes[j] = enc_align((size_t)n * c * (2 * H) * (2 * H) * sizeof(float));
        l.total += 2 * l.lvl_bytes[j];
        const size_t act = (size_t)c * n * bwd_chunks(4 * H * H) * 5 * sizeof(double);
        const size_t dw = bwd_dw_plan(j, H, n).part_bytes;
        l.scratch = act > l.scratch ? act : l.scratch;
        l.scratch = dw > l.scratch ? dw : l.scratch;
        H *= 2;
    }
    l.p_bytes = enc_align((size_t)n * img * img * sizeof(float));
    l.total += l.p_bytes + l.lvl_bytes[kEncLevels - 1] + l.lvl_bytes[kEncLevels - 2];
    return l;
}

struct TrainPtrs {
    float *last, *skip[kEncLevels], *y[kEncLevels], *r[kEncLevels], *p, *g[2];
};

inline TrainPtrs train_ptrs(const TrainWs& l, char* ws) {
    TrainPtrs t;
    char* at = ws + 2 * l.seg.buf_bytes + l.seg.part_bytes;
    for (int lv = 0; lv < kEncLevels; ++lv) {
        t.skip[lv] = (float*)at;
        at += l.seg.skip_bytes[lv];
    }
    t.last = (float*)at;
    at += l.seg.last_bytes;
    for (int j = 0; j < kEncLevels; ++j) {
        t.y[j] = (float*)at;
        t.r[j] = (float*)(at + l.lvl_bytes[j]);
        at += 2 * l.lvl_bytes[j];
    }
    t.p = (float*)at;
    at += l.p_bytes;
    t.g[0] = (float*)at;
    t.g[1] = (float*)(at + l.lvl_bytes[kEncLevels - 1]);
    return t;
}

// The five up levels on t.last and t.skip, keeping y_j, r_j and p: 5 launches.  bn: batch statistics (3 launches per level
// more; the scale / shift slots carry gamma / beta).
static void dec_train_forward(int img, const float* dec_packed, int n, const TrainPtrs& t, float* prob, hipStream_t st,
                              const BnTrain* bn = nullptr) {
    const float* w = dec_packed;
    const float* cls = dec_packed + dec_packed_floats() - (kEncCh + 1);
    const float* x = t.last;
    int H = img >> kEncLevels;
    for (int j = 0; j < kEncLevels; ++j) {
        const int lv = kEncLevels - 1 - j;
        const int c = kEncCh << lv;
        const bool last = j == kEncLevels - 1;
        dec_launch_up(x, t.y[j], t.skip[lv], w, 2 * c, c, H, n, last ? cls : nullptr, prob, t.p, st, t.r[j]);
        if (bn) {
            const float* gamma = w + 9LL * 2 * c * c + c;
            bn_fwd_layer(*bn, 16 + j, c, 4 * H * H, n, gamma, gamma + c, t.r[j], t.y[j], t.skip[lv], nullptr, last ? cls : nullptr,
                         prob, t.p, st);
        }
        w += 9LL * 2 * c * c + 3LL * c;
        x = t.y[j];
        H *= 2;
    }
}

// Encoder (17 launches) + decoder (5 launches), every decoder activation kept.
static void seg_train_forward(int img, int dil, bool residual, bool separable, const float* enc_packed, const float* dec_packed,
                              const float* obs, int n, char* ws, float* feats, float* prob, hipStream_t st) {
    const TrainWs l = train_ws_layout(img, n);
    const TrainPtrs t = train_ptrs(l, ws);
    EncKeep keep;
    for (int lv = 0; lv < kEncLevels; ++lv) keep.skip[lv] = t.skip[lv];
    keep.last = t.last;
    enc_forward(img, dil, residual, separable, enc_packed, obs, n, ws, feats, st, &keep);
    dec_train_forward(img, dec_packed, n, t, prob, st);
}

template <int T, int CIB, int COB>
static void bwd_launch_dw(const DwPlan& p, const float* x, const float* du, float* part, int cin, int cout, int H,
                          hipStream_t st) {
    hipLaunchKernelGGL((occ_dec_bwd_dw_kernel<T, CIB, COB>), dim3(p.slices, p.grid_y), dim3(256), 0, st, x, du, part, cin, cout, H,
                       p.tiles_x, p.total_tiles, p.tps);
}

// The four (ci, co) tiles of bwd_dw_plan.
static void dec_launch_dw(const DwPlan& p, const float* x, const float* du, float* part, int cin, int cout, int H, hipStream_t st) {
    if (p.cob == 64) bwd_launch_dw<4, 64, 64>(p, x, du, part, cin, cout, H, st);
    else if (p.cob == 32) bwd_launch_dw<4, 64, 32>(p, x, du, part, cin, cout, H, st);
    else if (p.cob == 16) bwd_launch_dw<8, 32, 16>(p, x, du, part, cin, cout, H, st);
    else bwd_launch_dw<8, 16, 8>(p, x, du, part, cin, cout, H, st);
}

// The input gradient of one level: dx (n, cin, H, H) from du (n, cout, 2H, 2H).
static void dec_launch_dx(const float* du, float* dx, const float* w, int cin, int cout, int H, int n, hipStream_t st) {
    const int T = enc_tile(H);
    const TileLaunch l = tile_launch(T, H, cin / kBwdDxCIG, n);
    if (T == 16) hipLaunchKernelGGL((occ_dec_bwd_dx_kernel<16>), l.grid, l.block, 0, st, du, dx, w, cin, cout, H, l.tiles_x);
    else hipLaunchKernelGGL((occ_dec_bwd_dx_kernel<8>), l.grid, l.block, 0, st, du, dx, w, cin, cout, H, l.tiles_x);
}

// What follows the activation step of one layer, the decoder's or the encoder's: the block partials of its `sums`
// per-channel sums (in scratch, n_part per sum and channel) added into dst, then the weight gradient from the layer's input
// and dU: launch_dw(part) writes the partials of plan p to scratch, which are added into the nout elements of gw (9 cin
// cout of a dense layer, cin cout of a pointwise one).  3 launches.
template <class LaunchDw>
static void bwd_layer_tail(const DwPlan& p, int nout, int cout, int n_part, int sums, const BwdActDst& dst, char* scratch, float* gw,
                           hipStream_t st, LaunchDw launch_dw) {
    hipLaunchKernelGGL(occ_dec_bwd_act_final_kernel, dim3(cout, sums), dim3(64), 0, st, (const double*)scratch, n_part, sums, dst);
    float* part = (float*)scratch;
    launch_dw(part);
    hipLaunchKernelGGL(occ_dec_bwd_sum_kernel, dim3((nout + 63) / 64), dim3(256), 0, st, part, p.slices * p.pb, nout, gw);
}

// Where the joint training (occ_fullnet_bwd.hpp) keeps the decoder's gradients that the encoder's backward reads.
struct DecJoin {
    float* dlast;              // (n, 256, S/32, S/32): the input gradient of level 0
    float* dskip[kEncLevels];  // dskip[lv], lv >= 1: the dY of level 4 - lv, which is d skip[lv]; dskip[0] is not stored
    float* du;                 // every level's dU, the size of y_4
};

// The backward of the latest forward on the tensors of t: per level, last first, the activation step (2 launches), the
// weight gradient (2 launches) and, above level 0, the input gradient: 24 launches.  grad_packed is overwritten.  Without
// join dY and dU alternate in t.g, dU written over dY.  With join the activation step is out of place and level 0 has an
// input gradient too: 25 launches.  bn: the forward ran with batch statistics; every activation step is bn_bwd_act (2
// launches per level more).
static void dec_backward(int img, const float* dec_packed, int n, const TrainPtrs& t, const float* grad_prob, char* scratch,
                         float* grad_packed, hipStream_t st, const DecJoin* join = nullptr, const BnTrain* bn = nullptr) {
    long long woff[kEncLevels];
    long long off = 0;
    for (int j = 0; j < kEncLevels; ++j) {
        const int c = kEncCh << (kEncLevels - 1 - j);
        woff[j] = off;
        off += 9LL * 2 * c * c + 3LL * c;
    }
    float* gcls = grad_packed + off;
    const float* cls = dec_packed + off;
    for (int j = kEncLevels - 1; j >= 0; --j) {
        const int c = kEncCh << (kEncLevels - 1 - j), cin = 2 * c;
        const int H = (img >> kEncLevels) << j, plane = 4 * H * H;
        const bool last = j == kEncLevels - 1;
        const float* w = dec_packed + woff[j];
        float* gw = grad_packed + woff[j];
        float* gbias = gw + 9LL * cin * c;
        const int lv = kEncLevels - 1 - j;
        float* g = join ? join->du : t.g[lv % 2];
        const float* dy = join ? join->dskip[lv] : g;
        const float* x = j == 0 ? t.last : t.y[j - 1];
        const int chunks = bwd_chunks(plane);
        const dim3 agrid(chunks, c, n);
        const BwdActDst dst = bn ? BwdActDst{{gbias, nullptr, nullptr, nullptr, nullptr}}
                                 : BwdActDst{{gbias + c, gbias + 2 * c, gbias, gcls, gcls + kEncCh}};
        if (bn) {
            const BnDy src = last ? BnDy{nullptr, nullptr, grad_prob, t.p, t.y[j], cls}
                                  : BnDy{dy, nullptr, nullptr, nullptr, nullptr, nullptr};
            bn_bwd_act(*bn, 16 + j, c, plane, n, src, g, t.r[j], w + 9LL * cin * c + c, gbias + c, gbias + 2 * c, gcls, scratch, st);
        } else if (last)
            hipLaunchKernelGGL((occ_dec_bwd_act_kernel<true>), agrid, dim3(256), 0, st, nullptr, g, t.r[j], w + 9LL * cin * c + c, c, plane,
                               grad_prob, t.p, t.y[j], cls, (double*)scratch);
        else
            hipLaunchKernelGGL((occ_dec_bwd_act_kernel<false>), agrid, dim3(256), 0, st, dy, g, t.r[j], w + 9LL * cin * c + c, c, plane,
                               nullptr, nullptr, nullptr, nullptr, (double*)scratch);
        const DwPlan p = bwd_dw_plan(j, H, n);
        bwd_layer_tail(p, 9 * cin * c, c, n * chunks, bn ? 1 : last ? 5 : 3, dst, scratch, gw, st,
                       [&](float* part) { dec_launch_dw(p, x, g, part, cin, c, H, st); });
        if (j > 0 || join)  // into the dY of level j - 1
            dec_launch_dx(g, !join ? t.g[(kEncLevels - j) % 2] : j > 0 ? join->dskip[lv + 1] : join->dlast, w, cin, c, H, n, st);
    }
}

static void seg_backward(int img, const float* dec_packed, int n, char* ws, const float* grad_prob, char* scratch,
                         float* grad_packed, hipStream_t st) {
    const TrainWs l = train_ws_layout(img, n);
    dec_backward(img, dec_packed, n, train_ptrs(l, ws), grad_prob, scratch, grad_packed, st);
}
