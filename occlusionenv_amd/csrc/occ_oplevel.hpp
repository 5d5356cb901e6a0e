// occ_oplevel.hpp -- operator-level K-buffer rasteriser (outputs in PyTorch3D layout) and its backward.
// Part of the single translation unit occ_kernels.hip (included inside namespace occ; not a stand-alone header).

// ------------------------------------------------------------------------------------------
// Operator-level replacement of PyTorch3D's _C.rasterize_meshes / _C.rasterize_meshes_backward (naive path,
// bin_size = 0).  The fused step() above never materialises these; this file exists for callers of the rasteriser
// itself (SURVEY.md §8b lower surface) and is written for exactness: no FMA contraction / reciprocal shortcuts, the
// arithmetic order is the one of SURVEY A.4.  Three forward kernels produce the same bits on all four outputs:
//   occ_rast_naive_fwd_kernel  one thread per pixel, all faces of its mesh (upstream's naive CUDA kernel); any K
//   occ_rast_tiled_fwd_kernel  one wave per 8x8 tile, faces in order, lists in LDS: meshes with clipped pairs; K <= 128
//   occ_rast_quad_fwd_kernel   one wave per 4x4 tile, four faces in flight: meshes without pairs; K <= 128
// (128: 64 lists * K * 8 bytes of LDS against 64 KiB; the C entry point hands a larger K to the naive kernel.)
// Every rule they share is written once, below, and each kernel only decides WHICH faces a pixel looks at, in what
// order, and WHERE its list lives:
//   k_centre                           NDC centre of a pixel
//   kbuf_rejected                      per-face rejects
//   kbuf_bbox, KbufTile, kbuf_tile,    the face's bbox +- sqrt(blur); a tile's pixel, centre range and face test
//     kbuf_tile_hit
//   kbuf_bary, kbuf_closest_edge       pre-clip barycentrics and the closest edge (restated in the dists backward: see there)
//   kbuf_eval                          per-(face, pixel) evaluation: bbox test ... blur test
//   kbuf_pair_takes_slot               the clipped-pair rule's decision
//   kbuf_after                         the (z, face) order of every scan, sort and merge
//   KbufOut, kbuf_store, kbuf_fill     one output entry; the -1 of the empty slots
//   KbufCol, kbuf_col_farthest,        a lane's list in LDS (tiled and quad): farthest entry, insertion sort, entry
//     kbuf_col_sort, kbuf_emit         to output slot (distance and barycentrics re-derived from the face)
// ------------------------------------------------------------------------------------------
#pragma clang fp contract(off)
__device__ __forceinline__ float k_edge(float px, float py, float ax, float ay, float bx, float by) {
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}
__device__ __forceinline__ float k_seg(float px, float py, float ax, float ay, float bx, float by) {
    const float bax = bx - ax, bay = by - ay;
    const float l2 = bax * bax + bay * bay;
    if (l2 <= kEpsilon) return (px - bx) * (px - bx) + (py - by) * (py - by);
    float t = (bax * (px - ax) + bay * (py - ay)) / l2;
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    const float qx = ax + t * bax - px, qy = ay + t * bay - py;
    return qx * qx + qy * qy;
}
// NDC centre of pixel i on an axis of `size` pixels: decreases with i (+X is left, +Y is up)
__device__ __forceinline__ float k_centre(int i, int size) {
    return -1.0f + (2.0f * (float)(size - 1 - i) + 1.0f) / (float)size;
}

struct KbufArgs {
    const float* face_verts;      // (F,3,3)
    const int64_t* first_idx;     // (N)
    const int64_t* num_faces;     // (N)
    const int64_t* neighbor;      // (F) or null
    int N, H, W, K;
    float blur;
    int persp, clipb, cull;
    int64_t* p2f;  // (N,H,W,K)
    float* zbuf;   // (N,H,W,K)
    float* bary;   // (N,H,W,K,3)
    float* dists;  // (N,H,W,K)
};
struct KbufFace {
    float x0, y0, z0, x1, y1, z1, x2, y2, z2;
};
__device__ __forceinline__ KbufFace kbuf_load(const float* __restrict__ face_verts, int64_t f) {
    const float* v = face_verts + f * 9;
    return KbufFace{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]};
}
// per-face rejects: back face (when culling), degenerate area, wholly behind the camera
__device__ __forceinline__ bool kbuf_rejected(const KbufFace& v, int cull) {
    const float area = k_edge(v.x0, v.y0, v.x1, v.y1, v.x2, v.y2);
    return (cull && area < 0.0f) || (area <= kEpsilon && area >= -kEpsilon) || fmaxf(fmaxf(v.z0, v.z1), v.z2) < 0.0f;
}
// the face's bbox widened by sqb = sqrt(blur)
struct KbufBox {
    float xmin, xmax, ymin, ymax;
};
__device__ __forceinline__ KbufBox kbuf_bbox(const KbufFace& v, float sqb) {
    return KbufBox{fminf(fminf(v.x0, v.x1), v.x2) - sqb, fmaxf(fmaxf(v.x0, v.x1), v.x2) + sqb,
                   fminf(fminf(v.y0, v.y1), v.y2) - sqb, fmaxf(fmaxf(v.y0, v.y1), v.y2) + sqb};
}
// pre-clip barycentrics: area-normalised edge functions, perspective-corrected on request.  All three > 0 = inside.
struct KbufBary {
    float p0, p1, p2;
};
__device__ __forceinline__ KbufBary kbuf_bary(const KbufFace& v, float xf, float yf, int persp) {
    const float ar = k_edge(v.x2, v.y2, v.x0, v.y0, v.x1, v.y1) + kEpsilon;
    KbufBary p{k_edge(xf, yf, v.x1, v.y1, v.x2, v.y2) / ar, k_edge(xf, yf, v.x2, v.y2, v.x0, v.y0) / ar,
               k_edge(xf, yf, v.x0, v.y0, v.x1, v.y1) / ar};
    if (persp) {
        const float w0 = p.p0 * v.z1 * v.z2, w1 = v.z0 * p.p1 * v.z2, w2 = v.z0 * v.z1 * p.p2;
        const float den = fmaxf(w0 + w1 + w2, kEpsilon);
        p.p0 = w0 / den; p.p1 = w1 / den; p.p2 = w2 / den;
    }
    return p;
}
// closest edge at (xf, yf): its squared distance and amin = 0 / 1 / 2 for edge 01 / 02 / 12 (a tie goes to the lower one)
struct KbufEdge {
    float dist;
    int amin;
};
__device__ __forceinline__ KbufEdge kbuf_closest_edge(const KbufFace& v, float xf, float yf) {
    const float e01 = k_seg(xf, yf, v.x0, v.y0, v.x1, v.y1), e02 = k_seg(xf, yf, v.x0, v.y0, v.x2, v.y2),
                e12 = k_seg(xf, yf, v.x1, v.y1, v.x2, v.y2);
    return KbufEdge{fminf(fminf(e01, e02), e12), (e01 <= e02 && e01 <= e12) ? 0 : ((e02 <= e01 && e02 <= e12) ? 1 : 2)};
}

struct KbufHit {
    bool ok;      // the face is a candidate at this pixel
    bool inside;
    float pz, dist, c0, c1, c2;
    int amin;
};
// per-(face, pixel) evaluation after the per-face rejects: bbox test, barycentrics, clip, depth, closest edge, blur test
__device__ __forceinline__ KbufHit kbuf_eval(const KbufArgs& a, const KbufFace& v, float xf, float yf, float sqb) {
    KbufHit h;
    h.ok = false;
    h.inside = false;
    h.pz = h.dist = h.c0 = h.c1 = h.c2 = 0.f;
    h.amin = 0;
    const KbufBox bb = kbuf_bbox(v, sqb);
    if (!((bb.xmin <= xf && xf <= bb.xmax) && (bb.ymin <= yf && yf <= bb.ymax))) return h;
    const KbufBary p = kbuf_bary(v, xf, yf, a.persp);
    float c0 = p.p0, c1 = p.p1, c2 = p.p2;
    if (a.clipb) {
        c0 = fmaxf(p.p0, 0.0f); c1 = fmaxf(p.p1, 0.0f); c2 = fmaxf(p.p2, 0.0f);
        const float sm = fmaxf(c0 + c1 + c2, kBaryClipMin);
        c0 /= sm; c1 /= sm; c2 /= sm;
    }
    const float pz = c0 * v.z0 + c1 * v.z1 + c2 * v.z2;
    if (pz < 0.0f) return h;
    const KbufEdge e = kbuf_closest_edge(v, xf, yf);
    h.amin = e.amin;
    h.inside = p.p0 > 0.0f && p.p1 > 0.0f && p.p2 > 0.0f;
    if (!h.inside && e.dist >= a.blur) return h;
    h.ok = true;
    h.pz = pz; h.dist = e.dist; h.c0 = c0; h.c1 = c1; h.c2 = c2;
    return h;
}

// clipped-pair rule for a face f whose sibling nb is in the pixel's list: f takes the sibling's slot when
// its closest edge is closer than the sibling's - unless the two closest edges are the diagonal the pair shares (the tie
// definition of DESIGN.md §2).  (amin_nb, dist_nb): the sibling's closest edge at this pixel.
__device__ __forceinline__ bool kbuf_pair_takes_slot(int64_t f, const KbufHit& h, int64_t nb, int amin_nb, float dist_nb) {
    const bool shared_tie = (nb == f - 1 && amin_nb == 2 && h.amin == 0) || (nb == f + 1 && amin_nb == 0 && h.amin == 2);
    return !shared_tie && h.dist < dist_nb;
}
// the order of the lists: does (za, fa) come after (zb, fb)?
__device__ __forceinline__ bool kbuf_after(float za, int64_t fa, float zb, int64_t fb) {
    return za > zb || (za == zb && fa > fb);
}
// the same with the faces still in memory (the naive kernel's list): they are loaded on a depth tie only
__device__ __forceinline__ bool kbuf_after(float za, const int64_t* fa, float zb, const int64_t* fb) {
    return za == zb ? kbuf_after(za, *fa, zb, *fb) : za > zb;
}

// the K output slots of a pixel
struct KbufOut {
    int64_t* f;
    float *z, *d, *b;
};
__device__ __forceinline__ KbufOut kbuf_out(const KbufArgs& a, long pix) {
    return KbufOut{a.p2f + pix * a.K, a.zbuf + pix * a.K, a.dists + pix * a.K, a.bary + pix * a.K * 3};
}
__device__ __forceinline__ void kbuf_store(const KbufOut& o, int r, int64_t f, float z, const KbufHit& h) {
    o.f[r] = f; o.z[r] = z; o.d[r] = h.inside ? -h.dist : h.dist;
    o.b[r * 3] = h.c0; o.b[r * 3 + 1] = h.c1; o.b[r * 3 + 2] = h.c2;
}
// empty slots = -1: slots i, i + s, ... below K
__device__ __forceinline__ void kbuf_fill(const KbufOut& o, int i, int K, int s) {
    for (; i < K; i += s) {
        o.f[i] = -1; o.z[i] = -1.0f; o.d[i] = -1.0f;
        o.b[i * 3] = o.b[i * 3 + 1] = o.b[i * 3 + 2] = -1.0f;
    }
}

// ------------------------------------------------------------------------------------------
// occ_rast_naive_fwd_kernel: the structure of upstream's naive CUDA kernel - one thread per pixel, all faces of its
// mesh in order, replace-the-farthest K list kept directly in the output arrays, bubble sort at the end.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void occ_rast_naive_fwd_kernel(KbufArgs a) {
    const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long npix = (long)a.N * a.H * a.W;
    if (pix >= npix) return;
    const int n = (int)(pix / ((long)a.H * a.W));
    const int rem = (int)(pix - (long)n * a.H * a.W);
    const int yi = rem / a.W, xi = rem - yi * a.W;
    const float yf = k_centre(yi, a.H), xf = k_centre(xi, a.W);
    const float sqb = sqrtf(a.blur);
    const int K = a.K;
    const KbufOut o = kbuf_out(a, pix);
    int qn = 0;
    const int64_t f0 = a.first_idx[n], f1 = f0 + a.num_faces[n];
    for (int64_t f = f0; f < f1; ++f) {
        const KbufFace v = kbuf_load(a.face_verts, f);
        if (kbuf_rejected(v, a.cull)) continue;
        const KbufHit h = kbuf_eval(a, v, xf, yf, sqb);
        if (!h.ok) continue;
        int itop = -1;
        const int64_t nb = a.neighbor ? a.neighbor[f] : -1;
        if (nb != -1) {
            for (int i = 0; i < qn; ++i)
                if (o.f[i] == nb) { itop = i; break; }
        }
        int slot = -1;
        if (itop != -1) {
            // (the sibling's distance is read back from its dists slot)
            const KbufEdge g = kbuf_closest_edge(kbuf_load(a.face_verts, nb), xf, yf);
            if (kbuf_pair_takes_slot(f, h, nb, g.amin, fabsf(o.d[itop]))) slot = itop;
        } else if (qn < K) {
            slot = qn++;
        } else {
            // full: the candidate displaces the farthest entry if it comes before it
            int im = 0;
            for (int i = 1; i < K; ++i)
                if (kbuf_after(o.z[i], o.f + i, o.z[im], o.f + im)) im = i;
            if (kbuf_after(o.z[im], o.f + im, h.pz, &f)) slot = im;
        }
        if (slot >= 0) kbuf_store(o, slot, f, h.pz, h);
    }
    // ascending (z, f)
    for (int i = 0; i < qn - 1; ++i)
        for (int j = 0; j < qn - 1 - i; ++j)
            if (kbuf_after(o.z[j], o.f + j, o.z[j + 1], o.f + j + 1)) {
                const int64_t tf = o.f[j]; o.f[j] = o.f[j + 1]; o.f[j + 1] = tf;
                float t = o.z[j]; o.z[j] = o.z[j + 1]; o.z[j + 1] = t;
                t = o.d[j]; o.d[j] = o.d[j + 1]; o.d[j + 1] = t;
#pragma unroll
                for (int c = 0; c < 3; ++c) { t = o.b[j * 3 + c]; o.b[j * 3 + c] = o.b[(j + 1) * 3 + c]; o.b[(j + 1) * 3 + c] = t; }
            }
    kbuf_fill(o, qn, K, 1);
}

// ------------------------------------------------------------------------------------------
// The two tiled producers of the same K-buffers (occ_rasterize_meshes_tiled): one wave per (mesh, tile).
//   * Faces are taken 64 at a time, one per lane; a lane applies the per-face rejects and asks whether the face's bbox
//     +- sqrt(blur) can hold ANY pixel centre of the tile.  A face that fails fails kbuf_eval's own bbox test at every
//     pixel of the tile, so skipping it changes nothing.
//   * A lane's list keeps (depth, face) only, in LDS: [K][64] depths, then [K][64] packed face indices, entry i of lane
//     l at [i * 64 + l] (lane-contiguous: no bank conflicts).  Signed distance and barycentrics are NOT carried along
//     but re-derived from the face at the end - the same expressions on the same inputs give the same bits.
//   * At the end every lane sorts its entries by (depth, face) in LDS and writes its output slots once.
// ------------------------------------------------------------------------------------------
// the wave's tile of side T (8 or 4) and the lane's pixel p (row-major) of it
struct KbufTile {
    int xi, yi;
    bool valid;                    // the pixel is inside the image
    float xf, yf;
    float xmin, xmax, ymin, ymax;  // range of the tile's pixel centres
};
template <int T>
__device__ __forceinline__ KbufTile kbuf_tile(const KbufArgs& a, int t, int tiles_x, int p) {
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    KbufTile r;
    r.xi = tx * T + (p & (T - 1));
    r.yi = ty * T + (p >> (T == 8 ? 3 : 2));
    r.valid = r.xi < a.W && r.yi < a.H;
    r.xf = k_centre(r.xi, a.W);
    r.yf = k_centre(r.yi, a.H);
    r.xmax = k_centre(tx * T, a.W);
    r.xmin = k_centre(min(tx * T + T - 1, a.W - 1), a.W);
    r.ymax = k_centre(ty * T, a.H);
    r.ymin = k_centre(min(ty * T + T - 1, a.H - 1), a.H);
    return r;
}
// can the face be a candidate at some pixel of the tile?  necessary: it is not rejected and the two ranges overlap
__device__ __forceinline__ bool kbuf_tile_hit(const KbufTile& t, const KbufFace& v, int cull, float sqb) {
    const KbufBox bb = kbuf_bbox(v, sqb);
    return !kbuf_rejected(v, cull) && bb.xmin <= t.xmax && t.xmin <= bb.xmax && bb.ymin <= t.ymax && t.ymin <= bb.ymax;
}

// the list of lane `lane` in the wave's LDS
struct KbufCol {
    float* sz;  // [K][64] depths
    int* sf;    // [K][64] packed face indices
    int lane;
    __device__ __forceinline__ float z(int i) const { return sz[i * 64 + lane]; }
    __device__ __forceinline__ int f(int i) const { return sf[i * 64 + lane]; }
    __device__ __forceinline__ void set(int i, float z_, int f_) const { sz[i * 64 + lane] = z_; sf[i * 64 + lane] = f_; }
};
__device__ __forceinline__ KbufCol kbuf_col(unsigned char* smem, int K, int lane) {
    return KbufCol{reinterpret_cast<float*>(smem), reinterpret_cast<int*>(smem) + 64 * K, lane};
}
struct KbufFar {
    float z;
    int f, i;
};
// farthest of the K entries of a full list
__device__ __forceinline__ KbufFar kbuf_col_farthest(const KbufCol& c, int K) {
    KbufFar m{c.z(0), c.f(0), 0};
    for (int i = 1; i < K; ++i) {
        const float zi = c.z(i);
        const int fi = c.f(i);
        if (kbuf_after(zi, fi, m.z, m.f)) m = KbufFar{zi, fi, i};
    }
    return m;
}
// ascending (z, f): insertion sort of the first qn entries
__device__ __forceinline__ void kbuf_col_sort(const KbufCol& c, int qn) {
    for (int i = 1; i < qn; ++i) {
        const float zi = c.z(i);
        const int fi = c.f(i);
        int j = i - 1;
        while (j >= 0) {
            const float zj = c.z(j);
            const int fj = c.f(j);
            if (!kbuf_after(zj, fj, zi, fi)) break;
            c.set(j + 1, zj, fj);
            --j;
        }
        c.set(j + 1, zi, fi);
    }
}
// list entry (z, f) of the pixel at (xf, yf) -> output slot r
__device__ __forceinline__ void kbuf_emit(const KbufArgs& a, const KbufOut& o, int r, float z, int f, float xf, float yf, float sqb) {
    kbuf_store(o, r, f, z, kbuf_eval(a, kbuf_load(a.face_verts, f), xf, yf, sqb));
}

// Does mesh n hold a clipped-face pair?  (PyTorch3D's clip_faces hands the rasteriser a neighbour array whenever clipping is
// enabled - all -1 unless a face straddled the clip plane - so "no array" is the rare case and "an array without pairs" the
// common one.)  Every wave of the two tiled kernels asks this for its mesh first: a coalesced pass over the mesh's slice of
// the array, a few microseconds; the kernel whose mode the mesh is not in returns at once.
__device__ __forceinline__ bool mesh_has_pairs(const KbufArgs& a, int n, int lane) {
    if (!a.neighbor) return false;
    const int64_t f0 = a.first_idx[n], f1 = f0 + a.num_faces[n];
    bool any = false;
    for (int64_t fc = f0; fc < f1; fc += 64) {
        const int64_t fl = fc + lane;
        any = any || (fl < f1 && a.neighbor[fl] != -1);
    }
    return __ballot(any) != 0ull;
}

// ------------------------------------------------------------------------------------------
// occ_rast_tiled_fwd_kernel: 8x8 tiles, lane = pixel.  The faces that pass the tile test are visited in ascending face
// order by all 64 pixels - the order the naive kernel sees them in, which the pair rule depends on - and the list rules
// are the naive kernel's, on the LDS list (no dependent global loads per entry and candidate).
// (ordered_only_with_pairs: the order-free kernel below was launched as well and takes the meshes without pairs)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void occ_rast_tiled_fwd_kernel(KbufArgs a, int tiles_x, int tiles_y, int ordered_only_with_pairs) {
    extern __shared__ unsigned char kb_smem[];
    const int K = a.K, lane = threadIdx.x;
    const KbufCol c = kbuf_col(kb_smem, K, lane);
    const int tpm = tiles_x * tiles_y;
    const int n = blockIdx.x / tpm;
    if (ordered_only_with_pairs && !mesh_has_pairs(a, n, lane)) return;
    const KbufTile t = kbuf_tile<8>(a, blockIdx.x - n * tpm, tiles_x, lane);
    const float xf = t.xf, yf = t.yf;
    const float sqb = sqrtf(a.blur);
    int qn = 0;
    const int64_t f0 = a.first_idx[n], f1 = f0 + a.num_faces[n];
    for (int64_t fc = f0; fc < f1; fc += 64) {
        const int64_t fl = fc + lane;
        const bool hit = fl < f1 && kbuf_tile_hit(t, kbuf_load(a.face_verts, fl), a.cull, sqb);
        unsigned long long m = __ballot(hit);
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            const int64_t f = fc + b;
            const KbufHit h = kbuf_eval(a, kbuf_load(a.face_verts, f), xf, yf, sqb);  // wave-uniform address
            if (!(t.valid && h.ok)) continue;
            int itop = -1;
            const int64_t nb = a.neighbor ? a.neighbor[f] : -1;
            if (nb != -1) {
                for (int i = 0; i < qn; ++i)
                    if ((int64_t)c.f(i) == nb) { itop = i; break; }
            }
            int slot = -1;
            if (itop != -1) {
                // (the sibling's distance is recomputed: what the naive kernel reads back from its dists slot is this minimum)
                const KbufEdge g = kbuf_closest_edge(kbuf_load(a.face_verts, nb), xf, yf);
                if (kbuf_pair_takes_slot(f, h, nb, g.amin, g.dist)) slot = itop;
            } else if (qn < K) {
                slot = qn++;
            } else {
                // full: the candidate displaces the farthest entry if it comes before it
                const KbufFar far = kbuf_col_farthest(c, K);
                if (kbuf_after(far.z, far.f, h.pz, f)) slot = far.i;
            }
            if (slot >= 0) c.set(slot, h.pz, (int)f);
        }
    }
    if (!t.valid) return;
    kbuf_col_sort(c, qn);
    const KbufOut o = kbuf_out(a, ((long)n * a.H + t.yi) * a.W + t.xi);
    for (int i = 0; i < qn; ++i) kbuf_emit(a, o, i, c.z(i), c.f(i), xf, yf, sqb);
    kbuf_fill(o, qn, K, 1);
}

// ------------------------------------------------------------------------------------------
// occ_rast_quad_fwd_kernel - 4x4 tiles, FOUR faces in flight (sub-pixel meshes).
// Without clipped-face pairs (no neighbour array, or one that is -1 for every face of the mesh - mesh_has_pairs above: the
// case of every mesh the camera is not inside) the K-buffer of a pixel is simply the K smallest (depth, face) among its
// candidates - independent of the order the faces arrive in - so the arrival order may be given up for parallelism:
//   * lane = (pixel of the tile, quarter): the 16 pixels x 4 lanes each; the four lanes of a pixel take the tile's faces
//     in turn and keep a K-list each (same LDS as the 8x8 kernel's 64 lists).  A wave's evaluation pass covers four
//     faces, a face's bbox +- sqrt(blur) covers most of a 4x4 tile (it covered a third of an 8x8 one), and a tile's
//     margin ring holds 2.25x fewer faces: ~9x fewer passes per tile, four times as many tiles to fill the chip with.
//   * a face's nine floats come from the lane that loaded them in the tile test (cross-lane read) instead of a second,
//     dependent memory read per surviving face.
//   * the farthest entry of a full list is cached (depth, face, slot): a candidate that does not displace it costs one
//     compare instead of a scan of the list; the scan runs only after a replacement.
//   * at the end every lane sorts its list, finds the rank of each of its entries in the union of the pixel's four lists
//     (three monotone cursors into the siblings' sorted lists) and writes the entries ranked below K.
// Meshes with pairs keep the 8x8 kernel above: the pair rule asks whether the sibling is in the list AT THE TIME the
// face arrives.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void occ_rast_quad_fwd_kernel(KbufArgs a, int tiles_x, int tiles_y) {
    extern __shared__ unsigned char kb_smem[];
    const int K = a.K, lane = threadIdx.x;
    const KbufCol c = kbuf_col(kb_smem, K, lane);
    const int tpm = tiles_x * tiles_y;
    const int n = blockIdx.x / tpm;
    if (mesh_has_pairs(a, n, lane)) return;  // the ordered 8x8 kernel takes this mesh
    const int pl = lane & 15, sub = lane >> 4;  // pixel of the tile, quarter
    const KbufTile t = kbuf_tile<4>(a, blockIdx.x - n * tpm, tiles_x, pl);
    const float xf = t.xf, yf = t.yf;
    const float sqb = sqrtf(a.blur);
    int qn = 0;
    KbufFar far{0.f, 0, 0};  // farthest entry of the list once it is full
    const int64_t f0 = a.first_idx[n], f1 = f0 + a.num_faces[n];
    for (int64_t fc = f0; fc < f1; fc += 64) {
        const int64_t fl = fc + lane;
        bool hit = false;
        KbufFace v{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (fl < f1) {
            v = kbuf_load(a.face_verts, fl);
            hit = kbuf_tile_hit(t, v, a.cull, sqb);
        }
        unsigned long long m = __ballot(hit);
        while (m) {  // four surviving faces per pass, one per quarter
            int bsel = -1;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (m) {
                    const int b = __builtin_ctzll(m);
                    m &= m - 1;
                    if (sub == q) bsel = b;
                }
            }
            const int src = bsel < 0 ? lane : bsel;
            KbufFace u;
            u.x0 = __shfl(v.x0, src, 64); u.y0 = __shfl(v.y0, src, 64); u.z0 = __shfl(v.z0, src, 64);
            u.x1 = __shfl(v.x1, src, 64); u.y1 = __shfl(v.y1, src, 64); u.z1 = __shfl(v.z1, src, 64);
            u.x2 = __shfl(v.x2, src, 64); u.y2 = __shfl(v.y2, src, 64); u.z2 = __shfl(v.z2, src, 64);
            if (bsel < 0 || !t.valid) continue;
            const KbufHit h = kbuf_eval(a, u, xf, yf, sqb);
            if (!h.ok) continue;
            const int f = (int)(fc + bsel);
            int slot = -1;
            if (qn < K)
                slot = qn++;
            else if (kbuf_after(far.z, far.f, h.pz, f))  // full: the candidate displaces the farthest entry
                slot = far.i;
            if (slot >= 0) {
                c.set(slot, h.pz, f);
                if (qn == K) far = kbuf_col_farthest(c, K);  // the list has just filled up, or its farthest entry was replaced
            }
        }
    }
    kbuf_col_sort(c, qn);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // the pixel's four sorted lists -> one: rank of each own entry in the union (faces are distinct, so no ties)
    const KbufCol c1 = kbuf_col(kb_smem, K, pl + 16 * ((sub + 1) & 3)), c2 = kbuf_col(kb_smem, K, pl + 16 * ((sub + 2) & 3)),
                  c3 = kbuf_col(kb_smem, K, pl + 16 * ((sub + 3) & 3));
    const int n1 = __shfl(qn, c1.lane, 64), n2 = __shfl(qn, c2.lane, 64), n3 = __shfl(qn, c3.lane, 64);
    if (!t.valid) return;
    const int total = min(K, qn + n1 + n2 + n3);
    const KbufOut o = kbuf_out(a, ((long)n * a.H + t.yi) * a.W + t.xi);
    int p1 = 0, p2 = 0, p3 = 0;
    for (int i = 0; i < qn; ++i) {
        const float z = c.z(i);
        const int f = c.f(i);
        while (p1 < n1 && kbuf_after(z, f, c1.z(p1), c1.f(p1))) ++p1;
        while (p2 < n2 && kbuf_after(z, f, c2.z(p2), c2.f(p2))) ++p2;
        while (p3 < n3 && kbuf_after(z, f, c3.z(p3), c3.f(p3))) ++p3;
        const int rank = i + p1 + p2 + p3;
        if (rank >= K) break;
        kbuf_emit(a, o, rank, z, f, xf, yf, sqb);
    }
    kbuf_fill(o, total + sub, K, 4);
}

// dists part of RasterizeMeshesBackward: one thread per (pixel, k), atomicAdd into grad_face_verts.
// Its results are sums of float atomics, so the kernel's machine code is what is held fixed: the body restates kbuf_bary
// and kbuf_closest_edge in place (calling them gave another instruction schedule).  inside: max(p, 0) > 0 under clipb is
// the same predicate as the forward's p > 0 on the pre-clip values; the closest edge keeps a third comparison, and a
// NaN among the distances leaves through the last else.
__global__ __launch_bounds__(256) void occ_rast_naive_bwd_kernel(const float* __restrict__ face_verts,
                                                                 const int64_t* __restrict__ p2f,
                                                                 const float* __restrict__ grad_dists, int N, int H, int W,
                                                                 int K, int persp, int clipb,
                                                                 float* __restrict__ grad_face_verts) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long tot = (long)N * H * W * K;
    if (t >= tot) return;
    const int64_t f = p2f[t];
    if (f < 0) return;
    const long pix = t / K;
    const int rem = (int)(pix % ((long)H * W));
    const int yi = rem / W, xi = rem - yi * W;
    const float yf = k_centre(yi, H), xf = k_centre(xi, W);
    const float* v = face_verts + f * 9;
    const float x0 = v[0], y0 = v[1], z0 = v[2], x1 = v[3], y1 = v[4], z1 = v[5], x2 = v[6], y2 = v[7], z2 = v[8];
    const float ar = k_edge(x2, y2, x0, y0, x1, y1) + kEpsilon;
    float p0 = k_edge(xf, yf, x1, y1, x2, y2) / ar, p1 = k_edge(xf, yf, x2, y2, x0, y0) / ar, p2 = k_edge(xf, yf, x0, y0, x1, y1) / ar;
    if (persp) {
        const float w0 = p0 * z1 * z2, w1 = z0 * p1 * z2, w2 = z0 * z1 * p2;
        const float den = fmaxf(w0 + w1 + w2, kEpsilon);
        p0 = w0 / den; p1 = w1 / den; p2 = w2 / den;
    }
    if (clipb) { p0 = fmaxf(p0, 0.f); p1 = fmaxf(p1, 0.f); p2 = fmaxf(p2, 0.f); }
    const bool inside = p0 > 0.0f && p1 > 0.0f && p2 > 0.0f;
    const float g = (inside ? -1.0f : 1.0f) * grad_dists[t];
    const float e01 = k_seg(xf, yf, x0, y0, x1, y1), e02 = k_seg(xf, yf, x0, y0, x2, y2), e12 = k_seg(xf, yf, x1, y1, x2, y2);
    int ia, ib;
    if (e01 <= e02 && e01 <= e12) { ia = 0; ib = 1; }
    else if (e02 <= e01 && e02 <= e12) { ia = 0; ib = 2; }
    else if (e12 <= e01 && e12 <= e02) { ia = 1; ib = 2; }
    else return;  // a NaN among the distances
    const float ax = v[ia * 3], ay = v[ia * 3 + 1], bx = v[ib * 3], by = v[ib * 3 + 1];
    const float bax = bx - ax, bay = by - ay;
    float tt = (bax * (xf - ax) + bay * (yf - ay)) / (bax * bax + bay * bay + kEpsilon);
    tt = fminf(fmaxf(tt, 0.0f), 1.0f);
    const float dx = (1.0f - tt) * ax + tt * bx - xf, dy = (1.0f - tt) * ay + tt * by - yf;
    float* gf = grad_face_verts + f * 9;
    atomicAdd(gf + ia * 3, g * (1.0f - tt) * 2.0f * dx);
    atomicAdd(gf + ia * 3 + 1, g * (1.0f - tt) * 2.0f * dy);
    atomicAdd(gf + ib * 3, g * tt * 2.0f * dx);
    atomicAdd(gf + ib * 3 + 1, g * tt * 2.0f * dy);
}

// ------------------------------------------------------------------------------------------
// zbuf / bary part of RasterizeMeshesBackward.  Zero on the OcclusionEnv path (the silhouette shader reads
// dists only), built for callers of the rasteriser that shade with barycentrics or depth.  One thread per (pixel, k):
// the forward formulas of A.4 - area-normalised edge functions, perspective correction, lower-bound clip with
// renormalisation, depth - are re-evaluated in FORWARD mode, once per coordinate of the face (nine passes of a
// value + one-derivative pair), and each pass's directional derivative of (bary, zbuf) is contracted with the
// incoming gradients and added into grad_face_verts.  Kinks (max with a floor, clip at 0) take the derivative of the
// active branch, 0 on the floor - the convention of [P3D]'s Barycentric*Backward.
// (The D1 formulas restate kbuf_bary / kbuf_eval on value-derivative pairs; they are not templated over the number type.)
// ------------------------------------------------------------------------------------------
struct D1 {
    float v, d;
};
__device__ __forceinline__ D1 operator+(D1 a, D1 b) { return {a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ D1 operator-(D1 a, D1 b) { return {a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ D1 operator*(D1 a, D1 b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
__device__ __forceinline__ D1 operator/(D1 a, D1 b) { const float q = a.v / b.v; return {q, (a.d - q * b.d) / b.v}; }
__device__ __forceinline__ D1 d1_const(float c) { return {c, 0.f}; }
__device__ __forceinline__ D1 d1_max(D1 a, float floor_) { return a.v > floor_ ? a : D1{floor_, 0.f}; }
__device__ __forceinline__ D1 d1_edge(D1 px, D1 py, D1 ax, D1 ay, D1 bx, D1 by) { return (px - ax) * (by - ay) - (py - ay) * (bx - ax); }

__global__ __launch_bounds__(256) void occ_rast_bwd_zbary_kernel(const float* __restrict__ face_verts,
                                                                 const int64_t* __restrict__ p2f,
                                                                 const float* __restrict__ grad_zbuf,
                                                                 const float* __restrict__ grad_bary, int N, int H, int W,
                                                                 int K, int persp, int clipb,
                                                                 float* __restrict__ grad_face_verts) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long tot = (long)N * H * W * K;
    if (t >= tot) return;
    const int64_t f = p2f[t];
    if (f < 0) return;
    const float gz = grad_zbuf ? grad_zbuf[t] : 0.f;
    const float g0 = grad_bary ? grad_bary[t * 3] : 0.f, g1 = grad_bary ? grad_bary[t * 3 + 1] : 0.f,
                g2 = grad_bary ? grad_bary[t * 3 + 2] : 0.f;
    if (gz == 0.f && g0 == 0.f && g1 == 0.f && g2 == 0.f) return;
    const long pix = t / K;
    const int rem = (int)(pix % ((long)H * W));
    const int yi = rem / W, xi = rem - yi * W;
    const float yf = k_centre(yi, H), xf = k_centre(xi, W);
    const float* v = face_verts + f * 9;
    float* gf = grad_face_verts + f * 9;
    const D1 px = d1_const(xf), py = d1_const(yf);
    for (int j = 0; j < 9; ++j) {  // directional derivative along coordinate j of the face
        D1 c[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) c[i] = D1{v[i], i == j ? 1.f : 0.f};
        const D1 x0 = c[0], y0 = c[1], z0 = c[2], x1 = c[3], y1 = c[4], z1 = c[5], x2 = c[6], y2 = c[7], z2 = c[8];
        const D1 ar = d1_edge(x2, y2, x0, y0, x1, y1) + d1_const(kEpsilon);
        D1 p0 = d1_edge(px, py, x1, y1, x2, y2) / ar, p1 = d1_edge(px, py, x2, y2, x0, y0) / ar, p2 = d1_edge(px, py, x0, y0, x1, y1) / ar;
        if (persp) {
            const D1 w0 = p0 * z1 * z2, w1 = z0 * p1 * z2, w2 = z0 * z1 * p2;
            const D1 den = d1_max(w0 + w1 + w2, kEpsilon);
            p0 = w0 / den; p1 = w1 / den; p2 = w2 / den;
        }
        if (clipb) {
            p0 = d1_max(p0, 0.0f); p1 = d1_max(p1, 0.0f); p2 = d1_max(p2, 0.0f);
            const D1 sm = d1_max(p0 + p1 + p2, kBaryClipMin);
            p0 = p0 / sm; p1 = p1 / sm; p2 = p2 / sm;
        }
        const D1 pz = p0 * z0 + p1 * z1 + p2 * z2;
        const float g = g0 * p0.d + g1 * p1.d + g2 * p2.d + gz * pz.d;
        if (g != 0.f) atomicAdd(gf + j, g);
    }
}
#pragma clang fp contract(fast)
