// occ_kernels.hip -- hand-written CDNA4 (gfx950) kernels for the batched OcclusionEnv step().
//
// What the reference does per environment through PyTorch3D (4 renders, ~200 autograd nodes,
// /root/reference/environment.py:352-396) is done here for N environments in a fixed handful of launches:
//
//   occ_camera_kernel   one thread per env : action -> (el, az) -> C -> look_at R,T, carrying
//                       forward-mode tangents d/d(el,az) of R and T (environment.py:356-368)
//   occ_setup_kernel    one block per (env, object): gather pool verts, world->view->NDC
//                       (MeshRasterizer.transform), z-clip (clip_faces), cull, per-face record
//                       with NDC verts + tangents + invariants, ORDERED compaction (face order is
//                       PyTorch3D's tie-break order), packed tile bbox, object tile rect
//   occ_order_kernel    work items (env, object, 8x8-pixel tile) in cost order, heaviest first per XCD queue
//                       (occ_scan_kernel: plain rect order when the workspace has no order buffer)
//   occ_raster2_kernel  persistent wave64 per work item: lane = (face, pixel) PAIR over the pixels of every face's
//                       pixel bbox inside the tile (on-the-fly binning by ballot over chunk boxes and pixel bboxes,
//                       records staged in LDS by cooperative 16-B loads): soft silhouette (K nearest-z sigmoid
//                       product) + hard nearest face of ONE object in one sweep, per-pixel state in LDS, candidate
//                       K-buffer = wave-compacted log streamed to HBM/L2 in full lines, exact top-K-by-z selection
//                       (cooperative LDS-histogram radix select) when a pixel has more than K candidates
//   occ_combine_kernel  one thread per pixel: occlusion image of the three silhouettes, loss and
//                       d loss/d(el,az) partials, nearest-object pick + flat shading, outputs
//   occ_reduce_kernel   one wave per env: fixed-order sum of the per-block partials
//   occ_finish_kernel   reward bookkeeping + action Jacobian (environment.py:381-392,356-361)
//
// The gradient is carried in FORWARD mode (two tangent directions, el and az) through the very
// same sweep that renders: d alpha/d theta = -(A/sigma) * sum_k p_k * d dist_k/d theta needs no
// second pass over the K-buffer, no atomics into grad_face_verts and no saved fragments.  It
// equals what autograd + _C.rasterize_meshes_backward produce.
//
//   occ_enc16_*_kernel  the bf16 inference mode of the separable encoder (occ_encoder_bf16.hpp): bf16 storage, MFMA contractions
//   occ_enc_*_kernel    the frozen encoder of the PPO features (occ_encoder.hpp): fused separable layer, dense 3x3
//                       conv, last down fused with the average pool
//   occ_dec_up_kernel   the segmentation decoder of the same network (occ_decoder.hpp): transposed conv + skip add per
//                       launch, classifier and sigmoid fused into the last; occ_seg_metrics_kernel: accuracy / IoU counts
//                       The three conv forwards (occ_enc_sep_kernel, occ_enc_dense_kernel, occ_dec_up_kernel) exist once:
//                       instantiated with TRAIN they also store what a backward reads, and are the training forwards
//   occ_dec_bwd_*       training of that decoder with the encoder frozen (occ_decoder_bwd.hpp): the up kernel with TRAIN,
//                       then activation step, input gradient and weight gradient per level, fixed-order sums
//                       The fixed-order f64 reductions of every training backward (block partials, wave-final sum, pixel-
//                       lane fold of a K-split weight gradient) exist once, as device helpers at the top of that file
//   occ_enc_bwd_*       training of the encoder (occ_encoder_bwd.hpp): one training forward walk and one backward walk for
//   occ_sep_bwd_*       the dense and the separable encoder, per layer the activation step, weight and input gradients;
//                       the separable layer's own backward kernels (occ_sepenc_bwd.hpp); the joint step with the decoder
//                       (occ_fullnet_bwd.hpp), one for both encoder forms, has host code only
//   occ_bn_*            batch-statistics BatchNorm for that joint step (occ_bn_train.hpp): per layer the statistics and y
//                       after the conv kernel, and a sums pass, a per-channel kernel and an act pass in place of the
//                       activation step
//   occ_seg_criterion_* the pretrainer's criterion on that map (occ_criterion.hpp): Dice / BCE sums and the counts in one
//                       read, fixed-order f64 sums, and the gradient with respect to the prediction
//   occ_adamw_kernel    the optimizer of that joint step (occ_adamw.hpp): AdamW in packed order on both parts and the grad
//                       head, the BatchNorm chain rule and the fold of the next forward's packed buffers, one launch
//   occ_augment_*       the pretrainer's input pipeline on a device-resident dataset (occ_augment.hpp): gather by frame
//                       index, torchvision's colour jitter with PIL's roundings, flip, /255 and Normalize: a luminance-
//                       sum pass for contrast's mean and an output pass
//   occ_datapack_*      rendered frames into that dataset's store (occ_datapack.hpp): img_as_ubyte, depth * 51 and the
//                       occlusion label per pixel, then PIL's convert("1") error diffusion in place, one wave per frame
//   occ_jpeg_*          the JPEG round trip in place in that store (occ_jpeg.hpp): libjpeg's 4:2:0 encode and decode without
//                       the entropy coding, a pass per 32 x 32 tile through LDS and the chroma upsampling pass
//   occ_episode_kernel  the episode bookkeeping of the batched controller evaluation (occ_episode.hpp): the controller's
//                       action update, traces, finished / cap test and the freeze of the envs that are through, one launch
//
// No MFMA: the path is rasterisation.  fp32 throughout.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "occ_constants.h"
#include "occlusionenv_amd.h"

namespace occ {

#include "occ_common.hpp"
#include "occ_camera.hpp"
#include "occ_setup.hpp"
#include "occ_eval.hpp"
#include "occ_raster2.hpp"
#include "occ_combine.hpp"
#include "occ_blend.hpp"
#include "occ_reset.hpp"
#include "occ_oplevel.hpp"
#include "occ_ppo.hpp"
#include "occ_encoder.hpp"
#include "occ_encoder_bf16.hpp"
#include "occ_decoder.hpp"
#include "occ_decoder_bwd.hpp"
#include "occ_encoder_bwd.hpp"
#include "occ_sepenc_bwd.hpp"
#include "occ_fullnet_bwd.hpp"
#include "occ_bn_train.hpp"
#include "occ_criterion.hpp"
#include "occ_adamw.hpp"
#include "occ_augment.hpp"
#include "occ_datapack.hpp"
#include "occ_resize.hpp"
#include "occ_jpeg.hpp"
#include "occ_rollout.hpp"
#include "occ_episode.hpp"

}  // namespace occ

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
using namespace occ;

extern "C" int occ_abi_version(void) { return OCC_ABI_VERSION; }

// ---- measurement hooks ---------------------------------------------------------------------
namespace {
constexpr int kProfMax = 4096;
bool g_prof_on = false;
int g_prof_n = 0;
hipEvent_t g_prof_ev[2 * kProfMax];
int g_prof_nenv[kProfMax];
bool g_prof_created = false;
}  // namespace

extern "C" int occ_profile_enable(int on) {
    if (on && !g_prof_created) {
        for (int i = 0; i < 2 * kProfMax; ++i)
            if (hipEventCreate(&g_prof_ev[i]) != hipSuccess) return OCC_ERR_LAUNCH;
        g_prof_created = true;
    }
    g_prof_on = on != 0;
    g_prof_n = 0;
    return OCC_OK;
}

extern "C" int occ_profile_read(double* ms_sum, int* launches) {
    if (!ms_sum || !launches) return OCC_ERR_ARG;
    double tot = 0.0;
    int big = 0, cnt = 0;
    for (int i = 0; i < g_prof_n; ++i) big = g_prof_nenv[i] > big ? g_prof_nenv[i] : big;
    for (int i = 0; i < g_prof_n; ++i) {
        float ms = 0.f;
        if (hipEventSynchronize(g_prof_ev[2 * i + 1]) != hipSuccess) return OCC_ERR_LAUNCH;
        if (hipEventElapsedTime(&ms, g_prof_ev[2 * i], g_prof_ev[2 * i + 1]) != hipSuccess) return OCC_ERR_LAUNCH;
        if (g_prof_nenv[i] != big) continue;  // full-batch launches only (auto-resets render tiny batches)
        tot += ms;
        cnt += 1;
    }
    *ms_sum = tot;
    *launches = cnt;
    g_prof_n = 0;
    return OCC_OK;
}

#ifdef OCC_DBG_STATS
extern "C" int occ_debug_stats(unsigned long long* out16) {
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(occ::g_dbg_stats), 32 * sizeof(unsigned long long)) != hipSuccess) return 2;  // (32 slots)
    unsigned long long z[32] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(occ::g_dbg_stats), z, sizeof(z)) == hipSuccess ? 0 : 2;
}
#endif

#ifdef OCC_DBG_TIME
extern "C" int occ_debug_time(unsigned long long* out112) {
    if (hipMemcpyFromSymbol(out112, HIP_SYMBOL(occ::g_dbg_time), 112 * sizeof(unsigned long long)) != hipSuccess) return 2;
    unsigned long long z[112] = {0};
    z[16] = ~0ull;
    for (int i = 96; i < 104; ++i) z[i] = ~0ull;
    return hipMemcpyToSymbol(HIP_SYMBOL(occ::g_dbg_time), z, sizeof(z)) == hipSuccess ? 0 : 2;
}
#endif

#ifdef OCC_DBG_ENDS
extern "C" int occ_debug_ends(unsigned long long* out16384) {
    return hipMemcpyFromSymbol(out16384, HIP_SYMBOL(occ::g_dbg_ends), 4 * 4096 * sizeof(unsigned long long)) == hipSuccess ? 0 : 2;
}
#endif

#ifdef OCC_DBG_BOUNDS
extern "C" int occ_debug_fault(int* out8) {
    return hipMemcpyFromSymbol(out8, HIP_SYMBOL(occ::g_dbg_fault), 8 * sizeof(int)) == hipSuccess ? 0 : 2;
}
#endif

extern "C" int occ_device_cu_count(void) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1;
    return prop.multiProcessorCount;
}

static bool scene_ok(const OccScene* s) {
    return s && s->pool_verts && s->pool_faces && s->mesh_vert_off && s->mesh_face_off && s->scene_mesh &&
           s->scene_offset && s->n_env > 0 && s->img >= OCC_TILE && s->img % OCC_TILE == 0 && s->img <= 2048 &&
           s->rec_cap > 0 && s->shader >= OCC_SHADER_FLAT && s->shader <= OCC_SHADER_SOFT_PHONG &&
           (s->shader == OCC_SHADER_FLAT || s->pool_vnormals);
}

extern "C" int occ_workspace_query(const OccScene* scene, int n_slots, OccWorkspaceSizes* out) {
    if (!scene || !out || scene->n_env <= 0 || scene->img < OCC_TILE || scene->img % OCC_TILE || scene->rec_cap <= 0)
        return OCC_ERR_ARG;
    if (n_slots <= 0) {
        const int cus = occ_device_cu_count();
        n_slots = (cus > 0 ? cus : 256) * 8;
    }
    const size_t N = (size_t)scene->n_env, cap = (size_t)scene->rec_cap;
    out->rec_bytes = N * 3 * cap * OCC_REC_STRIDE * sizeof(float);
    out->rec_bbox_bytes = N * 3 * cap * 4 * sizeof(uint32_t);
    out->scan_bytes = N * 3 * cap * 4 * sizeof(uint32_t);
    out->rec_cbox_bytes = N * 3 * ((cap + 63) / 64) * 4 * sizeof(uint32_t);
    out->nrec_bytes = N * 3 * sizeof(int32_t);
    out->objrect_bytes = N * 3 * 4 * sizeof(int32_t);
    out->queue_bytes = 8 * kQueueStride * sizeof(uint32_t);  // eight queue heads, one 128-B line each
    out->lists_bytes = (size_t)n_slots * OCC_LOG_BYTES;  // per-wave K-buffer: the compacted candidate log
    const size_t S2 = (size_t)scene->img * scene->img;
    out->partials_bytes = N * ((S2 + 255) / 256) * 4 * sizeof(float);
    out->offsets_bytes = (size_t)(8 * xcd_slots(scene->n_env) + 1) * sizeof(int32_t);
    out->obj_alpha_bytes = N * 3 * S2 * sizeof(float);
    out->obj_grad_bytes = N * 3 * S2 * 2 * sizeof(float);
    out->obj_hz_bytes = N * 3 * S2 * sizeof(float);
    out->obj_hrec_bytes = N * 3 * S2 * sizeof(int32_t);
    out->status_bytes = N * sizeof(int32_t);
    out->n_slots = n_slots;
    out->rec_off_bytes = (N * 3 + 1) * sizeof(int64_t);
    {   // work-item order: header + per-object class offsets + per-tile (rank, class) + the item list
        const size_t T = (size_t)(scene->img / 8) * (scene->img / 8);
        out->order_bytes = (ord_items_word(scene->n_env, scene->img) + N * 3 * T * 2) * sizeof(uint32_t);
    }
    return OCC_OK;
}

extern "C" int occ_record_sizes(int64_t rec_total, int n_env, OccWorkspaceSizes* io) {
    if (!io || rec_total <= 0 || n_env <= 0 || (rec_total & 63)) return OCC_ERR_ARG;
    const size_t T = (size_t)rec_total;
    io->rec_bytes = T * OCC_REC_STRIDE * sizeof(float);
    io->rec_bbox_bytes = T * 4 * sizeof(uint32_t);
    io->scan_bytes = T * 4 * sizeof(uint32_t);
    io->rec_cbox_bytes = (T / 64) * 4 * sizeof(uint32_t);
    io->rec_off_bytes = ((size_t)n_env * 3 + 1) * sizeof(int64_t);
    return OCC_OK;
}

extern "C" int occ_camera(int mode, const float* action, float* el, float* az, const float* radius, float* cam,
                          float* cam_pos_out, int n_env, void* stream) {
    if (!cam || n_env <= 0) return OCC_ERR_ARG;
    if (mode == OCC_CAM_STEP && (!action || !el || !az || !radius)) return OCC_ERR_ARG;
    if (mode == OCC_CAM_LOOKAT && (!el || !az || !radius)) return OCC_ERR_ARG;
    if (mode == OCC_CAM_POSITION && !action) return OCC_ERR_ARG;
    if (mode < 0 || mode > 2) return OCC_ERR_ARG;
    hipLaunchKernelGGL(occ_camera_kernel, dim3((n_env + 63) / 64), dim3(64), 0, (hipStream_t)stream, mode, action, el, az,
                       radius, cam, cam_pos_out, n_env);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

// OCC_DEBUG_SYNC=1 in the environment: every launch of occ_render is announced on stderr and waited for, so that a
// faulting kernel is the last one named (diagnostics only; serialises the stream).  The only getenv of the library.
static bool dbg_sync_on() {
    static int on = -1;
    if (on < 0) {
        const char* e = getenv("OCC_DEBUG_SYNC");
        on = (e && e[0] && e[0] != '0') ? 1 : 0;
    }
    return on == 1;
}
#define OCC_DBG_SYNC(name)                                                          \
    do {                                                                            \
        if (dbg_sync_on()) {                                                        \
            fprintf(stderr, "[occ] %s launched (n_env %d) ...", name, scene->n_env); \
            fflush(stderr);                                                         \
            const hipError_t e_ = hipStreamSynchronize(st);                         \
            fprintf(stderr, " %s\n", e_ == hipSuccess ? "ok" : hipGetErrorString(e_)); \
            fflush(stderr);                                                         \
        }                                                                           \
    } while (0)

extern "C" int occ_render(const OccScene* scene, const float* cam, const OccWorkspace* ws, const OccRenderOut* out,
                          int flags, int faces_per_pixel, void* stream) {
    return occ_step(scene, nullptr, const_cast<float*>(cam), ws, out, flags, faces_per_pixel, stream);
}

extern "C" int occ_step(const OccScene* scene, const OccCameraArgs* camera, float* cam, const OccWorkspace* ws,
                        const OccRenderOut* out, int flags, int faces_per_pixel, void* stream) {
    if (!scene_ok(scene) || !cam || !ws || !out) return OCC_ERR_ARG;
    OccCameraArgs ca{};
    if (camera) {
        ca = *camera;
        if (ca.n <= 0 || ca.n > scene->n_env || ca.mode < 0 || ca.mode > 2) return OCC_ERR_ARG;
        if (ca.mode == OCC_CAM_STEP && (!ca.action || !ca.el || !ca.az || !ca.radius)) return OCC_ERR_ARG;
        if (ca.mode == OCC_CAM_LOOKAT && (!ca.el || !ca.az || !ca.radius)) return OCC_ERR_ARG;
        if (ca.mode == OCC_CAM_POSITION && !ca.action) return OCC_ERR_ARG;
    }
    if ((out->rect_prev != nullptr) != (out->rect_next != nullptr) || (out->rect_prev && out->rect_prev == out->rect_next)) return OCC_ERR_ARG;
    if ((out->arect_prev != nullptr) != (out->arect_next != nullptr) || (out->arect_prev && out->arect_prev == out->arect_next)) return OCC_ERR_ARG;
    FinishArgs fin{};
    if (out->finish) {
        const OccStepFinish& f = *out->finish;
        if (!(flags & OCC_RENDER_SOFT) || !out->loss || !f.full_reward || !f.object_mass || !f.reward || !f.done || f.n_step <= 0 ||
            f.n_step > scene->n_env || (f.grad_action && (flags & OCC_RENDER_GRAD) && !out->grad_elaz))
            return OCC_ERR_ARG;
        fin = FinishArgs{f.full_reward, f.object_mass, f.reward, f.done, f.grad_action, cam, f.n_step};
    }
    if (!ws->rec || !ws->rec_bbox || !ws->nrec || !ws->objrect || !ws->queue || !ws->lists || !ws->partials ||
        !ws->status || !ws->rec_cbox || !ws->scan || !ws->offsets || !ws->obj_alpha || !ws->obj_grad || !ws->obj_hz || !ws->obj_hrec ||
        ws->n_slots <= 0)
        return OCC_ERR_ARG;
    const bool soft = flags & OCC_RENDER_SOFT, hard = flags & OCC_RENDER_HARD, grad = flags & OCC_RENDER_GRAD;
    if (!soft && !hard) return OCC_ERR_ARG;
    if (grad && !soft) return OCC_ERR_ARG;
    if (hard && !out->obs) return OCC_ERR_ARG;
    if (soft && (faces_per_pixel <= 0 || faces_per_pixel > OCC_MAX_K)) return OCC_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int N = scene->n_env;
    const OccWorkspace& wsv = *ws;
    if (ws->rec_off && (ws->rec_total <= 0 || (ws->rec_total & 63))) return OCC_ERR_ARG;
    static_assert(kOrdBlk <= 1024, "occ_recoff_kernel zeroes the order header with one block");
    // prologue: zero the queue heads and the order header, lay out the variable record spans
    hipLaunchKernelGGL(occ_recoff_kernel, dim3(1 + (ca.n + 1023) / 1024), dim3(1024), 0, st, *scene, (long long*)ws->rec_off,
                       (long long)ws->rec_total, ws->status, ws->queue, wsv.order, ca, cam);
    OCC_DBG_SYNC("recoff");
    // world-space vertices of an object staged in LDS when they fit (OccScene.max_mesh_verts; 0 = gather from global memory)
    int vcap = scene->max_mesh_verts > 0 ? ((scene->max_mesh_verts + 63) & ~63) : 0;
    if (vcap > kSetupVcapMax) vcap = kSetupVcapMax;
    {   // the staged vertices come on top of the kernel's static LDS: never ask for more than the device gives a block
        static int lds_room = -1;  // bytes of dynamic LDS occ_setup_kernel can have (queried once)
        if (lds_room < 0) {
            int dev = 0;
            hipDeviceProp_t prop;
            hipFuncAttributes fa;
            lds_room = 0;
            if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess &&
                hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&occ_setup_kernel<true, kSetupTB>)) == hipSuccess &&
                prop.sharedMemPerBlock > fa.sharedSizeBytes)
                lds_room = (int)(prop.sharedMemPerBlock - fa.sharedSizeBytes);
        }
        const int fit = (lds_room / 12) & ~63;
        if (vcap > fit) vcap = fit;  // (0: gather from global memory, same results)
    }
    const size_t vlds = (size_t)vcap * 3 * sizeof(float);
    if (grad)
        hipLaunchKernelGGL((occ_setup_kernel<true, kSetupTB>), dim3(N * 3), dim3(kSetupTB), vlds, st, *scene, cam, wsv, vcap);
    else
        hipLaunchKernelGGL((occ_setup_kernel<false, kSetupTB>), dim3(N * 3), dim3(kSetupTB), vlds, st, *scene, cam, wsv, vcap);
    OCC_DBG_SYNC("setup");
    const bool may_sort = scene->rec_cap >= kSortMin;  // dense objects only: front-to-back scan order (LDS sort buffer: 8192 keys = 64 KiB)
    const int sort_cap = kSortCap;
    const size_t sort_lds = may_sort ? (size_t)sort_cap * sizeof(unsigned long long) : 0;
    if (may_sort && !wsv.order) {
        hipLaunchKernelGGL(occ_sort_kernel, dim3(N * 3), dim3(256), sort_lds, st, *scene, *ws, sort_cap);
        OCC_DBG_SYNC("sort");
    }
    if (hipGetLastError() != hipSuccess) return OCC_ERR_LAUNCH;
    RasterParams P;
    P.sc = *scene;
    P.ws = wsv;
    P.out = *out;
    P.cam = cam;
    P.K = faces_per_pixel;
    P.ntx = scene->img / OCC_TILE;
    {   // small launches: split every tile into row groups until the expected work items fill about half the grid
        // (an object's rect covers a few per cent of the image: 0.04 x tiles is the typical count at radius 4)
        const double est = (double)N * 3.0 * P.ntx * P.ntx * 0.04;
        int sl = 0;
        while (sl < 3 && est * (double)(2 << sl) <= (double)ws->n_slots) ++sl;
        P.split_log2 = sl;
    }
    if (wsv.order) {
        // (One launch for sort + order - occ_sort_order_kernel - was measured in round 5: 18.9 us against 5 + 5 for the two:
        // the sort's 64 KB of LDS lets two blocks share a CU, and the order pass then runs at that occupancy.  It is used
        // where no object can be dense - nothing to sort, no LDS.)
        if (may_sort) {
            hipLaunchKernelGGL(occ_sort_kernel, dim3(N * 3), dim3(256), sort_lds, st, *scene, *ws, sort_cap);
            OCC_DBG_SYNC("sort");
            hipLaunchKernelGGL(occ_order_kernel, dim3(N * 3), dim3(64), 0, st, ws->objrect, ws->nrec, wsv.order, N, scene->img);
        } else {
            hipLaunchKernelGGL(occ_sort_order_kernel, dim3(N * 3), dim3(64), 0, st, *scene, wsv, 0);
        }
        OCC_DBG_SYNC("order");
    } else {
        hipLaunchKernelGGL(occ_scan_kernel, dim3(1), dim3(1024), 0, st, ws->objrect, ws->nrec, ws->offsets, N, 1);
        OCC_DBG_SYNC("scan");
    }
    if (hipGetLastError() != hipSuccess) return OCC_ERR_LAUNCH;
    const dim3 grid(ws->n_slots), block(64);
    const bool prof = g_prof_on && g_prof_n < kProfMax;
    if (prof) (void)hipEventRecord(g_prof_ev[2 * g_prof_n], st);
    const int bpe = (scene->img * scene->img + 255) / 256;
    // thread blocks per env of the combine kernel: enough of them for a small launch, few enough that a big one does
    // not start tens of thousands of blocks that find nothing to do (occ_combine_kernel)
    int cG = bpe / 16 > (4096 + N - 1) / N ? bpe / 16 : (4096 + N - 1) / N;
    if (cG > bpe) cG = bpe;
    if (cG < 1) cG = 1;
    const dim3 cgrid(N * cG), cblock(256);
#define OCC_LAUNCH(SOFT_, HARD_, GRAD_)                                                             \
    do {                                                                                            \
        hipLaunchKernelGGL((occ_raster2_kernel<SOFT_, HARD_, GRAD_>), grid, block, 0, st, P);       \
        OCC_DBG_SYNC("raster");                                                                     \
        if (prof) {                                                                                 \
            (void)hipEventRecord(g_prof_ev[2 * g_prof_n + 1], st);                                  \
            g_prof_nenv[g_prof_n] = N;                                                              \
            g_prof_n += 1;                                                                          \
        }                                                                                           \
        hipLaunchKernelGGL((occ_combine_kernel<SOFT_, HARD_, GRAD_>), cgrid, cblock, 0, st, P, bpe, cG); \
        OCC_DBG_SYNC("combine");                                                                    \
    } while (0)
    if (soft && hard && grad)
        OCC_LAUNCH(true, true, true);
    else if (soft && hard)
        OCC_LAUNCH(true, true, false);
    else if (soft && grad)
        OCC_LAUNCH(true, false, true);
    else if (soft)
        OCC_LAUNCH(true, false, false);
    else
        OCC_LAUNCH(false, true, false);
#undef OCC_LAUNCH
    if (hipGetLastError() != hipSuccess) return OCC_ERR_LAUNCH;
    if (soft && (out->loss || out->grad_elaz)) {
        hipLaunchKernelGGL(occ_reduce_kernel, dim3(N), dim3(64), 0, st, ws->partials, bpe, out->loss,
                           grad ? out->grad_elaz : nullptr, scene->skip, fin, wsv, scene->img);
        if (hipGetLastError() != hipSuccess) return OCC_ERR_LAUNCH;
    }
    return OCC_OK;
}

// the forward entry points' argument check; fills the kernels' argument block
static bool kbuf_args(KbufArgs* a, const float* face_verts, const int64_t* mesh_to_face_first_idx,
                      const int64_t* num_faces_per_mesh, const int64_t* clipped_faces_neighbor_idx, int n_meshes, int H, int W,
                      float blur_radius, int faces_per_pixel, int perspective_correct, int clip_barycentric_coords,
                      int cull_backfaces, int64_t* pix_to_face, float* zbuf, float* bary, float* dists) {
    if (!face_verts || !mesh_to_face_first_idx || !num_faces_per_mesh || !pix_to_face || !zbuf || !bary || !dists ||
        n_meshes <= 0 || H <= 0 || W <= 0 || faces_per_pixel <= 0 || blur_radius < 0.f)
        return false;
    *a = KbufArgs{face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, n_meshes, H, W,
                  faces_per_pixel, blur_radius, perspective_correct, clip_barycentric_coords, cull_backfaces, pix_to_face,
                  zbuf, bary, dists};
    return true;
}

static int kbuf_launch_naive(const KbufArgs& a, hipStream_t st) {
    const long npix = (long)a.N * a.H * a.W;
    hipLaunchKernelGGL(occ_rast_naive_fwd_kernel, dim3((unsigned)((npix + 63) / 64)), dim3(64), 0, st, a);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_rasterize_meshes_naive(const float* face_verts, const int64_t* mesh_to_face_first_idx,
                                          const int64_t* num_faces_per_mesh, const int64_t* clipped_faces_neighbor_idx,
                                          int n_meshes, int H, int W, float blur_radius, int faces_per_pixel,
                                          int perspective_correct, int clip_barycentric_coords, int cull_backfaces,
                                          int64_t* pix_to_face, float* zbuf, float* bary, float* dists, void* stream) {
    KbufArgs a;
    if (!kbuf_args(&a, face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, n_meshes, H, W,
                   blur_radius, faces_per_pixel, perspective_correct, clip_barycentric_coords, cull_backfaces, pix_to_face,
                   zbuf, bary, dists))
        return OCC_ERR_ARG;
    return kbuf_launch_naive(a, (hipStream_t)stream);
}

extern "C" int occ_rasterize_meshes_tiled(const float* face_verts, const int64_t* mesh_to_face_first_idx,
                                          const int64_t* num_faces_per_mesh, const int64_t* clipped_faces_neighbor_idx,
                                          int n_meshes, int H, int W, float blur_radius, int faces_per_pixel,
                                          int perspective_correct, int clip_barycentric_coords, int cull_backfaces,
                                          int64_t* pix_to_face, float* zbuf, float* bary, float* dists, void* stream) {
    KbufArgs a;
    if (!kbuf_args(&a, face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, n_meshes, H, W,
                   blur_radius, faces_per_pixel, perspective_correct, clip_barycentric_coords, cull_backfaces, pix_to_face,
                   zbuf, bary, dists))
        return OCC_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)64 * faces_per_pixel * 8;
    if (lds > 64 * 1024)  // beyond the (depth, face) lists the kernels keep in LDS (K > 128): same results from the naive kernel
        return kbuf_launch_naive(a, st);
    // meshes without clipped-face pairs (no neighbour array, or all -1 for the mesh): the K-buffer does not depend on the
    // arrival order - 4x4 tiles, four faces in flight; meshes with pairs: 8x8 tiles, faces in order.  With an array both
    // kernels are launched and every wave finds out first which of the two its mesh belongs to.
    const int qx = (W + 3) / 4, qy = (H + 3) / 4;
    hipLaunchKernelGGL(occ_rast_quad_fwd_kernel, dim3((unsigned)(n_meshes * qx * qy)), dim3(64), lds, st, a, qx, qy);
    if (clipped_faces_neighbor_idx) {
        const int tiles_x = (W + 7) / 8, tiles_y = (H + 7) / 8;
        hipLaunchKernelGGL(occ_rast_tiled_fwd_kernel, dim3((unsigned)(n_meshes * tiles_x * tiles_y)), dim3(64), lds, st, a,
                           tiles_x, tiles_y, 1);
    }
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_rasterize_meshes_backward(const float* face_verts, const int64_t* pix_to_face, const float* grad_zbuf,
                                             const float* grad_bary, const float* grad_dists, int64_t n_faces, int n_meshes,
                                             int H, int W, int faces_per_pixel, int perspective_correct,
                                             int clip_barycentric_coords, float* grad_face_verts, void* stream) {
    if (!face_verts || !pix_to_face || !grad_face_verts || n_faces <= 0 || n_meshes <= 0 || H <= 0 || W <= 0 ||
        faces_per_pixel <= 0)
        return OCC_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(grad_face_verts, 0, (size_t)n_faces * 9 * sizeof(float), st) != hipSuccess) return OCC_ERR_LAUNCH;
    const long tot = (long)n_meshes * H * W * faces_per_pixel;
    const dim3 grid((unsigned)((tot + 255) / 256)), block(256);
    if (grad_dists)
        hipLaunchKernelGGL(occ_rast_naive_bwd_kernel, grid, block, 0, st, face_verts, pix_to_face, grad_dists, n_meshes, H, W,
                           faces_per_pixel, perspective_correct, clip_barycentric_coords, grad_face_verts);
    if (grad_zbuf || grad_bary)
        hipLaunchKernelGGL(occ_rast_bwd_zbary_kernel, grid, block, 0, st, face_verts, pix_to_face, grad_zbuf, grad_bary,
                           n_meshes, H, W, faces_per_pixel, perspective_correct, clip_barycentric_coords, grad_face_verts);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

// the dists gradient alone: the call above with a required grad_dists and no other gradient
extern "C" int occ_rasterize_meshes_backward_dists(const float* face_verts, const int64_t* pix_to_face,
                                                   const float* grad_dists, int64_t n_faces, int n_meshes, int H, int W,
                                                   int faces_per_pixel, int perspective_correct,
                                                   int clip_barycentric_coords, float* grad_face_verts, void* stream) {
    if (!grad_dists) return OCC_ERR_ARG;
    return occ_rasterize_meshes_backward(face_verts, pix_to_face, nullptr, nullptr, grad_dists, n_faces, n_meshes, H, W,
                                         faces_per_pixel, perspective_correct, clip_barycentric_coords, grad_face_verts, stream);
}

extern "C" int occ_sigmoid_alpha_blend_fwd(const float* dists, const int64_t* pix_to_face, int64_t n_pix, int faces_per_pixel,
                                           float sigma, float* images, void* stream) {
    if (!dists || !pix_to_face || !images || n_pix <= 0 || faces_per_pixel <= 0 || !(sigma > 0.f)) return OCC_ERR_ARG;
    hipLaunchKernelGGL(occ_blend_fwd_kernel, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dists,
                       pix_to_face, (long)n_pix, faces_per_pixel, sigma, images);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_sigmoid_alpha_blend_bwd(const float* dists, const int64_t* pix_to_face, const float* grad_images,
                                           int64_t n_pix, int faces_per_pixel, float sigma, float* grad_dists, void* stream) {
    if (!dists || !pix_to_face || !grad_images || !grad_dists || n_pix <= 0 || faces_per_pixel <= 0 || !(sigma > 0.f))
        return OCC_ERR_ARG;
    hipLaunchKernelGGL(occ_blend_bwd_kernel, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dists,
                       pix_to_face, grad_images, (long)n_pix, faces_per_pixel, sigma, grad_dists);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_ppo_max_blocks(void) { return OCC_PPO_MAX_BLOCKS; }

extern "C" int occ_ppo_update(const float* feats, const float* actions, const float* old_logprob, const float* returns,
                              int64_t M, float action_var, float eps_clip, float lr_actor, float lr_critic, float beta1,
                              float beta2, float adam_eps, const OccPpoState* state, int n_epochs, float* losses,
                              float* scratch, uint32_t* counter, void* stream) {
    static_assert(kPpoFeat == OCC_PPO_FEATURES && kPpoParams == OCC_PPO_PARAMS, "occ_ppo.hpp and the header disagree");
    if (!feats || !actions || !old_logprob || !returns || M <= 0 || !(action_var > 0.f) || !state || n_epochs < 0 || !losses ||
        !scratch || !counter || !state->w_a || !state->b_a || !state->w_v || !state->b_v || !state->adam_m || !state->adam_v ||
        !state->adam_step)
        return OCC_ERR_ARG;
    PpoArgs A;
    A.feats = feats; A.actions = actions; A.old_lp = old_logprob; A.returns = returns; A.M = (long long)M;
    A.inv_var = 1.0f / action_var;
    // MultivariateNormal(mean, var I) in two dimensions: log-density constant and entropy (PPO.py:62-104)
    const float log2pi = 1.8378770664093453f, logdet = 2.0f * logf(action_var);
    A.lp_const = -0.5f * (2.0f * log2pi + logdet);
    A.ent_term = 0.01f * 0.5f * (2.0f * (1.0f + log2pi) + logdet);
    A.eps_clip = eps_clip;
    A.lr_actor = lr_actor; A.lr_critic = lr_critic; A.beta1 = beta1; A.beta2 = beta2; A.adam_eps = adam_eps;
    A.w_a = state->w_a; A.b_a = state->b_a; A.w_v = state->w_v; A.b_v = state->b_v;
    A.m = state->adam_m; A.v = state->adam_v; A.step = state->adam_step;
    A.partials = scratch; A.counter = counter;
    // A wave takes ~12 samples of a 10^4-sample rollout: 64 blocks of 16 waves, few rows for the last block's sum.  The
    // replicated learner of an 8-GPU node sees 8 x the samples: from 2^16 samples on, twice the blocks (measured, us per
    // epoch at 12 800 / 51 200 / 102 400 samples: 64 blocks 40 / 67 / 106, 128 blocks 49 / 69 / 88, 256 blocks 50 / 103 / 115:
    // more rows cost the last block more than the extra waves save until the sample loop dominates).
    const long long cap = M >= 65536 ? OCC_PPO_MAX_BLOCKS : (OCC_PPO_MAX_BLOCKS < 64 ? OCC_PPO_MAX_BLOCKS : 64);
    const long long want = (M + 16 * 8 - 1) / (16 * 8);
    const unsigned blocks = (unsigned)(want < 1 ? 1 : (want > cap ? cap : want));
    for (int e = 0; e < n_epochs; ++e) {
        A.losses = losses + 2 * e;
        hipLaunchKernelGGL(occ_ppo_epoch_kernel, dim3(blocks), dim3(kPpoThreads), 0, (hipStream_t)stream, A);
    }
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_pool8(const float* obs, int64_t n, int img, float* feats, void* stream) {
    if (!obs || !feats || n <= 0 || img < 8 || img % 8) return OCC_ERR_ARG;
    const dim3 grid((unsigned)(n * 4 * 8));
    if ((img / 8) % 4 == 0)
        hipLaunchKernelGGL(occ_pool8_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, obs, feats, img);
    else
        hipLaunchKernelGGL(occ_pool8_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, obs, feats, img);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_step_flags(const uint8_t* done, const float* loss_all, const int32_t* status, int n_env, int n_reserve,
                              int32_t* flags, void* stream) {
    if (!done || !status || !flags || n_env <= 0 || n_reserve < 0 || (n_reserve > 0 && !loss_all)) return OCC_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int tot = n_env + n_reserve;
    hipLaunchKernelGGL(occ_flags_kernel, dim3((tot + 255) / 256), dim3(256), 0, st, done, loss_all, status, n_env, n_reserve,
                       flags);
    hipLaunchKernelGGL(occ_status_any_kernel, dim3((tot + 255) / 256), dim3(256), 0, st, status, tot, flags + tot);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_reset_commit(const int32_t* pairs, int n, float* el, float* az, float* radius, float* campos, float* cam,
                                float* alphas, float* full_reward, float* object_mass, int32_t* scene_mesh,
                                float* scene_offset, float* obs, const float* obs_all, const float* loss_all, int img,
                                void* stream) {
    if (n == 0) return OCC_OK;
    if (!pairs || n < 0 || !el || !az || !radius || !campos || !cam || !alphas || !full_reward || !object_mass ||
        !scene_mesh || !scene_offset || !obs || !obs_all || !loss_all || img <= 0)
        return OCC_ERR_ARG;
    CommitArgs a{pairs, n, el, az, radius, campos, cam, alphas, full_reward, object_mass, scene_mesh, scene_offset,
                 obs, obs_all, loss_all, img};
    hipLaunchKernelGGL(occ_commit_kernel, dim3(n, 3), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_auto_reset(const uint8_t* done, const float* loss_all, const int32_t* status, int n_env, int n_reserve,
                              int32_t* rs_state, int32_t* rs_tries, const OccEnvState* st, float* obs_all,
                              const float* full_state_all, const OccReserveStore* store, float* term_obs, int img,
                              int32_t* pairs, int32_t* report, const OccAutoResetOpts* opts, void* stream) {
    if (!done || !loss_all || !status || n_env <= 0 || n_reserve <= 0 || n_reserve > 512 || !rs_state || !rs_tries || !st ||
        !obs_all || !full_state_all || !store || !term_obs || img < OCC_TILE || img % OCC_TILE || !pairs || !report)
        return OCC_ERR_ARG;
    if (!st->el || !st->az || !st->radius || !st->campos || !st->cam || !st->alphas || !st->full_reward || !st->object_mass ||
        !st->scene_mesh || !st->scene_offset || !store->obs || !store->full_state || !store->loss || !store->skip)
        return OCC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    OccAutoResetOpts o{};
    if (opts) o = *opts;
    if (o.max_ep_len > 0 && !o.age) return OCC_ERR_ARG;
    if (o.norm_flags && !o.slot_objsum) return OCC_ERR_ARG;
    int32_t* was_pending = pairs + 2 + 2 * n_reserve;  // third section of the scratch
    PairArgs pa{done, loss_all, status, n_env, n_reserve, rs_state, rs_tries, pairs, report, store->skip, o.age, o.max_ep_len,
                was_pending, o.report_host};
    hipLaunchKernelGGL(occ_pair_kernel, dim3(1), dim3(1024), 0, s, pa);
    StashCommitArgs ca{was_pending, report + n_env + n_reserve, *st, obs_all, full_state_all, loss_all, *store, term_obs, img, n_env,
                       o.age, o.rect, o.arect, o.reset_full_state, o.norm_flags, o.slot_objsum};
    hipLaunchKernelGGL(occ_stash_commit_kernel, dim3(n_reserve, 1 + commit_obs_blocks(img) + commit_alpha_blocks(img)), dim3(256), 0, s, ca);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_object_mass(const float* alphas, int n_rows, int img, const int32_t* gate, int gate_value, float* out,
                               void* stream) {
    if (!alphas || !out || n_rows <= 0 || img <= 0) return OCC_ERR_ARG;
    hipLaunchKernelGGL(occ_object_mass_kernel, dim3(n_rows), dim3(256), 0, (hipStream_t)stream, alphas, img, gate, gate_value, out);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_reserve_refill(const int32_t* packed, int n, int n_env, int n_reserve, int32_t* scene_mesh,
                                  float* scene_offset, int32_t* rs_state, int32_t* skip, void* stream) {
    if (n == 0) return OCC_OK;
    if (!packed || n < 0 || n_env <= 0 || n_reserve <= 0 || !scene_mesh || !scene_offset || !rs_state || !skip) return OCC_ERR_ARG;
    hipLaunchKernelGGL(occ_refill_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, packed, n, n_env, n_reserve, scene_mesh,
                       scene_offset, rs_state, skip);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_episode_advance(const uint8_t* done, const float* reward, const float* full_reward, const float* grad,
                                   const float* pred, const float* noise, int rule, float lr, int step, int max_step, int n_env,
                                   float* action, int32_t* active, int32_t* skip, int32_t* iterations, uint8_t* finished,
                                   int32_t* nan_steps, float* trace_reward, float* trace_full_reward, int32_t* report,
                                   void* stream) {
    if (!done || !action || !active || !skip || !iterations || !finished || !nan_steps || !report || n_env <= 0 || max_step <= 0 ||
        step < 0 || step >= max_step || rule < OCC_EPISODE_GRADIENT || rule > OCC_EPISODE_AGENT)
        return OCC_ERR_ARG;
    if ((rule == OCC_EPISODE_GRADIENT && !grad) || (rule == OCC_EPISODE_RANDOM && !noise) || (rule >= OCC_EPISODE_MODEL && !pred))
        return OCC_ERR_ARG;
    if ((trace_reward && !reward) || (trace_full_reward && !full_reward)) return OCC_ERR_ARG;
    EpisodeArgs a{done, reward, full_reward, grad, pred, noise, rule, lr, step, max_step, n_env, action, active, skip, iterations,
                  finished, nan_steps, trace_reward, trace_full_reward, report};
    const int threads = n_env >= 1024 ? 1024 : ((n_env + 63) & ~63);
    hipLaunchKernelGGL(occ_episode_kernel, dim3(1), dim3(threads), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_ppo_act(const float* feats, const float* w_a, const float* b_a, const float* noise, float action_std,
                           int n_env, float* action, float* logprob, float* mean, float* feat_buf, float* action_buf,
                           float* logprob_buf, int t, int T, void* stream) {
    if (!feats || !w_a || !b_a || !noise || !(action_std > 0.f) || n_env <= 0 || !action || !logprob) return OCC_ERR_ARG;
    const bool buffered = feat_buf || action_buf || logprob_buf;
    if (buffered && (!feat_buf || !action_buf || !logprob_buf || T <= 0 || t < 0 || t >= T)) return OCC_ERR_ARG;
    PpoActArgs A;
    A.feats = feats; A.w_a = w_a; A.b_a = b_a; A.noise = noise; A.action_std = action_std; A.n = n_env;
    // The variance is the f32 square, and 1 / var the f32 quotient occ_ppo_update forms from a variance it is given: the
    // quadratic term is then the epoch's, bit for bit.  The constant is formed in double and rounded once: near std = 0.4
    // the two logarithms cancel (the constant passes through zero), and occ_ppo_update's f32 sum is then a hundred ulps of
    // the constant off - 4e-8 in absolute terms, which is all the first epoch's recomputed log-probability differs by.
    const float action_var = action_std * action_std;
    A.inv_var = 1.0f / action_var;
    A.lp_const = (float)(-0.5 * (2.0 * 1.8378770664093453 + 2.0 * log((double)action_var)));
    A.action = action; A.logprob = logprob; A.mean = mean;
    A.feat_buf = feat_buf; A.action_buf = action_buf; A.logprob_buf = logprob_buf;
    A.row0 = buffered ? (long long)t * n_env : 0;
    hipLaunchKernelGGL(occ_ppo_act_kernel, dim3((n_env + kActWaves - 1) / kActWaves), dim3(64 * kActWaves), 0, (hipStream_t)stream, A);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_rollout_advance(const float* reward, const uint8_t* done, const int32_t* code, int n_env, int t, int T,
                                   int64_t timestep, float* rewards, float* dones, const OccRolloutState* state, int cap,
                                   void* stream) {
    if (!reward || !done || !code || n_env <= 0 || cap <= 0 || !state) return OCC_ERR_ARG;
    if (!state->ep_return || !state->ep_len || !state->ring_env || !state->ring_return || !state->ring_length ||
        !state->ring_code || !state->ring_timestep || !state->ring_running || !state->n_episodes || !state->code_counts || !state->sums || !state->running)
        return OCC_ERR_ARG;
    const bool buffered = rewards || dones;
    if (buffered && (!rewards || !dones || T <= 0 || t < 0 || t >= T)) return OCC_ERR_ARG;
    RolloutArgs a;
    a.reward = reward; a.done = done; a.code = code; a.n = n_env; a.cap = cap;
    a.row0 = buffered ? (long long)t * n_env : 0;
    a.timestep = (long long)timestep;
    a.rewards = rewards; a.dones = dones; a.ep_return = state->ep_return; a.ep_len = state->ep_len;
    a.ring_env = state->ring_env; a.ring_return = state->ring_return; a.ring_length = state->ring_length;
    a.ring_code = state->ring_code; a.ring_timestep = (long long*)state->ring_timestep; a.ring_running = state->ring_running;
    a.n_episodes = (long long*)state->n_episodes; a.code_counts = (long long*)state->code_counts;
    a.sums = state->sums; a.running = state->running;
    // (always 16 waves: block_prefix_1024 adds up the counts of all sixteen)
    hipLaunchKernelGGL(occ_rollout_advance_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_ppo_returns(const float* rewards, const float* dones, int T, int n_env, float gamma, float* returns,
                               float* raw_returns, double* stats, void* stream) {
    if (!rewards || !dones || !returns || !stats || T <= 0 || n_env <= 0 || (int64_t)T * n_env < 2) return OCC_ERR_ARG;
    ReturnsArgs a{rewards, dones, T, n_env, gamma, returns, raw_returns, stats};
    hipLaunchKernelGGL(occ_ppo_returns_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_step_finish(const float* loss, const float* grad_elaz, const float* cam, float* full_reward,
                               const float* object_mass, float* reward, uint8_t* done, float* grad_action, int n_env,
                               void* stream) {
    if (!loss || !cam || !full_reward || !object_mass || !reward || !done || n_env <= 0) return OCC_ERR_ARG;
    hipLaunchKernelGGL(occ_finish_kernel, dim3((n_env + 63) / 64), dim3(64), 0, (hipStream_t)stream, loss, grad_elaz, cam,
                       full_reward, object_mass, reward, done, grad_action, n_env);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

static bool enc_cfg_ok(const OccEncoderConfig* c) {
    return c && c->img >= 32 && c->img <= 1024 && (c->dilation == 1 || c->dilation == 2) && (c->residual == 0 || c->residual == 1) &&
           (c->separable == 0 || c->separable == 1);
}

extern "C" int64_t occ_encoder_packed_floats(const OccEncoderConfig* cfg) {
    if (!cfg || (cfg->separable != 0 && cfg->separable != 1)) return -1;
    return enc_packed_floats(cfg->separable != 0);
}

extern "C" int occ_encoder_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* bytes) {
    if (!enc_cfg_ok(cfg) || n_env <= 0 || !bytes) return OCC_ERR_ARG;
    size_t buf, part;
    enc_ws_layout(cfg->img, n_env, &buf, &part);
    *bytes = 3 * buf + part;
    return OCC_OK;
}

extern "C" int occ_encoder_forward_masked(const OccEncoderConfig* cfg, const float* packed_weights, const float* obs, int n_env,
                                          void* ws, size_t ws_bytes, float* feats, const int32_t* skip, void* stream) {
    static_assert(kEncFeat == OCC_ENCODER_FEATURES, "occ_encoder.hpp and the header disagree");
    if (!enc_cfg_ok(cfg) || !packed_weights || !obs || n_env <= 0 || n_env > 65535 || !ws || !feats) return OCC_ERR_ARG;
    size_t need = 0;
    occ_encoder_workspace_query(cfg, n_env, &need);
    if (ws_bytes < need) return OCC_ERR_ARG;
    enc_forward(cfg->img, cfg->dilation, cfg->residual != 0, cfg->separable != 0, packed_weights, obs, n_env, (char*)ws, feats,
                (hipStream_t)stream, nullptr, skip);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_encoder_forward(const OccEncoderConfig* cfg, const float* packed_weights, const float* obs, int n_env, void* ws,
                                   size_t ws_bytes, float* feats, void* stream) {
    return occ_encoder_forward_masked(cfg, packed_weights, obs, n_env, ws, ws_bytes, feats, nullptr, stream);
}

// ---- bf16 inference mode of the separable encoder (occ_encoder_bf16.hpp) --------------------------------------------------
extern "C" int64_t occ_encoder_bf16_packed_bytes(const OccEncoderConfig* cfg) {
    if (!cfg || cfg->separable != 1) return -1;
    return enc16_packed_bytes();
}

extern "C" int occ_encoder_bf16_pack(const OccEncoderConfig* cfg, const float* packed_f32, void* out) {
    if (!cfg || cfg->separable != 1 || !packed_f32 || !out) return OCC_ERR_ARG;
    enc16_pack(packed_f32, (char*)out);
    return OCC_OK;
}

extern "C" int occ_encoder_bf16_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* bytes) {
    if (!enc_cfg_ok(cfg) || cfg->separable != 1 || n_env <= 0 || !bytes) return OCC_ERR_ARG;
    size_t buf, part;
    enc16_ws_layout(cfg->img, n_env, &buf, &part);
    *bytes = 3 * buf + part;
    return OCC_OK;
}

extern "C" int occ_encoder_forward_bf16(const OccEncoderConfig* cfg, const void* packed_bf16, const float* obs, int n_env, void* ws,
                                        size_t ws_bytes, float* feats, const int32_t* skip, void* stream) {
    if (!enc_cfg_ok(cfg) || cfg->separable != 1 || !packed_bf16 || !obs || n_env <= 0 || n_env > 65535 || !ws || !feats)
        return OCC_ERR_ARG;
    if (((uintptr_t)packed_bf16 | (uintptr_t)ws) & 15) return OCC_ERR_ARG;  // 16-byte accesses
    size_t need = 0;
    occ_encoder_bf16_workspace_query(cfg, n_env, &need);
    if (ws_bytes < need) return OCC_ERR_ARG;
    enc16_forward(cfg->img, cfg->dilation, cfg->residual != 0, (const char*)packed_bf16, obs, n_env, (char*)ws, feats,
                  (hipStream_t)stream, skip);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

// ---- segmentation decoder (occ_decoder.hpp) ----------------------------------------------------------------------------
extern "C" int64_t occ_decoder_packed_floats(const OccEncoderConfig* cfg) {
    if (!cfg || (cfg->separable != 0 && cfg->separable != 1)) return -1;
    return dec_packed_floats();  // the up layers are dense transposed convs whatever the encoder's form
}

extern "C" int occ_segment_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* bytes) {
    if (!enc_cfg_ok(cfg) || cfg->img % 32 != 0 || n_env <= 0 || !bytes) return OCC_ERR_ARG;
    *bytes = seg_ws_layout(cfg->img, n_env).total;
    return OCC_OK;
}

extern "C" int occ_segment_forward_masked(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed,
                                          const float* obs, int n_env, void* ws, size_t ws_bytes, float* feats, float* prob,
                                          float* logit, float* dec_feat, const int32_t* skip, void* stream) {
    if (!enc_cfg_ok(cfg) || cfg->img % 32 != 0 || !enc_packed || !dec_packed || !obs || n_env <= 0 || n_env > 65535 || !ws ||
        !feats || !prob)
        return OCC_ERR_ARG;
    // the quad rows are stored as float2
    if ((((uintptr_t)ws | (uintptr_t)prob | (uintptr_t)logit | (uintptr_t)dec_feat) & 7) != 0) return OCC_ERR_ARG;
    size_t need = 0;
    occ_segment_workspace_query(cfg, n_env, &need);
    if (ws_bytes < need) return OCC_ERR_ARG;
    seg_forward(cfg->img, cfg->dilation, cfg->residual != 0, cfg->separable != 0, enc_packed, dec_packed, obs, n_env, (char*)ws,
                feats, prob, logit, dec_feat, (hipStream_t)stream, skip);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_segment_forward(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed, const float* obs,
                                   int n_env, void* ws, size_t ws_bytes, float* feats, float* prob, float* logit, float* dec_feat,
                                   void* stream) {
    return occ_segment_forward_masked(cfg, enc_packed, dec_packed, obs, n_env, ws, ws_bytes, feats, prob, logit, dec_feat, nullptr,
                                      stream);
}

// ---- training (occ_decoder_bwd.hpp, occ_encoder_bwd.hpp, occ_fullnet_bwd.hpp): the argument checks ----------------------
static bool seg_train_cfg_ok(const OccEncoderConfig* c, int n_env) {
    return enc_cfg_ok(c) && c->img % 32 == 0 && n_env >= 1 && n_env <= 65535;
}
static bool enc_train_cfg_ok(const OccEncoderConfig* c, int n_env) {
    return enc_cfg_ok(c) && c->separable == 0 && c->dilation == 1 && n_env >= 1 && n_env <= 65535;
}
static bool full_train_cfg_ok(const OccEncoderConfig* c, int n_env) { return enc_train_cfg_ok(c, n_env) && c->img % 32 == 0; }
static bool sep_train_cfg_ok(const OccEncoderConfig* c, int n_env) {
    return enc_cfg_ok(c) && c->separable == 1 && n_env >= 1 && n_env <= 65535;
}
static bool sep_full_train_cfg_ok(const OccEncoderConfig* c, int n_env) { return sep_train_cfg_ok(c, n_env) && c->img % 32 == 0; }

template <class... P>
static bool non_null(P... p) {
    return (... && (p != nullptr));
}
// every pointer a multiple of `bytes` (a power of two): 16 where planes are read as float4 or partials are doubles, 8 where
// quad rows are stored as float2, 4 for plain f32
template <class... P>
static bool aligned(uintptr_t bytes, P... p) {
    return ((... | (uintptr_t)p) & (bytes - 1)) == 0;
}
// the answer of the training workspace queries
template <class Layout>
static int train_sizes(const Layout& l, size_t* ws_bytes, size_t* scratch_bytes) {
    *ws_bytes = l.total;
    *scratch_bytes = l.scratch;
    return OCC_OK;
}

// ---- decoder training (occ_decoder_bwd.hpp) ------------------------------------------------------------------------------
extern "C" int occ_segment_train_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* ws_bytes, size_t* scratch_bytes) {
    if (!seg_train_cfg_ok(cfg, n_env) || !non_null(ws_bytes, scratch_bytes)) return OCC_ERR_ARG;
    return train_sizes(train_ws_layout(cfg->img, n_env), ws_bytes, scratch_bytes);
}

extern "C" int occ_segment_train_forward(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed,
                                         const float* obs, int n_env, void* ws, size_t ws_bytes, float* feats, float* prob,
                                         void* stream) {
    if (!seg_train_cfg_ok(cfg, n_env) || !non_null(enc_packed, dec_packed, obs, ws, feats, prob)) return OCC_ERR_ARG;
    if (!aligned(16, ws) || !aligned(8, prob)) return OCC_ERR_ARG;
    if (ws_bytes < train_ws_layout(cfg->img, n_env).total) return OCC_ERR_ARG;
    seg_train_forward(cfg->img, cfg->dilation, cfg->residual != 0, cfg->separable != 0, enc_packed, dec_packed, obs, n_env,
                      (char*)ws, feats, prob, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_segment_backward(const OccEncoderConfig* cfg, const float* dec_packed, int n_env, void* ws, size_t ws_bytes,
                                    const float* grad_prob, void* scratch, size_t scratch_bytes, float* grad_packed, void* stream) {
    if (!seg_train_cfg_ok(cfg, n_env) || !non_null(dec_packed, ws, grad_prob, scratch, grad_packed)) return OCC_ERR_ARG;
    if (!aligned(16, ws, grad_prob, scratch)) return OCC_ERR_ARG;
    const TrainWs l = train_ws_layout(cfg->img, n_env);
    if (ws_bytes < l.total || scratch_bytes < l.scratch) return OCC_ERR_ARG;
    seg_backward(cfg->img, dec_packed, n_env, (char*)ws, grad_prob, (char*)scratch, grad_packed, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

// ---- encoder training (occ_encoder_bwd.hpp, occ_sepenc_bwd.hpp) and joint training (occ_fullnet_bwd.hpp) -----------------
// Each entry point exists for the dense encoder (which refuses a separable config or dilation != 1) and for the separable
// one (which refuses a dense config): a pair shares its body, given its config predicate and its form.
typedef bool (*TrainCfgOk)(const OccEncoderConfig*, int);

static int enc_train_query(TrainCfgOk ok, bool separable, const OccEncoderConfig* cfg, int n_env, size_t* ws_bytes,
                           size_t* scratch_bytes) {
    if (!ok(cfg, n_env) || !non_null(ws_bytes, scratch_bytes)) return OCC_ERR_ARG;
    return train_sizes(enc_train_ws_layout(cfg->img, n_env, separable), ws_bytes, scratch_bytes);
}

static int enc_train_fwd(TrainCfgOk ok, bool separable, const OccEncoderConfig* cfg, const float* packed, const float* obs, int n_env,
                         void* ws, size_t ws_bytes, float* feats, void* stream) {
    if (!ok(cfg, n_env) || !non_null(packed, obs, ws, feats)) return OCC_ERR_ARG;
    if (!aligned(16, ws) || !aligned(4, packed, obs, feats)) return OCC_ERR_ARG;
    if (ws_bytes < enc_train_ws_layout(cfg->img, n_env, separable).total) return OCC_ERR_ARG;
    enc_train_forward(cfg->img, cfg->dilation, cfg->residual != 0, separable, packed, obs, n_env, (char*)ws, feats,
                      (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

static int enc_train_bwd(TrainCfgOk ok, bool separable, const OccEncoderConfig* cfg, const float* packed, int n_env, void* ws,
                         size_t ws_bytes, const float* grad_feats, void* scratch, size_t scratch_bytes, float* grad_packed,
                         void* stream) {
    if (!ok(cfg, n_env) || !non_null(packed, ws, grad_feats, scratch, grad_packed)) return OCC_ERR_ARG;
    if (!aligned(16, ws, scratch) || !aligned(4, packed, grad_feats, grad_packed)) return OCC_ERR_ARG;
    const EncTrainWs l = enc_train_ws_layout(cfg->img, n_env, separable);
    if (ws_bytes < l.total || scratch_bytes < l.scratch) return OCC_ERR_ARG;
    enc_backward(cfg->img, cfg->dilation, cfg->residual != 0, separable, packed, n_env, (char*)ws, grad_feats, (char*)scratch,
                 grad_packed, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

static int full_train_query(TrainCfgOk ok, bool separable, const OccEncoderConfig* cfg, int n_env, size_t* ws_bytes,
                            size_t* scratch_bytes) {
    if (!ok(cfg, n_env) || !non_null(ws_bytes, scratch_bytes)) return OCC_ERR_ARG;
    return train_sizes(full_train_ws_layout(cfg->img, n_env, separable), ws_bytes, scratch_bytes);
}

static int full_train_fwd(TrainCfgOk ok, bool separable, const OccEncoderConfig* cfg, const float* enc_packed,
                          const float* dec_packed, const float* obs, int n_env, void* ws, size_t ws_bytes, float* feats,
                          float* prob, void* stream) {
    if (!ok(cfg, n_env) || !non_null(enc_packed, dec_packed, obs, ws, feats, prob)) return OCC_ERR_ARG;
    if (!aligned(16, ws) || !aligned(8, prob) || !aligned(4, enc_packed, dec_packed, obs, feats)) return OCC_ERR_ARG;
    if (ws_bytes < full_train_ws_layout(cfg->img, n_env, separable).total) return OCC_ERR_ARG;
    full_train_forward(cfg->img, cfg->dilation, cfg->residual != 0, separable, enc_packed, dec_packed, obs, n_env, (char*)ws, feats,
                       prob, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

static int full_train_bwd(TrainCfgOk ok, bool separable, const OccEncoderConfig* cfg, const float* enc_packed,
                          const float* dec_packed, int n_env, void* ws, size_t ws_bytes, const float* grad_feats,
                          const float* grad_prob, void* scratch, size_t scratch_bytes, float* grad_enc_packed,
                          float* grad_dec_packed, void* stream) {
    if (!ok(cfg, n_env) || !non_null(enc_packed, dec_packed, ws, grad_feats, grad_prob, scratch, grad_enc_packed, grad_dec_packed))
        return OCC_ERR_ARG;
    if (!aligned(16, ws, scratch, grad_prob) || !aligned(4, enc_packed, dec_packed, grad_feats, grad_enc_packed, grad_dec_packed))
        return OCC_ERR_ARG;
    const FullTrainWs l = full_train_ws_layout(cfg->img, n_env, separable);
    if (ws_bytes < l.total || scratch_bytes < l.scratch) return OCC_ERR_ARG;
    full_backward(cfg->img, cfg->dilation, cfg->residual != 0, separable, enc_packed, dec_packed, n_env, (char*)ws, grad_feats,
                  grad_prob, (char*)scratch, grad_enc_packed, grad_dec_packed, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_encoder_train_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* ws_bytes, size_t* scratch_bytes) {
    return enc_train_query(enc_train_cfg_ok, false, cfg, n_env, ws_bytes, scratch_bytes);
}

extern "C" int occ_encoder_train_forward(const OccEncoderConfig* cfg, const float* packed, const float* obs, int n_env, void* ws,
                                         size_t ws_bytes, float* feats, void* stream) {
    return enc_train_fwd(enc_train_cfg_ok, false, cfg, packed, obs, n_env, ws, ws_bytes, feats, stream);
}

extern "C" int occ_encoder_backward(const OccEncoderConfig* cfg, const float* packed, int n_env, void* ws, size_t ws_bytes,
                                    const float* grad_feats, void* scratch, size_t scratch_bytes, float* grad_packed, void* stream) {
    return enc_train_bwd(enc_train_cfg_ok, false, cfg, packed, n_env, ws, ws_bytes, grad_feats, scratch, scratch_bytes, grad_packed,
                         stream);
}

extern "C" int occ_sep_encoder_train_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* ws_bytes,
                                                     size_t* scratch_bytes) {
    return enc_train_query(sep_train_cfg_ok, true, cfg, n_env, ws_bytes, scratch_bytes);
}

extern "C" int occ_sep_encoder_train_forward(const OccEncoderConfig* cfg, const float* packed, const float* obs, int n_env, void* ws,
                                             size_t ws_bytes, float* feats, void* stream) {
    return enc_train_fwd(sep_train_cfg_ok, true, cfg, packed, obs, n_env, ws, ws_bytes, feats, stream);
}

extern "C" int occ_sep_encoder_backward(const OccEncoderConfig* cfg, const float* packed, int n_env, void* ws, size_t ws_bytes,
                                        const float* grad_feats, void* scratch, size_t scratch_bytes, float* grad_packed,
                                        void* stream) {
    return enc_train_bwd(sep_train_cfg_ok, true, cfg, packed, n_env, ws, ws_bytes, grad_feats, scratch, scratch_bytes, grad_packed,
                         stream);
}

extern "C" int occ_fullnet_train_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* ws_bytes, size_t* scratch_bytes) {
    return full_train_query(full_train_cfg_ok, false, cfg, n_env, ws_bytes, scratch_bytes);
}

extern "C" int occ_fullnet_train_forward(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed,
                                         const float* obs, int n_env, void* ws, size_t ws_bytes, float* feats, float* prob,
                                         void* stream) {
    return full_train_fwd(full_train_cfg_ok, false, cfg, enc_packed, dec_packed, obs, n_env, ws, ws_bytes, feats, prob, stream);
}

extern "C" int occ_fullnet_backward(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed, int n_env,
                                    void* ws, size_t ws_bytes, const float* grad_feats, const float* grad_prob, void* scratch,
                                    size_t scratch_bytes, float* grad_enc_packed, float* grad_dec_packed, void* stream) {
    return full_train_bwd(full_train_cfg_ok, false, cfg, enc_packed, dec_packed, n_env, ws, ws_bytes, grad_feats, grad_prob, scratch,
                          scratch_bytes, grad_enc_packed, grad_dec_packed, stream);
}

extern "C" int occ_sep_fullnet_train_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* ws_bytes,
                                                     size_t* scratch_bytes) {
    return full_train_query(sep_full_train_cfg_ok, true, cfg, n_env, ws_bytes, scratch_bytes);
}

extern "C" int occ_sep_fullnet_train_forward(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed,
                                             const float* obs, int n_env, void* ws, size_t ws_bytes, float* feats, float* prob,
                                             void* stream) {
    return full_train_fwd(sep_full_train_cfg_ok, true, cfg, enc_packed, dec_packed, obs, n_env, ws, ws_bytes, feats, prob, stream);
}

extern "C" int occ_sep_fullnet_backward(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed, int n_env,
                                        void* ws, size_t ws_bytes, const float* grad_feats, const float* grad_prob, void* scratch,
                                        size_t scratch_bytes, float* grad_enc_packed, float* grad_dec_packed, void* stream) {
    return full_train_bwd(sep_full_train_cfg_ok, true, cfg, enc_packed, dec_packed, n_env, ws, ws_bytes, grad_feats, grad_prob,
                          scratch, scratch_bytes, grad_enc_packed, grad_dec_packed, stream);
}

// ---- joint training with batch-statistics BatchNorm (occ_bn_train.hpp): one entry point for both encoder forms ----------
static bool full_bn_cfg_ok(const OccEncoderConfig* c, int n_env) {
    if (!c) return false;
    return (c->separable ? sep_full_train_cfg_ok(c, n_env) : full_train_cfg_ok(c, n_env)) && bn_train_shape_ok(c->img, n_env);
}

extern "C" int occ_fullnet_bn_train_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* ws_bytes,
                                                    size_t* scratch_bytes) {
    if (!full_bn_cfg_ok(cfg, n_env) || !non_null(ws_bytes, scratch_bytes)) return OCC_ERR_ARG;
    const FullBnTrainWs l = full_bn_train_ws_layout(cfg->img, n_env, cfg->separable != 0);
    *ws_bytes = l.total;
    *scratch_bytes = l.full.scratch;
    return OCC_OK;
}

extern "C" int occ_fullnet_bn_train_forward(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed,
                                            const float* obs, int n_env, void* ws, size_t ws_bytes, float* feats, float* prob,
                                            float* bn_stats, void* stream) {
    if (!full_bn_cfg_ok(cfg, n_env) || !non_null(enc_packed, dec_packed, obs, ws, feats, prob, bn_stats)) return OCC_ERR_ARG;
    if (!aligned(16, ws, prob) || !aligned(4, enc_packed, dec_packed, obs, feats, bn_stats)) return OCC_ERR_ARG;
    const FullBnTrainWs l = full_bn_train_ws_layout(cfg->img, n_env, cfg->separable != 0);
    if (ws_bytes < l.total) return OCC_ERR_ARG;
    const BnTrain bn = full_bn_ptrs(l, (char*)ws, bn_stats);
    full_train_forward(cfg->img, cfg->dilation, cfg->residual != 0, cfg->separable != 0, enc_packed, dec_packed, obs, n_env,
                       (char*)ws, feats, prob, (hipStream_t)stream, &bn);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_fullnet_bn_backward(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed, int n_env,
                                       void* ws, size_t ws_bytes, const float* grad_feats, const float* grad_prob, void* scratch,
                                       size_t scratch_bytes, float* grad_enc_packed, float* grad_dec_packed, void* stream) {
    if (!full_bn_cfg_ok(cfg, n_env) ||
        !non_null(enc_packed, dec_packed, ws, grad_feats, grad_prob, scratch, grad_enc_packed, grad_dec_packed))
        return OCC_ERR_ARG;
    if (!aligned(16, ws, scratch, grad_prob) || !aligned(4, enc_packed, dec_packed, grad_feats, grad_enc_packed, grad_dec_packed))
        return OCC_ERR_ARG;
    const FullBnTrainWs l = full_bn_train_ws_layout(cfg->img, n_env, cfg->separable != 0);
    if (ws_bytes < l.total || scratch_bytes < l.full.scratch) return OCC_ERR_ARG;
    const BnTrain bn = full_bn_ptrs(l, (char*)ws, nullptr);
    full_backward(cfg->img, cfg->dilation, cfg->residual != 0, cfg->separable != 0, enc_packed, dec_packed, n_env, (char*)ws,
                  grad_feats, grad_prob, (char*)scratch, grad_enc_packed, grad_dec_packed, (hipStream_t)stream, &bn);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

// ---- AdamW on the packed parameters of the joint step (occ_adamw.hpp) ------------------------------------------------------
extern "C" int occ_net_adamw_query(const OccEncoderConfig* cfg, int64_t* enc_floats, int64_t* dec_floats, int64_t* stat_floats) {
    if (!enc_cfg_ok(cfg) || !non_null(enc_floats, dec_floats, stat_floats)) return OCC_ERR_ARG;
    AdamwArgs a = {};
    int stat = 0;
    adamw_plan(cfg->separable != 0, 0, &a, &stat);
    *enc_floats = enc_packed_floats(cfg->separable != 0);
    *dec_floats = dec_packed_floats();
    *stat_floats = stat;
    return OCC_OK;
}

static bool adamw_parts_ok(const OccEncoderConfig* cfg, const float* enc_theta, const float* enc_packed, const float* dec_theta,
                           const float* dec_packed, const float* stats, int bn_mode) {
    return enc_cfg_ok(cfg) && non_null(enc_theta, enc_packed, dec_theta, dec_packed, stats) && (bn_mode == 0 || bn_mode == 1) &&
           aligned(16, enc_theta, enc_packed, dec_theta, dec_packed, stats);
}

extern "C" int occ_net_adamw_step(const OccEncoderConfig* cfg, float* enc_theta, float* enc_m, float* enc_v, const float* enc_grad,
                                  float* enc_packed, float* dec_theta, float* dec_m, float* dec_v, const float* dec_grad,
                                  float* dec_packed, const float* stats, float* head_theta, float* head_m, float* head_v,
                                  const float* head_grad, int64_t head_count, double lr, double beta1, double beta2, double eps,
                                  double weight_decay, int64_t step, int bn_mode, void* stream) {
    if (!adamw_parts_ok(cfg, enc_theta, enc_packed, dec_theta, dec_packed, stats, bn_mode) ||
        !non_null(enc_m, enc_v, enc_grad, dec_m, dec_v, dec_grad) || !aligned(16, enc_m, enc_v, enc_grad, dec_m, dec_v, dec_grad))
        return OCC_ERR_ARG;
    if (head_count < 0 || head_count > (1 << 24)) return OCC_ERR_ARG;
    if (head_count > 0 && (!non_null(head_theta, head_m, head_v, head_grad) || !aligned(16, head_theta, head_m, head_v, head_grad)))
        return OCC_ERR_ARG;
    // !(x >= 0) also refuses a NaN
    if (step <= 0 || !(eps > 0.0) || !(lr >= 0.0) || !(weight_decay >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) ||
        !(beta2 >= 0.0 && beta2 < 1.0))
        return OCC_ERR_ARG;
    AdamwArgs a = {};
    a.part[0] = AdamwPart{enc_theta, enc_m, enc_v, enc_grad, enc_packed};
    a.part[1] = AdamwPart{dec_theta, dec_m, dec_v, dec_grad, dec_packed};
    a.part[2] = AdamwPart{head_theta, head_m, head_v, head_grad, nullptr};
    a.stats = stats;
    a.fold = bn_mode == 0;
    // torch.optim.AdamW's scalars (_single_tensor_adam), in double as Python forms them
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    a.k = AdamwCoef{(float)(1.0 - lr * weight_decay), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)(-(lr / bc1)),
                    (float)sqrt(bc2), (float)eps};
    adamw_launch<true>(cfg->separable != 0, (int)head_count, a, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_net_adamw_fold(const OccEncoderConfig* cfg, const float* enc_theta, float* enc_packed, const float* dec_theta,
                                  float* dec_packed, const float* stats, int bn_mode, void* stream) {
    if (!adamw_parts_ok(cfg, enc_theta, enc_packed, dec_theta, dec_packed, stats, bn_mode)) return OCC_ERR_ARG;
    AdamwArgs a = {};
    a.part[0] = AdamwPart{const_cast<float*>(enc_theta), nullptr, nullptr, nullptr, enc_packed};
    a.part[1] = AdamwPart{const_cast<float*>(dec_theta), nullptr, nullptr, nullptr, dec_packed};
    a.stats = stats;
    a.fold = bn_mode == 0;
    adamw_launch<false>(cfg->separable != 0, 0, a, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

// ---- the pretraining input pipeline (occ_augment.hpp) ----------------------------------------------------------------------
static bool augment_shape_ok(int img, int n) { return img >= 1 && (int64_t)img * img <= (int64_t)kAugMaxPixels && n >= 1 && n <= 65535; }

extern "C" int occ_augment_query(int img, int n, size_t* workspace_bytes) {
    if (!augment_shape_ok(img, n) || !workspace_bytes) return OCC_ERR_ARG;
    *workspace_bytes = (size_t)n * aug_blocks_per_image(img) * sizeof(uint32_t);
    return OCC_OK;
}

extern "C" int occ_augment_batch(const uint32_t* rgbl, const int16_t* depth, const float* pos, const float* grad, int m_frames,
                                 int img, const int64_t* idx, const OccAugmentParams* params, int n, int normalize, float* out_img,
                                 float* out_label, float* out_grad, float* out_pos, void* workspace, void* stream) {
    if (!augment_shape_ok(img, n) || m_frames < 1) return OCC_ERR_ARG;
    if (!non_null(rgbl, depth, pos, grad, idx, out_img, out_label, out_grad, out_pos) || (params && !workspace)) return OCC_ERR_ARG;
    const dim3 grid(aug_blocks_per_image(img), n);
    hipStream_t st = (hipStream_t)stream;
    if (params)
        hipLaunchKernelGGL(occ_augment_sum_kernel, grid, dim3(kAugBlock), 0, st, rgbl, m_frames, img * img, idx, params,
                           (uint32_t*)workspace);
    hipLaunchKernelGGL(occ_augment_out_kernel, grid, dim3(kAugBlock), 0, st, rgbl, depth, pos, grad, m_frames, img, idx, params,
                       (const uint32_t*)workspace, normalize, out_img, out_label, out_grad, out_pos);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

// ---- rendered frames into the resident dataset (occ_datapack.hpp) ----------------------------------------------------------
extern "C" int occ_dataset_pack(const float* obs, const float* alpha, int alpha_stride, int n, int img, const int64_t* slot,
                                uint32_t* rgbl, int16_t* depth, int m_frames, int label_mode, void* stream) {
    if (!non_null(obs, alpha, slot, rgbl, depth)) return OCC_ERR_ARG;
    if (img < 1 || (int64_t)img * img > (int64_t)kPackMaxPixels || n < 1 || n > 65535 || m_frames < 1 || alpha_stride < 1 ||
        (label_mode != 0 && label_mode != 1))
        return OCC_ERR_ARG;
    static_assert((int64_t)kDitherMaxImg * kDitherMaxImg == (int64_t)kPackMaxPixels, "the errors row in LDS covers every legal img");
    hipStream_t st = (hipStream_t)stream;
    const int pixels = img * img;
    hipLaunchKernelGGL(occ_datapack_point_kernel, dim3((pixels + kPackBlock - 1) / kPackBlock, n), dim3(kPackBlock), 0, st, obs, alpha,
                       alpha_stride, pixels, slot, rgbl, depth, m_frames, label_mode);
    if (label_mode == 0)
        hipLaunchKernelGGL(occ_datapack_dither_kernel, dim3(n), dim3(kDitherRows), 0, st, slot, rgbl, img, m_frames);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

// ---- PIL's resize between two resident stores (occ_resize.hpp) -------------------------------------------------------------
static bool resize_shape_ok(int src_img, int dst_img, int n) {
    return src_img >= 1 && dst_img >= 1 && (int64_t)src_img * src_img <= (int64_t)kResizeMaxPixels &&
           (int64_t)dst_img * dst_img <= (int64_t)kResizeMaxPixels && n >= 1 && n <= 65535 && resize_ratio_ok(src_img, dst_img);
}

extern "C" int occ_dataset_resize_query(int src_img, int dst_img, int n, size_t* workspace_bytes) {
    if (!resize_shape_ok(src_img, dst_img, n) || !workspace_bytes) return OCC_ERR_ARG;
    *workspace_bytes = resize_table_bytes(src_img, dst_img);
    return OCC_OK;
}

extern "C" int occ_dataset_resize(const uint32_t* src_rgbl, const int16_t* src_depth, int n, int src_img, const int64_t* slot,
                                  uint32_t* dst_rgbl, int16_t* dst_depth, int m_frames, int dst_img, void* workspace, void* stream) {
    if (!non_null(src_rgbl, src_depth, slot, dst_rgbl, dst_depth, workspace) || ((uintptr_t)workspace & 7) != 0) return OCC_ERR_ARG;
    if (!resize_shape_ok(src_img, dst_img, n) || m_frames < 1) return OCC_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int R = src_img, S = dst_img, K = resize_taps(R, S);
    const ResizeTables t = resize_tables(workspace, R, S);
    const int tiles = (S + kResizeTile - 1) / kResizeTile;
    hipLaunchKernelGGL(occ_resize_table_kernel, dim3((S + 63) / 64), dim3(64), 0, st, R, S, K, t);
    hipLaunchKernelGGL(occ_resize_kernel, dim3(tiles * tiles, n), dim3(kResizeBlock), 0, st, src_rgbl, src_depth, R, slot, dst_rgbl,
                       dst_depth, m_frames, S, K, t);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

// ---- the JPEG round trip in place in the resident store (occ_jpeg.hpp) ------------------------------------------------------
static bool jpeg_shape_ok(int img, int n, int quality) {
    return img >= 1 && img <= kJpegMaxImg && n >= 1 && n <= 65535 && quality >= 1 && quality <= 100;
}

extern "C" int occ_dataset_jpeg_query(int img, int n, int quality, size_t* workspace_bytes) {
    if (!jpeg_shape_ok(img, n, quality) || !workspace_bytes) return OCC_ERR_ARG;
    const size_t cs = (size_t)jpeg_chroma_side(img);
    *workspace_bytes = (size_t)n * cs * cs * sizeof(uint16_t);
    return OCC_OK;
}

extern "C" int occ_dataset_jpeg(uint32_t* rgbl, int m_frames, int img, const int64_t* slot, int n, int quality, void* workspace,
                                void* stream) {
    if (!non_null(rgbl, slot, workspace) || ((uintptr_t)workspace & 1) != 0) return OCC_ERR_ARG;
    if (!jpeg_shape_ok(img, n, quality) || m_frames < 1) return OCC_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const JpegTables tab = jpeg_tables(quality);
    const int tiles = (img + kJpegTile - 1) / kJpegTile, cs = jpeg_chroma_side(img);
    hipLaunchKernelGGL(occ_jpeg_block_kernel, dim3(tiles * tiles, n), dim3(kJpegBlock), 0, st, rgbl, m_frames, img, slot, tab,
                       (uint16_t*)workspace, cs);
    hipLaunchKernelGGL(occ_jpeg_upsample_kernel, dim3((img * img + kJpegBlock - 1) / kJpegBlock, n), dim3(kJpegBlock), 0, st, rgbl,
                       m_frames, img, slot, (const uint16_t*)workspace, cs);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_seg_metrics(const float* pred, const float* target, int target_stride, int n_env, int img, int64_t* counts,
                               void* stream) {
    if (!pred || !target || !counts || target_stride < 1 || n_env <= 0 || n_env > 65535 || img < 1 || img > 1024)
        return OCC_ERR_ARG;
    const int npix = img * img;
    if (hipMemsetAsync(counts, 0, (size_t)n_env * 3 * sizeof(int64_t), (hipStream_t)stream) != hipSuccess) return OCC_ERR_LAUNCH;
    hipLaunchKernelGGL(occ_seg_metrics_kernel, dim3((npix + kSegMetricsPerBlock - 1) / kSegMetricsPerBlock, n_env),
                       dim3(kSegMetricsBlock), 0, (hipStream_t)stream, pred, target, target_stride, npix,
                       (unsigned long long*)counts);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

// ---- pretrainer criterion (occ_criterion.hpp) ----------------------------------------------------------------------------
static bool crit_args_ok(const void* pred, const void* target, int target_stride, int n_env, int img) {
    return pred && target && target_stride >= 1 && n_env > 0 && n_env <= 65535 && img >= 1 && img <= 1024;
}

extern "C" size_t occ_seg_criterion_scratch_bytes(int n_env, int img) {
    if (n_env <= 0 || n_env > 65535 || img < 1 || img > 1024) return 0;
    return (size_t)n_env * crit_blocks(img * img) * 4 * sizeof(double);
}

extern "C" int occ_seg_criterion(const float* pred, const float* target, int target_stride, int n_env, int img, double* sums,
                                 int64_t* counts, void* scratch, void* stream) {
    if (!crit_args_ok(pred, target, target_stride, n_env, img) || !sums || !scratch || ((uintptr_t)scratch & 7) != 0)
        return OCC_ERR_ARG;
    const int npix = img * img;
    hipStream_t st = (hipStream_t)stream;
    if (counts && hipMemsetAsync(counts, 0, (size_t)n_env * 3 * sizeof(int64_t), st) != hipSuccess) return OCC_ERR_LAUNCH;
    crit_launch(pred, target, target_stride, n_env, npix, (double*)scratch, (unsigned long long*)counts, st);
    hipLaunchKernelGGL(occ_seg_criterion_final_kernel, dim3((n_env * 4 + 63) / 64), dim3(64), 0, st, (const double*)scratch,
                       crit_blocks(npix), n_env, sums);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}

extern "C" int occ_seg_criterion_grad(const float* pred, const float* target, int target_stride, int n_env, int img, int mode,
                                      const double* coef, float* grad_pred, void* stream) {
    if (!crit_args_ok(pred, target, target_stride, n_env, img) || !coef || !grad_pred ||
        (mode != OCC_CRITERION_DICE && mode != OCC_CRITERION_BCE))
        return OCC_ERR_ARG;
    if (mode == OCC_CRITERION_BCE)
        crit_grad_launch<true>(pred, target, target_stride, n_env, img * img, coef, grad_pred, (hipStream_t)stream);
    else
        crit_grad_launch<false>(pred, target, target_stride, n_env, img * img, coef, grad_pred, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? OCC_OK : OCC_ERR_LAUNCH;
}
