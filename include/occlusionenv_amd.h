/*
 * occlusionenv_amd.h -- C ABI of the MI355X (gfx950) OcclusionEnv step() hot path.
 *
 * Drop-in boundary: these entry points replace, for a whole batch of N
 * environments at once, what /root/reference/environment.py does per environment through
 * PyTorch3D:
 *   - camera:   environment.py:356-368 (step), :308 (reset, look_at_view_transform),
 *               :334-335 (render)                                   -> occ_camera
 *   - renders:  silhouette_renderer(...) x3 + phong_renderer(...)   (environment.py:310,
 *               316-318, 370-372, 375) incl. MeshRasterizer.transform, clip_faces,
 *               _C.rasterize_meshes (K=100 soft / K=1 hard), SoftSilhouetteShader,
 *               HardFlatShader, observation packing (:376-378), occlusion image (:319,:373)
 *               and loss (:322,:381), plus d loss / d(elevation, azimuth) that the
 *               reference obtains from autograd + _C.rasterize_meshes_backward
 *                                                                   -> occ_render
 *   - reward bookkeeping environment.py:382-392 and the action Jacobian :356-361
 *                                                                   -> occ_step_finish
 *   - the operator-level replacement of _C.rasterize_meshes / _C.rasterize_meshes_backward (K-buffer in
 *     PyTorch3D layout, naive path)                                 -> occ_rasterize_meshes_naive,
 *                                                                      occ_rasterize_meshes_backward_dists
 *   - PyTorch3D sigmoid_alpha_blend on those K-buffers (SoftSilhouetteShader, environment.py:263)
 *                                                                   -> occ_sigmoid_alpha_blend_fwd / _bwd
 *   - SimpleVecEnv.step_wait's per-step host hand-off and auto-reset (SubProcVecEnv.py:209-218)
 *                                                                   -> occ_step_flags, occ_reset_commit,
 *                                                                      occ_auto_reset, occ_reserve_refill
 *   - the frozen FullNetwork / PredictorNet encoder whose pooled feature PPO.select_action stores (PPO.py:47,152-162,
 *     model.py:88-101,142-164), inference only                     -> occ_encoder_forward
 *   - the segmentation decoder of the same network (model.py:25-33,52-67,109-166: the predicted occlusion map, the third
 *     output of FullNetwork.forward / the output of Segmenter.forward), inference only, and the accuracy / IoU counts
 *     the pretrainer judges it by (pretrainer.py:127-141)          -> occ_segment_forward, occ_seg_metrics
 *     fine-tuning of that decoder with the encoder frozen (additive in ABI 12) -> occ_segment_train_forward, occ_segment_backward
 *   - the pretrainer's segmentation criterion on that map (pretrainer.py:89,127-141,176-189; loss.py:24-39
 *     BinaryDiceLoss, nn.BCELoss): the sums of both losses and the counts in one read, and the gradient with respect to the
 *     prediction                                                   -> occ_seg_criterion, occ_seg_criterion_grad
 *
 * Conventions: plain pointers and sizes only; every pointer is DEVICE memory owned by the
 * caller (PyTorch's ROCm allocator in the Python host); calls are asynchronous on `stream`
 * (a hipStream_t passed as void*; NULL = default stream); nothing is allocated, freed or
 * synchronised inside; return value 0 = launched OK, nonzero = bad arguments / launch failure
 * (see OCC_ERR_*).  Per-environment device-side status words report data-dependent failures
 * (OCC_STATUS_*).
 */
#ifndef OCCLUSIONENV_AMD_H
#define OCCLUSIONENV_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCC_ABI_VERSION 12

/* return codes */
#define OCC_OK 0
#define OCC_ERR_ARG 1    /* null pointer / bad size */
#define OCC_ERR_LAUNCH 2 /* hipLaunch failed (hipGetLastError != success) */

/* per-env status bits written by the kernels (0 = fine) */
#define OCC_STATUS_LIST_OVERFLOW 1 /* internal error: a pixel of a tile whose cost class rules it out held more than K candidates */
#define OCC_STATUS_REC_OVERFLOW 2  /* more visible (clipped) faces than record capacity */

/* layout constants shared with the host */
#define OCC_CAM_STRIDE 48  /* floats per env in the camera buffer */
#define OCC_REC_STRIDE 32  /* floats per projected-face record (eight 16-byte parts = one 128-byte line) */
#define OCC_TILE 8         /* image sides must be a multiple of this */
#define OCC_BLOCK 4        /* unit of OccWorkspace.objrect: 4x4-pixel blocks (a raster work item = 2x2 blocks = one 8x8 tile) */
#ifndef OCC_LOG_CAP
#define OCC_LOG_CAP 12288  /* candidate-log entries per persistent wave (20 B each); a log about to fill up is compacted
                              in place to every overflowing pixel's K nearest.  Must be >= 64*OCC_MAX_K + 2048 + 64 */
#endif
#define OCC_LOG_ENTRY_BYTES 30 /* (depth key u32, pixel | face sequence << 6 u32) + payload (1-p, p dd/del, p dd/daz) f32 x3
                                  + 8 + 2 B of the selection's compacted copy of the entries of the pixels that hold more than K
                                  (the entry again, and its index in the log) */
#define OCC_MAX_K 128      /* largest faces_per_pixel the fused path accepts */

/* occ_camera modes */
#define OCC_CAM_STEP 0     /* environment.py:356-368: action -> el/az += 0.05*n -> C -> look_at */
#define OCC_CAM_LOOKAT 1   /* environment.py:308: look_at_view_transform(radius, el, az)        */
#define OCC_CAM_POSITION 2 /* environment.py:334-335: look_at_rotation(camera_position)         */

/* OccScene.shader */
#define OCC_SHADER_FLAT 0
#define OCC_SHADER_HARD_PHONG 1
#define OCC_SHADER_SOFT_PHONG 2

/* occ_render flags */
#define OCC_RENDER_SOFT 1  /* three soft silhouettes + occlusion image + loss */
#define OCC_RENDER_HARD 2  /* flat-shaded RGB-D observation of the joined scene */
#define OCC_RENDER_GRAD 4  /* also d loss / d(el, az) (needs OCC_CAM_STEP tangents) */

/* GPU-resident mesh pool + per-env scene description (all device pointers). */
typedef struct OccScene {
    const float* pool_verts;      /* (sumV,3) */
    const int32_t* pool_faces;    /* (sumF,3) vertex ids local to their mesh */
    const int32_t* mesh_vert_off; /* (n_meshes+1) */
    const int32_t* mesh_face_off; /* (n_meshes+1) */
    const int32_t* scene_mesh;    /* (n_env,3) pool mesh id of object 1..3 (environment.py:193) */
    const float* scene_offset;    /* (n_env,3,3) world offset of each object (environment.py:148,171) */
    int32_t n_meshes;
    int32_t n_env;
    int32_t img;       /* S: image side in pixels, multiple of 8, <= 2048 */
    int32_t rec_cap;   /* fixed layout: record capacity of every (env, object), >= 2 x faces of the largest mesh;
                          variable layout (OccWorkspace.rec_off): upper bound of any object's span */
    /* optional per-face texture atlases (PyTorch3D TexturesAtlas, environment.py:127,152,175); NULL = all white */
    const float* pool_atlas;        /* packed (sum over textured meshes of F*R*R*3) */
    const int64_t* mesh_atlas_off;  /* (n_meshes) float offset of each mesh's atlas in pool_atlas, -1 = white vertices */
    int32_t atlas_res;              /* R */
    /* optional (n_env) int32: nonzero = do not render this scene row in this launch (its outputs are left
     * untouched, and in an occ_step launch so are its camera row, el / az, cam_pos_out and the OccStepFinish state);
     * used for reserve slots that are not under test (occ_auto_reset keeps it up to date) and for the envs an
     * evaluation has frozen (occ_episode_advance) */
    const int32_t* skip;
    /* optional (n_env,S,S) f32 weight of every pixel's term of the loss: loss = sum_p w_p * full_state[p,3]^2 and
     * its gradient likewise (NULL = 1 everywhere = environment.py:381).  Images are not affected.  Used to score a
     * region of interest, and by the parity tests to leave out pixels classified as exact ties. */
    const float* pix_weight;
    /* Shader of the RGB-D observation (environment.py:281-283): OCC_SHADER_FLAT = HardFlatShader (what the reference
     * runs), OCC_SHADER_HARD_PHONG / OCC_SHADER_SOFT_PHONG = the two alternatives it keeps commented out (per-pixel
     * Phong shading with interpolated vertex normals; soft = softmax_rgb_blend with default BlendParams).  The Phong
     * shaders need pool_vnormals (sumV,3): [P3D] Meshes.verts_normals_packed() of every pool mesh. */
    int32_t shader;
    const float* pool_vnormals;
    /* Largest vertex count of any pool mesh, a sizing hint: the setup kernel stages an object's (<= 4 096) world-space
     * vertices in LDS once instead of gathering three corners per face from global memory; larger objects, or 0 here,
     * keep the global gathers.  Results are identical either way. */
    int32_t max_mesh_verts;
} OccScene;

/* Caller-allocated scratch; sizes from occ_workspace_query(). */
typedef struct OccWorkspace {
    float* rec;         /* (n_env,3,rec_cap,OCC_REC_STRIDE) projected face records */
    uint32_t* rec_bbox; /* (n_env,3,rec_cap,4) scan rows of the objects occ_sort_kernel re-sorted front to back (4 096..8 192 records); untouched otherwise (until ABI v7: a per-record bbox row, written for every record) */
    uint32_t* scan;     /* (n_env,3,rec_cap,4) per record, in face order: pixel bbox xl|yl<<16, xh|yh<<16|corner-cut bits<<28 (img <= 2048), key of its nearest vertex depth, record index (the raster scan order unless re-sorted, see rec_bbox) */
    int32_t* nrec;      /* (n_env,3) */
    int32_t* objrect;   /* (n_env,3,4) block rect bx0,by0,bx1,by1 (inclusive, OCC_BLOCK-pixel units) */
    uint32_t* queue;    /* (8,32) one work-queue head per XCD group, a 128-B line each (zeroed by occ_render) */
    float* lists;       /* (n_slots, OCC_LOG_CAP*OCC_LOG_ENTRY_BYTES) per-wave K-buffer = wave-compacted candidate log:
                           OCC_LOG_CAP payloads of 12 B, then OCC_LOG_CAP (key, tag) pairs of 8 B (structure of arrays), then
                           OCC_LOG_CAP x (8 + 2) B for the exact top-K's compacted copy of the entries it has to rank */
    float* partials;    /* (n_env,ceil(S*S/256),4) per-block loss / gradient partial sums */
    int32_t* status;    /* (n_env) OCC_STATUS_* bits, OR-ed in; caller clears */
    int32_t* offsets;   /* (8*3*ceil(n_env/8)+1) rect order only (order == NULL): first work item of every (env, object), XCD-major */
    uint32_t* rec_cbox; /* (n_env,3,ceil(rec_cap/64),4) union pixel bbox + nearest depth key of every 64-entry scan chunk */
    float* obj_alpha;   /* (n_env,3,S,S) per-object silhouette alpha, valid inside the object's tile rect */
    float* obj_grad;    /* (n_env,3,S,S,2) d alpha / d(el, az) */
    float* obj_hz;      /* (n_env,3,S,S) depth of the nearest face of the object (3e38 = none) */
    int32_t* obj_hrec;  /* (n_env,3,S,S) its record index, -1 = none */
    int32_t n_slots;    /* persistent waves = blocks occ_raster2_kernel is launched with */
    /* Optional variable record layout: rec / rec_bbox / scan hold rec_total records in all and every (env, object)
     * gets room for ITS mesh (2 x faces, rounded up to 64) at record offset rec_off[env*3+obj]; rec_off
     * (3*n_env+1 int64) is filled by occ_render.  NULL = fixed stride rec_cap per (env, object). */
    int64_t* rec_off;
    int64_t rec_total;
    /* Optional work-item ORDER of occ_raster2_kernel (NULL = rect order): the tiles of all objects sorted by an
     * estimate of their cost (faces whose pixel bbox touches the tile), heaviest first inside every XCD queue, so
     * that the longest tiles start first and the launch does not end on a few stragglers.  u32 words:
     *   [0..8] first item of every XCD queue and the total, [16 + 32 q + c] tiles of cost class c in queue q,
     *   [512 + 32 (env*3+obj) + c] where the object's class-c tiles start inside the class,
     *   then (n_env,3,T) per tile: rank inside the object's class << 5 | class   (T = (S/8)^2 tiles per image),
     *   then (one pad word if needed for 8-byte alignment and) (n_env*3*T) items
     *   (env*3+obj, tile index inside the object's rect | class << 24), 8 B each.
     * occ_render zeroes the first 512 words. */
    uint32_t* order;
} OccWorkspace;

typedef struct OccWorkspaceSizes {
    size_t rec_bytes, rec_bbox_bytes, nrec_bytes, objrect_bytes, queue_bytes, lists_bytes,
        partials_bytes, status_bytes, offsets_bytes, obj_alpha_bytes, obj_grad_bytes, obj_hz_bytes,
        obj_hrec_bytes, rec_cbox_bytes, scan_bytes;
    int32_t n_slots; /* recommended persistent-wave count for this device */
    size_t rec_off_bytes;
    size_t order_bytes;
} OccWorkspaceSizes;

/*
 * Optional tail of a STEP launch: the reward bookkeeping of occ_step_finish (environment.py:381-392) done by the very
 * launch that reduces the loss (one dependent launch less per step).  Rows [0, n_step) are stepping envs; rows beyond
 * (reserve scenes riding along) only get their loss.
 */
typedef struct OccStepFinish {
    float* full_reward;       /* (n_step) in/out */
    const float* object_mass; /* (n_step) */
    float* reward;            /* (n_step) out */
    uint8_t* done;            /* (n_step) out, 0 / 1 */
    float* grad_action;       /* (n_step,2) out or NULL; needs OccRenderOut.grad_elaz */
    int32_t n_step;
} OccStepFinish;

/* Outputs of one batched render (device pointers; any may be NULL if the flag is off). */
typedef struct OccRenderOut {
    float* obs;        /* (n_env,4,S,S)  RGB + view-space depth, -1 background (environment.py:376-378) */
    float* full_state; /* (n_env,S,S,4)  i1*i2+i2*i3+i1*i3, RGB == 3 (environment.py:373) */
    float* alphas;     /* (n_env,3,S,S)  alpha channel of the three silhouettes */
    float* loss;       /* (n_env)        sum(full_state[...,3]^2) (environment.py:381) */
    float* grad_elaz;  /* (n_env,2)      d loss / d(elevation, azimuth) */
    /*
     * Optional REGION TRACKING of persistent output buffers (an output ring, the alphas state): three quarters of a
     * 128 x 128 frame are background, and a freshly allocated output has every one of those pixels written every step.
     * rect_prev (n_env,4) int32 pixel rects x0,y0,x1,y1 (inclusive; x1 < x0 = empty): the caller GUARANTEES that obs and
     * full_state of row e hold their background values (1,1,1,-1 / 3,3,3,0) everywhere outside rect_prev[e].  The
     * launch then writes only the 256-pixel blocks that meet this step's object rects or rect_prev[e] and stores this
     * step's union rect in rect_next[e] (skipped rows: rect_next = rect_prev).  NULL = every pixel is written.
     * arect_prev / arect_next: the same for alphas (background 0).  prev and next must be different arrays.
     */
    const int32_t* rect_prev;
    int32_t* rect_next;
    const int32_t* arect_prev;
    int32_t* arect_next;
    const OccStepFinish* finish; /* host pointer, read during the call; NULL = loss / gradient only */
} OccRenderOut;

/* Optional head of a STEP launch: the camera update of occ_camera done by the launch's prologue kernel (one dependent
 * launch less per step).  Arguments as occ_camera; cam_pos_out2 (n,3): a second copy of C (the step's info["position"]
 * snapshot) or NULL. */
typedef struct OccCameraArgs {
    int32_t mode;
    const float* action;
    float* el;
    float* az;
    const float* radius;
    float* cam_pos_out;
    float* cam_pos_out2;
    int32_t n;
} OccCameraArgs;

int occ_abi_version(void);

/* number of CUs of the current device (used to size n_slots); <=0 on failure. Host-side query only. */
int occ_device_cu_count(void);

int occ_workspace_query(const OccScene* scene, int n_slots, OccWorkspaceSizes* out);

/* Sizes of the record arrays (rec, rec_bbox, scan, rec_cbox, rec_off) of a variable-layout workspace holding
 * rec_total records for n_env scenes; the other fields of *inout are left as occ_workspace_query set them. */
int occ_record_sizes(int64_t rec_total, int n_env, OccWorkspaceSizes* inout);

/*
 * Camera for N envs.  cam: (N,OCC_CAM_STRIDE) floats =
 *   [0..8] R row-major, [9..11] T, [12..14] C, [15..23] dR/d el, [24..26] dT/d el,
 *   [27..35] dR/d az, [36..38] dT/d az, [39..42] d(el,az)/d(action) row-major, [43] el, [44] az.
 * OCC_CAM_STEP:     action (N,2); el, az (N) updated IN PLACE (environment.py:360-361); radius (N).
 * OCC_CAM_LOOKAT:   el, az, radius (N) read; action ignored.
 * OCC_CAM_POSITION: action points to camera positions (N,3); el, az, radius ignored.
 * cam_pos_out (N,3) receives C when non-NULL (environment.py:363-365).
 */
int occ_camera(int mode, const float* action, float* el, float* az, const float* radius,
               float* cam, float* cam_pos_out, int n_env, void* stream);

/* Projection + z-clipping + culling + ordered face-record build, per-(env, object, tile) rasterisation
 * (soft silhouette + nearest hard face), per-pixel combine (occlusion image, shading, loss and forward-mode
 * gradient) and the per-env reduction, for all envs. */
int occ_render(const OccScene* scene, const float* cam, const OccWorkspace* ws,
               const OccRenderOut* out, int flags, int faces_per_pixel, void* stream);

/* occ_render with the step's camera update folded into its prologue launch: rows [0, camera->n) of cam are written
 * from (action, el, az, radius) first (OccCameraArgs; NULL = cam is ready, exactly occ_render).  Together with
 * OccRenderOut.finish this is the whole of OcclusionEnv.step() (environment.py:352-396) for N envs in one call. */
int occ_step(const OccScene* scene, const OccCameraArgs* camera, float* cam, const OccWorkspace* ws,
             const OccRenderOut* out, int flags, int faces_per_pixel, void* stream);

/*
 * Reward bookkeeping of step() (environment.py:381-392) for N envs:
 *   reward = (full_reward - loss)/object_mass + (5 if loss < 0.1 else -0.2); full_reward <- loss;
 *   done = loss < 0.1;  grad_action = -(1/object_mass) * J^T grad_elaz  (d reward / d action).
 */
int occ_step_finish(const float* loss, const float* grad_elaz, const float* cam,
                    float* full_reward, const float* object_mass, float* reward, uint8_t* done,
                    float* grad_action, int n_env, void* stream);

/*
 * Operator-level drop-in for PyTorch3D's `_C.rasterize_meshes` (naive path, bin_size = 0) and the `dists` part of
 * `_C.rasterize_meshes_backward` - the ops environment.py reaches through MeshRasterizer (:258-262, :276-280;
 * signatures in SURVEY.md §8b).  face_verts (F,3,3) = (x_ndc, y_ndc, z_view) AFTER clip_faces; outputs in
 * PyTorch3D's layout: pix_to_face (N,H,W,K) int64 (packed face index, -1 empty), zbuf, dists (N,H,W,K),
 * bary (N,H,W,K,3), slots ascending in (z, face).  Built for exactness (reference arithmetic order, no FMA
 * contraction), not speed: the fused occ_render never materialises these buffers.
 * grad_face_verts (F,3,3) is overwritten; the dists entry point gives x,y their gradient (zbuf / bary gradients - zero on the
 * OcclusionEnv path - come from occ_rasterize_meshes_backward below).
 */
int occ_rasterize_meshes_naive(const float* face_verts, const int64_t* mesh_to_face_first_idx,
                               const int64_t* num_faces_per_mesh, const int64_t* clipped_faces_neighbor_idx,
                               int n_meshes, int H, int W, float blur_radius, int faces_per_pixel,
                               int perspective_correct, int clip_barycentric_coords, int cull_backfaces,
                               int64_t* pix_to_face, float* zbuf, float* bary, float* dists, void* stream);
/*
 * The same K-buffers, bit for bit, from a tiled kernel: one wave per (mesh, tile) looks only at the faces whose
 * bbox +- sqrt(blur) can reach a pixel centre of the tile and keeps the (depth, face) lists in LDS (F / faces-per-tile
 * times less evaluation work than the naive kernel; the producer callers of MeshRasterizer should use).  For a mesh
 * without clipped-face pairs (clipped_faces_neighbor_idx == NULL, or -1 for every face of the mesh: found out on the
 * device, mesh by mesh) a pixel's K-buffer is the K smallest (depth, face) of its candidates whatever their arrival order:
 * 4x4-pixel tiles, four faces in flight per wave, four partial lists per pixel merged by rank at the end (round 4:
 * 10.6 -> 1.2 ms for a 5 120-face mesh at 128x128, K = 100; the teapot at 256x256 1.06 -> 0.22 ms).  A mesh with pairs:
 * 8x8 tiles, faces in order.  Same arguments; faces_per_pixel above 128 (64 KiB of lists) is served by the naive kernel.
 */
int occ_rasterize_meshes_tiled(const float* face_verts, const int64_t* mesh_to_face_first_idx,
                               const int64_t* num_faces_per_mesh, const int64_t* clipped_faces_neighbor_idx,
                               int n_meshes, int H, int W, float blur_radius, int faces_per_pixel,
                               int perspective_correct, int clip_barycentric_coords, int cull_backfaces,
                               int64_t* pix_to_face, float* zbuf, float* bary, float* dists, void* stream);
int occ_rasterize_meshes_backward_dists(const float* face_verts, const int64_t* pix_to_face, const float* grad_dists,
                                        int64_t n_faces, int n_meshes, int H, int W, int faces_per_pixel,
                                        int perspective_correct, int clip_barycentric_coords, float* grad_face_verts,
                                        void* stream);

/*
 * The whole of `_C.rasterize_meshes_backward`: grad_face_verts (F,3,3), overwritten, from any of grad_zbuf (N,H,W,K),
 * grad_bary (N,H,W,K,3), grad_dists (N,H,W,K) - NULL = that output carries no gradient.  The dists part is
 * occ_rasterize_meshes_backward_dists; zbuf / bary gradients (zero on the OcclusionEnv path) differentiate the
 * area-normalised, perspective-corrected, clipped barycentrics and the depth they interpolate.
 */
int occ_rasterize_meshes_backward(const float* face_verts, const int64_t* pix_to_face, const float* grad_zbuf,
                                  const float* grad_bary, const float* grad_dists, int64_t n_faces, int n_meshes, int H, int W,
                                  int faces_per_pixel, int perspective_correct, int clip_barycentric_coords,
                                  float* grad_face_verts, void* stream);

/*
 * [P3D] sigmoid_alpha_blend (SoftSilhouetteShader, environment.py:263) on K-buffers in PyTorch3D layout:
 *   alpha[p] = 1 - prod_k (1 - sigmoid(-dists[p,k] / sigma) * [pix_to_face[p,k] >= 0]),   images (n_pix,4) RGBA, RGB = 1.
 * Backward: grad_dists[p,k] from grad_images (only the alpha channel carries gradient).
 */
int occ_sigmoid_alpha_blend_fwd(const float* dists, const int64_t* pix_to_face, int64_t n_pix, int faces_per_pixel,
                                float sigma, float* images, void* stream);
int occ_sigmoid_alpha_blend_bwd(const float* dists, const int64_t* pix_to_face, const float* grad_images, int64_t n_pix,
                                int faces_per_pixel, float sigma, float* grad_dists, void* stream);

/*
 * The K epochs of PPO.update (PPO.py:196-217) for the heads-only learner of the vectorised env: the reference optimises
 * action_head (256 -> 2) and value_head (256 -> 1) only (PPO.py:113-116; model.py:153-154,168-171 detaches the features),
 * with the fixed diagonal Gaussian of ActorCritic (PPO.py:62-104) and torch.optim.Adam.  ONE launch per epoch: forward,
 * clipped-surrogate loss, backward and the Adam step over the 771 parameters; parameters, moments and step count are
 * updated in place.  feats (M,256), actions (M,2), old_logprob (M), returns (M) [already normalised, PPO.py:187-188];
 * losses (n_epochs,2) receives (total loss, value loss) of every epoch; scratch: OCC_PPO_SCRATCH_FLOATS floats;
 * counter: one zeroed uint32 (left at zero).  Adam moments m, v: 771 floats each in the order W_a | b_a | W_v | b_v.
 */
#define OCC_PPO_FEATURES 256
#define OCC_PPO_PARAMS (3 * OCC_PPO_FEATURES + 3)
#ifndef OCC_PPO_MAX_BLOCKS
#define OCC_PPO_MAX_BLOCKS 128
#endif
#define OCC_PPO_SCRATCH_FLOATS (OCC_PPO_MAX_BLOCKS * (OCC_PPO_PARAMS + 2))
typedef struct OccPpoState {
    float *w_a, *b_a, *w_v, *b_v; /* action_head.weight (2,256), .bias (2), value_head.weight (1,256), .bias (1) */
    float *adam_m, *adam_v;       /* OCC_PPO_PARAMS each */
    float* adam_step;             /* (1) step count as float (torch's capturable Adam keeps it on the device too) */
} OccPpoState;
/* The block cap this library was built with (OCC_PPO_MAX_BLOCKS): scratch must hold occ_ppo_max_blocks() * (OCC_PPO_PARAMS + 2) floats. */
int occ_ppo_max_blocks(void);
int occ_ppo_update(const float* feats, const float* actions, const float* old_logprob, const float* returns, int64_t M,
                   float action_var, float eps_clip, float lr_actor, float lr_critic, float beta1, float beta2,
                   float adam_eps, const OccPpoState* state, int n_epochs, float* losses, float* scratch,
                   uint32_t* counter, void* stream);

/*
 * The rollout record's 256 features (PPO.py:155-158 stores the frozen encoder's pooled feature of the acting state; the
 * network itself is outside this path): 4 channels x 8 x 8 average pooling of the observation, obs (n,4,img,img) ->
 * feats (n,256) in the order of adaptive_avg_pool2d(obs, 8).reshape(n, 256).  img: a multiple of 8.
 */
int occ_pool8(const float* obs, int64_t n, int img, float* feats, void* stream);

/*
 * Frozen encoder (model.py:8-101, eval mode): Encoder(ch=8, levels=5, layers=2, k=3, dilation, bias=True, residual,
 * separable) on obs (n_env,4,S,S) f32 -> feats (n_env,256) = AdaptiveAvgPool2d(1) of the last down output.  The skip
 * outputs and the decoder are not computed.  Layers: initial Conv(4 -> 8, dilation 1); per level i (c = 8 * 2^i) Layer 1
 * and Layer 2 Conv(c -> c, dilation), y = Layer2(Layer1(x)) (+ x if residual), down = dense 3x3 stride-2 Conv(c -> 2c,
 * dilation 1).  Every Conv is bn(relu(conv(x))) with BN folded to a per-channel affine: scale = gamma / sqrt(var + 1e-5),
 * shift = beta - mean * scale.  Spatial sizes halve with ceiling at every down (100 -> 50 -> 25 -> 13 -> 7 -> 4).
 * f32 arithmetic with f32 accumulation; no atomics (features are bitwise independent of n_env and of an env's position);
 * 17 launches on `stream`, nothing allocated or synchronised (capturable).
 *
 * Packed weights (occ_encoder_packed_floats floats), layers in the order initial, then per level Layer 1, Layer 2, down;
 * per layer, in the order the kernels read them:
 *   separable Conv(cin -> cout):  dw_v[cin][3] (the (3,1) depthwise taps, top to bottom) | dw_h[cin][3] (the (1,3) taps,
 *                                 left to right) | pw[cin][cout] (pointwise weight, TRANSPOSED) | bias[cout] |
 *                                 bn_scale[cout] | bn_shift[cout]
 *   dense Conv(cin -> cout):      w[cin][ky * 3 + kx][cout] (TRANSPOSED conv weight) | bias[cout] | bn_scale[cout] |
 *                                 bn_shift[cout]
 * The down convs are always dense; `separable` selects the form of the initial layer and of Layers 1 and 2.
 */
#define OCC_ENCODER_FEATURES 256
typedef struct OccEncoderConfig {
    int32_t img;       /* S, in [32, 1024] */
    int32_t dilation;  /* 1 or 2: dilation of Layers 1 and 2 (padding = dilation) */
    int32_t residual;  /* 0 / 1: ConvBlock.residual */
    int32_t separable; /* 0 / 1 */
} OccEncoderConfig;
/* Floats of the packed weight buffer for cfg->separable (independent of the other fields); -1 for a bad config. */
int64_t occ_encoder_packed_floats(const OccEncoderConfig* cfg);
/* Device workspace bytes occ_encoder_forward needs for n_env envs: three (n_env,8,S,S) f32 activation buffers and the
 * per-tile partials of the pooled feature. */
int occ_encoder_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* bytes);
/* n_env in [1, 65535]; ws of at least the queried bytes (256-byte aligned). */
int occ_encoder_forward(const OccEncoderConfig* cfg, const float* packed_weights, const float* obs, int n_env, void* ws,
                        size_t ws_bytes, float* feats, void* stream);
/*
 * occ_encoder_forward with a per-env skip mask (additive in ABI 12).  skip: device memory of n_env int32, read by the
 * kernels when they run (a captured call follows the values it finds at replay); NULL is occ_encoder_forward itself, and
 * occ_encoder_forward is this call with NULL.  An env with skip[env] != 0 is left alone, as OccScene.skip leaves it alone in
 * the engine: none of its blocks reads obs or writes anything, and its feats row KEEPS the bits it held before the call.
 * What the workspace holds for a skipped env afterwards is unspecified and is never read.  Every other env's row is
 * bitwise what the unmasked call writes.  Same 17 launches on the same grids (sized by n_env: the host needs no count of
 * the active envs); a skipped env costs its blocks' dispatch, not their work.  Workspace: occ_encoder_workspace_query.
 */
int occ_encoder_forward_masked(const OccEncoderConfig* cfg, const float* packed_weights, const float* obs, int n_env, void* ws,
                               size_t ws_bytes, float* feats, const int32_t* skip, void* stream);

/*
 * bf16 inference mode of the SEPARABLE encoder (additive in ABI 12; cfg->separable must be 1, any dilation / residual / S the
 * f32 path takes).  The same network, the same 17 launches, the same skip mask; what differs is where values are rounded
 * (always to nearest even, to bfloat16):
 *   - contraction operands: the depthwise pair's result (formed in f32, then rounded), the pointwise weights and the dense
 *     down weights; the contractions of 16 input channels and more run on v_mfma_f32_32x32x16_bf16, f32 accumulation;
 *   - stored activations: relu(conv) * bn_scale + bn_shift (+ the residual, read back as bf16, added in f32) is rounded once
 *     when stored.  The last down is not stored: the pooled feature is summed from its unrounded f32 values in a fixed order.
 * The observation, the depthwise taps, biases, BN scale / shift, every accumulator and epilogue, the pool partials and
 * feats are f32.  No atomics: feats are bitwise independent of n_env, of an env's position and of repeat calls.  The
 * activations are kept channel-last, (n, H, W, c) bf16.
 *
 * Packed buffer (occ_encoder_bf16_packed_bytes bytes; occ_encoder_bf16_pack makes it from the f32 buffer of
 * occ_encoder_packed_floats, on the host): the layers in the f32 order, each 16-byte aligned:
 *   cin <= 8 (initial, level 0's Layer 1, Layer 2 and down): the f32 layout above, float for float, with every pw[][] / w[][][]
 *     entry replaced by its bf16 rounding widened back to f32 (the low 16 bits are zero).
 *   separable Conv(c -> c), c >= 16:  dw[c / 8][6][8] f32: per group of 8 channels the taps v0 v1 v2 h0 h1 h2, each for the
 *     group's 8 channels | F[c / 16][max(c, 32) / 32][64][8] bf16 | bias[c] | bn_scale[c] | bn_shift[c] f32
 *   down Conv(c -> 2c), c >= 16:      F[9 c / 16][2c / 32][64][8] bf16 | bias[2c] | bn_scale[2c] | bn_shift[2c] f32
 * F[kb][ct][lane][j] is the MFMA A fragment of k-step kb and weight tile ct: the weight of contraction index
 * k = 16 kb + 8 (lane >> 5) + j and output channel co = 32 ct + 16 ((m >> 2) & 1) + 4 (m >> 3) + (m & 3), m = lane & 31
 * (zero where co >= cout: c = 16 fills half a tile).  Separable: k is the input channel, the weight pw[k][co].  Down:
 * k = tap * c + ci, tap = ky * 3 + kx, the weight w[ci][tap][co].  Weights are rounded in integer arithmetic; all f32
 * parts are copied bit for bit.
 */
/* Bytes of the bf16 packed buffer; -1 unless cfg->separable == 1. */
int64_t occ_encoder_bf16_packed_bytes(const OccEncoderConfig* cfg);
/* Host only, no device call: packed_f32 (occ_encoder_packed_floats floats, host memory) -> out (occ_encoder_bf16_packed_bytes
 * bytes, host memory).  OCC_ERR_ARG unless cfg->separable == 1. */
int occ_encoder_bf16_pack(const OccEncoderConfig* cfg, const float* packed_f32, void* out);
/* Device workspace bytes of occ_encoder_forward_bf16: three (n_env,S,S,8) bf16 activation buffers and the f32 per-tile
 * partials (n_env, ceil(S_5 / 8)^2, 256), S_5 the side after five downs; each part rounded up to 256 bytes. */
int occ_encoder_bf16_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* bytes);
/* As occ_encoder_forward_masked (skip may be NULL) on the bf16 packed buffer (device memory, 16-byte aligned, as ws);
 * cfg->separable == 0 is OCC_ERR_ARG before any launch.  Nothing allocated or synchronised (capturable). */
int occ_encoder_forward_bf16(const OccEncoderConfig* cfg, const void* packed_bf16, const float* obs, int n_env, void* ws,
                             size_t ws_bytes, float* feats, const int32_t* skip, void* stream);

/*
 * Segmentation decoder (model.py:109-125 on top of the encoder above, eval mode): x = the last down output
 * (n_env,256,S/32,S/32); for j = 0..4, c = 128, 64, 32, 16, 8: x = up_j(x) + skip, where up_j = TrConv(2c -> c) =
 * bn(relu(ConvTranspose2d(2c, c, 3, stride 2, padding 1, output_padding 1))) (BN folded as above) and skip is the
 * encoder's feature of level 4 - j: Layer 2's output plus the residual when cfg->residual, the tensor the down conv reads.
 * Then logit = Conv2d(8, 1, 1)(x), prob = sigmoid(logit), both (n_env,1,S,S).  TrConvBlock.forward returns self.up(x)
 * (model.py:63-67): the `net` layers of the decoder blocks have no effect on the output, are not run and are not packed.
 * The skip add needs S % 32 == 0 (so does the reference).
 *
 * Packed decoder (occ_decoder_packed_floats floats): per up layer j, in decoder order,
 *   w[ci][ky * 3 + kx][co] (ConvTranspose2d weight (2c, c, 3, 3) with co moved last) | bias[c] | bn_scale[c] | bn_shift[c]
 * then the classifier: cls_w[8] | cls_b[1].
 *
 * occ_segment_forward runs the encoder (the same 17 launches on the same values: feats is bitwise what
 * occ_encoder_forward writes) keeping the five skip tensors and the last down output, then 5 decoder launches; the
 * classifier and the sigmoid are fused into the last.  22 launches on `stream`, nothing allocated or synchronised.
 * Workspace: two (n_env,8,S,S) activation buffers, the skips (1.94 such buffers), the last down output and the pool
 * partials: 3.97 buffers against the encoder's 3, i.e. 7.94 MiB per env at 256^2 and 31.75 MiB per env at 512^2
 * (256 envs x 256^2 or 64 envs x 512^2: 1.98 GiB).
 */
/* Floats of the packed decoder (the same for every valid cfg); -1 for a null cfg or a bad `separable`. */
int64_t occ_decoder_packed_floats(const OccEncoderConfig* cfg);
/* As occ_encoder_workspace_query; additionally cfg->img % 32 must be 0. */
int occ_segment_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* bytes);
/* feats (n_env,256) and prob (n_env,1,S,S) are required; logit (n_env,1,S,S) and dec_feat (n_env,8,S,S), the input of the
 * classifier, may be NULL and are then not stored.  Map pointers 8-byte aligned.  OCC_ERR_ARG before any launch for a null
 * required pointer, cfg->img % 32 != 0, n_env outside [1, 65535] or a short workspace. */
int occ_segment_forward(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed, const float* obs,
                        int n_env, void* ws, size_t ws_bytes, float* feats, float* prob, float* logit, float* dec_feat,
                        void* stream);
/*
 * occ_segment_forward with the skip mask of occ_encoder_forward_masked (additive in ABI 12; NULL is occ_segment_forward
 * itself).  An env with skip[env] != 0 keeps the bits of its rows of feats, prob, logit and dec_feat; its part of the
 * workspace (activations, skip tensors, partials) is unspecified and never read.  Every other env's rows are bitwise what
 * the unmasked call writes.  Same 22 launches; workspace: occ_segment_workspace_query.
 */
int occ_segment_forward_masked(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed, const float* obs,
                               int n_env, void* ws, size_t ws_bytes, float* feats, float* prob, float* logit, float* dec_feat,
                               const int32_t* skip, void* stream);
/*
 * Training of the decoder and the classifier with the encoder frozen (additive in ABI 12; csrc/occ_decoder_bwd.hpp).  The
 * decoder's BatchNorm runs with its running statistics, as in inference: with u = convT(x_j) + bias, r = relu(u),
 * y_j = bn_scale r + bn_shift + skip, the parameters that receive a gradient are w, bias, bn_scale, bn_shift of every up
 * layer and cls_w, cls_b.  Neither d obs, d skip nor any encoder gradient is computed here (occ_fullnet_backward below
 * joins this backward with the encoder's).
 *
 * occ_segment_train_forward is occ_segment_forward (feats and prob are the same to the bit) that keeps, in ws, every level's
 * input x_j, its relu output r_j, the decoder feature y_4 and prob.  Workspace, every part 256-byte aligned: the
 * workspace of occ_segment_forward (occ_segment_workspace_query bytes), then for j = 0..4 y_j | r_j, each
 * (n_env, 128 >> j, S/16 << j, S/16 << j) f32, then prob (n_env,S,S), then two gradient buffers of the sizes of y_4 and y_3.
 *
 * occ_segment_backward is the backward of the LATEST occ_segment_train_forward on ws (same cfg, n_env and dec_packed) for the
 * upstream gradient grad_prob = d loss / d prob (n_env,1,S,S) f32, 16-byte aligned.  grad_packed receives
 * occ_decoder_packed_floats floats in the layout of dec_packed: per level dw[ci][ky * 3 + kx][co] | dbias | dbn_scale |
 * dbn_shift, then dcls_w[8] | dcls_b; it is OVERWRITTEN, not accumulated.  The relu gate is the forward's own r > 0.
 * scratch: device memory of the queried scratch_bytes (16-byte aligned; block partials).  No floating-point atomics; block
 * partials are added in a fixed order in f64: every gradient is bitwise the same from call to call.  24 launches on
 * `stream`, nothing allocated or synchronised.  OCC_ERR_ARG before any launch for a null pointer, cfg->img % 32 != 0, n_env
 * outside [1, 65535], a misaligned or a short buffer.
 */
int occ_segment_train_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* ws_bytes, size_t* scratch_bytes);
int occ_segment_train_forward(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed, const float* obs,
                              int n_env, void* ws, size_t ws_bytes, float* feats, float* prob, void* stream);
int occ_segment_backward(const OccEncoderConfig* cfg, const float* dec_packed, int n_env, void* ws, size_t ws_bytes,
                         const float* grad_prob, void* scratch, size_t scratch_bytes, float* grad_packed, void* stream);

/*
 * Training of the dense encoder through its pooled feature (additive in ABI 12; csrc/occ_encoder_bwd.hpp): what
 * PredictorNet training (train_predict.py) needs below its Linear(256, 2) head.  Supported: cfg->separable == 0 and
 * cfg->dilation == 1, cfg->residual 0 or 1, img in [32, 1024] (odd intermediate sides included: they halve with ceiling).
 * BatchNorm runs with its running statistics: with u = conv(x) + bias, r = relu(u), y = bn_scale r + bn_shift (+ residual),
 * the parameters that receive a gradient are w, bias, bn_scale, bn_shift of all 16 layers.  No d obs is computed.
 *
 * occ_encoder_train_forward is occ_encoder_forward (feats are the same to the bit) that keeps, in ws, every layer's input
 * and relu output r.  Workspace, every part 256-byte aligned, f32, H_0 = S, H' = ceil(H / 2), c = 8 << lv:
 *   obs (n,4,S,S) | r_init (n,8,S,S) | per level lv = 0..4: a (n,c,H,H) | r1 | b | r2 | cc | rd (n,2c,H',H') |
 *   pool partials (n, tiles of the last down, 256) | three gradient buffers of (n,8,S,S)
 * (a: the block input = the previous down's output; b: Layer 1's output; cc: Layer 2's output plus the residual).
 * 30.31 MiB per env at 256^2 (128 envs: 3.79 GiB), 121.25 MiB per env at 512^2.  18 launches.
 *
 * occ_encoder_backward is the backward of the LATEST occ_encoder_train_forward on ws (same cfg, n_env and packed) for the
 * upstream gradient grad_feats = d loss / d feats (n_env,256) f32.  grad_packed receives occ_encoder_packed_floats floats
 * in the layout of packed: per layer dw[ci][ky * 3 + kx][co] | dbias | dbn_scale | dbn_shift; it is OVERWRITTEN, not
 * accumulated.  The relu gate is the forward's own r > 0.  scratch: device memory of the queried scratch_bytes (block
 * partials).  No floating-point atomics; block partials are added in a fixed order in f64: every gradient is bitwise the
 * same from call to call.  79 launches on `stream`, nothing allocated or synchronised.  OCC_ERR_ARG before any launch for
 * an unsupported cfg, a null pointer, n_env outside [1, 65535], ws or scratch not 16-byte aligned, or a short buffer.
 */
int occ_encoder_train_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* ws_bytes, size_t* scratch_bytes);
int occ_encoder_train_forward(const OccEncoderConfig* cfg, const float* packed, const float* obs, int n_env, void* ws,
                              size_t ws_bytes, float* feats, void* stream);
int occ_encoder_backward(const OccEncoderConfig* cfg, const float* packed, int n_env, void* ws, size_t ws_bytes,
                         const float* grad_feats, void* scratch, size_t scratch_bytes, float* grad_packed, void* stream);

/*
 * Training of the separable encoder through its pooled feature (additive in ABI 12; csrc/occ_sepenc_bwd.hpp): the
 * counterpart of the three entry points above for cfg->separable == 1, what training FullNetwork(8, dilation=2,
 * separable=True)'s encoder (PPO.py:47) or PredictorNet(8, separable=True) (pred_train.py:35) needs below the Linear(256, 2)
 * head.  Supported: cfg->separable == 1, cfg->dilation 1 or 2, cfg->residual 0 or 1, img in [32, 1024] (odd intermediate
 * sides included), n_env in [1, 65535].  A separable layer (initial at dilation 1; Layer 1 and Layer 2 of every level at
 * cfg->dilation) computes h = dw_h(dw_v(x)), u = pw h + bias, r = relu(u), y = bn_scale r + bn_shift (+ residual); the downs
 * are dense stride-2 convs at dilation 1.  BatchNorm runs with its running statistics.  The parameters that receive a
 * gradient are wv, wh, pw, bias, bn_scale, bn_shift of the 11 separable layers and w, bias, bn_scale, bn_shift of the 5
 * downs.  No d obs is computed.
 *
 * occ_sep_encoder_train_forward is occ_encoder_forward (feats are the same to the bit) that keeps, in ws, every layer's
 * input and relu output r.  The workspace is that of occ_encoder_train_workspace_query, part by part (the same tensors
 * are kept; h is rebuilt from x in the backward): every part 256-byte aligned, f32, H_0 = S, H' = ceil(H / 2), c = 8 << lv:
 *   obs (n,4,S,S) | r_init (n,8,S,S) | per level lv = 0..4: a (n,c,H,H) | r1 | b | r2 | cc | rd (n,2c,H',H') |
 *   pool partials (n, tiles of the last down, 256) | three gradient buffers g0 | g1 | g2 of (n,8,S,S)
 * 30.31 MiB per env at 256^2, 121.25 MiB per env at 512^2.  18 launches.
 *
 * occ_sep_encoder_backward is the backward of the LATEST occ_sep_encoder_train_forward on ws (same cfg, n_env and packed)
 * for grad_feats = d loss / d feats (n_env,256) f32.  packed and grad_packed use the separable layout of
 * occ_encoder_packed_floats (separable = 1): per separable layer dwv[ci][3] | dwh[ci][3] | dpw[ci][co] | dbias | dbn_scale
 * | dbn_shift, per down dw[ci][ky * 3 + kx][co] | dbias | dbn_scale | dbn_shift; grad_packed is OVERWRITTEN, not
 * accumulated.  The relu gate is the forward's own r > 0.  Within a level the gradient buffers rotate: the down's dY / dU
 * and then dH = pw^T dU of both layers in one, the dY of Layer 2's output (kept for the residual) in the second, Layer 2's
 * dU, Layer 1's dY / dU and the block input's gradient in the third.  scratch: device memory of the queried scratch_bytes:
 * the largest, over the layers, of the activation step's f64 block partials, the partial weight gradients of the K split
 * (pointwise: at most 1024 blocks per layer) and the f64 block partials of the nine depthwise correlation sums per input
 * channel.  No floating-point atomics; block partials are added in a fixed order in f64: every gradient is bitwise the same
 * from call to call.  112 launches on `stream`, nothing allocated or synchronised.  OCC_ERR_ARG before any launch for an
 * unsupported cfg (separable == 0 included), a null pointer, n_env outside [1, 65535], ws or scratch not 16-byte aligned,
 * or a short buffer.
 */
int occ_sep_encoder_train_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* ws_bytes, size_t* scratch_bytes);
int occ_sep_encoder_train_forward(const OccEncoderConfig* cfg, const float* packed, const float* obs, int n_env, void* ws,
                                  size_t ws_bytes, float* feats, void* stream);
int occ_sep_encoder_backward(const OccEncoderConfig* cfg, const float* packed, int n_env, void* ws, size_t ws_bytes,
                             const float* grad_feats, void* scratch, size_t scratch_bytes, float* grad_packed, void* stream);

/*
 * Joint training of the dense encoder, the decoder and the classifier (additive in ABI 12; csrc/occ_fullnet_bwd.hpp): one
 * step of pretrainer.py below its losses, for two upstream gradients at once.  Supported: cfg->separable == 0,
 * cfg->dilation == 1, cfg->residual 0 or 1, cfg->img % 32 == 0 in [32, 1024].  BatchNorm runs with its running statistics
 * in all 21 layers; the parameters that receive a gradient are those of occ_encoder_backward and of occ_segment_backward.
 * No d obs is computed.
 *
 * occ_fullnet_train_forward runs the encoder ONCE, as occ_encoder_train_forward does, with the last down also storing its
 * output, then the five up layers of occ_segment_train_forward on that output and on the level tensors cc (the skips, not
 * copied).  feats is bitwise what occ_encoder_forward writes, prob (8-byte aligned) what occ_segment_forward writes.
 * Workspace, every part 256-byte aligned, f32:
 *   the workspace of occ_encoder_train_forward, three gradient buffers g0 | g1 | g2 included |
 *   last (n,256,S/32,S/32) | for j = 0..4: y_j | r_j, each (n, 128 >> j, S/16 << j, S/16 << j) | prob (n,S,S) |
 *   dlast (n,256,S/32,S/32) | dskip_lv for lv = 1..4, (n, 8 << lv, S >> lv, S >> lv)
 * 23 launches.
 *
 * occ_fullnet_backward is the backward of the LATEST occ_fullnet_train_forward on ws (same cfg, n_env and packed buffers)
 * for grad_feats = d loss / d feats (n_env,256) and grad_prob = d loss / d prob (n_env,1,S,S; 16-byte aligned), both
 * required (zeros for an absent one).  The decoder runs first, the full-resolution level first, then the encoder, the
 * deepest level first.  Every decoder level's dY is the d skip of an encoder level: for lv >= 1 it is kept in dskip_lv (the
 * decoder's activation step writes dU to g0 instead of over dY) and added in the epilogue of the encoder's stride-2 input
 * gradient; for lv = 0 it is not stored but rebuilt there as grad_prob p (1 - p) cls_w[c] (0.94 buffers of (n,8,S,S) kept
 * instead of 1.94).  The deepest decoder level's input gradient goes to dlast and is added to grad_feats / (H H) in the
 * last down's activation step.  No join is a launch of its own.  grad_enc_packed (occ_encoder_packed_floats floats) and
 * grad_dec_packed (occ_decoder_packed_floats floats) are OVERWRITTEN, not accumulated, in the layouts of enc_packed and
 * dec_packed.  scratch: the queried scratch_bytes (16-byte aligned), the larger of the two single passes' scratch.  No
 * floating-point atomics; block partials are added in a fixed order in f64: every gradient is bitwise the same from call
 * to call, grad_dec_packed is bitwise what occ_segment_backward gives for the same grad_prob, and with grad_prob = 0
 * grad_enc_packed equals what occ_encoder_backward gives.  104 launches (decoder 25, encoder 79) on `stream`, nothing
 * allocated or synchronised.  OCC_ERR_ARG before any launch for an unsupported cfg, a null pointer, n_env outside
 * [1, 65535], a misaligned or a short buffer.
 */
int occ_fullnet_train_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* ws_bytes, size_t* scratch_bytes);
int occ_fullnet_train_forward(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed, const float* obs,
                              int n_env, void* ws, size_t ws_bytes, float* feats, float* prob, void* stream);
int occ_fullnet_backward(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed, int n_env, void* ws,
                         size_t ws_bytes, const float* grad_feats, const float* grad_prob, void* scratch, size_t scratch_bytes,
                         float* grad_enc_packed, float* grad_dec_packed, void* stream);

/*
 * Joint training of the SEPARABLE encoder, the decoder and the classifier (additive in ABI 12; csrc/occ_fullnet_bwd.hpp):
 * the three entry points above for cfg->separable == 1, the step that pretrains FullNetwork(8, dilation=2, separable=True)
 * (PPO.py:47; pretrainer.py --separable --dilation 2).  Supported: cfg->separable == 1, cfg->dilation 1 or 2, cfg->residual
 * 0 or 1, cfg->img % 32 == 0 in [32, 1024], n_env in [1, 65535]; a dense cfg is refused (occ_fullnet_* are for it).  The
 * arguments are those of the occ_fullnet_* functions with enc_packed / grad_enc_packed in the separable layout of
 * occ_encoder_packed_floats (separable = 1).  BatchNorm runs with its running statistics in all 21 layers; the parameters
 * that receive a gradient are those of occ_sep_encoder_backward and of occ_segment_backward.  No d obs is computed.
 *
 * occ_sep_fullnet_train_forward runs the encoder ONCE, as occ_sep_encoder_train_forward does, with the last down also
 * storing its output, then the five up layers on that output and on the level tensors cc (the skips, not copied).  feats is
 * bitwise what occ_encoder_forward writes, prob (8-byte aligned) what occ_segment_forward writes.  The workspace is that of
 * occ_fullnet_train_workspace_query, part by part (the separable training workspace is the dense one).  23 launches.
 *
 * occ_sep_fullnet_backward is the backward of the LATEST occ_sep_fullnet_train_forward on ws (same cfg, n_env and packed
 * buffers) for grad_feats (n_env,256) and grad_prob (n_env,1,S,S; 16-byte aligned), both required (zeros for an absent one).
 * The decoder runs first, then the separable encoder, the deepest level first.  The two passes meet in the encoder's downs,
 * which are dense in either form, exactly as in occ_fullnet_backward: dskip_lv is added in the epilogue of the level's
 * stride-2 input gradient (rebuilt from grad_prob and the kept prob at lv = 0) and dlast in the last down's activation
 * step; no join is a launch of its own, and the decoder's dU sits in g0, which the encoder pass first writes after the
 * decoder's last launch.  Both gradient buffers are OVERWRITTEN, not accumulated.  scratch: the queried scratch_bytes
 * (16-byte aligned), the larger of occ_sep_encoder_backward's and occ_segment_backward's.  No floating-point atomics;
 * block partials are added in a fixed order in f64: every gradient is bitwise the same from call to call,
 * grad_dec_packed is bitwise what occ_segment_backward gives for the same grad_prob, and with grad_prob = 0
 * grad_enc_packed equals what occ_sep_encoder_backward gives.  137 launches (decoder 25, encoder 112) on `stream`,
 * nothing allocated or synchronised.  OCC_ERR_ARG before any launch for an unsupported cfg, a null pointer, n_env outside
 * [1, 65535], a misaligned or a short buffer.
 */
int occ_sep_fullnet_train_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* ws_bytes, size_t* scratch_bytes);
int occ_sep_fullnet_train_forward(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed, const float* obs,
                                  int n_env, void* ws, size_t ws_bytes, float* feats, float* prob, void* stream);
int occ_sep_fullnet_backward(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed, int n_env, void* ws,
                             size_t ws_bytes, const float* grad_feats, const float* grad_prob, void* scratch, size_t scratch_bytes,
                             float* grad_enc_packed, float* grad_dec_packed, void* stream);

/*
 * The joint training step with batch-statistics ("train-mode") BatchNorm (additive in ABI 12; csrc/occ_bn_train.hpp):
 * nn.BatchNorm2d as pretrainer.py runs it after model.train(), in all 21 layers (16 encoder layers, 5 decoder levels), for
 * BOTH encoder forms: cfg->separable == 0 with the limits of occ_fullnet_*, cfg->separable == 1 with those of
 * occ_sep_fullnet_*.  The arguments are those of the occ_fullnet_* functions, with these differences.  enc_packed and
 * dec_packed carry gamma and beta (NOT folded) in every layer's scale / shift slots; grad_enc_packed and grad_dec_packed
 * carry d gamma and d beta there.  Per layer and channel c, over the M = n_env H W values of r = relu(u):
 *   mu = mean r, v = mean r^2 - mu^2 (biased), rstd = 1 / sqrt(v + 1e-5), y = gamma rstd (r - mu) + beta (+ the residual or
 *   the skip); the gradients go through mu and v: d beta = sum dY, d gamma = rstd (sum dY r - mu sum dY),
 *   dR = A dY + C r + B with A = gamma rstd, C = -A rstd d gamma / M, B = -A d beta / M - C mu (formed in f64).
 * Every layer needs M >= 2, i.e. n_env (S / 32)^2 >= 2: OCC_ERR_ARG otherwise (PyTorch raises there too).  The envs of a
 * call are coupled through the statistics: feats and prob are not those of the running-statistics step.
 *
 * occ_fullnet_bn_train_forward additionally writes bn_stats (2 x 1248 floats): per layer in packed order (the 16 encoder
 * layers, then the 5 decoder levels), mean[c] | var_biased[c], from which the caller moves its running statistics
 * (running_var takes var_biased M / (M - 1)).  prob is 16-byte aligned.  After each conv / up kernel of the joint forward,
 * which keeps r, three launches form the layer's statistics (f64 block partials per chunk of 4096 pixels, one wave per
 * channel adds them), and y; the last down's also writes feats (a fixed-order f64 mean of y), the last level's runs the
 * classifier and the sigmoid on the normalised y_4.  85 launches.
 * Workspace, every part 256-byte aligned: the workspace of occ_fullnet_train_workspace_query |
 *   coef: per layer in packed order s[c] | t[c] (f32; y = s r + t) | mu[c] | rstd[c] (f64): 24 x 1248 bytes |
 *   abc: A[256] | B[256] | C[256] (f32) of the layer whose backward is in flight |
 *   forward partials: the largest layer's c n_env ceil(H W / 4096) 2 doubles
 *
 * occ_fullnet_bn_backward is the backward of the LATEST occ_fullnet_bn_train_forward on ws.  Every activation step of
 * occ_fullnet_backward / occ_sep_fullnet_backward becomes a sums pass that forms dY as that step does and stores only f64
 * partials, a one-wave-per-channel kernel that writes d gamma, d beta (and the classifier's gradient) and A, B, C, and a pass
 * that writes dU = [r > 0] dR and the partials of d bias; weight gradients, input gradients and the joins are those of the
 * running-statistics step.  scratch: that of the joint step of the same form.  Both gradient buffers are OVERWRITTEN.  No
 * floating-point atomics, every sum in a fixed order in f64: bn_stats and every gradient are bitwise the same from call to
 * call.  146 launches (dense), 179 (separable) on `stream`, nothing allocated or synchronised.  OCC_ERR_ARG before any launch
 * for an unsupported cfg or shape, a null pointer, a misaligned or a short buffer.
 */
int occ_fullnet_bn_train_workspace_query(const OccEncoderConfig* cfg, int n_env, size_t* ws_bytes, size_t* scratch_bytes);
int occ_fullnet_bn_train_forward(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed, const float* obs,
                                 int n_env, void* ws, size_t ws_bytes, float* feats, float* prob, float* bn_stats, void* stream);
int occ_fullnet_bn_backward(const OccEncoderConfig* cfg, const float* enc_packed, const float* dec_packed, int n_env, void* ws,
                            size_t ws_bytes, const float* grad_feats, const float* grad_prob, void* scratch, size_t scratch_bytes,
                            float* grad_enc_packed, float* grad_dec_packed, void* stream);

/*
 * The optimizer of the joint training step (additive in ABI 12; csrc/occ_adamw.hpp): torch.optim.AdamW (pretrainer.py:91;
 * decoupled decay, amsgrad off, maximize off) on the PACKED parameters, so that a training step neither unpacks a gradient
 * nor packs a parameter.  Per part (the encoder of either form, cfg->separable; the decoder with the classifier) the caller
 * keeps, all in the packed order of occ_encoder_packed_floats / occ_decoder_packed_floats floats:
 *   theta   the master: every slot the raw parameter, a layer's scale / shift slots holding gamma and beta;
 *   m, v    AdamW's two moments;
 *   grad    the packed gradient exactly as occ_fullnet_backward / occ_sep_fullnet_backward / occ_fullnet_bn_backward wrote it;
 *   packed  the buffer the next train forward reads, written here.
 * stats: the running statistics of the 21 BatchNorm layers in packed order (16 encoder layers, 5 decoder levels),
 * mean[c] | var[c] per layer, the layout of bn_stats: 2 x 1248 floats.
 *
 * occ_net_adamw_query(cfg, &enc_floats, &dec_floats, &stat_floats): the three sizes in floats; no GPU is touched.
 *
 * occ_net_adamw_step(cfg, enc_theta, enc_m, enc_v, enc_grad, enc_packed, dec_theta, dec_m, dec_v, dec_grad, dec_packed,
 *                    stats, head_theta, head_m, head_v, head_grad, head_count, lr, beta1, beta2, eps, weight_decay, step,
 *                    bn_mode, stream)
 * head_*: an optional plain segment of head_count floats (the grad head) that takes the same step; head_count == 0: the four
 * pointers are not read.  step is 1-based; the bias corrections bc1 = 1 - beta1^step, bc2 = 1 - beta2^step are formed on the
 * host in double, as torch.optim.AdamW forms them, and every scalar reaches the kernel rounded to f32 once.  Every slot g, p:
 *   p *= 1 - lr weight_decay;  m += (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g g;
 *   p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)                                                   (f32)
 * with the roundings of torch's foreach implementation on the device written out (every torch op rounds on its own, the
 * multiply-add inside lerp_, addcmul_ and addcdiv_ is fused), so that from equal inputs it gives torch's bits.
 * The decay applies to every slot, gamma, beta and the biases included (the reference's single parameter group), to gamma
 * and never to the folded scale.
 *   bn_mode 0 (running statistics): a layer's gradient slots hold d scale, d shift.  With rstd = 1 / sqrt(var + 1e-5):
 *     d gamma = (d scale - mean d shift) rstd, d beta = d shift; after the update packed gets scale = gamma rstd and
 *     shift = beta - mean scale of the UPDATED gamma, beta.  Both in f64, every operation rounded on its own (no fused
 *     multiply-add), rounded to f32 once: bitwise what unfused f64 tensor operations give.
 *   bn_mode 1 (batch statistics, occ_fullnet_bn_*): the slots hold d gamma, d beta; packed gets gamma, beta; stats is not read.
 * Every other slot of packed is a copy of theta.  One thread owns a channel's (gamma, beta) pair.  ONE launch on `stream` for
 * both parts and the head; no atomics, no reductions: the result is bitwise the same from call to call.
 *
 * occ_net_adamw_fold(cfg, enc_theta, enc_packed, dec_theta, dec_packed, stats, bn_mode, stream): writes both packed buffers
 * from the masters as the step does after its update, and nothing else: for the first forward, and after a change of the
 * BatchNorm mode or of the running statistics.  One launch.
 *
 * Every pointer is 16-byte aligned.  OCC_ERR_ARG before anything is launched for a bad cfg (img is checked as everywhere,
 * the layout does not depend on it), a null or misaligned pointer, head_count < 0, step <= 0, eps <= 0, lr < 0,
 * weight_decay < 0, a beta outside [0, 1) or a bn_mode other than 0 and 1.
 */
int occ_net_adamw_query(const OccEncoderConfig* cfg, int64_t* enc_floats, int64_t* dec_floats, int64_t* stat_floats);
int occ_net_adamw_step(const OccEncoderConfig* cfg, float* enc_theta, float* enc_m, float* enc_v, const float* enc_grad,
                       float* enc_packed, float* dec_theta, float* dec_m, float* dec_v, const float* dec_grad, float* dec_packed,
                       const float* stats, float* head_theta, float* head_m, float* head_v, const float* head_grad,
                       int64_t head_count, double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                       int bn_mode, void* stream);
int occ_net_adamw_fold(const OccEncoderConfig* cfg, const float* enc_theta, float* enc_packed, const float* dec_theta,
                       float* dec_packed, const float* stats, int bn_mode, void* stream);

/*
 * The pretraining input pipeline (additive in ABI 12; csrc/occ_augment.hpp): what dataset.py:53-92 does per item between
 * the decoded, resized frame and the tensors of a batch, for a dataset that is resident on the device.  Decoding and
 * resizing are deterministic and happen once, on the host; what is random per epoch (the shuffle, ColorJitter(0.3, 0.3,
 * 0.2, 0.1), the flip) is a gather by frame index plus point arithmetic here.
 *
 * The store (device memory, only read), M frames of S x S pixels (S = img):
 *   rgbl   uint32[M][S][S]  one word per pixel, R | G << 8 | B << 16 | label << 24, label 0 or 1
 *   depth  int16[M][S][S]   the mode-"I" depth image as resized (PIL's bicubic filter can leave [0, 255])
 *   pos    float[M][2]      dataset.py:62
 *   grad   float[M][2]      the gradient label as the caller wants it returned (dataset.py:84-89: (sin a, cos a))
 *
 * OccAugmentParams, one per sample: what ColorJitter.get_params and dataset.py:72 draw.  order holds the four ops of the
 * jitter, 2 bits each, the first op in the low bits: 0 brightness, 1 contrast, 2 saturation, 3 hue (every op once).
 * hue_shift is the byte torchvision adds to the H band, int(hue_factor * 255) & 255.  jitter == 0 skips all four ops.
 *
 * occ_augment_query(img, n, &workspace_bytes): the size of the workspace of a call (4-byte aligned device memory, the
 * per-block luminance sums; its contents mean nothing between calls); no GPU is touched.
 *
 * occ_augment_batch(rgbl, depth, pos, grad, m_frames, img, idx, params, n, normalize, out_img, out_label, out_grad, out_pos,
 *                   workspace, stream)
 * idx: int64[n] on the device, frame numbers in [0, m_frames), in any order, repeats allowed.  Keeping them in range is the
 * caller's duty; the kernels clamp them, so that no address outside the store is ever formed.  Sample i gets
 *   out_img[i]    float[4][S][S]  R, G, B after the jitter, and the depth; level / 255, with normalize != 0 then
 *                                 (c - 0.5) / 0.25 on all four planes (dataset.py:28-31,77-81)
 *   out_label[i]  float[1][S][S]  0 or 1 (dataset.py:82 divides by 255 once more; this does not)
 *   out_grad[i], out_pos[i]  float[2]  the frame's rows
 * and with params[i].flip != 0 output column x of the three images is source column S - 1 - x.  Arithmetic of the jitter,
 * per channel on 8-bit levels, which is PIL's (torchvision's PIL path) rounding for rounding:
 *   L = (R 19595 + G 38470 + B 7471 + 0x8000) >> 16                                               convert("L")
 *   blend(deg, x, f): t = (float)deg + f * (float)(x - deg) in f32, product and sum rounded separately; for 0 <= f <= 1
 *     the truncation of t, else 0 for t <= 0, 255 for t >= 255, else the truncation                ImagingBlend
 *   brightness: deg = 0.  saturation: deg = L of the pixel.  contrast: deg = (int)(sum L / (double)(S S) + 0.5) over the
 *     whole image as it stands when contrast's turn comes.
 *   hue: RGB -> HSV as PIL's rgb2hsv_row (f32 divisions; 2.0 + rc - bc, h / 6.0 + 1.0, h * 255.0 and s * 255.0 in f64),
 *     h = (h + hue_shift) & 255, HSV -> RGB as PIL's hsv2rgb_row (all f32, floor(x + 0.5)).
 * No multiply-add of these is fused.  tests/augment_model.py is this arithmetic in numpy, checked against PIL.
 *
 * params may be NULL: no sample is jittered or flipped (a validation batch), and workspace is not used and may be NULL.
 * At most two launches on `stream`: the luminance-sum pass (samples with jitter == 0 leave it at once; skipped altogether
 * for params == NULL, the one case the host can see) and the output pass.  Nothing is allocated or synchronised, no atomics,
 * no memset, integer sums: the outputs are bitwise the same from call to call.
 * OCC_ERR_ARG before any launch for a null pointer (other than the two above), img < 1, img * img > 2^24 (the u32
 * luminance sum must not overflow), n < 1, n > 65535, m_frames < 1.
 */
typedef struct OccAugmentParams {
    float brightness, contrast, saturation; /* the three blend factors */
    int32_t hue_shift;                      /* 0..255 */
    int32_t order;                          /* four 2-bit op codes, first op in the low bits */
    int32_t jitter;                         /* 0: none of the four ops */
    int32_t flip;                           /* != 0: mirrored left to right */
    int32_t pad;
} OccAugmentParams;
int occ_augment_query(int img, int n, size_t* workspace_bytes);
int occ_augment_batch(const uint32_t* rgbl, const int16_t* depth, const float* pos, const float* grad, int m_frames, int img,
                      const int64_t* idx, const OccAugmentParams* params, int n, int normalize, float* out_img,
                      float* out_label, float* out_grad, float* out_pos, void* workspace, void* stream);

/*
 * Packing rendered frames into the resident dataset (additive in ABI 12; csrc/occ_datapack.hpp): what
 * dataset_io.RunWriter.write_frame (datasetGenerator.py:102-112) followed by DeviceDataset.from_directory at the same size
 * does to a frame between the engine's step and the store above, without the files and without the JPEG.
 *
 * occ_dataset_pack(obs, alpha, alpha_stride, n, img, slot, rgbl, depth, m_frames, label_mode, stream)
 *   obs    float[n][4][S][S]  the engine's observation (S = img): three colour planes and the view depth, -1 = background
 *   alpha  read at alpha[(env * S * S + pixel) * alpha_stride]: 1 = an (n,S,S) image, 4 = the alpha channel of the
 *          (n,S,S,4) full_state when the pointer is that of its channel 3 (the convention of occ_seg_metrics)
 *   slot   int64[n] on the device: the frame of the store env i writes.  Any value outside [0, m_frames) skips env i; no
 *          address is formed from it.  Keeping the in-range slots of one call distinct is the caller's duty.
 *   rgbl, depth  the store of occ_augment_batch, m_frames frames; frames no slot names are not touched
 * Per written pixel, with u8(x) = clip(rint((double)x * 255.0), 0, 255), round-half-even, NaN -> 0 (skimage's
 * img_as_ubyte as dataset_io._ubyte states it):
 *   colours  the word's R byte is u8(obs[2]), G is u8(obs[1]), B is u8(obs[0]): the writer saves BGR (cv2.imwrite of an
 *            RGB array), the reader opens the file as RGB
 *   depth    d = obs[3], d == -1 -> 0; t = d * 51.0f, one f32 product; stored (int16) is the truncation of t, with what the
 *            C cast leaves undefined defined: t <= 0 or NaN -> 0, t >= 255 -> 255
 *   label    a8 = u8(alpha), then with
 *            label_mode 0: PIL's convert("1") of the S x S image a8, which is what the reader applies to the Occl file:
 *              Floyd-Steinberg error diffusion exactly as Convert.c tobilevel does it.  int errors[S + 1] starts at zero
 *              and persists across rows; per row l = l0 = l1 = 0, and for x = 0 .. S - 1:
 *                l = clip8(a8[x] + (l + errors[x + 1]) / 16)        (C division: toward zero)
 *                out = l > 128 ? 255 : 0;  e = l - out
 *                errors[x] = 3 e + l0;  l0 = 5 e + l1;  l1 = e;  l = 7 e
 *              and errors[S] = l0 after the row.  The label is out != 0.
 *            label_mode 1: alpha > 0.5f, the rule pretrainer.py:134 and occ_seg_metrics apply to a target (NOT what the
 *              files give: soft silhouette edges dither)
 *            stored as 0 or 1 in bits 24..31 of the word.
 * At most two launches on `stream`: a point pass over the pixels, which for label_mode 0 parks a8 in the label byte, and
 * the dither pass in place on that byte (one wave per frame, rows of a 64-row band two columns apart; skipped for
 * label_mode 1).  Nothing is allocated or synchronised, no atomics, integer arithmetic after the three conversions: the
 * store is bitwise the same from call to call.  tests/datapack_model.py is this arithmetic in numpy, checked against PIL.
 * OCC_ERR_ARG before any launch for a null pointer, img < 1, img * img > 2^24, n < 1, n > 65535, m_frames < 1,
 * alpha_stride < 1 or a label_mode other than 0 and 1.
 */
int occ_dataset_pack(const float* obs, const float* alpha, int alpha_stride, int n, int img, const int64_t* slot,
                     uint32_t* rgbl, int16_t* depth, int m_frames, int label_mode, void* stream);

/*
 * Resizing frames between resident stores (additive in ABI 12; csrc/occ_resize.hpp): PIL's Image.resize(size) without a
 * filter argument, which is what the reference's reader applies to every item (dataset.py:65-67; it renders at 512 x 512
 * and trains at 256 x 256): BICUBIC for the "RGB" and the "I" image, NEAREST for the "1" image.  With occ_dataset_pack at
 * the rendering size in front of it, a frame gets the bits of RunWriter followed by from_directory at another size (the
 * JPEG apart): the dither runs at the rendering size and the resize picks from its result.
 *
 * occ_dataset_resize_query(src_img, dst_img, n, &workspace_bytes): the size of the workspace of a call; no GPU is touched.
 *
 * occ_dataset_resize(src_rgbl, src_depth, n, src_img, slot, dst_rgbl, dst_depth, m_frames, dst_img, workspace, stream)
 *   src_rgbl, src_depth  n frames of R x R pixels (R = src_img), the words and int16 planes of occ_augment_batch; only read
 *   slot   int64[n] on the device: the frame of the destination source frame i is resized into.  Any value outside
 *          [0, m_frames) skips frame i; no address is formed from it.  Keeping the in-range slots distinct is the caller's duty.
 *   dst_rgbl, dst_depth  m_frames frames of S x S pixels (S = dst_img); frames no slot names are not touched.  The two
 *          stores must not overlap.
 *   workspace  8-byte aligned device memory of the queried size.  The call fills it itself, in its first launch:
 *          with K = min((int)ceil(support) * 2 + 1, R), in this order and without padding
 *            double k[S][K], int32 kk[S][K], int32 bounds[S][2] (xmin, count), int32 nearest[S]
 *          as below.  Its contents mean nothing between calls.
 * The table, one for both axes (Resample.c precompute_coeffs; f64, every operation rounded on its own):
 *   scale = R / S, fs = max(scale, 1.0), support = 2.0 * fs, ss = 1.0 / fs; per output index xx
 *   center = (xx + 0.5) * scale; xmin = max((int)(center - support + 0.5), 0);
 *   count = min((int)(center + support + 0.5), R) - xmin; w[x] = f((x + xmin - center + 0.5) * ss) for x < count, ww their
 *   sum in that order, k[x] = w[x] / ww (0 from count on), with f(x) for x = |x| and a = -0.5:
 *   x < 1: ((a + 2) x - (a + 3)) x x + 1; x < 2: (((x - 5) x + 8) x - 4) a; else 0.
 *   kk[x] = (int)(k[x] * 2^22 + (k[x] < 0 ? -0.5 : 0.5))                                     normalize_coeffs_8bpc
 *   nearest: a = R / S; xo = a * 0.5; nearest[x] = (int)xo; xo += a -- a running sum (Geometry.c ImagingScaleAffine),
 *   clamped to [0, R - 1]
 * Per pixel, the horizontal pass first, its result feeding the vertical pass:
 *   R, G, B  acc = 2^21 + sum pixel * kk[x] in int32; clip(acc >> 22, 0, 255), an arithmetic shift
 *   depth    acc = 0.0; acc = acc + (double)pixel * k[x] in tap order, product and sum rounded separately;
 *            (int)(acc + (acc < 0 ? -0.5 : 0.5)), an int32 between the passes; the final value saturated to int16 (PIL's
 *            wherever PIL's fits; anything that came from occ_dataset_pack does)
 *   label    the label of source pixel (nearest[y], nearest[x])
 * Supported sizes: min(R, ceil((min(32, S) - 1) * R / S + 4 * max(R / S, 1)) + 2) <= 72, the input window of one 32 x 32
 * output tile in LDS: every R / S <= 2, integer or not, upscaling by any factor, and any S for R <= 72.
 * Two launches on `stream`: the table, then one fused pass (window into LDS, horizontal pass into LDS, vertical pass).
 * Nothing is allocated or synchronised, no atomics, plain stores, sums in a fixed order: the store is bitwise the same from
 * call to call.  tests/resize_model.py is this arithmetic in numpy, checked against PIL.
 * OCC_ERR_ARG before any launch for a null pointer, a workspace that is not 8-byte aligned, a size < 1, a size with
 * img * img > 2^24, n < 1, n > 65535, m_frames < 1 or an unsupported pair of sizes.
 */
int occ_dataset_resize_query(int src_img, int dst_img, int n, size_t* workspace_bytes);
int occ_dataset_resize(const uint32_t* src_rgbl, const int16_t* src_depth, int n, int src_img, const int64_t* slot,
                       uint32_t* dst_rgbl, int16_t* dst_depth, int m_frames, int dst_img, void* workspace, void* stream);

/*
 * JPEG round trip in the resident store (additive in ABI 12; csrc/occ_jpeg.hpp): what writing a frame's colours as a
 * baseline JPEG and decoding the file again does to them, which is what the reference trains on (datasetGenerator.py:104
 * writes every colour image as a 4:2:0 JPEG at the rendering size).  Entropy coding is lossless, so the round trip is a
 * function of the pixels and the two quantisation tables.  With occ_dataset_pack in front of it (and occ_dataset_resize
 * behind it) a frame gets the bits of RunWriter followed by from_directory, colours included.
 *
 * occ_dataset_jpeg_query(img, n, quality, &workspace_bytes): the size of the workspace of a call, n * cs * cs * 2 bytes
 *   with cs = 8 * ceil(img / 16); no GPU is touched.  OCC_ERR_ARG for img outside 1 .. 4096, n outside 1 .. 65535, quality
 *   outside 1 .. 100 or a null pointer.
 *
 * occ_dataset_jpeg(rgbl, m_frames, img, slot, n, quality, workspace, stream)
 *   rgbl   the words of the store of occ_augment_batch, m_frames frames of S x S pixels (S = img), changed in place: the
 *          three colour bytes of frame slot[i] are replaced by the round trip of those same three bytes taken as the file's
 *          R, G, B (the store holds them in file order; occ_dataset_pack has swapped B and R).  The label byte is kept; the
 *          depth plane is not an argument.  Frames no slot names are not touched.
 *   slot   int64[n] on the device.  Any value outside [0, m_frames) skips entry i; no address is formed from it.  Keeping
 *          the in-range slots distinct is the caller's duty.
 *   workspace  2-byte aligned device memory of the queried size: per entry i a cs x cs plane of Cb' | Cr' << 8, the
 *          reconstructed chroma samples between the two launches.  Its contents mean nothing between calls.
 * The arithmetic is libjpeg's with its defaults (YCbCr, 2x2 luminance sampling, the slow-integer DCT, fancy upsampling), in
 * int32 with arithmetic shifts, no floating point; D(x, n) = (x + (1 << (n - 1))) >> n:
 *   tables   the luminance and chrominance tables of the JPEG specification, Annex K; scale = 5000 / quality below 50, else
 *            200 - 2 quality; entry = clip((base * scale + 50) / 100, 1, 255).  Computed on the host in the call and
 *            handed to the kernel by value.
 *   convert  Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
 *            Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
 *   edges    columns past the image replicate the last column (out to a multiple of 16); input rows replicate the last row
 *            up to an even height only; C = (the 2 x 2 sum + bias) >> 2 with bias 1 in even and 2 in odd chroma columns;
 *            then every plane, the downsampled chroma planes too, is padded to a multiple of 8 rows with its own last row
 *   DCT      jfdctint.c on sample - 128, rows then columns; quantisation c = (|v| + 4 q) / (8 q) with the sign of v put
 *            back, truncating; coefficient = c * q; jidctint.c, columns (D(., 11)) then rows (D(., 18)), + 128, clipped
 *   upsample jdsample.c h2v2_fancy_upsample on the chroma planes cropped to ceil(S / 2): for row 2 r + v,
 *            s[x] = 3 C[r][x] + C[r - 1 + 2 v][x]; out[2 x] = (3 s[x] + s[x - 1] + 8) >> 4,
 *            out[2 x + 1] = (3 s[x] + s[x + 1] + 7) >> 4; a missing row or column is the row or column itself
 *   convert  with u = Cb - 128, v = Cr - 128: R = Y + ((91881 v + 32768) >> 16), B = Y + ((116130 u + 32768) >> 16),
 *            G = Y + ((-22554 u - 46802 v + 32768) >> 16), clipped to 0 .. 255
 * Two launches on `stream`: one block per 32 x 32 tile (convert, downsample, both transforms through LDS; Y' into the
 * word's low byte, Cb' and Cr' into the workspace), then the upsampling and conversion back per pixel.  Nothing is
 * allocated or synchronised, no atomics, plain stores: the store is bitwise the same from call to call.
 * tests/jpeg_model.py is this arithmetic in numpy, checked against PIL (Pillow with libjpeg-turbo).
 * OCC_ERR_ARG before any launch for a null pointer, a workspace at an odd address, img outside 1 .. 4096, n outside
 * 1 .. 65535, quality outside 1 .. 100 or m_frames < 1.
 */
int occ_dataset_jpeg_query(int img, int n, int quality, size_t* workspace_bytes);
int occ_dataset_jpeg(uint32_t* rgbl, int m_frames, int img, const int64_t* slot, int n, int quality, void* workspace,
                     void* stream);

/*
 * The counts of pretrainer.py:133-139 per env: with p = pred > 0.5 and t = target > 0.5 over the img x img pixels,
 * counts[env] = { #(p == t), #(p and t), #(p or t) } (int64).  pred is (n_env,img,img) contiguous; target is read at
 * target[(env * img * img + pixel) * target_stride] (1 = contiguous, 4 = the alpha channel of an (n_env,img,img,4)
 * image).  Integer sums: the result does not depend on scheduling.  counts is cleared on `stream` first.
 */
int occ_seg_metrics(const float* pred, const float* target, int target_stride, int n_env, int img, int64_t* counts,
                    void* stream);

/*
 * The pretrainer's segmentation criterion (pretrainer.py:89: BinaryDiceLoss() or nn.BCELoss(); :127-141 and :176-189: the
 * loss and the accuracy / IoU lines) from ONE read of pred and target.  pred, target, target_stride, n_env and img as for
 * occ_seg_metrics (same limits, same status returns); target may be soft, in [0,1].  Per env, with p = pred, t = target:
 *   sums[env] = { sum p t, sum p^2, sum t^2, sum -(t max(log p, -100) + (1 - t) max(log(1 - p), -100)) }   (double)
 * the first three being what loss.py:29-30 sums for p = 2, the fourth nn.BCELoss's per-pixel term with its clamp;
 *   counts[env] = the three int64 counts of occ_seg_metrics, bit-identical; counts may be NULL.
 * BinaryDiceLoss per env = 1 - (sums[0] + smooth) / (sums[1] + sums[2] + smooth); BCELoss = sum_env sums[3] / (n img^2).
 * No floating-point atomics and a fixed summation order, every addition in f64: sums[env] is bitwise independent of n_env,
 * of the env's position, of how a caller splits the batch over calls, and of the run.  scratch: device memory of
 * occ_seg_criterion_scratch_bytes(n_env, img) bytes (8-byte aligned; the per-block partial sums), 0 for bad arguments.
 * Two launches (and the clearing of counts) on `stream`.
 */
size_t occ_seg_criterion_scratch_bytes(int n_env, int img);
int occ_seg_criterion(const float* pred, const float* target, int target_stride, int n_env, int img, double* sums,
                      int64_t* counts, void* scratch, void* stream);
/*
 * The criterion's gradient with respect to pred, elementwise; grad_pred (n_env,img,img) f32 is overwritten.
 *   OCC_CRITERION_DICE: grad = coef[env][0] t + coef[env][1] p.  With num = sums[0] + smooth, den = sums[1] + sums[2] +
 *     smooth and u the upstream gradient of the env's loss 1 - num / den (reduction folded in): coef = { -u / den,
 *     2 u num / den^2 }.
 *   OCC_CRITERION_BCE: grad = coef[env][0] (p - t) / max(p (1 - p), 1e-12), the backward rule of nn.BCELoss;
 *     coef[env][0] = upstream / (n img^2), coef[env][1] is not read.
 * coef is (n_env,2) double on the device.  One launch.
 */
#define OCC_CRITERION_DICE 0
#define OCC_CRITERION_BCE 1
int occ_seg_criterion_grad(const float* pred, const float* target, int target_stride, int n_env, int img, int mode,
                           const double* coef, float* grad_pred, void* stream);

/*
 * Host hand-off of SimpleVecEnv.step_wait (SubProcVecEnv.py:209-218): one int32 buffer
 *   flags[0..n_env) = done, flags[n_env..n_env+n_reserve) = reserve scene passes reset()'s acceptance test
 *   (loss > 0.1, environment.py:327), flags[n_env+n_reserve] = some status word is non-zero
 * so that the host needs ONE device-to-host copy per batched step.  status has n_env+n_reserve words.
 */
int occ_step_flags(const uint8_t* done, const float* loss_all, const int32_t* status, int n_env, int n_reserve,
                   int32_t* flags, void* stream);

/*
 * Auto-reset commit ("obs = self.envs[env_idx].reset()", SubProcVecEnv.py:214, from a pre-rendered candidate):
 * for k < n, env row pairs[2k] takes over row pairs[2k+1] of every per-env state array (el, az, radius, cam,
 * alphas, scene) with camera_position = 0, full_reward = loss, object_mass = loss + 1 (environment.py:302-324),
 * and obs[dst] = obs_all[src].  All arrays hold n_env + n_reserve rows except campos/full_reward/object_mass/obs
 * (n_env rows).
 */
int occ_reset_commit(const int32_t* pairs, int n, float* el, float* az, float* radius, float* campos, float* cam,
                     float* alphas, float* full_reward, float* object_mass, int32_t* scene_mesh, float* scene_offset,
                     float* obs, const float* obs_all, const float* loss_all, int img, void* stream);

/*
 * Device-side auto-reset (the whole of "if buf_done: obs = self.envs[env_idx].reset()", SubProcVecEnv.py:209-218,
 * incl. reset()'s rejection loop environment.py:288-327) for a batched step whose launch also rendered n_reserve
 * speculative reset scenes (rows n_env .. n_env+n_reserve-1 of every *_all array, reset camera).
 *
 * Reserve slot life cycle (rs_state): OCC_RS_EMPTY -- host uploads a scene (occ_reserve_refill) --> OCC_RS_PENDING
 * -- rendered by a step; loss > 0.1 or 10th try --> OCC_RS_READY (else back to EMPTY, try count kept) -- taken by
 * a finished env --> EMPTY (tries = 0).  Only the host leaves EMPTY, only the device leaves PENDING / READY.
 *
 * One call = two launches (three until ABI v8): (1) a single block ages the PENDING slots, lists finished envs and READY
 * slots in index order, pairs them and refreshes the skip mask (rendered next step = PENDING only); (2) per slot: the rows
 * this step rendered for a slot that was PENDING and is not taken now (observation, full_state, loss) are copied into the
 * persistent OccReserveStore - READY slots are not rendered again (OccScene.skip), their last render stays valid - and
 * every pair copies the slot's last render (this step's rows, or the store) and state into the env's rows (as
 * occ_reset_commit), saving the env's final observation to term_obs[slot] first (info["terminal_observation"]).
 * report (n_env + 2*n_reserve + 2 int32): [0,n_env) 1 = done, 2 = time limit (OccAutoResetOpts) | [n_env, +n_reserve) slot state AFTER the call |
 * [.., +n_reserve) env that took the slot this call or -1 | any status bit | finished envs left without a slot.
 * pairs: scratch, 2 + 3*n_reserve int32.  Arrays of OccEnvState hold n_env + n_reserve rows except
 * campos / full_reward / object_mass (n_env rows); obs_all has n_env + n_reserve rows.
 */
#define OCC_RS_EMPTY 0
#define OCC_RS_PENDING 1
#define OCC_RS_READY 2

typedef struct OccEnvState {
    float* el;
    float* az;
    float* radius;
    float* campos;
    float* cam;
    float* alphas;
    float* full_reward;
    float* object_mass;
    int32_t* scene_mesh;
    float* scene_offset;
} OccEnvState;

/* Persistent copy of what the last render of every reserve slot produced (a slot is only rendered while PENDING). */
typedef struct OccReserveStore {
    float* obs;        /* (n_reserve,4,S,S) */
    float* full_state; /* (n_reserve,S,S,4) */
    float* loss;       /* (n_reserve) */
    int32_t* skip;     /* (n_env + n_reserve) the OccScene.skip mask; rows >= n_env maintained here */
} OccReserveStore;

/* Optional extras of occ_auto_reset (NULL = none of them). */
typedef struct OccAutoResetOpts {
    /* Episode time limit (trainRL.py:22,191-229: `for t in range(1, max_ep_len + 1)` then env.reset(), is_terminal stays
     * False): age (n_env) = steps since the env's last reset, incremented by this call; an env whose age reaches
     * max_ep_len (> 0) is reset from the reserve like a finished one, with done left 0 (report value 2); a committed
     * env's age returns to 0.  age == NULL: no counting. */
    int32_t* age;
    int32_t max_ep_len;
    /* Region-tracking rects of obs_all and of the alphas state (OccRenderOut.rect_next / arect_next of the launch that
     * produced this step): a committed row holds a whole stored frame and is marked full-frame. */
    int32_t* rect;
    int32_t* arect;
    /* (n_reserve,S,S,4): receives the stored occlusion image of every slot taken in this call (what the reference's
     * env.image holds after reset(), environment.py:319). */
    float* reset_full_state;
    /* normWithObjectSize (environment.py:208,320,324): norm_flags (n_env) int32, nonzero = that env divides its reward by
     * objectMass = sum_px (a1 + a2 + a3)^2 + 1 of its reset render instead of loss + 1; slot_objsum (n_reserve) holds that
     * sum for the stored render of every reserve slot (occ_object_mass).  Both NULL: loss + 1 for every env. */
    const int32_t* norm_flags;
    const float* slot_objsum;
    /* A second copy of `report`, written by the pairing launch itself into PINNED HOST memory that the device can address
     * (hipHostMalloc / torch pin_memory): the host reads it after an event recorded behind this call - no copy launch.  Its
     * first n_env words must be ZERO on entry: only the entries of envs that are reset (1 / 2) are written. */
    int32_t* report_host;
} OccAutoResetOpts;

int occ_auto_reset(const uint8_t* done, const float* loss_all, const int32_t* status, int n_env, int n_reserve,
                   int32_t* rs_state, int32_t* rs_tries, const OccEnvState* st, float* obs_all, const float* full_state_all,
                   const OccReserveStore* store, float* term_obs, int img, int32_t* pairs, int32_t* report,
                   const OccAutoResetOpts* opts, void* stream);

/*
 * objectMass of reset() with normWithObjectSize (environment.py:320,324: self.objects = image1 + image2 + image3;
 * objectMass = sum(objects[..., 3] ** 2) + 1): out[r] = sum over the pixels of (a1 + a2 + a3)^2 for rows r of
 * alphas (n_rows,3,S,S), in a fixed summation order.  gate (n_rows) int32 or NULL: only rows with gate[r] == gate_value
 * are computed, the others keep what out holds (the reserve: rows rendered in this step are the OCC_RS_PENDING ones).
 */
int occ_object_mass(const float* alphas, int n_rows, int img, const int32_t* gate, int gate_value, float* out, void* stream);

/*
 * Host -> reserve: n packed rows of 13 words (slot, mesh id x3, offset x9 as float bits) in device memory or in
 * pinned host memory the device can address (then no copy launch is needed: the rows are read when the kernel runs, so
 * the host must leave them alone until it has synchronised with something later on the stream); scatters them into scene_mesh / scene_offset rows n_env + slot and marks the slots OCC_RS_PENDING.
 */
int occ_reserve_refill(const int32_t* packed, int n, int n_env, int n_reserve, int32_t* scene_mesh, float* scene_offset,
                       int32_t* rs_state, int32_t* skip, void* stream);

/*
 * Episode bookkeeping of the batched controller evaluation (additive in ABI 12; csrc/occ_episode.hpp): what the
 * reference's evaluation loops do on the host after every env.step (test.py:92-255, iterator.py:104-204), for n_env
 * envs in one launch after a batched step with index `step` (0-based) of at most max_step.
 *   done (n) u8, reward (n), full_reward (n)   the step's outputs (the reward arrays are read for the traces only)
 *   grad (n,2)   the step's d reward / d action          read by OCC_EPISODE_GRADIENT only
 *   noise (n,2)  standard normal draws                   read by OCC_EPISODE_RANDOM only
 *   pred (n,2)   the network's predicted gradient, or the agent's sampled action   read by _MODEL and _AGENT only
 * State, per env: action (n,2) f32, active (n) int32, skip (n) int32 (the OccScene.skip mask of the next step),
 * iterations (n) int32, finished (n) u8, nan_steps (n) int32; trace_reward / trace_full_reward (max_step, n) f32 or NULL,
 * pre-filled by the caller (with NaN).  For an env with active != 0:
 *   GRADIENT  a NaN in grad: nan_steps += 1 and nothing else of this step happens (`continue`, iterator.py:118-120);
 *             otherwise action = fadd(action, fmul(lr, grad)): two roundings, as torch's `action += lr * action.grad`
 *   RANDOM    action = fadd(action, fmul(lr, noise))
 *   MODEL     action = fmul(-lr, pred)                    (lr is the reference's step_lr)
 *   AGENT     action = pred
 * then (not on a NaN step) row `step` of the traces is written; done: iterations = step + 1, finished = 1, active = 0,
 * skip = 1; else step == max_step - 1 (the cap, test.py:122-124): iterations = step + 1, active = 0, skip = 1.  The cap
 * also ends an env on a NaN step (the reference would leave no entry for such an episode).  An env with active == 0 has
 * nothing read and nothing written.  report[0] = the number of envs still active after the call.
 * One launch of one block on `stream`; no atomics, nothing allocated or synchronised.  OCC_ERR_ARG before the launch for
 * a null pointer among those the rule reads or the state, a trace without its input, n_env < 1, a rule outside 0..3, or
 * step outside [0, max_step).
 */
#define OCC_EPISODE_GRADIENT 0
#define OCC_EPISODE_RANDOM 1
#define OCC_EPISODE_MODEL 2
#define OCC_EPISODE_AGENT 3
int occ_episode_advance(const uint8_t* done, const float* reward, const float* full_reward, const float* grad,
                        const float* pred, const float* noise, int rule, float lr, int step, int max_step, int n_env,
                        float* action, int32_t* active, int32_t* skip, int32_t* iterations, uint8_t* finished,
                        int32_t* nan_steps, float* trace_reward, float* trace_full_reward, int32_t* report, void* stream);

/*
 * The PPO training loop on the device (additive in ABI 12; csrc/occ_rollout.hpp, tests/rollout_model.py): what
 * trainRL.py:189-247 and PPO.py:152-188 do on the host around every env.step, for n_env envs per launch.  All three:
 * one launch on `stream`, no atomics, nothing allocated or synchronised, OCC_ERR_ARG before the launch.
 *
 * occ_ppo_act (one wave per env): the old policy's action for feats (n,256) f32 -
 *   mean = feats w_a^T + b_a  (w_a (2,256), b_a (2));  action = fadd(mean, fmul(noise, action_std))  (noise (n,2): the
 *   caller's standard normal draws);  logprob = -0.5 sum_j (a_j - mean_j)^2 / var - 0.5 (2 log 2 pi + 2 log var), with
 *   var = action_std^2 in f32 - in the lane partition, reduction and expressions of occ_ppo_update's epoch, so that the
 *   epoch recomputes the same mean and quadratic term for the sample when it is given the same f32 var; the constant is
 *   rounded once from double here (occ_ppo_update sums it in f32, which loses up to 1e-7 where the logarithms cancel).
 *   action (n,2) and logprob (n) are written, mean (n,2) if not NULL.  feat_buf (T,n,256), action_buf (T,n,2),
 *   logprob_buf (T,n): all three or none; row t of each also receives the env's feature row, action and logprob.
 *   Row e of every output depends on row e of the inputs only.  OCC_ERR_ARG: a null pointer among the required ones,
 *   n_env < 1, action_std <= 0 (or NaN), some but not all buffers, or with buffers T < 1 or t outside [0, T).
 *
 * occ_rollout_advance (one block), after the step's occ_auto_reset: reward (n) f32, done (n) u8, code (n) int32 with
 *   0 = the episode goes on, 1 = it ended done, 2 = it ended by the time limit (the first n_env words of occ_auto_reset's
 *   report).  Per env: ep_return = fadd(ep_return, reward), ep_len += 1, and with rewards / dones ((T,n) f32, both or
 *   neither) rewards[t,e] = reward[e], dones[t,e] = done[e] ? 1 : 0.  Then for every env with code != 0, in env-index
 *   order: running = the first episode ever ? return : fadd(fmul(0.95f, running), fmul(0.05f, return)) (trainRL.py:236),
 *   entry (env, ep_return, ep_len, code, timestep, running) goes to slot (n_episodes % cap) of the ring, n_episodes += 1,
 *   code_counts[code - 1] += 1, sums += (return, length) in f64, and the env's ep_return / ep_len restart at zero.
 *   Entries the host has not read when n_episodes passes them by cap are overwritten.  OCC_ERR_ARG: a null pointer among
 *   reward / done / code / the state, n_env < 1, cap < 1, one buffer without the other, or with buffers T < 1 or t
 *   outside [0, T).
 *
 * occ_ppo_returns (one block): rewards, dones (T,n) f32 -> per env the reversed scan of PPO.py:178-185,
 *   running = fadd(r, fmul(fmul(gamma, running), 1 - done)), to raw_returns (T n) if not NULL; stats[0] = mean and
 *   stats[1] = unbiased standard deviation of the M = T n returns in f64 (two passes, a summation order fixed by M);
 *   returns (M) = fdiv(fsub(ret, (float)mean), fadd((float)std, 1e-7f)), the tensor occ_ppo_update takes.
 *   OCC_ERR_ARG: a null pointer (raw_returns may be NULL), T < 1, n_env < 1 or M < 2 (the deviation is undefined).
 */
typedef struct OccRolloutState {
    float* ep_return;             /* (n_env) */
    int32_t* ep_len;              /* (n_env) */
    int32_t* ring_env;            /* (cap) each */
    float* ring_return;
    int32_t* ring_length;
    int32_t* ring_code;
    int64_t* ring_timestep;
    float* ring_running;          /* the running reward after the entry's episode */
    int64_t* n_episodes;         /* (1) every completion ever */
    int64_t* code_counts;         /* (2) ended done, ended by the time limit */
    double* sums;                 /* (2) sum of the completed returns, of their lengths */
    float* running;               /* (1) the running reward */
} OccRolloutState;
int occ_ppo_act(const float* feats, const float* w_a, const float* b_a, const float* noise, float action_std, int n_env,
                float* action, float* logprob, float* mean, float* feat_buf, float* action_buf, float* logprob_buf, int t,
                int T, void* stream);
int occ_rollout_advance(const float* reward, const uint8_t* done, const int32_t* code, int n_env, int t, int T,
                        int64_t timestep, float* rewards, float* dones, const OccRolloutState* state, int cap, void* stream);
int occ_ppo_returns(const float* rewards, const float* dones, int T, int n_env, float gamma, float* returns,
                    float* raw_returns, double* stats, void* stream);

/*
 * Measurement hooks (bench.py only; not part of the reference surface).  While enabled, occ_render
 * brackets its dominant kernel (occ_raster2_kernel) with HIP events on the launch stream.
 * occ_profile_read synchronises the recorded events (host sync!), returns the summed duration in
 * milliseconds and the number of launches since the last read -- counting only the launches with the
 * largest n_env seen (full batches; auto-resets render tiny ones) -- and resets the ring (max 4096 launches).
 */
int occ_profile_enable(int on);
int occ_profile_read(double* ms_sum, int* launches);

#ifdef __cplusplus
}
#endif
#endif /* OCCLUSIONENV_AMD_H */
