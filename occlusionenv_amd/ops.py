"""Operator-level drop-in for ``pytorch3d.renderer.mesh.rasterize_meshes`` as the reference reaches it through
``MeshRasterizer`` (/root/reference/environment.py:258-262, :276-280): the naive
(``bin_size=0``) rasteriser with K-buffer outputs in PyTorch3D's layout, differentiable w.r.t. ``face_verts``
through ``dists``, ``zbuf`` and ``bary_coords``.  ``OcclusionEnv.step`` does NOT go through here (it uses the fused ``occ_render``); this is for
callers of the rasteriser itself and for parity tests at that boundary.

Also here, for callers that train ``model.py`` with PyTorch-ROCm autograd: the pretrainer's segmentation criterion
(pretrainer.py:89,127-141; loss.py's ``BinaryDiceLoss``, ``nn.BCELoss`` and the accuracy / IoU counts) as ``seg_criterion``,
``binary_dice_loss`` and ``binary_cross_entropy`` (csrc/occ_criterion.hpp).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _native as nat


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class _RasterizeFaceVerts(torch.autograd.Function):
    @staticmethod
    def forward(ctx, face_verts, first_idx, num_faces, neighbor, H, W, blur_radius, K, persp, clipb, cull, naive=False):
        lib = nat.load()
        if not face_verts.is_cuda:
            raise nat.NativeError("rasterize_meshes needs CUDA/ROCm tensors; there is no CPU fallback")
        fv = face_verts.detach().contiguous().float()
        dev = fv.device
        N = int(first_idx.numel())
        first_idx = first_idx.to(dev, torch.int64).contiguous()
        num_faces = num_faces.to(dev, torch.int64).contiguous()
        nb = None if neighbor is None else neighbor.to(dev, torch.int64).contiguous()
        p2f = torch.empty(N, H, W, K, dtype=torch.int64, device=dev)
        zbuf = torch.empty(N, H, W, K, dtype=torch.float32, device=dev)
        bary = torch.empty(N, H, W, K, 3, dtype=torch.float32, device=dev)
        dists = torch.empty(N, H, W, K, dtype=torch.float32, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        fn = lib.occ_rasterize_meshes_naive if naive else lib.occ_rasterize_meshes_tiled
        nat.check(fn(_p(fv), _p(first_idx), _p(num_faces), _p(nb), N, H, W, float(blur_radius), K, int(persp), int(clipb),
                     int(cull), _p(p2f), _p(zbuf), _p(bary), _p(dists), st), "occ_rasterize_meshes")
        ctx.save_for_backward(fv, p2f)
        ctx.cfg = (N, H, W, K, int(persp), int(clipb))
        ctx.mark_non_differentiable(p2f)
        ctx.set_materialize_grads(False)
        return p2f, zbuf, bary, dists

    @staticmethod
    def backward(ctx, g_p2f, g_z, g_bary, g_dists):
        fv, p2f = ctx.saved_tensors
        N, H, W, K, persp, clipb = ctx.cfg
        if g_dists is None and g_z is None and g_bary is None:
            return (torch.zeros_like(fv),) + (None,) * 11
        lib = nat.load()
        gfv = torch.empty_like(fv)
        st = C.c_void_p(torch.cuda.current_stream(fv.device).cuda_stream)

        def c32(g):
            return None if g is None else g.contiguous().float()

        gz, gb, gd = c32(g_z), c32(g_bary), c32(g_dists)
        nat.check(lib.occ_rasterize_meshes_backward(_p(fv), _p(p2f), _p(gz), _p(gb), _p(gd), fv.shape[0], N, H, W, K, persp,
                                                    clipb, _p(gfv), st), "occ_rasterize_meshes_backward")
        return (gfv,) + (None,) * 11


def rasterize_meshes(face_verts: torch.Tensor, mesh_to_face_first_idx: torch.Tensor, num_faces_per_mesh: torch.Tensor,
                     image_size: int = 256, blur_radius: float = 0.0, faces_per_pixel: int = 8,
                     perspective_correct: bool = False, clip_barycentric_coords: bool = False,
                     cull_backfaces: bool = False, clipped_faces_neighbor_idx: Optional[torch.Tensor] = None,
                     naive: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(pix_to_face, zbuf, bary_coords, dists)`` like PyTorch3D's ``_C.rasterize_meshes`` with ``bin_size=0``.
    ``face_verts`` (F,3,3) packed (x_ndc, y_ndc, z_view) of all meshes (already z-clipped, see
    ``clipped_faces_neighbor_idx``); ``image_size`` int or (H, W).  ``naive=True`` runs the one-thread-per-pixel kernel
    over all faces instead of the tiled one (``occ_rasterize_meshes_tiled``); the outputs are bit-identical."""
    H, W = (image_size, image_size) if isinstance(image_size, int) else image_size
    return _RasterizeFaceVerts.apply(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx,
                                     int(H), int(W), blur_radius, int(faces_per_pixel), perspective_correct,
                                     clip_barycentric_coords, cull_backfaces, bool(naive))


class _SigmoidAlphaBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dists, pix_to_face, sigma):
        lib = nat.load()
        if not dists.is_cuda:
            raise nat.NativeError("sigmoid_alpha_blend needs CUDA/ROCm tensors; there is no CPU fallback")
        d = dists.detach().contiguous().float()
        p2f = pix_to_face.to(d.device, torch.int64).contiguous()
        K = d.shape[-1]
        n_pix = d.numel() // K
        images = torch.empty(d.shape[:-1] + (4,), dtype=torch.float32, device=d.device)
        st = C.c_void_p(torch.cuda.current_stream(d.device).cuda_stream)
        nat.check(lib.occ_sigmoid_alpha_blend_fwd(_p(d), _p(p2f), n_pix, K, float(sigma), _p(images), st),
                  "occ_sigmoid_alpha_blend_fwd")
        ctx.save_for_backward(d, p2f)
        ctx.sigma = float(sigma)
        return images

    @staticmethod
    def backward(ctx, g_images):
        d, p2f = ctx.saved_tensors
        lib = nat.load()
        K = d.shape[-1]
        gd = torch.empty_like(d)
        st = C.c_void_p(torch.cuda.current_stream(d.device).cuda_stream)
        nat.check(lib.occ_sigmoid_alpha_blend_bwd(_p(d), _p(p2f), _p(g_images.contiguous().float()), d.numel() // K, K,
                                                  ctx.sigma, _p(gd), st), "occ_sigmoid_alpha_blend_bwd")
        return gd, None, None


def sigmoid_alpha_blend(dists: torch.Tensor, pix_to_face: torch.Tensor, sigma: float = 1e-4) -> torch.Tensor:
    """PyTorch3D ``sigmoid_alpha_blend`` as ``SoftSilhouetteShader`` applies it (environment.py:242,263): K-buffers
    ``(N,H,W,K)`` -> RGBA images ``(N,H,W,4)`` with RGB = 1 and alpha = 1 - prod_k (1 - sigmoid(-d_k / sigma) [face >= 0]);
    differentiable w.r.t. ``dists``.  With ``rasterize_meshes`` this is the reference's silhouette renderer at
    operator level."""
    return _SigmoidAlphaBlend.apply(dists, pix_to_face, sigma)


# ---- the pretrainer's segmentation criterion (csrc/occ_criterion.hpp) ---------------------------------------------------
def _criterion_args(pred: torch.Tensor, target: torch.Tensor):
    """-> (pred (N,S,S) f32 contiguous, target (N,S,S) f32, the target's pixel stride): the checks of ``encoder._maps``
    and the stride rule of ``encoder.seg_counts``, before any native call."""
    from .encoder import _maps

    pred, target = _maps(pred, "pred").detach().contiguous(), _maps(target, "target").detach()
    if pred.shape != target.shape or pred.device != target.device:
        raise ValueError(f"pred {tuple(pred.shape)} on {pred.device} and target {tuple(target.shape)} on {target.device} differ")
    img = int(pred.shape[1])
    if img > 1024:
        raise ValueError(f"image side {img} above 1024")
    k = target.stride(2)
    if not (k >= 1 and target.stride(1) == k * img and target.stride(0) == k * img * img):
        target, k = target.contiguous(), 1
    return pred, target, int(k)


def _seg_criterion(pred: torch.Tensor, target: torch.Tensor, k: int):
    """(sums (N,4) f64, counts (N,3) int64) of checked arguments: one occ_seg_criterion per 65 535 envs."""
    lib = nat.load()
    n, img = int(pred.shape[0]), int(pred.shape[1])
    sums = torch.empty(n, 4, dtype=torch.float64, device=pred.device)
    counts = torch.empty(n, 3, dtype=torch.int64, device=pred.device)
    if n == 0:
        return sums, counts
    st = C.c_void_p(torch.cuda.current_stream(pred.device).cuda_stream)
    scratch = torch.empty(int(lib.occ_seg_criterion_scratch_bytes(min(n, 65535), img)) // 8, dtype=torch.float64, device=pred.device)
    for lo in range(0, n, 65535):
        m = min(65535, n - lo)
        nat.check(lib.occ_seg_criterion(_p(pred[lo:]), _p(target[lo:]), k, m, img, _p(sums[lo:]), _p(counts[lo:]), _p(scratch), st),
                  "occ_seg_criterion")
    return sums, counts


@torch.no_grad()
def seg_criterion(pred: torch.Tensor, target: torch.Tensor) -> dict:
    """Everything the pretrainer's segmentation criterion and its metrics need (pretrainer.py:127-141), per env, from one
    read of the maps: f64 ``s_pt`` = sum p t, ``s_pp`` = sum p^2, ``s_tt`` = sum t^2, ``s_bce`` = the sum of nn.BCELoss's
    per-pixel terms (logs clamped at -100), and the int64 ``correct``, ``intersection``, ``union`` of
    ``FrozenEncoder.occlusion_metrics``; all (N,) on the device.  pred (N,1,S,S) or (N,S,S); target likewise, soft or
    binary; a strided view such as ``full_state[..., 3]`` is read in place.  Takes no gradient: see ``binary_dice_loss``
    and ``binary_cross_entropy``.  A per-env result does not depend, bitwise, on the batch around it."""
    pred, target, k = _criterion_args(pred, target)
    sums, counts = _seg_criterion(pred, target, k)
    return dict(s_pt=sums[:, 0], s_pp=sums[:, 1], s_tt=sums[:, 2], s_bce=sums[:, 3], correct=counts[:, 0],
                intersection=counts[:, 1], union=counts[:, 2])


def dice_from_sums(s_pt, s_pp, s_tt, smooth=1.0):
    """loss.py:29-32 per env from the sums: (loss, num, den) with loss = 1 - num / den."""
    num, den = s_pt + smooth, s_pp + s_tt + smooth
    return 1.0 - num / den, num, den


def _criterion_grad(pred, target, k, mode, coef):
    lib = nat.load()
    n, img = int(pred.shape[0]), int(pred.shape[1])
    grad = torch.empty_like(pred)
    coef = coef.to(torch.float64).contiguous()
    st = C.c_void_p(torch.cuda.current_stream(pred.device).cuda_stream)
    for lo in range(0, n, 65535):
        nat.check(lib.occ_seg_criterion_grad(_p(pred[lo:]), _p(target[lo:]), k, min(65535, n - lo), img, mode, _p(coef[lo:]),
                                             _p(grad[lo:]), st), "occ_seg_criterion_grad")
    return grad


class _BinaryDiceLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, smooth, reduction):
        p, t, k = _criterion_args(pred, target)
        sums, _counts = _seg_criterion(p, t, k)
        loss, num, den = dice_from_sums(sums[:, 0], sums[:, 1], sums[:, 2], smooth)
        ctx.save_for_backward(p, t, num, den)
        ctx.cfg = (k, reduction, pred.shape, pred.dtype)
        out = loss.mean() if reduction == "mean" else loss.sum() if reduction == "sum" else loss
        return out.to(p.dtype)

    @staticmethod
    def backward(ctx, g):
        p, t, num, den = ctx.saved_tensors
        k, reduction, shape, dtype = ctx.cfg
        n = int(p.shape[0])
        if n == 0:
            return torch.zeros(shape, dtype=dtype, device=p.device), None, None, None
        u = g.to(torch.float64).expand(n) if reduction == "none" else g.to(torch.float64).reshape(1).expand(n)
        if reduction == "mean":
            u = u / n
        coef = torch.stack([-u / den, 2.0 * u * num / (den * den)], 1)  # d(1 - num/den)/dp = -t/den + 2 p num/den^2
        return _criterion_grad(p, t, k, nat.CRITERION_DICE, coef).reshape(shape).to(dtype), None, None, None


class _BinaryCrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        p, t, k = _criterion_args(pred, target)
        sums, _counts = _seg_criterion(p, t, k)
        ctx.save_for_backward(p, t)
        ctx.cfg = (k, pred.shape, pred.dtype)
        return (sums[:, 3].sum() / max(p.numel(), 1)).to(p.dtype)

    @staticmethod
    def backward(ctx, g):
        p, t = ctx.saved_tensors
        k, shape, dtype = ctx.cfg
        n = int(p.shape[0])
        if n == 0:
            return torch.zeros(shape, dtype=dtype, device=p.device), None
        coef = torch.zeros(n, 2, dtype=torch.float64, device=p.device)
        coef[:, 0] = g.to(torch.float64) / p.numel()
        return _criterion_grad(p, t, k, nat.CRITERION_BCE, coef).reshape(shape).to(dtype), None


def binary_dice_loss(pred: torch.Tensor, target: torch.Tensor, smooth: float = 1.0, reduction: str = "mean", p: int = 2) -> torch.Tensor:
    """loss.py's ``BinaryDiceLoss(smooth, p=2, reduction)(pred, target)`` (pretrainer.py:89,128): per env
    1 - (sum p t + smooth) / (sum p^2 + sum t^2 + smooth), then ``"mean"`` over the batch, ``"sum"``, or ``"none"`` ->
    (N,).  Differentiable w.r.t. ``pred`` only; one native pass forward (``seg_criterion``'s) and one backward.  The loss
    is formed in f64 and returned in pred's dtype."""
    if p != 2:
        raise ValueError(f"binary_dice_loss: only p = 2 (the reference's default and only use) is supported, got {p}")
    if reduction not in ("mean", "sum", "none"):
        raise ValueError("Unexpected reduction {}".format(reduction))
    return _BinaryDiceLoss.apply(pred, target, float(smooth), reduction)


def binary_cross_entropy(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """``nn.BCELoss()(pred, target)`` (pretrainer.py:89): the mean over all pixels of -(t log p + (1 - t) log(1 - p)) with
    both logs clamped at -100; backward (p - t) / max(p (1 - p), 1e-12) / numel.  Differentiable w.r.t. ``pred`` only."""
    return _BinaryCrossEntropy.apply(pred, target)
