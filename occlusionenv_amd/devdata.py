"""The pretraining input pipeline on the device (csrc/occ_augment.hpp, ``occ_augment_batch``): the reference's
``dataset.py`` for a dataset that is resident in device memory.

``dataset.py:53-92`` decodes, resizes, jitters (``ColorJitter(0.3, 0.3, 0.2, 0.1)``), flips, scales and normalises every
item on the CPU, every epoch.  Decoding and resizing give the same result every time, so here they happen once:
``DeviceDataset`` keeps every frame as one u32 word (R, G, B, label) and one int16 (depth) per pixel, 6 bytes, and a
batch is a gather by frame index plus the per-sample arithmetic of the jitter, the flip, ``/ 255`` and
``Normalize(0.5, 0.25)`` in two native launches.  The jitter is torchvision's PIL path rounding for rounding
(``tests/augment_model.py`` is the same arithmetic in numpy, checked against PIL), so a batch has the bits the reference's
loader would produce from the same draws.  Not reproduced: the reference's worker RNG stream (the draws come from one CPU
``torch.Generator``, vectorised over the epoch) and its second ``/ 255`` on the label (``dataset.py:82``); the label here
is 0 or 1, as ``dataset_io.OcclusionDataset`` returns it.

Batches are ``(img, occlusion, grad, pos)``, the reference's order, which is what ``harness.pretrain_epoch`` and
``harness.validate_pretrained`` unpack.  There is no CPU path: a store on the CPU (``device="cpu"``) can be inspected
(``unpack``) but ``batch`` raises.

The store can also be filled on the device (csrc/occ_datapack.hpp, ``occ_dataset_pack``): ``DeviceDataset.empty`` plus
``put`` per engine step, which is what ``generate_resident`` does in ``dataset_io.generate``'s loop.  ``put`` gives a frame
the bits the writer and ``from_directory`` at the same size would (``tests/datapack_model.py``), the JPEG apart unless
``put(jpeg=quality)`` asks for it (below).

The resize is reproduced too (csrc/occ_resize.hpp, ``occ_dataset_resize``): the reference renders 512 x 512 and its reader
shrinks every item to 256 x 256 with ``Image.resize`` (``dataset.py:65-67``: bicubic for the colours and the depth, nearest
for the dithered label).  ``put(resize=True)`` packs at the rendering size and resizes into the store,
``generate_resident(size=256)`` does that for every step of an env that renders at 512, and ``resized`` does it to a whole
store; the arithmetic is PIL's bit for bit (``tests/resize_model.py``, checked against PIL and against the files).

So is the JPEG (csrc/occ_jpeg.hpp, ``occ_dataset_jpeg``), the one lossy stage of that path: the reference writes every
colour image as a 4:2:0 baseline JPEG at the rendering size (``datasetGenerator.py:104``) and trains on the decoded result.
Entropy coding is lossless, so writing and reading the file is integer arithmetic on the pixels and two quantisation tables
(``tests/jpeg_model.py``, checked against PIL's save and open bit for bit).  ``DeviceDataset.jpeg(quality)`` does it in
place, ``put(jpeg=quality)`` where the file would be written (after the pack at the rendering size, before the resize) and
``generate_resident(jpeg=quality)`` in every step.  ``cv2.imwrite``, the reference's writer, defaults to quality 95 and
PIL's ``save`` to 75; ``dataset_io.RunWriter(jpeg_quality=)`` sets it for the files.  So from the engine's step to the batch
everything is on the device, with the bits the reference's files-and-PIL path would give, colours included.
Still not reproduced: the worker RNG stream (above), and the pairing ``from_directory`` inherits from the
reference's lexicographic file sort (``0, 1, 10, .., 19, 2, ..`` against numerically ordered labels: images of runs with
more than 10 frames get other frames' ``pos`` / ``grad``); a generated store is run-major, frame ``j`` numeric, every image
with its own labels.
"""
from __future__ import annotations

import ctypes as C
import glob
import os.path as osp
import pickle

import numpy as np
import torch
from PIL import Image

from . import _native as nat

#: one record of ``OccAugmentParams`` (include/occlusionenv_amd.h), 32 bytes
PARAMS_DTYPE = np.dtype([("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"), ("hue_shift", "<i4"),
                         ("order", "<i4"), ("jitter", "<i4"), ("flip", "<i4"), ("pad", "<i4")])
assert PARAMS_DTYPE.itemsize == C.sizeof(nat.OccAugmentParams) == 32

#: ``label_mode`` of ``occ_dataset_pack``
LABEL_MODES = {"dither": 0, "threshold": 1}


def draw_params(n: int, generator: torch.Generator, jitter=(0.3, 0.3, 0.2, 0.1), flip: float = 0.5) -> np.ndarray:
    """``n`` records of ``PARAMS_DTYPE`` drawn from the CPU ``generator`` as ``ColorJitter.get_params`` and
    ``dataset.py:72`` draw them per item: a permutation of the four ops (brightness 0, contrast 1, saturation 2, hue 3;
    the first op in the low two bits of ``order``), brightness / contrast / saturation uniform in ``[max(0, 1 - x), 1 + x]``,
    hue uniform in ``[-h, h]``, and the flip coin (``rand > 1 - flip``).  The hue factor becomes the byte torchvision adds
    to the H band: ``int(hue * 255) & 255``, a truncation toward zero, then the wrap.  ``jitter=None``: no jitter;
    ``flip=0``: no flip."""
    n = int(n)
    p = np.zeros(n, PARAMS_DTYPE)
    p["brightness"] = p["contrast"] = p["saturation"] = 1.0
    p["order"] = 0 | 1 << 2 | 2 << 4 | 3 << 6
    if jitter is not None:
        b, c, s, h = (float(x) for x in jitter)
        if min(b, c, s) < 0 or not 0 <= h <= 0.5:
            raise ValueError("draw_params: jitter = (brightness, contrast, saturation, hue) with hue in [0, 0.5]")
        perm = torch.rand(n, 4, generator=generator).argsort(1).to(torch.int32)
        u = torch.rand(n, 4, generator=generator, dtype=torch.float32)
        for k, (name, x) in enumerate((("brightness", b), ("contrast", c), ("saturation", s))):
            lo, hi = max(0.0, 1.0 - x), 1.0 + x
            p[name] = np.clip((lo + (hi - lo) * u[:, k]).numpy(), np.float32(lo), np.float32(hi))
        hue = (-h + 2.0 * h * u[:, 3].double()).numpy()
        p["hue_shift"] = np.trunc(hue * 255.0).astype(np.int32) & 255
        p["order"] = (perm[:, 0] | perm[:, 1] << 2 | perm[:, 2] << 4 | perm[:, 3] << 6).numpy()
        p["jitter"] = 1
    if flip:
        p["flip"] = (torch.rand(n, generator=generator) > 1.0 - float(flip)).to(torch.int32).numpy()
    return p


def _params_tensor(params: np.ndarray) -> torch.Tensor:
    """The records as an (n, 8) int32 host tensor (the three factors as their f32 bits)."""
    params = np.ascontiguousarray(params)
    if params.dtype != PARAMS_DTYPE or params.ndim != 1:
        raise ValueError("params: a 1-d array of devdata.PARAMS_DTYPE records (devdata.draw_params)")
    return torch.from_numpy(params.view(np.int32).reshape(-1, 8))


def sincos_grad(grad: np.ndarray) -> np.ndarray:
    """``dataset.py:84-89`` for every row of an (M, 2) f64 array: ``alpha = arctan(g0 / g1)``, nan -> 0, ``(sin, cos)``
    in f64, rounded to f32."""
    g = torch.from_numpy(np.ascontiguousarray(grad, dtype=np.float64).reshape(-1, 2))
    alpha = torch.arctan(g[:, 0] / g[:, 1])
    alpha[torch.isnan(alpha)] = 0
    return torch.stack([torch.sin(alpha), torch.cos(alpha)], 1).float().numpy()


def resize_workspace_bytes(src_size: int, dst_size: int, n: int = 1) -> int:
    """``occ_dataset_resize_query``: the workspace of a resize of ``n`` frames from ``src_size`` to ``dst_size``, or
    ``ValueError`` for a pair of sizes the kernel does not take (csrc/occ_resize.hpp: ``src / dst <= 2``, any upscaling,
    any ``dst`` for ``src <= 72``; both within 1 .. 4096).  No GPU is touched."""
    need = C.c_size_t()
    if nat.load().occ_dataset_resize_query(int(src_size), int(dst_size), int(n), C.byref(need)) != 0:
        raise ValueError("resize %d -> %d of %d frames is not supported: sizes in 1 .. 4096, src / dst <= 2 or src <= 72, "
                         "1 .. 65535 frames" % (src_size, dst_size, n))
    return int(need.value)


def _quality(jpeg, who: str) -> int:
    if isinstance(jpeg, bool) or not isinstance(jpeg, (int, np.integer)) or not 1 <= int(jpeg) <= 100:
        raise ValueError("%s: the JPEG quality is an integer in 1 .. 100" % who)
    return int(jpeg)


def jpeg_workspace_bytes(size: int, n: int = 1, quality: int = 75) -> int:
    """``occ_dataset_jpeg_query``: the workspace of a JPEG round trip of ``n`` frames of ``size`` x ``size`` pixels, or
    ``ValueError`` for what the library refuses (``size`` outside 1 .. 4096, ``n`` outside 1 .. 65535, ``quality`` outside
    1 .. 100).  No GPU is touched."""
    need = C.c_size_t()
    if nat.load().occ_dataset_jpeg_query(int(size), int(n), int(quality), C.byref(need)) != 0:
        raise ValueError("JPEG round trip of %d frames of %d x %d at quality %d is not supported: sizes in 1 .. 4096, "
                         "1 .. 65535 frames, quality 1 .. 100" % (n, size, size, quality))
    return int(need.value)


class DeviceDataset:
    """A decoded, resized dataset resident on ``device``: ``rgbl`` (M,S,S) int32 words ``R | G << 8 | B << 16 | label << 24``,
    ``depth`` (M,S,S) int16, ``pos`` and ``grad`` (M,2) f32.  Build it with ``from_directory`` or ``from_arrays``, or
    ``empty`` and ``put`` (``generate_resident``)."""

    def __init__(self, rgbl: torch.Tensor, depth: torch.Tensor, pos: torch.Tensor, grad: torch.Tensor, split: str = ""):
        M, S = rgbl.shape[0], rgbl.shape[1]
        if rgbl.dtype != torch.int32 or depth.dtype != torch.int16 or rgbl.shape != (M, S, S) or depth.shape != (M, S, S):
            raise ValueError("DeviceDataset: rgbl (M,S,S) int32 and depth (M,S,S) int16")
        if pos.shape != (M, 2) or grad.shape != (M, 2) or pos.dtype != torch.float32 or grad.dtype != torch.float32:
            raise ValueError("DeviceDataset: pos and grad (M,2) float32")
        if M < 1 or S < 1 or S * S > 1 << 24:
            raise ValueError("DeviceDataset: at least one frame, S^2 <= 2^24")
        self.rgbl, self.depth, self.pos, self.grad = (t.contiguous() for t in (rgbl, depth, pos, grad))
        self.split, self.size, self.device = split, S, rgbl.device
        self._staging = {}  # (n, R) -> the store put(resize=True) packs n frames of R x R into

    def __len__(self) -> int:
        return self.rgbl.shape[0]

    @classmethod
    def from_arrays(cls, rgb_u8, depth_i16, label_u8, pos, grad, device, split: str = "", grad_mode: str = "sincos"):
        """``rgb_u8`` (M,S,S,3) uint8, ``depth_i16`` (M,S,S) integers that fit int16, ``label_u8`` (M,S,S) (non-zero = 1),
        ``pos`` and ``grad`` (M,2).  ``grad_mode="sincos"`` stores ``sincos_grad(grad)``, ``"raw"`` the pair as it is."""
        if grad_mode not in ("sincos", "raw"):
            raise ValueError("grad_mode: 'sincos' or 'raw'")
        rgb = np.asarray(rgb_u8)
        if rgb.dtype != np.uint8 or rgb.ndim != 4 or rgb.shape[3] != 3 or rgb.shape[1] != rgb.shape[2]:
            raise ValueError("rgb_u8: (M,S,S,3) uint8")
        d = np.asarray(depth_i16)
        if d.shape != rgb.shape[:3] or d.dtype.kind not in "iu" or (d.size and (d.min() < -32768 or d.max() > 32767)):
            raise ValueError("depth_i16: (M,S,S) integers within int16")
        lab = np.asarray(label_u8)
        if lab.shape != rgb.shape[:3]:
            raise ValueError("label_u8: (M,S,S)")
        c = rgb.astype(np.uint32)
        word = c[..., 0] | c[..., 1] << 8 | c[..., 2] << 16 | (lab != 0).astype(np.uint32) << 24
        g = np.asarray(grad, dtype=np.float64).reshape(-1, 2)
        g32 = sincos_grad(g) if grad_mode == "sincos" else g.astype(np.float32)
        dev = torch.device(device)
        return cls(torch.from_numpy(word.view(np.int32)).to(dev), torch.from_numpy(d.astype(np.int16)).to(dev),
                   torch.from_numpy(np.asarray(pos, dtype=np.float64).reshape(-1, 2).astype(np.float32)).to(dev),
                   torch.from_numpy(np.ascontiguousarray(g32)).to(dev), split=split)

    @classmethod
    def from_directory(cls, root: str, split: str = "", size=(256, 256), device="cuda", grad_mode: str = "sincos"):
        """The files of ``dataset_io.OcclusionDataset(root, split, size)`` (same discovery, same label parsing), every
        frame decoded and resized once exactly as that reader does (RGB with the default filter, depth in mode "I", the
        label in mode "1"); ``size`` must be square."""
        if size[0] != size[1]:
            raise ValueError("DeviceDataset: size must be square")
        base = osp.join(root, split)
        images = sorted(glob.glob(base + "/**/RGB/*.jpg", recursive=True))
        depths = sorted(glob.glob(base + "/**/Depth/*.png", recursive=True))
        labels = sorted(glob.glob(base + "/**/Occl/*.png", recursive=True))
        pos, grad = [], []
        for lfile in sorted(glob.glob(base + "/**/*.pickle", recursive=True)):
            with open(lfile, "rb") as fh:
                arr = np.asarray(pickle.load(fh)).reshape([-1, 5])
            pos.append(arr[:, 1:3])
            grad.append(arr[:, 3:5])
        M = sum(a.shape[0] for a in pos)
        if M < 1 or not len(images) == len(depths) == len(labels) == M:
            raise ValueError("DeviceDataset: %d labels, %d / %d / %d RGB / Depth / Occl files under %s"
                             % (M, len(images), len(depths), len(labels), base))
        S = int(size[0])
        rgb, dep, lab = np.empty((M, S, S, 3), np.uint8), np.empty((M, S, S), np.int32), np.empty((M, S, S), np.uint8)
        for i in range(M):
            rgb[i] = np.asarray(Image.open(images[i]).convert("RGB").resize(size))
            dep[i] = np.asarray(Image.open(depths[i]).convert("I").resize(size))
            lab[i] = np.asarray(Image.open(labels[i]).convert("1").resize(size))
        return cls.from_arrays(rgb, dep, lab, np.concatenate(pos, 0), np.concatenate(grad, 0), device, split=split,
                               grad_mode=grad_mode)

    @classmethod
    def empty(cls, m_frames: int, size: int, device, split: str = ""):
        """A zeroed store of ``m_frames`` frames of ``size`` x ``size`` pixels on ``device``, to be filled with ``put``."""
        M, S, dev = int(m_frames), int(size), torch.device(device)
        if M < 1 or S < 1:
            raise ValueError("DeviceDataset.empty: at least one frame of at least one pixel")
        return cls(torch.zeros((M, S, S), dtype=torch.int32, device=dev), torch.zeros((M, S, S), dtype=torch.int16, device=dev),
                   torch.zeros((M, 2), dtype=torch.float32, device=dev), torch.zeros((M, 2), dtype=torch.float32, device=dev),
                   split=split)

    def _resize_into(self, src_rgbl: torch.Tensor, src_depth: torch.Tensor, slots_dev: torch.Tensor) -> None:
        """One ``occ_dataset_resize``: frame ``i`` of the (n,R,R) pair on this store's device into frame ``slots_dev[i]``."""
        n, R = int(src_rgbl.shape[0]), int(src_rgbl.shape[1])
        lib = nat.load()
        with torch.cuda.device(self.device):
            ws = torch.empty(resize_workspace_bytes(R, self.size, n) // 4, dtype=torch.int32, device=self.device)
            nat.check(lib.occ_dataset_resize(nat.ptr(src_rgbl), nat.ptr(src_depth), n, R, nat.ptr(slots_dev), nat.ptr(self.rgbl),
                                             nat.ptr(self.depth), len(self), self.size, nat.ptr(ws), nat.stream_ptr(self.device)),
                      "occ_dataset_resize")

    def resized(self, size: int) -> "DeviceDataset":
        """A new store of ``size`` x ``size`` frames on the same device: every frame through ``occ_dataset_resize``
        (csrc/occ_resize.hpp), which is PIL's ``Image.resize`` as the reference's reader calls it (bicubic colours and
        depth, nearest label; tests/resize_model.py); ``pos``, ``grad`` and ``split`` are carried over.
        ``size == self.size`` gives a copy."""
        if isinstance(size, bool) or not isinstance(size, (int, np.integer)):
            raise ValueError("resized: size is an integer")
        S = int(size)
        if S == self.size:
            return DeviceDataset(self.rgbl.clone(), self.depth.clone(), self.pos.clone(), self.grad.clone(), split=self.split)
        resize_workspace_bytes(self.size, S)  # ValueError for sizes the kernel does not take
        if self.device.type != "cuda":
            raise nat.NativeError("DeviceDataset.resized runs on the GPU only (this store is on %s); there is no CPU path" % self.device)
        out = DeviceDataset.empty(len(self), S, self.device, split=self.split)
        out.pos.copy_(self.pos)
        out.grad.copy_(self.grad)
        for lo, rows in nat.row_chunks(len(self), 65535):
            out._resize_into(self.rgbl[lo:lo + rows], self.depth[lo:lo + rows],
                             torch.arange(lo, lo + rows, dtype=torch.int64, device=self.device))
        return out

    def _jpeg_slots(self, slots_dev: torch.Tensor, quality: int) -> None:
        """One ``occ_dataset_jpeg`` on the frames ``slots_dev`` (int64 on this store's device, at most 65535)."""
        n = int(slots_dev.shape[0])
        with torch.cuda.device(self.device):
            ws = torch.empty(jpeg_workspace_bytes(self.size, n, quality) // 2, dtype=torch.int16, device=self.device)
            nat.check(nat.load().occ_dataset_jpeg(nat.ptr(self.rgbl), len(self), self.size, nat.ptr(slots_dev), n, quality,
                                                  nat.ptr(ws), nat.stream_ptr(self.device)), "occ_dataset_jpeg")

    def jpeg(self, quality: int, frames=None) -> None:
        """The colours of all frames, or of the distinct frame numbers ``frames`` (a host tensor or a list), through
        ``occ_dataset_jpeg`` (csrc/occ_jpeg.hpp) in place: what ``Image.save(format="JPEG", quality=quality)`` and
        ``Image.open(...).convert("RGB")`` do to them (libjpeg's 4:2:0 baseline round trip; tests/jpeg_model.py).  Depth,
        label, ``pos`` and ``grad`` stay."""
        q = _quality(quality, "jpeg")
        jpeg_workspace_bytes(self.size, 1, q)  # ValueError for a size the kernel does not take
        idx = None
        if frames is not None:
            idx = torch.as_tensor(frames).reshape(-1)
            if idx.is_floating_point() or idx.dtype == torch.bool:
                raise ValueError("jpeg: frames are integers")
            idx = idx.to("cpu", torch.int64)
            if idx.numel() < 1 or int(idx.min()) < 0 or int(idx.max()) >= len(self) or idx.unique().numel() != idx.numel():
                raise ValueError("jpeg: frames are distinct frame numbers in [0, %d)" % len(self))
        if self.device.type != "cuda":
            raise nat.NativeError("DeviceDataset.jpeg runs on the GPU only (this store is on %s); there is no CPU path" % self.device)
        if idx is None:
            idx = torch.arange(len(self), dtype=torch.int64)
        idx = idx.to(self.device)
        for lo, rows in nat.row_chunks(int(idx.numel()), 65535):
            self._jpeg_slots(idx[lo:lo + rows].contiguous(), q)

    def put(self, obs: torch.Tensor, full_state: torch.Tensor, slots, pos=None, grad=None, label: str = "dither",
            resize: bool = False, jpeg=None) -> None:
        """Write the frames of one engine step into the store, on the device, in one ``occ_dataset_pack`` call
        (csrc/occ_datapack.hpp): env ``i`` of ``obs`` (n,4,S,S) and ``full_state`` (n,S,S,4; its alpha channel is the
        occlusion image; an (n,S,S) alpha image is taken too) becomes frame ``slots[i]`` with the bits
        ``dataset_io.RunWriter`` and ``from_directory`` at the same size would give it, the JPEG apart (see ``jpeg``):
        ``img_as_ubyte``
        colours with B and R swapped, ``depth * 51`` truncated, and the label by ``label="dither"`` (PIL's
        ``convert("1")`` of the 8-bit alpha, what the reader does to the file) or ``"threshold"`` (``alpha > 0.5``, the
        rule of ``pretrainer.py:134``).  ``slots``: n int64 on the device or the host; an env whose slot is outside
        ``[0, len(self))`` is skipped, in-range slots must be distinct.  ``pos`` / ``grad``: (n,2) rows stored as they are
        for the slots in range (an indexed copy; selecting the rows reads the mask back, so a caller that must not
        synchronise keeps its labels itself, as ``generate_resident`` does).

        ``resize=False``: there is no resize, ``obs`` has the store's size.  ``resize=True``: an ``obs`` of another size
        R x R is packed at R (either label rule; the dither runs at R) into a staging store of ``n`` frames that the
        dataset keeps per ``(n, R)``, and the staged frames go through ``occ_dataset_resize`` (csrc/occ_resize.hpp) into
        ``slots``: the bits of the writer at R and ``from_directory`` at the store's size, the JPEG apart (see ``jpeg``).  With R
        equal to the store's size it is the single pack call.

        ``jpeg``: None, or the quality (1 .. 100) of the JPEG round trip (``occ_dataset_jpeg``, csrc/occ_jpeg.hpp) that
        then runs on the packed colours where the writer's file would be: after the pack at R, before the resize, so on
        the staging store with ``resize=True`` and R != S, on the named slots otherwise.  The frames then have the bits of
        ``RunWriter(jpeg_quality=jpeg)`` and ``from_directory``, colours included."""
        if label not in LABEL_MODES:
            raise ValueError("label: 'dither' or 'threshold'")
        q = None if jpeg is None else _quality(jpeg, "put")
        S = self.size
        if obs.ndim != 4 or obs.shape[1] != 4 or obs.shape[-1] != obs.shape[-2] or (not resize and obs.shape[-1] != S):
            raise ValueError("put: obs (n,4,%d,%d): the env renders at the dataset's size (resize=True: at any square size)" % (S, S))
        n, R = int(obs.shape[0]), int(obs.shape[-1])
        if tuple(full_state.shape) not in ((n, R, R, 4), (n, R, R)):
            raise ValueError("put: full_state (n,%d,%d,4) or an alpha image (n,%d,%d)" % (R, R, R, R))
        if not 1 <= n <= 65535:
            raise ValueError("put: 1 .. 65535 envs")
        s = torch.as_tensor(slots)
        if s.is_floating_point() or s.dtype == torch.bool or s.numel() != n:
            raise ValueError("put: slots are n integers")
        if R != S:
            resize_workspace_bytes(R, S, n)  # ValueError for sizes the kernel does not take
        if q is not None:
            jpeg_workspace_bytes(R, n, q)
        if self.device.type != "cuda":
            raise nat.NativeError("DeviceDataset.put runs on the GPU only (this store is on %s); there is no CPU path" % self.device)
        s = s.reshape(n).to(self.device, torch.int64).contiguous()
        obs = obs.detach().to(self.device, torch.float32).contiguous()
        fs = full_state.detach().to(self.device, torch.float32).contiguous()
        stride = 4 if fs.ndim == 4 else 1
        with torch.cuda.device(self.device):
            into, into_slots = self, s
            if R != S:
                into = self._staging.get((n, R))
                if into is None:
                    into = self._staging[(n, R)] = DeviceDataset.empty(n, R, self.device)
                ok = (s >= 0) & (s < len(self))
                into_slots = torch.where(ok, torch.arange(n, dtype=torch.int64, device=self.device), torch.full_like(s, -1))
            nat.check(nat.load().occ_dataset_pack(nat.ptr(obs), nat.ptr(fs, 12 if stride == 4 else 0), stride, n, R,
                                                  nat.ptr(into_slots), nat.ptr(into.rgbl), nat.ptr(into.depth), len(into),
                                                  LABEL_MODES[label], nat.stream_ptr(self.device)), "occ_dataset_pack")
            if q is not None:
                into._jpeg_slots(into_slots, q)
            if R != S:
                self._resize_into(into.rgbl, into.depth, s)
            if pos is not None or grad is not None:
                ok = (s >= 0) & (s < len(self))
                for dst, src in ((self.pos, pos), (self.grad, grad)):
                    if src is not None:
                        src = torch.as_tensor(src).to(self.device, torch.float32).reshape(n, 2)
                        dst[s[ok]] = src[ok]

    def unpack(self, i: int):
        """Frame ``i`` of the store on the host: ``(rgb (S,S,3) uint8, depth (S,S) int16, label (S,S) uint8)``."""
        w = self.rgbl[i].cpu().numpy().view(np.uint32)
        rgb = np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], -1).astype(np.uint8)
        return rgb, self.depth[i].cpu().numpy(), (w >> 24).astype(np.uint8)

    def _run(self, idx_dev: torch.Tensor, params_dev, normalize: bool):
        """One ``occ_augment_batch``: ``idx_dev`` (n,) int64 and ``params_dev`` (n,8) int32 or None, on the device."""
        if self.device.type != "cuda":
            raise nat.NativeError("DeviceDataset.batch runs on the GPU only (this store is on %s); there is no CPU path" % self.device)
        lib = nat.load()
        n, S = int(idx_dev.shape[0]), self.size
        with torch.cuda.device(self.device):
            opt = dict(dtype=torch.float32, device=self.device)
            img, occl = torch.empty((n, 4, S, S), **opt), torch.empty((n, 1, S, S), **opt)
            grad, pos = torch.empty((n, 2), **opt), torch.empty((n, 2), **opt)
            ws = None
            if params_dev is not None:
                need = C.c_size_t()
                nat.check(lib.occ_augment_query(S, n, C.byref(need)), "occ_augment_query")
                ws = torch.empty(need.value // 4, dtype=torch.int32, device=self.device)
            nat.check(lib.occ_augment_batch(nat.ptr(self.rgbl), nat.ptr(self.depth), nat.ptr(self.pos), nat.ptr(self.grad), len(self),
                                            S, nat.ptr(idx_dev), nat.ptr(params_dev), n, int(bool(normalize)), nat.ptr(img),
                                            nat.ptr(occl), nat.ptr(grad), nat.ptr(pos), nat.ptr(ws), nat.stream_ptr(self.device)),
                      "occ_augment_batch")
        return img, occl, grad, pos

    def _check_indices(self, indices) -> torch.Tensor:
        idx = torch.as_tensor(indices).reshape(-1)
        if idx.is_cuda or idx.is_floating_point() or idx.dtype == torch.bool:
            raise ValueError("indices: a host tensor or list of integers")
        idx = idx.to(torch.int64)
        if idx.numel() < 1 or idx.numel() > 65535 or int(idx.min()) < 0 or int(idx.max()) >= len(self):
            raise ValueError("indices: 1 .. 65535 frame numbers in [0, %d)" % len(self))
        return idx

    def batch(self, indices, params=None, normalize: bool = True):
        """``(img (n,4,S,S), occlusion (n,1,S,S), grad (n,2), pos (n,2))`` of the frames ``indices`` (a host tensor or a
        list; checked against the store on the host; repeats and any order allowed), f32 on the device, fresh tensors.
        ``params``: ``n`` records of ``PARAMS_DTYPE`` (``draw_params``); None: no jitter, no flip, one launch instead of
        two.  ``normalize``: ``(x - 0.5) / 0.25`` on the four planes of ``img``, as ``dataset.py:81``."""
        idx = self._check_indices(indices)
        pt = None
        if params is not None:
            pt = _params_tensor(params)
            if pt.shape[0] != idx.numel():
                raise ValueError("params: one record per index")
            pt = pt.to(self.device)
        return self._run(idx.to(self.device), pt, normalize)

    def loader(self, batch_size: int = 128, shuffle: bool = True, train=None, generator=None, drop_last: bool = False,
               normalize: bool = True, jitter=(0.3, 0.3, 0.2, 0.1), flip: float = 0.5):
        """A re-iterable of batches with ``__len__``, for ``harness.pretrain`` / ``pretrain_epoch`` / ``validate_pretrained``.
        ``train`` (default: ``split == "train"``) switches jitter and flip on, as ``dataset.py:69``.  See ``EpochLoader``."""
        return EpochLoader(self, batch_size, shuffle, self.split == "train" if train is None else bool(train), generator,
                           drop_last, normalize, jitter, flip)


class EpochLoader:
    """Every ``iter()`` draws a fresh permutation (``shuffle``) and fresh parameters (``train``) for the whole epoch from
    ``generator`` (a CPU ``torch.Generator``; None: a new one seeded from torch's global RNG), uploads the epoch's indices
    and parameters in one copy each, and yields one ``occ_augment_batch`` per batch.

    Lifetime: every batch is four freshly allocated tensors that nothing here touches again, so a consumer may keep any
    number of batches.  Only the epoch's index and parameter uploads are shared between the batches of one epoch; they are
    read-only and stay alive as long as the iterator does."""

    def __init__(self, ds: DeviceDataset, batch_size: int, shuffle: bool, train: bool, generator, drop_last: bool,
                 normalize: bool, jitter, flip: float):
        if not 1 <= int(batch_size) <= 65535:
            raise ValueError("batch_size: 1 .. 65535")
        if generator is None:
            generator = torch.Generator().manual_seed(int(torch.empty((), dtype=torch.int64).random_()))
        self.ds, self.batch_size, self.shuffle, self.train = ds, int(batch_size), bool(shuffle), bool(train)
        self.generator, self.drop_last, self.normalize, self.jitter, self.flip = generator, bool(drop_last), normalize, jitter, flip

    def __len__(self) -> int:
        M, B = len(self.ds), self.batch_size
        return M // B if self.drop_last else (M + B - 1) // B

    def __iter__(self):
        ds, M, B = self.ds, len(self.ds), self.batch_size
        order = torch.randperm(M, generator=self.generator) if self.shuffle else torch.arange(M)
        params = None
        if self.train and (self.jitter is not None or self.flip):
            params = _params_tensor(draw_params(M, self.generator, self.jitter, self.flip)).to(ds.device)
        order = order.to(ds.device)
        for b in range(len(self)):
            lo, hi = b * B, min(M, (b + 1) * B)
            yield ds._run(order[lo:hi], None if params is None else params[lo:hi], self.normalize)


def generate_resident(venv, num_runs: int, num_frames: int = 20, lr: float = 2.5e-2, generator=None, max_steps: int = 0,
                      label: str = "dither", grad_mode: str = "sincos", split: str = "train", size=None,
                      jpeg=None) -> DeviceDataset:
    """``dataset_io.generate``'s loop (datasetGenerator.py:76-124) into a ``DeviceDataset`` instead of files: ``num_runs``
    runs of ``num_frames`` frames at the env's own size, frame ``j`` of run ``r`` at index ``r * num_frames + j`` with its
    own ``pos`` (elevation, azimuth) and ``grad``.  Nothing of a frame leaves the device: every step is one
    ``DeviceDataset.put``, and the frame counters, the mask of written frames and the slots are device tensors; one scalar
    per step comes back, for the loop condition.

    The semantics are ``generate``'s: one scene per run, the engine stepped directly after ``reset()`` and ``_drain()``, a
    frame whose gradient is NaN retried with the SAME action without advancing that run's counter, a fresh action only
    after a written frame, ``RuntimeError`` after ``max_steps`` (default ``50 * num_frames``) steps of a round.  With the
    same ``generator`` and ``num_runs == venv.num_envs`` the actions are the ones ``generate`` draws.  ``num_runs`` above
    ``venv.num_envs`` runs in rounds of ``num_envs`` with a ``reset()`` between them; the envs of a last partial round
    beyond ``num_runs`` write nothing.  ``grad_mode="sincos"`` turns the raw f32 gradients into ``sincos_grad`` at the end
    (M x 2 values, on the host: the bits ``from_directory`` computes from the pickled values), ``"raw"`` keeps them.

    ``size``: None stores the frames at the env's own size.  Another ``size`` gives a store of that size, every step going
    through ``put(resize=True)``: rendered at the env's size (the reference: 512), packed there, resized on the device as
    the reference's reader resizes its files (to 256), see ``DeviceDataset.put``.

    ``jpeg``: None, or the JPEG quality every ``put`` is given: the colours go through the writer's JPEG at the rendering
    size, as ``dataset_io.generate(jpeg_quality=)`` followed by ``from_directory`` would have them."""
    if grad_mode not in ("sincos", "raw"):
        raise ValueError("grad_mode: 'sincos' or 'raw'")
    if label not in LABEL_MODES:
        raise ValueError("label: 'dither' or 'threshold'")
    num_runs, num_frames = int(num_runs), int(num_frames)
    if num_runs < 1 or num_frames < 1:
        raise ValueError("generate_resident: at least one run of one frame")
    eng, N = venv.engine, venv.num_envs
    dev, M = eng.device, num_runs * num_frames
    if jpeg is not None:
        jpeg_workspace_bytes(eng.S, N, _quality(jpeg, "generate_resident"))  # ValueError for what the kernel does not take
        if dev.type != "cuda":
            raise nat.NativeError("generate_resident(jpeg=) runs on the GPU only (the engine is on %s); there is no CPU path" % dev)
    if size is not None:
        if isinstance(size, bool) or not isinstance(size, (int, np.integer)):
            raise ValueError("generate_resident: size is an integer or None")
        if int(size) != eng.S:
            resize_workspace_bytes(eng.S, int(size), N)  # ValueError for sizes the kernel does not take
            if dev.type != "cuda":
                raise nat.NativeError("generate_resident(size=) runs on the GPU only (the engine is on %s); there is no CPU path" % dev)
    ds = DeviceDataset.empty(M, eng.S if size is None else int(size), dev, split=split)
    # row M takes what the envs without a frame in a step scatter
    elaz = torch.zeros((M + 1, 2), dtype=torch.float32, device=dev)
    graw = torch.zeros((M + 1, 2), dtype=torch.float32, device=dev)
    limit = max_steps or 50 * num_frames
    for first in range(0, num_runs, N):
        venv.reset()
        venv._drain()  # no auto-reset report may be pending while the engine is driven directly
        run = first + torch.arange(N, dtype=torch.int64, device=dev)
        live = run < num_runs
        frame = torch.zeros(N, dtype=torch.int64, device=dev)
        action = lr * torch.randn(N, 2, device=dev, generator=generator)
        steps = 0
        while True:
            pending = live & (frame < num_frames)
            if not bool(pending.any()):  # the one value read back per step
                break
            if steps >= limit:
                raise RuntimeError("generate_resident(): gradients stayed NaN for %d steps" % steps)
            steps += 1
            a = action.clone().requires_grad_(True)
            obs, rewards, dones, full_state, loss = eng.step(a)
            rewards.sum().backward()
            g = a.grad.detach()
            good = pending & ~torch.isnan(g).any(1)
            slot = torch.where(good, run * num_frames + frame, torch.full_like(frame, -1))
            ds.put(obs, full_state, slot, label=label, resize=size is not None, jpeg=jpeg)
            row = torch.where(good, slot, torch.full_like(frame, M))
            elaz[row] = torch.stack([eng.elevation.reshape(N), eng.azimuth.reshape(N)], 1).to(torch.float32)
            graw[row] = g.to(torch.float32)
            fresh = lr * torch.randn(N, 2, device=dev, generator=generator)
            frame = frame + good.to(torch.int64)
            action = torch.where(good[:, None], fresh, action)  # a new action only after a frame was written
    ds.pos = elaz[:M].contiguous()
    g = graw[:M].cpu().numpy().astype(np.float64)
    ds.grad = torch.from_numpy(np.ascontiguousarray(sincos_grad(g) if grad_mode == "sincos" else g.astype(np.float32))).to(dev)
    return ds
