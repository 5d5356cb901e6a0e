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


class DeviceDataset:
    """A decoded, resized dataset resident on ``device``: ``rgbl`` (M,S,S) int32 words ``R | G << 8 | B << 16 | label << 24``,
    ``depth`` (M,S,S) int16, ``pos`` and ``grad`` (M,2) f32.  Build it with ``from_directory`` or ``from_arrays``."""

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
