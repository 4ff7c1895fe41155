"""The reference's input pipeline on the GPU, from the decoded image on.

`collate_images`: the tail only -- `ToTensor` + `Normalize(mean, std)` of the image transforms (modules/lightning_modules/single.py:248-262) and
the `pad_sequence(..., padding_value=0.0)` of `collate_fn` (multi.py:155-164) in one kernel, from already resized and cropped uint8 images.

`StudyImageTransform`: the whole transform (single.py:229-262) from the decoded full-size uint8 images -- `Resize(384)` -> `CenterCrop(384)`
(test) or `RandomCrop(384, pad_if_needed)` -> `RandomRotation(5)` (train) -> `ToTensor` -> `Normalize` -> `pad_sequence` -- in two launches per
batch (csrc/pixels_transform.hip), byte-identical to what torchvision's PIL backend computes: Pillow's antialiased bilinear `Image.resize` (two
8-bit passes with 22-bit integer weights) and its nearest-neighbour `Image.rotate` (16.16 fixed point). The weight tables and the rotation
integers are computed HERE, on the host, in float64 and in Pillow's operation order (the device library is built with -ffp-contract=fast and does
integer work only). Only JPEG decode stays in the dataloader workers; what crosses PCIe is the decoded 8-bit image.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from ._lib import LIB

IMAGENET_MEAN = (0.485, 0.456, 0.406)          # image_processor.image_mean / image_std of microsoft/cvt-21-384-22k
IMAGENET_STD = (0.229, 0.224, 0.225)


def collate_images(studies, device, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """studies: list (one entry per study) of uint8 tensors [n_i, H, W, 3] (HWC, as PIL / decode hands them over).
    -> `images` fp32 [B, max n_i, 3, H, W] on `device`, normalised, zero-padded like the reference batch['images']."""
    counts = [int(s.shape[0]) for s in studies]
    H, W = int(studies[0].shape[1]), int(studies[0].shape[2])
    packed = torch.cat([s.reshape(-1, H, W, 3) for s in studies], dim=0).contiguous()
    assert packed.dtype == torch.uint8
    first = torch.zeros(len(studies) + 1, dtype=torch.int64)
    first[1:] = torch.cumsum(torch.tensor(counts, dtype=torch.int64), 0)
    packed, first = packed.to(device, non_blocking=True), first.to(device, non_blocking=True)
    B, Nmax = len(studies), max(counts)
    out = torch.empty((B, Nmax, 3, H, W), dtype=torch.float32, device=device)
    LIB.call("cxr_pixels_u8_to_f32", ops._p(packed), ops._p(first), ops._p(out), B, Nmax, H, W, *[float(m) for m in mean], *[float(s) for s in std],
             ops._s())
    return out


# ---------------------------------------------------------------------------------------------- the whole transform: host side
def resized_hw(H, W, S):
    """torchvision `Resize(S)` with an int: the short edge becomes S, the long edge int(S * long / short) -> (oh, ow)"""
    short, long_ = (W, H) if W <= H else (H, W)
    new_long = int(S * long_ / short)
    return (new_long, S) if W <= H else (S, new_long)


def center_crop_offsets(oh, ow, S):
    """torchvision `CenterCrop(S)`: Python's round, i.e. half to even (a difference of 77 gives 38, 79 gives 40) -> (top, left)"""
    return int(round((oh - S) / 2.0)), int(round((ow - S) / 2.0))


@functools.lru_cache(maxsize=256)
def resample_table(in_size, out_size):
    """Pillow's bilinear coefficients of one axis (Resample.c precompute_coeffs + normalize_coeffs_8bpc), float64 in Pillow's operation order
    -> (ksize, first tap int32 [out], taps int32 [out], weights int32 [out, ksize] with 22 fractional bits, 0 beyond `taps`). Read-only arrays:
    the result is cached per (in, out) pair (MIMIC-CXR has few distinct image sizes)."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)                  # C cast: truncation toward zero
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    t = np.arange(ksize, dtype=np.int64)
    arg = (((t[None, :] + xmin[:, None]) - center[:, None]) + 0.5) * ss
    w = np.maximum(0.0, 1.0 - np.abs(arg))
    w[t[None, :] >= n[:, None]] = 0.0
    ww = np.zeros(out_size, dtype=np.float64)
    for j in range(ksize):                                                                   # tap by tap, like Pillow: not a pairwise sum
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    k = np.trunc(w * 4194304.0 + 0.5).astype(np.int32)
    out = (ksize, xmin.astype(np.int32), n.astype(np.int32), k)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _table_ints(table):
    """device layout of one axis: bounds [out][2] = (first tap, taps), then weights [ksize][out]"""
    _, xmin, n, k = table
    return np.concatenate([np.stack([xmin, n], axis=1).ravel(), np.ascontiguousarray(k.T).ravel()]).astype(np.int32)


ROTATION_IDENTITY = (65536, 0, 32768, 0, 65536, 32768)


def rotation_integers(angle, S):
    """`Image.rotate(angle, NEAREST, expand=False, center=None)` on an S x S image -> (a0..a5), the 16.16 integers of Pillow's affine_fixed:
    output pixel (x, y) copies input pixel ((a2 + a1 y + a0 x) >> 16, (a5 + a4 y + a3 x) >> 16). |angle| < 90 only (Pillow special-cases the
    multiples of 90)."""
    if not abs(angle) < 90:
        raise ValueError(f"rotation angle {angle!r}: only |angle| < 90 is supported")
    r = -math.radians(angle % 360.0)
    cx = cy = S / 2.0
    m0, m1, m3, m4 = round(math.cos(r), 15), round(math.sin(r), 15), round(-math.sin(r), 15), round(math.cos(r), 15)
    m2 = m0 * (-cx) + m1 * (-cy) + cx
    m5 = m3 * (-cx) + m4 * (-cy) + cy
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    return (fix(m0), fix(m1), fix(m2 + m0 * 0.5 + m1 * 0.5), fix(m3), fix(m4), fix(m5 + m3 * 0.5 + m4 * 0.5))


def _as_image(img):
    """-> (uint8 numpy array or device tensor, (H, W, C))"""
    if isinstance(img, torch.Tensor):
        a = img if img.is_cuda else img.numpy()
    elif isinstance(img, np.ndarray):
        a = img
    else:                                                                                    # PIL
        a = np.asarray(img if img.mode in ("L", "RGB") else img.convert("RGB"))
    if a.dtype not in (np.uint8, torch.uint8) or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError(f"an image must be uint8 [H, W] or [H, W, 3], got {a.dtype} {tuple(a.shape)}")
    return a, (int(a.shape[0]), int(a.shape[1]), 1 if a.ndim == 2 else 3)


class StudyImageTransform:
    """The reference's test (`train=False`) or train transforms plus `collate_fn`'s padding for a batch of studies, on the device."""

    def __init__(self, size=384, train=False, degrees=5.0, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        if int(size) <= 0:
            raise ValueError("size must be positive")
        if any(float(s) == 0.0 for s in std):
            raise ValueError("std must be non-zero")
        self.size, self.train, self.degrees = int(size), bool(train), float(degrees)
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        self._pinned = None                                                                  # grow-only staging buffer + the event of its last copy
        self._copied = None

    def draw(self, resized, generator=None):
        """torchvision's `get_params` order per image: RandomCrop's top, then left (no draw when the resized image is S x S already), then
        RandomRotation's angle -> (crops, angles)"""
        S, d = self.size, self.degrees
        crops, angles = [], []
        for oh, ow in resized:
            if (oh, ow) == (S, S):
                crops.append((0, 0))
            else:
                top = int(torch.randint(0, oh - S + 1, (1,), generator=generator).item())
                left = int(torch.randint(0, ow - S + 1, (1,), generator=generator).item())
                crops.append((top, left))
            angles.append(float(torch.empty(1).uniform_(-d, d, generator=generator).item()))
        return crops, angles

    def plan(self, shapes, crops=None, angles=None, generator=None, counts=None):
        """shapes: (H, W, C) or (H, W) of every source image, studies back to back; counts: images per study (default: one image each).
        -> a plain object: `resized`, `crops`, `rotations` (train only), `h_tables` / `v_tables` (per image: ksize, first tap, taps, weights) and
        the arrays the device call takes (`desc`, `tables`, source offsets and pitches, `src_bytes`, `inter`, `inter_bytes`, `n_bands`)."""
        S = self.size
        shapes = [(int(s[0]), int(s[1]), int(s[2]) if len(s) > 2 else 1) for s in shapes]
        n = len(shapes)
        counts = [1] * n if counts is None else [int(c) for c in counts]
        if n == 0 or sum(counts) != n or any(c < 0 for c in counts) or max(counts) == 0:
            raise ValueError("plan needs at least one image, and counts must add up to the number of images")
        for H, W, C in shapes:
            if H <= 0 or W <= 0 or C not in (1, 3):
                raise ValueError(f"bad image shape {(H, W, C)}")
        resized = [resized_hw(H, W, S) for H, W, _ in shapes]
        rotations = None
        if self.train:
            if crops is None or angles is None:
                dc, da = self.draw(resized, generator)
                crops, angles = (dc if crops is None else crops), (da if angles is None else angles)
            crops = [(int(t), int(l)) for t, l in crops]
            if len(crops) != n or len(angles) != n:
                raise ValueError("crops and angles need one entry per image")
            for (top, left), (oh, ow) in zip(crops, resized):
                if not (0 <= top <= oh - S and 0 <= left <= ow - S):
                    raise ValueError(f"crop {(top, left)} outside the resized image {(oh, ow)}")
            rotations = [rotation_integers(float(a), S) for a in angles]
        else:
            if crops is not None or angles is not None:
                raise ValueError("crops / angles belong to train mode")
            crops = [center_crop_offsets(oh, ow, S) for oh, ow in resized]

        h_tables = [resample_table(W, ow) for (_, W, _), (_, ow) in zip(shapes, resized)]
        v_tables = [resample_table(H, oh) for (H, _, _), (oh, _) in zip(shapes, resized)]
        tab_off, tab_parts, pos = {}, [], 0
        for (H, W, _), (oh, ow) in zip(shapes, resized):
            for key in ((W, ow), (H, oh)):
                if key not in tab_off:
                    part = _table_ints(resample_table(*key))
                    tab_off[key] = pos
                    tab_parts.append(part)
                    pos += part.size

        B, Nmax = len(counts), max(counts)
        desc = np.zeros((n, ops.IMAGE_TRANSFORM_DESC_INTS), dtype=np.int32)
        offsets, pitches, inter, bands = [], [], [], []
        src_pos = ws_pos = 0
        for i, ((H, W, C), (oh, ow), (top, left)) in enumerate(zip(shapes, resized, crops)):
            pitch = (W * C + 15) // 16 * 16
            if pitch > ops.IMAGE_TRANSFORM_BAND_BYTES:
                raise ValueError(f"a source row of {W * C} bytes exceeds the supported {ops.IMAGE_TRANSFORM_BAND_BYTES}")
            rot = rotations[i] if rotations is not None else ROTATION_IDENTITY
            desc[i, :14] = (src_pos // 16, H, W, C, pitch, oh, ow, top, left, tab_off[(W, ow)], h_tables[i][0], tab_off[(H, oh)], v_tables[i][0],
                            ws_pos // 16)
            desc[i, 16:22] = rot
            offsets.append(src_pos), pitches.append(pitch), inter.append((H, ow, C))
            rows = ops.IMAGE_TRANSFORM_BAND_BYTES // pitch
            bands += [(i, r) for r in range(0, H, rows)]
            src_pos += H * pitch
            ws_pos += (H * ow * C + 15) // 16 * 16
        slot_image = np.full((B, Nmax), -1, dtype=np.int32)
        i = 0
        for b, c in enumerate(counts):
            slot_image[b, :c] = np.arange(i, i + c)
            i += c
        return SimpleNamespace(size=S, train=self.train, shapes=shapes, counts=counts, B=B, Nmax=Nmax, n_images=n, resized=resized, crops=crops,
                               rotations=rotations, h_tables=h_tables, v_tables=v_tables, offsets=offsets, pitches=pitches, src_bytes=src_pos,
                               inter=inter, inter_bytes=ops.image_transform_workspace_bytes(inter), n_bands=len(bands),
                               desc=np.concatenate([desc.ravel(), slot_image.ravel(), np.asarray(bands, dtype=np.int32).ravel()]),
                               tables=np.concatenate(tab_parts))

    def _staging(self, nbytes):
        if self._copied is not None:
            self._copied.synchronize()                                                       # the previous batch's copy still reads the buffer
        if self._pinned is None or self._pinned.numel() < nbytes:
            self._pinned = torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True)
        return self._pinned[:nbytes]

    def transform(self, studies, device, crops=None, angles=None, generator=None, return_uint8=False):
        """studies: list (one entry per study) of lists of uint8 images [H, W] (grey) or [H, W, 3] -- numpy arrays, torch CPU or device tensors or
        PIL images, of any sizes. -> `images` fp32 [B, max n_i, 3, S, S] on `device`, normalised and zero-padded like the reference
        batch['images']; with return_uint8 also the transformed uint8 images [sum n_i, S, S, 3]. Host sources are packed into one pinned buffer
        and go up in one copy, descriptors and tables in one more; the transform itself is two launches whatever the number of images (a source
        that already lives on the device is copied into the packed buffer by a device copy of its own)."""
        device = torch.device(device)
        flat = [_as_image(img) for study in studies for img in study]
        plan = self.plan([s for _, s in flat], crops, angles, generator, counts=[len(study) for study in studies])
        on_gpu = device.type == "cuda"
        meta = torch.from_numpy(np.concatenate([plan.desc, plan.tables]))
        if any(not isinstance(a, torch.Tensor) for a, _ in flat):
            host = self._staging(plan.src_bytes) if on_gpu else torch.empty((plan.src_bytes,), dtype=torch.uint8)
            for (a, (H, W, C)), off, pitch in zip(flat, plan.offsets, plan.pitches):
                if not isinstance(a, torch.Tensor):
                    rows = torch.from_numpy(np.ascontiguousarray(a).reshape(H, W * C))
                    host[off:off + H * pitch].view(H, pitch)[:, :W * C].copy_(rows)
            src = host.to(device, non_blocking=True)
            if on_gpu:
                self._copied = torch.cuda.Event()
                self._copied.record()
        else:
            src = torch.empty((plan.src_bytes,), dtype=torch.uint8, device=device)
        for (a, (H, W, C)), off, pitch in zip(flat, plan.offsets, plan.pitches):
            if isinstance(a, torch.Tensor):
                src[off:off + H * pitch].view(H, pitch)[:, :W * C].copy_(a.reshape(H, W * C), non_blocking=True)
        meta = (meta.pin_memory() if on_gpu else meta).to(device, non_blocking=True)
        out, u8 = ops.image_transform(src, meta[:plan.desc.size], meta[plan.desc.size:], plan.n_images, plan.n_bands, plan.B, plan.Nmax, plan.size,
                                      self.mean, self.std, plan.inter_bytes, want_f32=True, want_u8=return_uint8)
        return (out, u8) if return_uint8 else out
