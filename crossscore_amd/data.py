"""Predict-time data side of the drop-in: which files form a (query, N references) item, and the GPU input stage.

Mirrors, for the predict path only:
  SimpleReference.get_paths            dataloading/dataset/simple_reference.py:42-84   sorted listdir of query_dir / reference_dir
  NeighbourSelector + SamplerRandom    dataloading/dataset/nvs_dataset.py:14-84, utils/neighbour/sampler.py:15-38
  load_content / resize_all / crops / T.Normalize   nvs_dataset.py:218-279,429-470, task/predict.py:68-93
The pixel work (x/255, antialiased resize, crop, normalise) runs on the GPU through cs_op_preprocess_u8 straight from the decoded
uint8 image; how a file becomes that image, on the host or on the device, is decode.py's.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, decode
from .decode import read_image_u8, read_metric_map_u16  # noqa: F401 -- decode_items and the tests find the two readers here
from .synth import IMAGENET_MEAN_STD

EMPTY = "empty_image"  # placeholder path the reference pads short reference lists with (sampler.py:22-27)


def resized_output_size(h: int, w: int, short: int) -> Tuple[int, int]:
    """torchvision T.Resize(int): the short side becomes `short`, the long side int(short * long / short_side)."""
    if h <= w:
        return short, int(short * w / h)
    return int(short * h / w), short


def list_paths(query_dir: str, reference_dir: str) -> Tuple[List[str], List[str]]:
    """simple_reference.py:53-58: every entry of the two directories, sorted by name."""
    query_dir, reference_dir = os.path.expanduser(query_dir), os.path.expanduser(reference_dir)
    q = [os.path.join(query_dir, p) for p in sorted(os.listdir(query_dir))]
    r = [os.path.join(reference_dir, p) for p in sorted(os.listdir(reference_dir))]
    return q, r


def sample_references(ref_list: Sequence[str], n_sample: int, deterministic: bool, rng=np.random) -> List[str]:
    """SamplerRandom.sample (utils/neighbour/sampler.py:19-38): first N when deterministic, else N without replacement from the
    global numpy RNG; a short list is padded with "empty_image" placeholders and permuted."""
    ref_list = list(ref_list)
    if n_sample > len(ref_list):
        result = ref_list + [EMPTY] * (n_sample - len(ref_list))
        return rng.permutation(result).tolist()
    if deterministic:
        return ref_list[:n_sample]
    return rng.choice(ref_list, n_sample, replace=False).tolist()


def metric_mode(metric_type: str, metric_min) -> int:
    """The GT map's load_content conversion (nvs_dataset.py:439-455) as a cs_op_metric_map_u16 mode."""
    if metric_type == "ssim":
        return _lib.METRIC_SSIM_0_1 if metric_min == 0 else _lib.METRIC_SSIM_M1_1
    if metric_type == "mae":
        return _lib.METRIC_MAE
    if metric_type == "mse":
        return _lib.METRIC_MSE
    raise ValueError(f"Invalid metric type {metric_type}")


def batch_files(items, zero_reference: bool = False, extra=None, skip=()) -> List[Tuple[str, bool]]:
    """The (path, gray16) list of the files a batch reads, in reading order: per item its query, its references in slot order (not the
    "empty_image" placeholders, not the paths in `skip`, none at all with zero_reference), then extra(item).  A file named twice is listed twice."""
    files: List[Tuple[str, bool]] = []
    for it in items:
        files.append((it["query/img"], False))
        if not zero_reference:
            files += [(p, False) for p in (it["reference/cross/imgs"] or ()) if p != EMPTY and p not in skip]  # (None: chosen on the device)
        if extra is not None:
            files += extra(it)
    return files


def plan_decodes(batches, zero_reference: bool, once_per_reference: bool, extra=None) -> List[List[Tuple[str, bool]]]:
    """Per batch its batch_files, the list decode_items reads; with a reference-token cache (once_per_reference) a reference is read by the first
    batch that names it only: later ones find its tokens.  (Fixed up front; the host path's `skip` follows the cache as it is at run time.)"""
    seen, plan = set(), []
    for its in batches:
        plan.append(batch_files(its, zero_reference, extra, seen if once_per_reference else ()))
        seen.update(p for it in its for p in (it["reference/cross/imgs"] or ()))
    return plan


class InputStage:
    """uint8 HWC images -> the normalised fp32 batch tensors CrossScoreNet.forward takes, on `device`."""

    def __init__(self, device: torch.device, resize_short_side: int = 518, crop_size: Optional[int] = None, integer_patches: bool = False,
                 patch: int = 14, mean_std: Sequence[float] = IMAGENET_MEAN_STD):
        self.device = device
        self.resize_short_side = int(resize_short_side)
        self.crop_size = crop_size
        self.integer_patches = integer_patches
        self.patch = patch
        self.mean_std = tuple(float(v) for v in mean_std)
        self._mean = (C.c_float * 3)(*mean_std[:3])
        self._std = (C.c_float * 3)(*mean_std[3:])
        self._scratch: Optional[torch.Tensor] = None
        ms = torch.tensor(list(mean_std), dtype=torch.float32)
        self.zero_image_value = ((torch.zeros(3) - ms[:3]) / ms[3:]).to(device)  # a black pixel after T.Normalize

    def geometry(self, h: int, w: int):
        """(resized (h, w), crop (y, x, h, w)) for an input of h x w: resize_all, then the deterministic crop (crop.py:19-22: i = j = 0)
        or the integer-patch crop (nvs_dataset.py:227-241)."""
        rs = resized_output_size(h, w, self.resize_short_side) if self.resize_short_side > 0 else (h, w)
        oh, ow = rs
        if self.crop_size is not None:
            oh = ow = int(self.crop_size)
            if oh > rs[0] or ow > rs[1]:
                raise ValueError(f"crop {oh}x{ow} larger than the resized image {rs[0]}x{rs[1]}")
        elif self.integer_patches:
            oh, ow = rs[0] - rs[0] % self.patch, rs[1] - rs[1] % self.patch
        return rs, (0, 0, oh, ow)

    def _device_image(self, img_u8) -> torch.Tensor:
        """The decoded image on the device: a host array goes up (a blocking pageable copy), a CUDA uint8 (h, w, 3) tensor (decode.ImageDecoder's
        output) is used where it is."""
        if isinstance(img_u8, torch.Tensor):
            if not img_u8.is_cuda or img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[2] != 3 or not img_u8.is_contiguous():
                raise ValueError(f"a device image must be a contiguous uint8 (h, w, 3) CUDA tensor, got {img_u8.dtype} {tuple(img_u8.shape)}")
            return img_u8
        return torch.from_numpy(img_u8).to(self.device, non_blocking=False)

    def __call__(self, img_u8, out: torch.Tensor) -> None:
        """Writes the processed image into `out` ((3, oh, ow) fp32 slice on the device).  img_u8: a host array or a CUDA uint8 tensor."""
        lib = _lib.load()
        h, w, _ = (int(v) for v in img_u8.shape)
        rs, crop = self.geometry(h, w)
        if tuple(out.shape) != (3, crop[2], crop[3]) or not out.is_contiguous() or out.dtype != torch.float32:
            raise ValueError(f"output slice must be contiguous fp32 (3,{crop[2]},{crop[3]}), got {tuple(out.shape)}")
        d_img = self._device_image(img_u8)
        scratch = None
        if rs != (h, w):
            need = h * rs[1] * 3
            if self._scratch is None or self._scratch.numel() < need:
                self._scratch = torch.empty((need,), dtype=torch.float32, device=self.device)
            scratch = C.c_void_p(self._scratch.data_ptr())
        _lib.check(lib.cs_op_preprocess_u8(C.c_void_p(d_img.data_ptr()), h, w, w * 3, rs[0], rs[1], crop[0], crop[1], crop[2], crop[3],
                                           self._mean, self._std, C.c_void_p(out.data_ptr()), scratch,
                                           C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        # d_img may be released once the stream has consumed it
        d_img.record_stream(torch.cuda.current_stream(self.device))


    def metric_map(self, map_u16: Optional[np.ndarray], query_hw: Tuple[int, int], mode: int, out: torch.Tensor) -> None:
        """metric_maps for one map: `out` is its (oh, ow) fp32 slice on the device."""
        self.metric_maps([map_u16], [query_hw], mode, out[None])

    def gt_metric_maps(self, renders: Sequence, gts: Sequence, kind: int) -> List[torch.Tensor]:
        """Ground-truth metric maps from the images themselves (cs_op_gt_metric_map_u8): pair i is (renders[i], gts[i]),
        each a uint8 (h, w, 3) image, a CUDA tensor or a host array as read_image_u8 returns it; returns per pair its (h, w) int16 device map
        (16-bit samples, unsigned in memory), the form metric_maps and writers.PngEncoder take.  kind: _lib.GTMAP_SSIM / GTMAP_MAE.  Queued on
        the current stream without waiting for it: host images go up from pinned memory (non-blocking copies), and one launch per source size
        covers the batch; the maps of one size are slices of one tensor, in pair order."""
        lib = _lib.load()
        if len(renders) != len(gts) or len(renders) == 0:
            raise ValueError("gt_metric_maps: one captured image per render, at least one pair")
        groups: Dict[Tuple[int, int], List[int]] = {}
        for i, (a, b) in enumerate(zip(renders, gts)):
            for im in (a, b):
                if im.dtype not in (np.uint8, torch.uint8) or im.ndim != 3 or im.shape[2] != 3:
                    raise ValueError(f"gt_metric_maps takes uint8 (h, w, 3) images, got {im.dtype} {tuple(im.shape)}")
            if tuple(a.shape) != tuple(b.shape):
                raise ValueError(f"render {a.shape[0]}x{a.shape[1]} and captured image {b.shape[0]}x{b.shape[1]} of pair {i} differ in size")
            groups.setdefault((int(a.shape[0]), int(a.shape[1])), []).append(i)
        stream = torch.cuda.current_stream(self.device)
        out: List[Optional[torch.Tensor]] = [None] * len(renders)
        for (h, w), idx in groups.items():
            n = len(idx)
            sides = []
            for src in (renders, gts):
                imgs = [src[i] for i in idx]
                host = [k for k, im in enumerate(imgs) if not isinstance(im, torch.Tensor)]
                up = None
                if host:
                    block = torch.empty((len(host), h, w, 3), dtype=torch.uint8, pin_memory=True)
                    bv = block.numpy()
                    for j, k in enumerate(host):
                        bv[j] = imgs[k]
                    up = block.to(self.device, non_blocking=True)  # pinned source: an asynchronous copy on the current stream
                if len(host) == n:
                    sides.append(up)
                    continue
                for j, k in enumerate(host):
                    imgs[k] = up[j]
                for im in imgs:
                    if not im.is_cuda:
                        raise ValueError("gt_metric_maps takes CUDA tensors or host arrays")
                    im.record_stream(stream)
                sides.append(torch.stack(imgs))  # images already on the device (the one-pass input stage's): gathered there
            maps = torch.empty((n, h, w), dtype=torch.int16, device=self.device)
            _lib.check(lib.cs_op_gt_metric_map_u8(C.c_void_p(sides[0].data_ptr()), C.c_void_p(sides[1].data_ptr()), n, h, w, h * w * 3, int(kind),
                                                  C.c_void_p(maps.data_ptr()), w, C.c_void_p(stream.cuda_stream)))
            for j, i in enumerate(idx):
                out[i] = maps[j]
        return out

    def metric_maps(self, maps: Sequence, query_hws: Sequence[Tuple[int, int]], mode: int, out: torch.Tensor) -> None:
        """GT stage of the test phase: writes the processed ground-truth maps of B queries of sizes query_hws into `out` ((B, oh, ow) fp32 on
        the device), each with its query's own resize and crop; None is the "empty_image" placeholder (0 for SSIM, NaN for MAE / MSE).  Queued
        on the current stream without waiting for it: the maps go up from pinned host memory (non-blocking copies), and one launch pair per
        source size covers the batch.  A map may also be a 16-bit (h, w) CUDA tensor (gt_metric_maps' output): it is used where it is."""
        lib = _lib.load()
        B = len(maps)
        if len(query_hws) != B or B == 0:
            raise ValueError("metric_maps: one query size per map, at least one map")
        geo, groups = [], {}
        for b, (m, hw) in enumerate(zip(maps, query_hws)):
            h, w = int(hw[0]), int(hw[1])
            on_device = isinstance(m, torch.Tensor)
            if on_device:
                if not m.is_cuda or m.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)) or m.dim() != 2:
                    raise ValueError(f"a device metric map must be a 16-bit (H, W) CUDA tensor, got {m.dtype} {tuple(m.shape)}")
                if tuple(m.shape) != (h, w):
                    raise ValueError(f"metric map {m.shape[0]}x{m.shape[1]} and its render {h}x{w} differ in size")
            elif m is not None:
                if m.dtype == np.int32:  # PIL's "I" mode for 16-bit PNGs
                    m = m.astype(np.uint16)
                if m.dtype != np.uint16 or m.ndim != 2:
                    raise ValueError(f"metric map must be a uint16 (H, W) array, got {m.dtype} {m.shape}")
                if tuple(m.shape) != (h, w):
                    raise ValueError(f"metric map {m.shape[0]}x{m.shape[1]} and its render {h}x{w} differ in size")
            geo.append(self.geometry(h, w))
            groups.setdefault(None if m is None else (h, w, True) if on_device else (h, w), []).append((b, m))
        oh, ow = geo[0][1][2:]
        if any(g[1][2:] != (oh, ow) for g in geo) or tuple(out.shape) != (B, oh, ow) or not out.is_contiguous() or out.dtype != torch.float32:
            raise ValueError(f"output must be contiguous fp32 ({B},{oh},{ow}) and every map must give that size, got {tuple(out.shape)}")
        stream = torch.cuda.current_stream(self.device)
        st = C.c_void_p(stream.cuda_stream)
        for key, members in groups.items():
            idx = [b for b, _ in members]
            n = len(idx)
            whole = n == B
            dst = out if whole else torch.empty((n, oh, ow), dtype=torch.float32, device=self.device)
            rs, crop = geo[idx[0]]
            if key is None:
                _lib.check(lib.cs_op_metric_map_u16(None, n, rs[0], rs[1], rs[1], int(mode), rs[0], rs[1], crop[0], crop[1], oh, ow,
                                                    C.c_void_p(dst.data_ptr()), None, st))
            else:
                h, w = key[:2]
                if len(key) == 3:  # maps already on the device: used in place when they are consecutive slices of one tensor, gathered otherwise
                    ms = [m for _, m in members]
                    first = ms[0].data_ptr()
                    in_place = all(m.is_contiguous() and m.data_ptr() == first + i * h * w * 2 for i, m in enumerate(ms))
                    d_maps = ms[0] if in_place else torch.stack([m.contiguous() for m in ms])
                    for m in ms:
                        m.record_stream(stream)
                else:
                    host = torch.empty((n, h, w), dtype=torch.int16, pin_memory=True)
                    hv = host.numpy()
                    for i, (_, m) in enumerate(members):
                        hv[i] = np.asarray(m, dtype=np.uint16).view(np.int16)
                    d_maps = host.to(self.device, non_blocking=True)  # pinned source: an asynchronous copy on the current stream
                scratch = torch.empty((n * h * rs[1],), dtype=torch.float32, device=self.device) if rs != (h, w) else None
                _lib.check(lib.cs_op_metric_map_u16(C.c_void_p(d_maps.data_ptr()), n, h, w, w, int(mode), rs[0], rs[1], crop[0], crop[1], oh, ow,
                                                    C.c_void_p(dst.data_ptr()), C.c_void_p(scratch.data_ptr()) if scratch is not None else None,
                                                    st))
            if not whole:
                for i, b in enumerate(idx):
                    out[b].copy_(dst[i])

    # -- the one-pass form (SURVEY.md 8f-4 as worded): nothing is computed here, the patch-embedding launch does the pixel work --------------
    def describe(self, img_u8):
        """The decoded image on the device with its geometry (model.U8Image), an entry of the model.U8Batch CrossScoreNet.forward and its
        siblings take.  img_u8: a host array or a CUDA uint8 tensor (no copy)."""
        from .model import U8Image
        h, w, _ = (int(v) for v in img_u8.shape)
        rs, crop = self.geometry(h, w)
        return U8Image(self._device_image(img_u8), h, w, rs, crop[0], crop[1])

    def placeholder(self, size):
        """The all-zero image (placeholders of short reference lists, zero_reference: nvs_dataset.py:459-470) of the processed size."""
        from .model import U8Image
        return U8Image(None, size[0], size[1], size)

    def batch(self, images, size):
        from .model import U8Batch
        return U8Batch(images, size, self.mean_std, device=self.device)

    def model_input(self, images, size, u8: bool, out: Optional[torch.Tensor] = None, lead: Optional[Tuple[int, ...]] = None):
        """Decoded images (host arrays or CUDA uint8 tensors; None = the all-zero placeholder, zeros BEFORE T.Normalize: nvs_dataset.py:459-470)
        of the processed size -> the form the model's methods take them in: a model.U8Batch (u8, the one-pass input stage: nothing is computed
        here), else the processed (len(images), 3, oh, ow) fp32 tensor, written into `out` when the caller keeps the images and returned as
        (*lead, 3, oh, ow) when the images are a batch's views, item-major: lead = (B, N)."""
        if u8:
            return self.batch([self.placeholder(size) if im is None else self.describe(im) for im in images], size)
        if out is None:
            out = torch.empty((len(images), 3, size[0], size[1]), dtype=torch.float32, device=self.device)
        for i, im in enumerate(images):
            if im is None:
                out[i] = self.zero_image_value[:, None, None]
            else:
                self(im, out[i])
        return out if lead is None else out.view(*lead, 3, size[0], size[1])


STRATEGIES = ("random", "similar")  # data.neighbour_config.strategy: the reference's sampler, and this build's choice by DINOv2 similarity


class SimpleReferenceItems:
    """Index -> file paths of one item, like NeighbourSelector.__getitem__ for the single-scene layout of SimpleReference."""

    def __init__(self, query_dir: str, reference_dir: str, neighbour_config) -> None:
        if neighbour_config["strategy"] not in STRATEGIES:
            raise NotImplementedError(f"neighbour strategy {neighbour_config['strategy']} (sampler.py:60-66 knows 'random'; this build adds 'similar')")
        self.strategy = str(neighbour_config["strategy"])
        self.query_paths, self.reference_paths = list_paths(query_dir, reference_dir)
        self.n_cross = int(neighbour_config["cross"])
        self.deterministic = bool(neighbour_config["deterministic"])

    def __len__(self) -> int:
        return len(self.query_paths)

    def __getitem__(self, idx: int) -> Dict[str, object]:
        if self.strategy == "similar":  # the views are chosen on the device (ReferenceBank, forward_select); no RNG is drawn
            return {"query/img": self.query_paths[idx], "query/score_map": EMPTY, "reference/cross/imgs": None}
        refs = sample_references(self.reference_paths, self.n_cross, self.deterministic) if self.n_cross > 0 else []
        return {"query/img": self.query_paths[idx], "query/score_map": EMPTY, "reference/cross/imgs": refs}


def decode_items(items: List[Dict[str, object]], zero_reference: bool = False, pool=None, skip=(), extra=None) -> Dict[str, np.ndarray]:
    """path -> decoded image for every file batch_files lists for the items, each path read once (host side; PIL releases the GIL while
    decoding, so a thread pool plays the role of the reference's DataLoader workers, task/predict.py:110-117): a uint8 image, or the 16-bit
    map of a gray16 entry of extra(item).  Reference paths in `skip` (already in the token cache) are not decoded; extras always are."""
    gray16: Dict[str, bool] = {}  # in reading order; a path listed twice is read as its first entry says
    for path, flag in batch_files(items, zero_reference, extra, skip):
        gray16.setdefault(path, flag)

    def read(path):
        return (read_metric_map_u16 if gray16[path] else read_image_u8)(path)

    return dict(zip(gray16, pool.map(read, gray16) if pool is not None else map(read, gray16)))


def item_paths(items: List[Dict[str, object]]) -> Dict[str, list]:
    """The batch's file paths in the collated layout the writers expect (default_collate turns the per-item list of N reference paths into N
    lists of B paths)."""
    if items[0]["reference/cross/imgs"] is None:  # strategy similar: scoring's consume fills the lists in from the batch's reference_index
        refs = None
    else:
        N = len(items[0]["reference/cross/imgs"])
        refs = [[it["reference/cross/imgs"][n] for it in items] for n in range(N)]
    return {"query/img": [it["query/img"] for it in items], "query/score_map": [it["query/score_map"] for it in items],
            "reference/cross/imgs": refs}


def _reference_image(path: str, decoded, stage: InputStage, size):
    """The decoded reference image (from `decoded`, else read here), checked against the query's processed size."""
    img = decoded[path] if path in decoded else read_image_u8(path)
    if stage.geometry(*img.shape[:2])[1][2:] != tuple(size):
        raise ValueError(f"{path}: processed size differs from the query's {size[0]}x{size[1]}")
    return img


def load_batch(items: List[Dict[str, object]], stage: InputStage, decoded: Optional[Dict[str, np.ndarray]] = None, u8: bool = False,
               references: bool = True, zero_reference: bool = False):
    """(batch, processed size): one batch dict with the keys `_core_step` reads (task/core.py:265-272) plus `item_paths`.  `decoded` holds
    images already read by decode_items (a reference image shared by several items of the batch is decoded once).
    u8: the one-pass input stage -- "query/img" and "reference/cross/imgs" are model.U8Batch objects (decoded images on the device + geometry)
    and no processed fp32 tensor exists; else (B, 3, oh, ow) and (B, N, 3, oh, ow) fp32 tensors.
    references=False: the references come from a ReferenceTokenCache and "reference/cross/imgs" is None."""
    decoded = decoded if decoded is not None else {}
    q_imgs = [decoded[it["query/img"]] if it["query/img"] in decoded else read_image_u8(it["query/img"]) for it in items]
    geo = {stage.geometry(*im.shape[:2])[1][2:] for im in q_imgs}
    if len(geo) != 1:
        raise ValueError(f"query images of one batch must share the processed size, got {sorted(geo)}")
    size = next(iter(geo))
    ref_lists = [it["reference/cross/imgs"] if references else () for it in items]
    # nvs_dataset.py:459-470: placeholders and zero_reference are all-zero images BEFORE T.Normalize -> (0 - mean) / std
    blank = lambda p: p == EMPTY or zero_reference  # noqa: E731
    query = stage.model_input(q_imgs, size, u8)
    refs = stage.model_input([None if blank(p) else _reference_image(p, decoded, stage, size) for ps in ref_lists for p in ps], size, u8,
                             lead=(len(items), len(ref_lists[0]))) if references else None
    return {"query/img": query, "reference/cross/imgs": refs, "item_paths": item_paths(items)}, size


class ReferenceTokenCache:
    """SURVEY.md 8f-3 inside the predict loop: references are sampled from one finite directory, so each reference image is
    pre-processed and encoded ONCE (CrossScoreNet.encode_references) and queries are scored with forward_cached -- the same bits
    as the full forward (tests/test_hip_forward.py), with 1 instead of 1 + N images through the encoder per query."""

    def __init__(self, net, stage: InputStage, keep_images: bool, max_images: int = 4096, from_u8: bool = False):
        self.net, self.stage, self.keep_images, self.max_images = net, stage, keep_images, max_images
        self.from_u8 = bool(from_u8) and not keep_images  # one-pass input stage: no processed fp32 image exists to keep
        self.tokens: Dict[object, torch.Tensor] = {}
        self.images: Dict[object, torch.Tensor] = {}

    def has(self, path: str) -> bool:
        return any(k[0] == path for k in self.tokens)

    def gather(self, ref_lists: List[List[str]], decoded: Dict[str, np.ndarray], size: Tuple[int, int], zero_reference: bool):
        """ref_lists: per item the N reference paths -> (tokens (B,N,Np,C) fp16, images (B,N,3,h,w) fp32 or None)."""
        oh, ow = size
        keys = [[(EMPTY if (p == EMPTY or zero_reference) else p, oh, ow) for p in refs] for refs in ref_lists]
        missing = list(dict.fromkeys(k for ks in keys for k in ks if k not in self.tokens))
        if missing:
            if len(self.tokens) + len(missing) > self.max_images:
                self.tokens.clear()
                self.images.clear()
                missing = list(dict.fromkeys(k for ks in keys for k in ks))
            imgs = [None if k[0] == EMPTY else _reference_image(k[0], decoded, self.stage, (oh, ow)) for k in missing]
            buf = self.stage.model_input(imgs, (oh, ow), self.from_u8)
            tok = self.net.encode_references(buf)
            for i, k in enumerate(missing):
                self.tokens[k] = tok[i]
                if self.keep_images:
                    self.images[k] = buf[i].clone()
        tokens = torch.stack([torch.stack([self.tokens[k] for k in ks]) for ks in keys])
        images = torch.stack([torch.stack([self.images[k] for k in ks]) for ks in keys]) if self.keep_images else None
        return tokens, images


class ReferenceBank:
    """data.neighbour_config.strategy=similar: every file of reference_dir is encoded ONCE, in chunks, into one contiguous
    (R, h*w, C) token tensor; the descriptors forward_select compares a query with are formed from it (CrossScoreNet.reference_descriptors).
    `bank` is the model.SelectionBank the forwards take, `paths` the files in bank order, `images` their processed fp32 images (R, 3, h, w) when
    keep_images (the writer's image_reference output) -- else None.

    groups (the test phase: nvs.NvsItems.groups, the candidate lists of the scenes this run scores) instead of paths: the bank holds the groups'
    files one group after the other -- `offsets` -- and behind them one more row, `blank_row`: the all-zero placeholder image ("empty_image",
    nvs_dataset.py:459-470), whose tokens stand in where a query's group has fewer than n_references files.  A query then chooses inside its own
    group only (CrossScoreNet.forward_select(group=...)); a file that several groups list is held once per group.

    decoder: the run's ImageDecoder (this_main.png_decoder / jpeg_decoder = gpu): a chunk's files are decoded on the device, `window` files per
    call; else PIL on `pool`.  from_u8: the one-pass input stage (a U8Batch goes to encode_references; no processed image exists, so not
    with keep_images)."""

    def __init__(self, net, stage: InputStage, paths: Sequence[str], size: Tuple[int, int], n_references: int, keep_images: bool = False,
                 max_images: int = 4096, from_u8: bool = False, decoder: Optional[decode.ImageDecoder] = None, pool=None, chunk: int = 32, window: int = 64,
                 groups: Optional[Sequence[Sequence[str]]] = None):
        from .model import SelectionBank
        self.offsets = None
        if groups is not None:
            groups = [[p for p in g if p != EMPTY] for g in groups]
            if not groups or any(len(g) == 0 for g in groups):
                raise ValueError("neighbour strategy similar: a query's candidate list holds no file")
            self.offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
            self.paths = [p for g in groups for p in g] + [EMPTY]
            R = len(self.paths)
            if R > max_images:
                raise ValueError(f"neighbour strategy similar keeps every candidate's tokens: the {len(groups)} candidate lists of this run hold "
                                 f"{R - 1} files (+ 1 placeholder), more than this_main.reference_cache_max_images={max_images}")
        else:
            self.paths = list(paths)
            R = len(self.paths)
            if R == 0:
                raise ValueError("neighbour strategy similar: reference_dir holds no file")
            if R > max_images:
                raise ValueError(f"neighbour strategy similar keeps every reference's tokens: reference_dir holds {R} files, more than "
                                 f"this_main.reference_cache_max_images={max_images}")
            if n_references > R:
                raise ValueError(f"neighbour strategy similar: neighbour_config.cross={n_references} exceeds the {R} files of reference_dir")
        n_files = R if groups is None else R - 1  # (the placeholder is no file)
        oh, ow = size
        from_u8 = bool(from_u8) and not keep_images
        step = max(1, min(int(chunk), int(window) if decoder is not None else int(chunk)))
        tokens = None
        self.images = torch.empty((R, 3, oh, ow), dtype=torch.float32, device=stage.device) if keep_images else None
        for r0 in range(0, n_files, step):
            part = self.paths[r0:min(r0 + step, n_files)]
            if decoder is not None:
                handle = decoder.decode(part)
                handle.wait(torch.cuda.current_stream(stage.device))
                handle.check()  # (set-up: the bank is complete before the first query is scored)
                imgs = handle.tensors
            else:
                imgs = list(pool.map(read_image_u8, part)) if pool is not None else [read_image_u8(p) for p in part]
            for p, im in zip(part, imgs):
                if stage.geometry(int(im.shape[0]), int(im.shape[1]))[1][2:] != (oh, ow):
                    raise ValueError(f"{p}: processed size differs from the query's {oh}x{ow}" +
                                     (": one bank has one patch grid; this_main.crop_mode=dataset_default gives the images of every scene one size"
                                      if groups is not None else ""))
            tok = net.encode_references(stage.model_input(imgs, size, from_u8, out=self.images[r0:r0 + len(part)] if keep_images else None))
            if tokens is None:
                tokens = torch.empty((R,) + tuple(tok.shape[1:]), dtype=tok.dtype, device=tok.device)
            tokens[r0:r0 + len(part)] = tok
        if groups is not None:  # the placeholder's row: zeros BEFORE T.Normalize, as load_batch and ReferenceTokenCache feed "empty_image"
            tokens[R - 1] = net.encode_references(stage.model_input([None], size, from_u8, out=self.images[R - 1:] if keep_images else None))[0]
            mean, centre, unit = net.reference_descriptors(tokens, self.offsets)
            self.bank = SelectionBank(tokens, mean, centre, unit, n_references, self.offsets, R - 1)
        else:
            mean, centre, unit = net.reference_descriptors(tokens)
            self.bank = SelectionBank(tokens, mean, centre, unit, n_references)
        self._real = {os.path.realpath(p): i for i, p in reversed(list(enumerate(self.paths[:n_files])))}

    def __len__(self) -> int:
        return len(self.paths)

    def index_of(self, path: str, group: Optional[int] = None) -> int:
        """The bank index of the file `path` names (by real path), or -1; with `group`, its row inside that group of a grouped bank."""
        if group is None or self.offsets is None:
            return self._real.get(os.path.realpath(path), -1)
        real = os.path.realpath(path)
        lo, hi = int(self.offsets[group]), int(self.offsets[group + 1])
        return next((i for i in range(lo, hi) if os.path.realpath(self.paths[i]) == real), -1)
