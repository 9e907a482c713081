"""Predict-time data side of the drop-in: which files form a (query, N references) item, and the GPU input stage.

Mirrors, for the predict path only:
  SimpleReference.get_paths            dataloading/dataset/simple_reference.py:42-84   sorted listdir of query_dir / reference_dir
  NeighbourSelector + SamplerRandom    dataloading/dataset/nvs_dataset.py:14-84, utils/neighbour/sampler.py:15-38
  load_content / resize_all / crops / T.Normalize   nvs_dataset.py:218-279,429-470, task/predict.py:68-93
The pixel work (x/255, antialiased resize, crop, normalise) runs on the GPU through cs_op_preprocess_u8 straight from the decoded
uint8 image; PNG/JPEG decoding stays on the host (PIL, as in utils/io/images.py:26-29) unless this_main.png_decoder=gpu hands the PNG files
and / or this_main.jpeg_decoder=gpu the baseline JPEG files to PngDecoder (cs_op_png_decode, cs_op_jpeg_decode: the compressed bytes go up and
the decoded images appear in device memory, the pixels PIL gives, bit for bit).  Files neither device decoder takes (interlaced or palette PNG,
progressive / CMYK / Adobe JPEG, ...) still go through PIL; this_main.jpeg_progressive=gpu adds complete progressive files (cs_op_jpeg_decode_ex).
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .config import this_main_choice
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


def read_image_u8(path: str) -> np.ndarray:
    """Decoded uint8 HWC RGB image (utils/io/images.py:26-29 keeps whatever channel count PIL returns; the model needs 3)."""
    from PIL import Image

    img = np.array(Image.open(path))
    if img.ndim == 2:
        img = np.repeat(img[:, :, None], 3, axis=2)
    if img.shape[2] == 4:
        img = img[:, :, :3]
    if img.dtype != np.uint8 or img.shape[2] != 3:
        raise ValueError(f"{path}: expected an 8-bit RGB image, got {img.dtype} {img.shape}")
    return np.ascontiguousarray(img)


def read_metric_map_u16(path: str) -> np.ndarray:
    """Decoded 16-bit metric map (utils/io/images.py:32-46 reads it with PIL).  PIL returns 16-bit PNGs as "I;16" (uint16) or "I" (int32)
    depending on its version; both come back as a contiguous uint16 (H, W) array."""
    from PIL import Image

    m = np.array(Image.open(path))
    if m.ndim != 2 or m.dtype not in (np.uint16, np.int32):
        raise ValueError(f"{path}: expected a 16-bit grayscale metric map, got {m.dtype} {m.shape}")
    if m.dtype == np.int32:
        if m.size and (m.min() < 0 or m.max() > 65535):
            raise ValueError(f"{path}: metric map samples outside 0..65535")
        m = m.astype(np.uint16)
    return np.ascontiguousarray(m)


def metric_mode(metric_type: str, metric_min) -> int:
    """The GT map's load_content conversion (nvs_dataset.py:439-455) as a cs_op_metric_map_u16 mode."""
    if metric_type == "ssim":
        return _lib.METRIC_SSIM_0_1 if metric_min == 0 else _lib.METRIC_SSIM_M1_1
    if metric_type == "mae":
        return _lib.METRIC_MAE
    if metric_type == "mse":
        return _lib.METRIC_MSE
    raise ValueError(f"Invalid metric type {metric_type}")


PNG_DECODERS = ("host", "gpu")
PNGDEC_STATUS = ("ok", "bad CRC-32", "bad Adler-32", "bad zlib header", "reserved block type", "stored LEN/NLEN mismatch",
                 "over-subscribed or incomplete code", "invalid symbol", "distance before the start of the stream", "stream too short",
                 "stream too long", "filter type above 4", "input exhausted", "IHDR differs from the size or format asked for", "bad chunk framing")


def png_decoder_choice(cfg) -> str:
    """this_main.png_decoder (this build's key): host (default) | gpu."""
    return this_main_choice(cfg, "png_decoder", PNG_DECODERS)


JPGDEC_STATUS = ("ok", "bad framing (SOI, a segment length past the file, no SOF / SOS)", "SOF differs from the size asked for, or a form the decoder does not take",
                 "bad Huffman or quantisation table", "bits that are no code of the table", "invalid symbol", "input exhausted", "missing, misnumbered or surplus restart marker",
                 "illegal scan, DQT / DRI behind the first scan, or an incomplete progression")


def jpeg_decoder_choice(cfg) -> str:
    """this_main.jpeg_decoder (this build's key): host (default) | gpu."""
    return this_main_choice(cfg, "jpeg_decoder", PNG_DECODERS)


def jpeg_progressive_choice(cfg) -> str:
    """this_main.jpeg_progressive (this build's key): host (default) | gpu.  gpu needs this_main.jpeg_decoder=gpu."""
    choice = this_main_choice(cfg, "jpeg_progressive", PNG_DECODERS)
    if choice == "gpu" and jpeg_decoder_choice(cfg) != "gpu":
        raise ValueError("this_main.jpeg_progressive=gpu needs this_main.jpeg_decoder=gpu: the progressive files join the device decoder's calls")
    return choice


def png_decode_window_choice(cfg) -> int:
    """this_main.png_decode_window (this build's key): files handed to the device decoder at once, default 64."""
    v = cfg.this_main.get("png_decode_window", 64)
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError(f"this_main.png_decode_window={v!r} must be a positive integer")
    return v


def read_file_bytes(path: str) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def probe_png(data: bytes):
    """cs_png_probe on a file's bytes: (info, spans (n, 2) uint32) when the device decoder takes the file, else (None, reason)."""
    lib = _lib.load()
    info = _lib.CsPngInfo()
    buf = bytes(data)  # ctypes passes the object's own buffer
    rc = lib.cs_png_probe(buf, len(data), C.byref(info), None, 0)
    if rc != _lib.CS_OK:
        return None, _lib.last_error()
    spans = np.zeros((info.num_idat, 2), dtype=np.uint32)
    rc = lib.cs_png_probe(buf, len(data), C.byref(info), C.c_void_p(spans.ctypes.data), info.num_idat)
    if rc != _lib.CS_OK:
        return None, _lib.last_error()
    return info, spans


def probe_jpeg(data: bytes, progressive: bool = False):
    """cs_jpeg_probe on a file's bytes: (info, None) when the device decoder takes the file, else (None, reason).  progressive=True is
    cs_jpeg_probe_ex with CS_JPEG_PROGRESSIVE: complete progressive files are taken too, and the first element is then (info, scan info)."""
    lib = _lib.load()
    info = _lib.CsJpegInfo()
    if progressive:
        scans = _lib.CsJpegScanInfo()
        rc = lib.cs_jpeg_probe_ex(bytes(data), len(data), _lib.JPEG_PROGRESSIVE, C.byref(info), C.byref(scans))
        return ((info, scans), None) if rc == _lib.CS_OK else (None, _lib.last_error())
    rc = lib.cs_jpeg_probe(bytes(data), len(data), C.byref(info))
    if rc != _lib.CS_OK:
        return None, _lib.last_error()
    return info, None


class PngDecodeHandle:
    """One PngDecoder.decode request: `tensors[i]` is the device image of `paths[i]`; `event` is recorded behind the last launch (and behind the
    copy of the status words to pinned memory).  wait(stream) orders a consumer stream behind the decode without waiting on the host;
    check() is the host wait: it raises ValueError naming the first file whose status is not zero."""

    def __init__(self, paths, tensors, event, groups, host_paths):
        self.paths, self.tensors, self.event, self._groups, self.host_paths = list(paths), list(tensors), event, groups, list(host_paths)
        self._checked = False

    def wait(self, stream=None) -> None:
        stream = stream if stream is not None else torch.cuda.current_stream()
        if self.event is not None:
            stream.wait_event(self.event)
            for t in self.tensors:
                t.record_stream(stream)

    def check(self) -> None:
        if self._checked:
            return
        if self.event is not None:
            self.event.synchronize()
        for paths, status, fmt in self._groups:
            st = status.numpy()
            bad = np.nonzero(st)[0]
            if bad.size:
                i = int(bad[0])
                code = int(st[i])
                table = JPGDEC_STATUS if fmt == "JPEG" else PNGDEC_STATUS
                what = table[code] if code < len(table) else "unknown"
                raise ValueError(f"{paths[i]}: the device {fmt} decoder rejected the file with status {code} ({what})")
        self._checked = True


class PngDecoder:
    """Counterpart of writers.PngEncoder on the input side: PNG files -> decoded images in device memory (cs_op_png_decode).

    decode(paths, gray16) reads the files' bytes on `pool`, probes them on the host (cs_png_probe), groups them by (H, W, kind), uploads each
    group from pinned memory with non-blocking copies and queues one decode launch per group on the decoder's own stream; nothing waits for the
    device.  Per path the handle holds a (H, W, 3) uint8 tensor (read_image_u8's array) or, with gray16=True, a (H, W) int16 tensor holding
    uint16 samples (the convention of InputStage.metric_maps).  A file the probe does not take (interlaced, palette, JPEG, ...) is decoded by
    PIL exactly as without the decoder and uploaded.  The status words travel to pinned memory behind the same event; handle.check() reads them.

    jpeg=True (this_main.jpeg_decoder=gpu) adds baseline JPEG: a file that begins FF D8 (sniffed by content, as PIL does, not by its name) and
    passes cs_jpeg_probe is grouped by (H, W) -- sampling is per file -- and decoded by cs_op_jpeg_decode through the same pinned block, event and
    status copy; a refused JPEG (progressive, CMYK, Adobe, ...) and any JPEG asked for as gray16 go through PIL as before.  Such files count in
    jpeg_stats() and not in stats().  png=False leaves the PNG files on the host path inside the decoder.

    progressive=True (this_main.jpeg_progressive=gpu; needs jpeg=True) probes with cs_jpeg_probe_ex: a complete progressive file joins the
    (H, W) group of the baseline files and the group goes through cs_op_jpeg_decode_ex with CS_JPEG_PROGRESSIVE.  Such files count in
    jpeg_stats()' jpeg_decoded_gpu like any JPEG decoded on the device; progressive_stats() says how many of the progressive files went where."""

    def __init__(self, device, pool=None, png=True, jpeg=False, progressive=False):
        if progressive and not jpeg:
            raise ValueError("PngDecoder: progressive=True needs jpeg=True")
        self.device = torch.device(device)
        self.pool = pool
        self.png, self.jpeg, self.progressive = bool(png), bool(jpeg), bool(progressive)
        self.progressive_gpu = 0
        self.progressive_host = 0
        self.stream = torch.cuda.Stream(self.device)
        self.files_gpu = 0
        self.files_host = 0
        self.jpeg_gpu = 0
        self.jpeg_host = 0

    def _map(self, fn, xs):
        return list(self.pool.map(fn, xs)) if self.pool is not None else [fn(x) for x in xs]

    def decode(self, paths: Sequence[str], gray16: "bool | Sequence[bool]" = False) -> PngDecodeHandle:
        lib = _lib.load()
        paths = list(paths)
        kinds = [bool(gray16)] * len(paths) if isinstance(gray16, (bool, int)) else [bool(g) for g in gray16]
        if len(kinds) != len(paths):
            raise ValueError("PngDecoder.decode: one gray16 flag per path")

        JPEG = -1  # the group kind of cs_op_jpeg_decode, beside _lib.PNG_GRAY16 / PNG_RGB8
        jpeg_mark = object()  # in the place of a PNG's span table
        progressive_mark = object()  # the same for a SOF2 file, with progressive=True
        flags = _lib.JPEG_PROGRESSIVE if self.progressive else 0

        def load(p):
            data = read_file_bytes(p)
            if self.jpeg and data[:2] == b"\xff\xd8":
                if self.progressive:
                    taken = probe_jpeg(data, True)[0]
                    return data, taken and taken[0], progressive_mark if is_progressive_jpeg(data) else jpeg_mark
                return data, probe_jpeg(data)[0], jpeg_mark
            if not self.png:
                return data, None, None
            info, spans = probe_png(data)
            return data, info, spans

        loaded = self._map(load, paths)
        tensors: List[Optional[torch.Tensor]] = [None] * len(paths)
        groups: Dict[Tuple[int, int, int], List[int]] = {}
        host_idx = []
        is_jpeg = [spans is jpeg_mark or spans is progressive_mark for _, _, spans in loaded]
        for i, (data, info, spans) in enumerate(loaded):
            want = _lib.PNG_GRAY16 if kinds[i] else _lib.PNG_RGB8
            if is_jpeg[i]:
                if info is None or kinds[i]:
                    host_idx.append(i)  # a JPEG the device decoder does not take, or one asked for as a 16-bit map: PIL
                else:
                    groups.setdefault((info.height, info.width, JPEG), []).append(i)
            elif info is None or info.kind != want:
                host_idx.append(i)  # not built on the device (or not the kind asked for): PIL, which also raises what it raised before
            else:
                groups.setdefault((info.height, info.width, info.kind), []).append(i)
        host_imgs = self._map(lambda i: (read_metric_map_u16 if kinds[i] else read_image_u8)(paths[i]), host_idx)
        done = []
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            st = C.c_void_p(self.stream.cuda_stream)
            for i, im in zip(host_idx, host_imgs):
                pinned = torch.empty(im.shape, dtype=torch.int16 if kinds[i] else torch.uint8, pin_memory=True)
                pinned.numpy()[...] = im.view(np.int16) if kinds[i] else im
                tensors[i] = pinned.to(self.device, non_blocking=True)
            for (h, w, kind), idx in groups.items():
                n = len(idx)
                lengths = np.array([len(loaded[i][0]) for i in idx], dtype=np.uint32)
                offsets = np.zeros((n,), dtype=np.uint64)
                offsets[1:] = np.cumsum(lengths.astype(np.uint64))[:-1]
                total = int(lengths.astype(np.uint64).sum())
                if kind == JPEG:
                    # one pinned block: file bytes | offsets (u64) | lengths, each part 8-byte aligned
                    at_off = (total + 7) // 8 * 8
                    at_len = at_off + n * 8
                    block = torch.empty((at_len + (n * 4 + 7) // 8 * 8,), dtype=torch.uint8, pin_memory=True)
                    bv = block.numpy()
                    for j, i in enumerate(idx):
                        bv[int(offsets[j]):int(offsets[j]) + int(lengths[j])] = np.frombuffer(loaded[i][0], dtype=np.uint8)
                    bv[at_off:at_off + n * 8] = offsets.view(np.uint8)
                    bv[at_len:at_len + n * 4] = lengths.view(np.uint8)
                    d_block = block.to(self.device, non_blocking=True)
                    base = d_block.data_ptr()
                    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=self.device)
                    status = torch.empty((n,), dtype=torch.int32, device=self.device)
                    work = torch.empty((lib.cs_jpeg_decode_workspace_bytes_ex(n, h, w, total, flags),), dtype=torch.uint8, device=self.device)
                    _lib.check(lib.cs_op_jpeg_decode_ex(C.c_void_p(base), C.c_void_p(base + at_off), C.c_void_p(base + at_len), total, n, h, w,
                                                        C.c_void_p(out.data_ptr()), h * w * 3, C.c_void_p(status.data_ptr()),
                                                        C.c_void_p(work.data_ptr()), flags, st))
                    host_status = torch.empty((n,), dtype=torch.int32, pin_memory=True)
                    host_status.copy_(status, non_blocking=True)
                    for j, i in enumerate(idx):
                        tensors[i] = out[j]
                    done.append(([paths[i] for i in idx], host_status, "JPEG"))
                    continue
                nspans = np.array([len(loaded[i][2]) for i in idx], dtype=np.uint32)
                span_off = np.zeros((n + 1,), dtype=np.uint32)
                span_off[1:] = np.cumsum(nspans)
                # one pinned block: file bytes | offsets (u64) | lengths | span offsets | spans, each part 8-byte aligned
                parts = [("files", total, 1), ("offsets", n * 8, 8), ("lengths", n * 4, 4), ("span_off", (n + 1) * 4, 4), ("spans", int(span_off[-1]) * 8, 4)]
                at, pos = {}, 0
                for name, nbytes, _ in parts:
                    at[name] = pos
                    pos += (nbytes + 7) // 8 * 8
                block = torch.empty((pos,), dtype=torch.uint8, pin_memory=True)
                bv = block.numpy()
                for j, i in enumerate(idx):
                    bv[int(offsets[j]):int(offsets[j]) + int(lengths[j])] = np.frombuffer(loaded[i][0], dtype=np.uint8)
                bv[at["offsets"]:at["offsets"] + n * 8] = offsets.view(np.uint8)
                bv[at["lengths"]:at["lengths"] + n * 4] = lengths.view(np.uint8)
                bv[at["span_off"]:at["span_off"] + (n + 1) * 4] = span_off.view(np.uint8)
                bv[at["spans"]:at["spans"] + int(span_off[-1]) * 8] = np.concatenate([loaded[i][2] for i in idx]).reshape(-1).view(np.uint8)
                d_block = block.to(self.device, non_blocking=True)
                base = d_block.data_ptr()
                out = torch.empty((n, h, w) if kind == _lib.PNG_GRAY16 else (n, h, w, 3), dtype=torch.int16 if kind == _lib.PNG_GRAY16 else torch.uint8,
                                  device=self.device)
                status = torch.empty((n,), dtype=torch.int32, device=self.device)
                work = torch.empty((lib.cs_png_decode_workspace_bytes(kind, n, h, w, total),), dtype=torch.uint8, device=self.device)
                _lib.check(lib.cs_op_png_decode(C.c_void_p(base + at["files"]), C.c_void_p(base + at["offsets"]), C.c_void_p(base + at["lengths"]),
                                                C.c_void_p(base + at["spans"]), C.c_void_p(base + at["span_off"]), total, n, kind, h, w,
                                                C.c_void_p(out.data_ptr()), h * w * (2 if kind == _lib.PNG_GRAY16 else 3),
                                                C.c_void_p(status.data_ptr()), C.c_void_p(work.data_ptr()), st))
                host_status = torch.empty((n,), dtype=torch.int32, pin_memory=True)
                host_status.copy_(status, non_blocking=True)
                for j, i in enumerate(idx):
                    tensors[i] = out[j]
                done.append(([paths[i] for i in idx], host_status, "PNG"))
            event = torch.cuda.Event()
            event.record(self.stream)
        jpeg_gpu = sum(len(g) for (_, _, kind), g in groups.items() if kind == JPEG)
        jpeg_host = sum(1 for i in host_idx if is_jpeg[i])
        self.jpeg_gpu += jpeg_gpu
        self.jpeg_host += jpeg_host
        progressive_host = sum(1 for i in host_idx if loaded[i][2] is progressive_mark)
        self.progressive_host += progressive_host
        self.progressive_gpu += sum(1 for _, _, spans in loaded if spans is progressive_mark) - progressive_host
        self.files_gpu += sum(len(g) for g in groups.values()) - jpeg_gpu
        self.files_host += len(host_idx) - jpeg_host
        return PngDecodeHandle(paths, tensors, event, done, [paths[i] for i in host_idx])

    def stats(self) -> Dict[str, int]:
        return {"png_decoded_gpu": self.files_gpu, "png_decoded_host": self.files_host}

    def jpeg_stats(self) -> Dict[str, int]:
        """Files that begin FF D8, counted only with jpeg=True (without it a JPEG is one more file of stats()' host count)."""
        return {"jpeg_decoded_gpu": self.jpeg_gpu, "jpeg_decoded_host": self.jpeg_host}


    def progressive_stats(self) -> Dict[str, int]:
        """Of the progressive (SOF2) files seen with progressive=True: decoded on the device / left to PIL (refused by cs_jpeg_probe_ex, or asked
        for as a 16-bit map)."""
        return {"jpeg_progressive_gpu": self.progressive_gpu, "jpeg_progressive_host": self.progressive_host}


def is_progressive_jpeg(data: bytes) -> bool:
    """True when the first frame header of a JPEG file's bytes is SOF2 (a walk over the marker segments; for progressive_stats())."""
    pos, n = 2, len(data)
    while pos + 4 <= n and data[pos] == 0xFF:
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return m == 0xC2
        elif m == 0xDA or m in (0x00, 0x01) or 0xD0 <= m <= 0xD9:
            return False
        else:
            pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    return False


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


class DecodeWindow:
    """The drivers' loader with this_main.png_decoder=gpu or this_main.jpeg_decoder=gpu: the files of all batches are known up front, so the decoder is handed a window of
    upcoming files (this_main.png_decode_window, independent of the batch size) and a file's decode latency hides behind earlier forwards.

    plan: per batch the ordered (path, gray16) list of what that batch reads.  fetch(b) returns {path: device tensor} for batch b with the
    current stream ordered behind the decodes it needs; whenever batch b holds a file that is not queued yet, windows of `window` files are
    queued from the first such file on (so a window smaller than a batch is several calls, a larger one reaches into the next batches).
    check(b) is the host side of batch b's status words: call it where the loop waits for that batch anyway."""

    def __init__(self, decoder: PngDecoder, plan: Sequence[Sequence[Tuple[str, bool]]], window: int):
        self.decoder, self.window = decoder, max(1, int(window))
        self.plan = [list(dict.fromkeys(p)) for p in plan]
        self.queue = [(b, path, g) for b, files in enumerate(self.plan) for path, g in files]
        self.next = 0  # first entry of the queue not handed to the decoder yet
        self.ready: Dict[Tuple[int, str, bool], Tuple[torch.Tensor, PngDecodeHandle]] = {}
        self.handles: Dict[int, List[PngDecodeHandle]] = {}

    def _queue_window(self) -> None:
        entries = self.queue[self.next:self.next + self.window]
        self.next += len(entries)
        uniq = list(dict.fromkeys((path, g) for _, path, g in entries))  # a file named by two batches of one window is decoded once
        handle = self.decoder.decode([p for p, _ in uniq], [g for _, g in uniq])
        where = {k: i for i, k in enumerate(uniq)}
        for b, path, g in entries:
            self.ready[(b, path, g)] = (handle.tensors[where[(path, g)]], handle)

    def fetch(self, b: int) -> Dict[str, torch.Tensor]:
        need = [(b, path, g) for path, g in self.plan[b]]
        while any(k not in self.ready for k in need):
            self._queue_window()
        out, handles = {}, []
        for k in need:
            t, h = self.ready.pop(k)
            out[k[1]] = t
            if all(h is not x for x in handles):
                handles.append(h)
        cur = torch.cuda.current_stream(self.decoder.device)
        for h in handles:
            h.wait(cur)
        self.handles[b] = handles
        return out

    def check(self, b: int) -> None:
        for h in self.handles.pop(b, []):
            h.check()


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
        """The decoded image on the device: a host array goes up (a blocking pageable copy), a CUDA uint8 (h, w, 3) tensor (data.PngDecoder's
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
        """The decoded image on the device with its geometry (model.U8Image) for CrossScoreNet.forward_u8 and its siblings.  img_u8: a host
        array or a CUDA uint8 tensor (no copy)."""
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


def decode_items(items: List[Dict[str, object]], zero_reference: bool = False, pool=None, skip=()) -> Dict[str, np.ndarray]:
    """path -> decoded uint8 image for every file the items name (host side; PIL releases the GIL while decoding, so a thread pool
    plays the role of the reference's DataLoader workers, task/predict.py:110-117).  Reference paths in `skip` (already in the
    token cache) are not decoded."""
    uniq = list(dict.fromkeys(p for p, _ in batch_files(items, zero_reference, skip=skip)))
    imgs = list(pool.map(read_image_u8, uniq)) if pool is not None else [read_image_u8(p) for p in uniq]
    return dict(zip(uniq, imgs))


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
    u8: the one-pass input stage -- "query/img" and "reference/cross/imgs" are model.U8Batch objects (decoded images on the device + geometry) for
    CrossScoreNet.forward_u8 and no processed fp32 tensor exists; else (B, 3, oh, ow) and (B, N, 3, oh, ow) fp32 tensors.
    references=False: the references come from a ReferenceTokenCache and "reference/cross/imgs" is None."""
    decoded = decoded if decoded is not None else {}
    q_imgs = [decoded[it["query/img"]] if it["query/img"] in decoded else read_image_u8(it["query/img"]) for it in items]
    geo = {stage.geometry(*im.shape[:2])[1][2:] for im in q_imgs}
    if len(geo) != 1:
        raise ValueError(f"query images of one batch must share the processed size, got {sorted(geo)}")
    size = oh, ow = next(iter(geo))
    ref_lists = [it["reference/cross/imgs"] if references else () for it in items]
    # nvs_dataset.py:459-470: placeholders and zero_reference are all-zero images BEFORE T.Normalize -> (0 - mean) / std
    blank = lambda p: p == EMPTY or zero_reference  # noqa: E731
    if u8:
        refs = stage.batch([stage.placeholder(size) if blank(p) else stage.describe(_reference_image(p, decoded, stage, size))
                            for ps in ref_lists for p in ps], size) if references else None
        query = stage.batch([stage.describe(qi) for qi in q_imgs], size)
    else:
        query = torch.empty((len(items), 3, oh, ow), dtype=torch.float32, device=stage.device)
        refs = torch.empty((len(items), len(ref_lists[0]), 3, oh, ow), dtype=torch.float32, device=stage.device) if references else None
        for b, (ps, qi) in enumerate(zip(ref_lists, q_imgs)):
            stage(qi, query[b])
            for n, p in enumerate(ps):
                if blank(p):
                    refs[b, n] = stage.zero_image_value[:, None, None]
                else:
                    stage(_reference_image(p, decoded, stage, size), refs[b, n])
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
            if self.from_u8:
                tok = self.net.encode_references_u8(self.stage.batch(
                    [self.stage.placeholder((oh, ow)) if im is None else self.stage.describe(im) for im in imgs], (oh, ow)))
            else:
                buf = torch.empty((len(missing), 3, oh, ow), dtype=torch.float32, device=self.stage.device)
                for i, im in enumerate(imgs):
                    if im is None:
                        buf[i] = self.stage.zero_image_value[:, None, None]
                    else:
                        self.stage(im, buf[i])
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

    decoder: the run's PngDecoder (this_main.png_decoder / jpeg_decoder = gpu): a chunk's files are decoded on the device, `window` files per
    call; else PIL on `pool`.  from_u8: the one-pass input stage (encode_references_u8; no processed image exists, so not with keep_images)."""

    def __init__(self, net, stage: InputStage, paths: Sequence[str], size: Tuple[int, int], n_references: int, keep_images: bool = False,
                 max_images: int = 4096, from_u8: bool = False, decoder: Optional[PngDecoder] = None, pool=None, chunk: int = 32, window: int = 64,
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
            if from_u8:
                tok = net.encode_references_u8(stage.batch([stage.describe(im) for im in imgs], (oh, ow)))
            else:
                buf = self.images[r0:r0 + len(part)] if keep_images else torch.empty((len(part), 3, oh, ow), dtype=torch.float32, device=stage.device)
                for i, im in enumerate(imgs):
                    stage(im, buf[i])
                tok = net.encode_references(buf)
            if tokens is None:
                tokens = torch.empty((R,) + tuple(tok.shape[1:]), dtype=tok.dtype, device=tok.device)
            tokens[r0:r0 + len(part)] = tok
        if groups is not None:  # the placeholder's row: zeros BEFORE T.Normalize, as load_batch and ReferenceTokenCache feed "empty_image"
            if from_u8:
                tokens[R - 1] = net.encode_references_u8(stage.batch([stage.placeholder((oh, ow))], (oh, ow)))[0]
            else:
                buf = self.images[R - 1:] if keep_images else torch.empty((1, 3, oh, ow), dtype=torch.float32, device=stage.device)
                buf[0] = stage.zero_image_value[:, None, None]
                tokens[R - 1] = net.encode_references(buf)[0]
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
