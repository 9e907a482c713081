"""Input decoding: a file's bytes -> the decoded image, on the host or in device memory.  Knows files, not items, batches or the model.

PNG/JPEG decoding stays on the host (PIL, as in utils/io/images.py:26-29) unless this_main.png_decoder=gpu hands the PNG files
and / or this_main.jpeg_decoder=gpu the baseline JPEG files to ImageDecoder (cs_op_png_decode, cs_op_jpeg_decode: the compressed bytes go up and
the decoded images appear in device memory, the pixels PIL gives, bit for bit).  Files neither device decoder takes (interlaced or palette PNG,
progressive / CMYK / Adobe JPEG, ...) still go through PIL; this_main.jpeg_progressive=gpu adds complete progressive files (cs_op_jpeg_decode_ex).
"""
from __future__ import annotations

import collections
import ctypes as C
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .config import this_main_choice


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


DECODER_CHOICES = ("host", "gpu")
PNGDEC_STATUS = ("ok", "bad CRC-32", "bad Adler-32", "bad zlib header", "reserved block type", "stored LEN/NLEN mismatch",
                 "over-subscribed or incomplete code", "invalid symbol", "distance before the start of the stream", "stream too short",
                 "stream too long", "filter type above 4", "input exhausted", "IHDR differs from the size or format asked for", "bad chunk framing")


def png_decoder_choice(cfg) -> str:
    """this_main.png_decoder (this build's key): host (default) | gpu."""
    return this_main_choice(cfg, "png_decoder", DECODER_CHOICES)


JPGDEC_STATUS = ("ok", "bad framing (SOI, a segment length past the file, no SOF / SOS)", "SOF differs from the size asked for, or a form the decoder does not take",
                 "bad Huffman or quantisation table", "bits that are no code of the table", "invalid symbol", "input exhausted", "missing, misnumbered or surplus restart marker",
                 "illegal scan, DQT / DRI behind the first scan, or an incomplete progression")


def jpeg_decoder_choice(cfg) -> str:
    """this_main.jpeg_decoder (this build's key): host (default) | gpu."""
    return this_main_choice(cfg, "jpeg_decoder", DECODER_CHOICES)


def jpeg_progressive_choice(cfg) -> str:
    """this_main.jpeg_progressive (this build's key): host (default) | gpu.  gpu needs this_main.jpeg_decoder=gpu."""
    choice = this_main_choice(cfg, "jpeg_progressive", DECODER_CHOICES)
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


class Probed(NamedTuple):
    """What the host probes say about one file's bytes.  fmt: "png" (the PNG signature), "jpeg" (FF D8, looked for only with jpeg=True) or None;
    info: the probe's CsPngInfo / CsJpegInfo when the device decoder takes the file, else None (the file goes to PIL); spans: a taken PNG's IDAT
    span table; progressive: a SOF2 file seen with progressive=True."""
    data: bytes
    fmt: Optional[str]
    info: object
    spans: Optional[np.ndarray]
    progressive: bool


PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def probe_file(data: bytes, png: bool = True, jpeg: bool = False, progressive: bool = False) -> Probed:
    """Routes a file's bytes by content (as PIL does, not by a name) through the host probes the decoder's flags allow.  No device is touched."""
    if jpeg and data[:2] == b"\xff\xd8":
        if progressive:
            taken = probe_jpeg(data, True)[0]
            return Probed(data, "jpeg", taken and taken[0], None, is_progressive_jpeg(data))
        return Probed(data, "jpeg", probe_jpeg(data)[0], None, False)
    if not png or data[:8] != PNG_SIGNATURE:
        return Probed(data, None, None, None, False)
    info, spans = probe_png(data)
    return Probed(data, "png", info, spans if info is not None else None, False)


def block_layout(lengths: Sequence[int], span_counts: Optional[Sequence[int]] = None) -> Tuple[Dict[str, int], int]:
    """One group's upload block: files | offsets (u64) | lengths (u32) | span_off (u32, n + 1) | spans (8 bytes each), each part padded to
    8 bytes; without span_counts (JPEG) the last two parts are absent.  -> ({part: byte offset}, block size)."""
    n = len(lengths)
    parts = [("files", sum(lengths)), ("offsets", n * 8), ("lengths", n * 4)]
    if span_counts is not None:
        parts += [("span_off", (n + 1) * 4), ("spans", sum(span_counts) * 8)]
    at, pos = {}, 0
    for name, nbytes in parts:
        at[name] = pos
        pos += (nbytes + 7) // 8 * 8
    return at, pos


def fill_block(bv: np.ndarray, at: Dict[str, int], files: Sequence[bytes], spans: Optional[Sequence[np.ndarray]] = None) -> None:
    """Writes block_layout's parts into the uint8 view `bv`: each file's bytes once, straight to their place; the padding is left as it is."""
    n = len(files)
    lengths = np.array([len(f) for f in files], dtype=np.uint32)
    offsets = np.zeros((n,), dtype=np.uint64)
    offsets[1:] = np.cumsum(lengths.astype(np.uint64))[:-1]
    for f, o in zip(files, offsets.tolist()):
        bv[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    bv[at["offsets"]:at["offsets"] + n * 8] = offsets.view(np.uint8)
    bv[at["lengths"]:at["lengths"] + n * 4] = lengths.view(np.uint8)
    if spans is not None:
        span_off = np.zeros((n + 1,), dtype=np.uint32)
        span_off[1:] = np.cumsum([len(s) for s in spans])
        bv[at["span_off"]:at["span_off"] + (n + 1) * 4] = span_off.view(np.uint8)
        bv[at["spans"]:at["spans"] + int(span_off[-1]) * 8] = np.concatenate(spans).reshape(-1).view(np.uint8)


def _launch_png(lib, base, at, total, n, kind, h, w, out, stride, status, flags, st):
    work = torch.empty((lib.cs_png_decode_workspace_bytes(kind, n, h, w, total),), dtype=torch.uint8, device=out.device)
    _lib.check(lib.cs_op_png_decode(C.c_void_p(base + at["files"]), C.c_void_p(base + at["offsets"]), C.c_void_p(base + at["lengths"]),
                                    C.c_void_p(base + at["spans"]), C.c_void_p(base + at["span_off"]), total, n, kind, h, w,
                                    C.c_void_p(out.data_ptr()), stride, C.c_void_p(status.data_ptr()), C.c_void_p(work.data_ptr()), st))


def _launch_jpeg(lib, base, at, total, n, kind, h, w, out, stride, status, flags, st):
    work = torch.empty((lib.cs_jpeg_decode_workspace_bytes_ex(n, h, w, total, flags),), dtype=torch.uint8, device=out.device)
    _lib.check(lib.cs_op_jpeg_decode_ex(C.c_void_p(base + at["files"]), C.c_void_p(base + at["offsets"]), C.c_void_p(base + at["lengths"]), total, n, h, w,
                                        C.c_void_p(out.data_ptr()), stride, C.c_void_p(status.data_ptr()), C.c_void_p(work.data_ptr()), flags, st))


# per format: the label of DecodeHandle.check(), its status table, and the workspace + launch call; the output is the kind's for both
FORMATS = {"png": ("PNG", PNGDEC_STATUS, _launch_png), "jpeg": ("JPEG", JPGDEC_STATUS, _launch_jpeg)}


class DecodeHandle:
    """One ImageDecoder.decode request: `tensors[i]` is the device image of `paths[i]`; `event` is recorded behind the last launch (and behind the
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
                label, table, _ = FORMATS[fmt]
                what = table[code] if code < len(table) else "unknown"
                raise ValueError(f"{paths[i]}: the device {label} decoder rejected the file with status {code} ({what})")
        self._checked = True


class ImageDecoder:
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
            raise ValueError("ImageDecoder: progressive=True needs jpeg=True")
        self.device = torch.device(device)
        self.pool = pool
        self.png, self.jpeg, self.progressive = bool(png), bool(jpeg), bool(progressive)
        self.counts = collections.Counter()  # the keys of the three *_stats(), counted where decode() routes a file
        self.stream = torch.cuda.Stream(self.device)

    def _map(self, fn, xs):
        return list(self.pool.map(fn, xs)) if self.pool is not None else [fn(x) for x in xs]

    def decode(self, paths: Sequence[str], gray16: "bool | Sequence[bool]" = False) -> DecodeHandle:
        lib = _lib.load()
        paths = list(paths)
        kinds = [bool(gray16)] * len(paths) if isinstance(gray16, (bool, int)) else [bool(g) for g in gray16]
        if len(kinds) != len(paths):
            raise ValueError("ImageDecoder.decode: one gray16 flag per path")
        flags = _lib.JPEG_PROGRESSIVE if self.progressive else 0

        probed = self._map(lambda p: probe_file(read_file_bytes(p), self.png, self.jpeg, self.progressive), paths)
        tensors: List[Optional[torch.Tensor]] = [None] * len(paths)
        groups: Dict[Tuple[str, int, int, int], List[int]] = {}
        host_idx = []
        for i, p in enumerate(probed):
            want = _lib.PNG_GRAY16 if kinds[i] else _lib.PNG_RGB8
            # PIL takes a file not built on the device, a PNG of another kind than asked for and a JPEG asked for as a 16-bit map (and raises
            # there what it raised before)
            taken = p.info is not None and (not kinds[i] if p.fmt == "jpeg" else p.info.kind == want)
            where = "gpu" if taken else "host"
            self.counts[f"{'jpeg' if p.fmt == 'jpeg' else 'png'}_decoded_{where}"] += 1
            if p.progressive:
                self.counts[f"jpeg_progressive_{where}"] += 1
            if taken:
                groups.setdefault((p.fmt, p.info.height, p.info.width, want), []).append(i)
            else:
                host_idx.append(i)
        host_imgs = self._map(lambda i: (read_metric_map_u16 if kinds[i] else read_image_u8)(paths[i]), host_idx)
        done = []
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            st = C.c_void_p(self.stream.cuda_stream)
            for i, im in zip(host_idx, host_imgs):
                pinned = torch.empty(im.shape, dtype=torch.int16 if kinds[i] else torch.uint8, pin_memory=True)
                pinned.numpy()[...] = im.view(np.int16) if kinds[i] else im
                tensors[i] = pinned.to(self.device, non_blocking=True)
            for (fmt, h, w, kind), idx in groups.items():
                n = len(idx)
                files = [probed[i].data for i in idx]
                spans = [probed[i].spans for i in idx] if fmt == "png" else None
                # one pinned block (block_layout): the files' bytes and the tables the kernels index them by
                lengths = [len(f) for f in files]
                at, size = block_layout(lengths, None if spans is None else [len(s) for s in spans])
                block = torch.empty((size,), dtype=torch.uint8, pin_memory=True)
                fill_block(block.numpy(), at, files, spans)
                d_block = block.to(self.device, non_blocking=True)
                gray = kind == _lib.PNG_GRAY16
                out = torch.empty((n, h, w) if gray else (n, h, w, 3), dtype=torch.int16 if gray else torch.uint8, device=self.device)
                status = torch.empty((n,), dtype=torch.int32, device=self.device)
                FORMATS[fmt][2](lib, d_block.data_ptr(), at, sum(lengths), n, kind, h, w, out, h * w * (2 if gray else 3), status, flags, st)
                host_status = torch.empty((n,), dtype=torch.int32, pin_memory=True)
                host_status.copy_(status, non_blocking=True)
                for j, i in enumerate(idx):
                    tensors[i] = out[j]
                done.append(([paths[i] for i in idx], host_status, fmt))
            event = torch.cuda.Event()
            event.record(self.stream)
        return DecodeHandle(paths, tensors, event, done, [paths[i] for i in host_idx])

    def stats(self) -> Dict[str, int]:
        return {k: self.counts[k] for k in ("png_decoded_gpu", "png_decoded_host")}

    def jpeg_stats(self) -> Dict[str, int]:
        """Files that begin FF D8, counted only with jpeg=True (without it a JPEG is one more file of stats()' host count)."""
        return {k: self.counts[k] for k in ("jpeg_decoded_gpu", "jpeg_decoded_host")}

    def progressive_stats(self) -> Dict[str, int]:
        """Of the progressive (SOF2) files seen with progressive=True: decoded on the device / left to PIL (refused by cs_jpeg_probe_ex, or asked
        for as a 16-bit map)."""
        return {k: self.counts[k] for k in ("jpeg_progressive_gpu", "jpeg_progressive_host")}


class DecodeWindow:
    """The drivers' loader with this_main.png_decoder=gpu or this_main.jpeg_decoder=gpu: the files of all batches are known up front, so the decoder is handed a window of
    upcoming files (this_main.png_decode_window, independent of the batch size) and a file's decode latency hides behind earlier forwards.

    plan: per batch the ordered (path, gray16) list of what that batch reads.  fetch(b) returns {path: device tensor} for batch b with the
    current stream ordered behind the decodes it needs; whenever batch b holds a file that is not queued yet, windows of `window` files are
    queued from the first such file on (so a window smaller than a batch is several calls, a larger one reaches into the next batches).
    check(b) is the host side of batch b's status words: call it where the loop waits for that batch anyway."""

    def __init__(self, decoder: ImageDecoder, plan: Sequence[Sequence[Tuple[str, bool]]], window: int):
        self.decoder, self.window = decoder, max(1, int(window))
        self.plan = [list(dict.fromkeys(p)) for p in plan]
        self.queue = [(b, path, g) for b, files in enumerate(self.plan) for path, g in files]
        self.next = 0  # first entry of the queue not handed to the decoder yet
        self.ready: Dict[Tuple[int, str, bool], Tuple[torch.Tensor, DecodeHandle]] = {}
        self.handles: Dict[int, List[DecodeHandle]] = {}

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
