"""The ground-truth side of the score summary: per frame the mean SSIM / MAE / MSE and the PSNR of its ground-truth metric maps, as the CSV the
reference's utils/evaluation/summarise_score_gt.py writes (utils/io/score_summariser.py:16-139), which summary.py lines up with the predicted
CSV of predict / evaluate (writers.ScoreSummariser).

    python -m crossscore_amd.summarise_gt --dir_in <.../res_540> --dir_out <dir> [-n workers] [-f True|False] [--fast_debug N]
                                          [--source files|compute] [--png_decoder host|gpu] [--jpeg_decoder host|gpu] [--jpeg_progressive host|gpu]

--source files (default) reads <iter>/metric_map/{ssim,mae}/ as the reference does; --source compute needs only renders/ and gt/ and forms the
same numbers from the image pairs, without the maps in memory or on disk.  The device returns four exact integer sums per frame
(cs_op_metric_map_sums_u16 / cs_op_gt_metric_sums_u8) and the five values follow on the host in fp64:
    ssim_-1_1 = S1 / (32767 n) - 1    ssim_0_1 = (S2 - 32767 n) / (32767 n)    mae = S3 / (65535 n)    mse = S4 / (65535^2 n)    psnr = -10 log10(mse)
The reference forms them as fp32 numpy means of fp32 pixels; the two agree to about 1e-7, so a printed "%.4f" differs only where a value lies
that close to a rounding boundary.  One process, one GPU; no CPU fallback.  list_frames, rows_from_sums and write_csv are the host logic and
need no GPU.
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import math
import os
import time
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

SOURCES = ("files", "compute")
COLUMNS = ["scene_name", "rendered_dir", "image_name", "gt_ssim_-1_1", "gt_ssim_0_1", "gt_mae", "gt_mse", "gt_psnr"]
BATCH_ROWS = 16  # the reference's DataLoader batch: --fast_debug N stops behind batch N
# ssim_path names the frame (the path its SSIM map has or would have); first / second are what is read: the ssim and mae maps (files) or the
# render and the captured image (compute)
Frame = namedtuple("Frame", "ssim_path first second")


def _walk_dirs(dir_in: str) -> Iterable[Tuple[str, List[str]]]:
    """(directory, names of its sub-directories) below dir_in as glob("**") sees them: hidden directories are not entered."""
    for root, dirs, _ in os.walk(dir_in, followlinks=True):
        dirs[:] = [d for d in dirs if not d.startswith(".")]
        yield root, dirs


def list_frames(dir_in, source: str = "files") -> List[Frame]:
    """files: every directory named metric_map below dir_in, sorted as strings (score_summariser.py:108: ours_1000, ours_30000, ours_7000;
    split.json is not consulted); in each the sorted names of ssim/ beside those of mae/.  compute: every directory that holds renders/ and
    gt/, in the same order, with metric_maps.pairs_of for the pairs."""
    if source not in SOURCES:
        raise ValueError(f"source={source!r} not supported: files | compute")
    dir_in = str(Path(dir_in).expanduser())
    frames: List[Frame] = []
    if source == "files":
        map_dirs = sorted(os.path.join(root, "metric_map") for root, dirs in _walk_dirs(dir_in) if "metric_map" in dirs)
        for md in map_dirs:
            names = sorted(os.listdir(os.path.join(md, "ssim")))
            if names != sorted(os.listdir(os.path.join(md, "mae"))):
                raise ValueError(f"{md}: ssim/ and mae/ do not hold the same file names")
            frames += [Frame(os.path.join(md, "ssim", n), os.path.join(md, "ssim", n), os.path.join(md, "mae", n)) for n in names]
        return frames
    from .metric_maps import pairs_of

    map_dirs = sorted(os.path.join(root, "metric_map") for root, dirs in _walk_dirs(dir_in) if "renders" in dirs and "gt" in dirs)
    for md in map_dirs:
        frames += [Frame(os.path.join(md, "ssim", n), rp, gp) for n, rp, gp in pairs_of(Path(md).parent)]
    return frames


def values_from_sums(s: Sequence[int], n: int) -> Tuple[float, float, float, float, float]:
    """The five values of a frame of n pixels from its four integer sums (S1, S2, S3, S4), in fp64; mse = 0 gives psnr = inf."""
    s1, s2, s3, s4 = (int(v) for v in s)
    mse = s4 / (65535 * 65535 * n)
    return (s1 / (32767 * n) - 1.0, (s2 - 32767 * n) / (32767 * n), s3 / (65535 * n), mse, -10.0 * math.log10(mse) if mse > 0 else math.inf)


def rows_from_sums(frames: Sequence[Frame], sums: Sequence[Sequence[int]], sizes: Sequence[Tuple[int, int]]) -> List[list]:
    """One CSV row per frame (score_summariser.py:119-136): scene_name is part -6 of the SSIM map's path, rendered_dir its parts up to the
    iteration directory joined without the leading "/" (as the predicted CSV's: the two join on it), image_name the name without "frame_"."""
    rows = []
    for fr, s, (h, w) in zip(frames, sums, sizes):
        parts = fr.ssim_path.split("/")
        if len(parts) < 6:
            raise ValueError(f"{fr.ssim_path}: expected <scene>/<split>/<iteration>/metric_map/ssim/<name>")
        rows.append([parts[-6], os.path.join(*parts[:-3]), parts[-1].replace("frame_", ""), *values_from_sums(s, h * w)])
    return rows


def csv_path(dir_in, dir_out) -> Path:
    dir_in = Path(dir_in).expanduser()
    return Path(dir_out).expanduser() / dir_in.parent.name / f"{dir_in.parents[1].name}.csv"


def _check_write(path: Path, force: bool) -> bool:
    """score_summariser.py:92-104, messages included."""
    if path.exists():
        if force:
            path.unlink()
            print(f"Write to csv {path} (OVERWRITE)")
            return True
        print(f"Write to csv {path} (SKIP)")
        return False
    print(f"Write to csv {path} (NORMAL)")
    return True


def write_csv(dir_in, dir_out, rows: Union[Sequence[list], Callable[[], Sequence[list]]], force: bool = False,
              fast_debug: int = -1) -> Optional[str]:
    """Writes <dir_out>/<dir_in.parent.name>/<dir_in.parents[1].name>.csv with float_format "%.4f" and returns its path, or None when the file
    exists and force is off (SKIP).  rows: the rows, or a function that forms them (not called on SKIP).  fast_debug N > 0 keeps the first
    (N + 1) * 16 rows."""
    path = csv_path(dir_in, dir_out)
    path.parent.mkdir(parents=True, exist_ok=True)
    if not _check_write(path, bool(force)):
        return None
    rows = rows() if callable(rows) else rows
    if fast_debug > 0:
        rows = rows[:(fast_debug + 1) * BATCH_ROWS]
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(COLUMNS)
        for r in rows:
            w.writerow(list(r[:3]) + ["%.4f" % v for v in r[3:]])
    return str(path)


# ------------------------------------------------------------------------------------------------------------------ device
def _block(items: Sequence, device):
    """Frames of one size as one device tensor: host arrays go up from one pinned block (a non-blocking copy), device tensors are gathered."""
    import torch

    if isinstance(items[0], torch.Tensor):
        return torch.stack(list(items))
    first = items[0]
    sixteen = first.dtype == np.uint16
    pinned = torch.empty((len(items),) + tuple(first.shape), dtype=torch.int16 if sixteen else torch.uint8, pin_memory=True)
    pv = pinned.numpy()
    for j, a in enumerate(items):
        pv[j] = a.view(np.int16) if sixteen else a
    return pinned.to(device, non_blocking=True)


def frame_sums(frames: Sequence[Frame], source: str = "files", png_decoder: str = "host", workers: int = 16,
               device=None, jpeg_decoder: str = "host", jpeg_progressive: str = "host") -> Tuple[List[Tuple[int, int, int, int]], List[Tuple[int, int]]]:
    """(sums, sizes) of the frames: per frame its four integer sums and its (H, W).  png_decoder / jpeg_decoder: who decodes the PNG / baseline JPEG
    files (decode.ImageDecoder when either is gpu)."""
    import torch

    from . import _lib
    from .decode import DECODER_CHOICES, ImageDecoder, read_image_u8, read_metric_map_u16
    from .metric_maps import GROUP

    if source not in SOURCES:
        raise ValueError(f"source={source!r} not supported: files | compute")
    if png_decoder not in DECODER_CHOICES:
        raise ValueError(f"png_decoder={png_decoder!r} not supported: host | gpu")
    if jpeg_decoder not in DECODER_CHOICES:
        raise ValueError(f"jpeg_decoder={jpeg_decoder!r} not supported: host | gpu")
    if jpeg_progressive not in DECODER_CHOICES:
        raise ValueError(f"jpeg_progressive={jpeg_progressive!r} not supported: host | gpu")
    if jpeg_progressive == "gpu" and jpeg_decoder != "gpu":
        raise ValueError("jpeg_progressive=gpu needs jpeg_decoder=gpu")
    if not torch.cuda.is_available():
        raise RuntimeError("crossscore_amd.summarise_gt needs a GPU: the frame sums have no CPU fallback")
    device = torch.device("cuda", 0) if device is None else torch.device(device)
    torch.cuda.set_device(device)
    lib = _lib.load()
    files = source == "files"
    sums: List[Optional[Tuple[int, int, int, int]]] = [None] * len(frames)
    sizes: List[Optional[Tuple[int, int]]] = [None] * len(frames)
    pending = []  # (event, pinned sums, frame indices, the launch's inputs and the decode handle: alive until the event)

    def drain(keep: int) -> None:
        while len(pending) > keep:
            event, host, idx, _ = pending.pop(0)
            event.synchronize()
            vals = host.numpy().view(np.uint64)
            for j, i in enumerate(idx):
                sums[i] = tuple(int(v) for v in vals[j])

    pool = ThreadPoolExecutor(max_workers=max(1, int(workers)))
    try:
        decoder = ImageDecoder(device, pool, png=png_decoder == "gpu", jpeg=jpeg_decoder == "gpu",
                             progressive=jpeg_progressive == "gpu") if "gpu" in (png_decoder, jpeg_decoder) else None
        stream = torch.cuda.current_stream(device)
        st = C.c_void_p(stream.cuda_stream)
        groups: List[List[int]] = []  # runs of at most GROUP frames of one directory
        for i, fr in enumerate(frames):
            if groups and len(groups[-1]) < GROUP and os.path.dirname(frames[groups[-1][0]].ssim_path) == os.path.dirname(fr.ssim_path):
                groups[-1].append(i)
            else:
                groups.append([i])
        for group in groups:
            paths = [p for i in group for p in (frames[i].first, frames[i].second)]
            handle = None
            if decoder is not None:
                handle = decoder.decode(paths, gray16=files)
                handle.wait(stream)
                imgs = handle.tensors
            else:
                imgs = list(pool.map(read_metric_map_u16 if files else read_image_u8, paths))
            by_size: Dict[Tuple[int, int], List[int]] = {}
            for k, i in enumerate(group):
                a, b = imgs[2 * k], imgs[2 * k + 1]
                if tuple(a.shape) != tuple(b.shape):
                    what = ("map", "map") if files else ("render", "captured image")
                    raise ValueError(f"{frames[i].first} is {a.shape[0]}x{a.shape[1]} and {frames[i].second} is {b.shape[0]}x{b.shape[1]}: the "
                                     f"{what[0]} and the {what[1]} of a frame must have one size")
                sizes[i] = (int(a.shape[0]), int(a.shape[1]))
                by_size.setdefault(sizes[i], []).append(k)
            n_total = len(group)
            d_sums = torch.empty((n_total, 4), dtype=torch.int64, device=device)
            order, held, at = [], [handle], 0
            for (h, w), ks in by_size.items():
                n = len(ks)
                first, second = _block([imgs[2 * k] for k in ks], device), _block([imgs[2 * k + 1] for k in ks], device)
                out = C.c_void_p(d_sums[at:at + n].data_ptr())
                if files:
                    _lib.check(lib.cs_op_metric_map_sums_u16(C.c_void_p(first.data_ptr()), C.c_void_p(second.data_ptr()), n, h, w, w, h * w, out, st))
                else:
                    _lib.check(lib.cs_op_gt_metric_sums_u8(C.c_void_p(first.data_ptr()), C.c_void_p(second.data_ptr()), n, h, w, h * w * 3, out, st))
                held += [first, second]
                order += [group[k] for k in ks]
                at += n
            host = torch.empty((n_total, 4), dtype=torch.int64, pin_memory=True)
            host.copy_(d_sums, non_blocking=True)  # the 32 bytes per frame: one copy per group
            event = torch.cuda.Event()
            event.record(stream)
            held.append(d_sums)
            pending.append((event, host, order, held))
            if handle is not None:
                # the files' status words are known only now, behind the queued launch and copy: for a rejected file the launch summed decode
                # output that was never written (allocated memory, so harmless), and the raise here discards those sums unread
                handle.check()
            drain(4)
        drain(0)
    finally:
        pool.shutdown()
    return sums, sizes


def summarise(dir_in, dir_out, num_workers: int = 16, force: bool = False, fast_debug: int = -1, source: str = "files",
              png_decoder: str = "host", jpeg_decoder: str = "host", jpeg_progressive: str = "host") -> Dict[str, object]:
    """Writes the CSV; returns {"csv": its path or None (SKIP), "frames", "seconds"}."""
    dir_in = str(Path(dir_in).expanduser())
    res: Dict[str, object] = {"frames": 0, "seconds": 0.0}

    def rows():
        t0 = time.perf_counter()
        frames = list_frames(dir_in, source)
        if fast_debug > 0:
            frames = frames[:(fast_debug + 1) * BATCH_ROWS]
        sums, sizes = frame_sums(frames, source, png_decoder, num_workers, jpeg_decoder=jpeg_decoder, jpeg_progressive=jpeg_progressive)
        res["frames"], res["seconds"] = len(frames), time.perf_counter() - t0
        return rows_from_sums(frames, sums, sizes)

    res["csv"] = write_csv(dir_in, dir_out, rows, force, fast_debug)
    return res


def _bool(v: str) -> bool:
    if v not in ("True", "False"):
        raise argparse.ArgumentTypeError("True or False")
    return v == "True"


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Summarise the ground truth results.")
    p.add_argument("--dir_in", type=str, required=True, help="The ground truth data dir that contains scene dirs.")
    p.add_argument("--dir_out", type=str, required=True, help="The output directory to save the summarised results.")
    p.add_argument("--fast_debug", type=int, default=-1, help="num batch of 16 frames to load for debug. Set to -1 to disable")
    p.add_argument("-n", "--num_workers", type=int, default=16)
    p.add_argument("-f", "--force", type=_bool, default=False)
    p.add_argument("--source", choices=SOURCES, default="files", help="files: read metric_map/; compute: form the sums from renders/ and gt/")
    p.add_argument("--png_decoder", choices=("host", "gpu"), default="host")
    p.add_argument("--jpeg_decoder", choices=("host", "gpu"), default="host", help="gpu: baseline JPEG files (captured images) are decoded on the device")
    p.add_argument("--jpeg_progressive", choices=("host", "gpu"), default="host", help="gpu: progressive JPEG files too (needs --jpeg_decoder gpu)")
    return p.parse_args(argv)


def main(argv: Optional[Iterable[str]] = None) -> int:
    a = parse_args(None if argv is None else list(argv))
    from . import configure_runtime
    configure_runtime()
    res = summarise(a.dir_in, a.dir_out, a.num_workers, a.force, a.fast_debug, a.source, a.png_decoder, a.jpeg_decoder, a.jpeg_progressive)
    if res["csv"] is not None:
        rate = res["frames"] / res["seconds"] if res["seconds"] > 0 else 0.0
        print(f"[crossscore_amd.summarise_gt] {res['frames']} frames ({a.source}, png_decoder={a.png_decoder}, jpeg_decoder={a.jpeg_decoder}), {rate:.1f} frames/s -> {res['csv']}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
