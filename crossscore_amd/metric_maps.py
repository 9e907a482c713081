"""Writes the ground-truth metric maps of an NvsDataset tree: the files `python -m crossscore_amd.evaluate` (this_main.gt_metric_maps=files)
and the reference's task/test.py read, which the reference ships no program for.

    python -m crossscore_amd.metric_maps data.dataset.path=<tree> [data.dataset.resolution=...] [this_main.data_split=...] [this_main.overwrite=True]

For every scene of the split, for `train` and `test`, and for every iteration directory <name>_<iter>:
    metric_map/ssim/<name>  and  metric_map/mae/<name>   16-bit gray PNGs formed from renders/<name> and gt/<name>
The maps come from cs_op_gt_metric_map_u8 (holds the definition), one launch per kind over a directory's pairs of
one size; the files come from cs_op_png_encode (CS_PNG_GRAY16) through writers.PngEncoder, so a file's bytes crossed PCIe compressed and the
pool threads only write them.  PIL on the pool threads compresses only above the encoder's 4096 x 4096 limit.  Files that exist are left
alone unless this_main.overwrite=True.  Iteration directories are sharded over the ranks (parallel.shard_bounds).  The config is
default_test.yaml's: data.dataset.path (a string or a list), data.dataset.resolution, data.dataset.num_gaussians_iters, this_main.data_split
and data.loader.validation.num_workers are read.
"""
from __future__ import annotations

import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

from . import _lib, parallel
from .config import load_config
from .data import InputStage
from .decode import read_image_u8
from .nvs import DATA_SPLITS
from .writers import PngEncoder, png_compression_choice, save_png, save_png_bytes

KINDS = (("ssim", _lib.GTMAP_SSIM), ("mae", _lib.GTMAP_MAE))
GROUP = 8  # pairs per launch and encode: bounds the pinned and device blocks of a directory of large images


def iteration_dirs(cfg) -> List[Path]:
    """Every <scene>/{train,test}/<name>_<iter> directory of the split's scenes, in the walker's order (nvs.NvsItems)."""
    d = cfg.data.dataset
    split = cfg.this_main.data_split
    if split not in DATA_SPLITS:
        raise ValueError(f"Unknown data_split {split}")
    roots = [d.path] if isinstance(d.path, str) else list(d.path)
    n_iters = int(d.get("num_gaussians_iters", -1))
    out = []
    for root in roots:
        res = d.get("resolution") if d.get("resolution") is not None else os.listdir(root)[0]
        base = Path(root, res)
        with open(base / "split.json") as f:
            scenes = json.load(f)[split]
        for scene in (p for p in (base / n for n in sorted(scenes)) if p.exists()):
            for sub in ("train", "test"):
                iters = sorted(os.listdir(scene / sub), key=lambda x: int(x.split("_")[-1]))
                out += [scene / sub / it for it in (iters[:n_iters] if n_iters > 0 else iters)]
    return out


def pairs_of(it_dir: Path) -> List[Tuple[str, str, str]]:
    """(name, render path, captured-image path) of one iteration directory; the two listings must name the same files."""
    names = sorted(os.listdir(it_dir / "renders"))
    if names != sorted(os.listdir(it_dir / "gt")):
        raise ValueError(f"{it_dir}: renders/ and gt/ do not hold the same file names")
    return [(n, str(it_dir / "renders" / n), str(it_dir / "gt" / n)) for n in names]


def generate(cfg) -> Dict[str, object]:
    """Returns {"written": [paths], "skipped": [paths], "seconds", "png_gpu_files", "png_host_files", "png_compression"} of this rank."""
    if not torch.cuda.is_available():
        raise RuntimeError("crossscore_amd.metric_maps needs a GPU: the maps have no CPU fallback")
    rank, local_rank, world = parallel.init_from_env()
    device = torch.device("cuda", local_rank if world > 1 else 0)
    torch.cuda.set_device(device)
    overwrite = bool(cfg.this_main.get("overwrite", False))
    dirs = iteration_dirs(cfg)
    lo, hi = parallel.shard_bounds(len(dirs), world, rank)
    stage = InputStage(device, resize_short_side=-1)
    png_compression = png_compression_choice(cfg)  # this_main.png_compression: fast (default) | compact
    enc = PngEncoder(png_compression)
    lib = _lib.load()
    workers = max(1, int(cfg.data.loader.validation.num_workers))
    pool = ThreadPoolExecutor(max_workers=workers)
    written: List[str] = []
    skipped: List[str] = []
    jobs = []
    n_gpu = n_host = 0
    t0 = time.perf_counter()
    try:
        for it_dir in dirs[lo:hi]:
            todo = []
            for name, rp, gp in pairs_of(it_dir):
                dst = {k: str(it_dir / "metric_map" / k / name) for k, _ in KINDS}
                want = [k for k, _ in KINDS if overwrite or not os.path.exists(dst[k])]
                skipped += [dst[k] for k, _ in KINDS if k not in want]
                if want:
                    todo.append((rp, gp, dst, want))
            if not todo:
                continue
            for k, _ in KINDS:
                os.makedirs(it_dir / "metric_map" / k, exist_ok=True)
            for g0 in range(0, len(todo), GROUP):
                group = todo[g0:g0 + GROUP]
                imgs = list(pool.map(read_image_u8, [p for rp, gp, _, _ in group for p in (rp, gp)]))
                renders, gts = imgs[0::2], imgs[1::2]
                for (rp, gp, _, _), r, g in zip(group, renders, gts):
                    if r.shape != g.shape:
                        raise ValueError(f"{rp} is {r.shape[0]}x{r.shape[1]} and {gp} is {g.shape[0]}x{g.shape[1]}: a render and the captured "
                                         "image of its view must have one size")
                for kname, kind in KINDS:
                    sel = [i for i, (_, _, _, want) in enumerate(group) if kname in want]
                    if not sel:
                        continue
                    maps = stage.gt_metric_maps([renders[i] for i in sel], [gts[i] for i in sel], kind)
                    by_size: Dict[Tuple[int, int], List[int]] = {}
                    for j, m in enumerate(maps):
                        by_size.setdefault(tuple(m.shape), []).append(j)
                    for (h, w), js in by_size.items():
                        block = torch.stack([maps[j] for j in js])
                        paths = [group[sel[j]][2][kname] for j in js]
                        if lib.cs_png_bound(_lib.PNG_GRAY16, h, w) > 0:
                            handle = enc.encode_async(block)
                            jobs += [pool.submit(save_png_bytes, p, handle, i) for i, p in enumerate(paths)]
                            n_gpu += len(paths)
                        else:  # above the device encoder's size limit: PIL on the pool threads
                            host = block.cpu().numpy().view(np.uint16)
                            jobs += [pool.submit(save_png, p, host[i]) for i, p in enumerate(paths)]
                            n_host += len(paths)
                        written += paths
                while len(jobs) > 8 * workers:  # bound the finished files held in pinned memory
                    jobs.pop(0).result()
        for j in jobs:
            j.result()
    finally:
        pool.shutdown()
    torch.cuda.synchronize(device)
    parallel.barrier()
    return {"written": written, "skipped": skipped, "seconds": time.perf_counter() - t0, "png_gpu_files": n_gpu, "png_host_files": n_host,
            "png_compression": png_compression}


def main(argv: Optional[Iterable[str]] = None) -> int:
    overrides = list(sys.argv[1:] if argv is None else argv)
    from . import configure_runtime
    configure_runtime()
    res = generate(load_config("default_test", overrides))
    for p in res["written"]:
        print(f"[crossscore_amd.metric_maps] wrote {p}")
    rate = len(res["written"]) / res["seconds"] if res["seconds"] > 0 else 0.0
    print(f"[crossscore_amd.metric_maps] {len(res['written'])} files written ({res['png_gpu_files']} compressed on the device, "
          f"{res['png_host_files']} by PIL), {len(res['skipped'])} existing files skipped, {rate:.1f} files/s")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
