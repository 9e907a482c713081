"""`task/test.py`-compatible driver: score every render of an NvsDataset tree against its ground-truth metric map on the GPU.

    python -m crossscore_amd.evaluate data.dataset.path=<tree> [trainer.ckpt_path_to_load=<ckpt>] [any a.b=c override of config/default_test.yaml]

What the reference does (task/test.py:21-140, task/core.py:201-213, 265-293, 379-417) and where it happens here:
  dataset / sampling                 get_dataset -> NvsDataset -> NeighbourSelector          -> crossscore_amd/nvs.py (NvsItems)
  images                             load_content, resize_all, crops, T.Normalize            -> data.InputStage (predict's input stage)
  GT maps                            load_content, resize_all, crops                         -> InputStage.metric_map (cs_op_metric_map_u16)
  GT maps without metric_map/ files  (the reference ships no program that writes them)        -> this_main.gt_metric_maps=compute:
                                                                                                InputStage.gt_metric_maps (cs_op_gt_metric_map_u8)
  forward                            CrossScoreNet                                           -> ForwardPipeline, reference-token cache, as predict
  L1 loss, Pearson, PSNR per batch   _core_step, on_test_batch_end, correlation, abs2psnr    -> cs_op_score_gt_stats (fp64 sums) + the host
  epoch values                       log_dict(on_step=False) -> Lightning's epoch mean        -> epoch_metrics()
  outputs                            CSVLogger version_<n>/metrics.csv, BatchWriter, score summary
Per batch the GT stage (the maps go up from pinned host memory with non-blocking copies; one launch pair per source size covers the
batch) and the statistics kernel are queued on the stream of the batch's forward, behind its score map; nothing waits for the device until
the batch is consumed (depth - 1 submits later), when its B x 6 sums are copied to the host.

this_main.gt_metric_maps (this build's key): files (default) reads <iter>/metric_map/{ssim,mae}/<name>, as the reference does; compute forms
the same 16-bit map on the device from renders/<name> and gt/<name> of the query's own iteration directory (MSE
uses the MAE kind) and hands it to the chain above: the captured image is decoded beside the render on the same worker pool and goes up from
pinned memory without blocking, the one-pass input stage's render bytes are used where they already are, and metric_map/ is never read.
Every later value is what files mode computes from a PNG of that map (python -m crossscore_amd.metric_maps writes those PNGs).

Epoch values: each of test/loss, test/loss_cross, test/corr_cross, test/psnr_cross is the batch-size-weighted mean of its per-batch values,
sum(bs * v) / sum(bs) -- Lightning's on_epoch mean for log_dict(on_step=False).  With several ranks the pairs (sum(bs * v), sum(bs)) are summed
over the ranks (parallel.sum_over_ranks) and the global weighted mean is reported; with one rank this is exactly Lightning's value
(Lightning 2.1.3's own sync_dist arithmetic, a mean of the ranks' means, was not available to compare with).  A NaN ground truth (the MAE / MSE
placeholder of a render without a metric map) makes its batch's values NaN and, through them, the epoch values: nothing is filtered.
Not reproduced: Lightning's Trainer and sampler (shuffle: True orders the items by torch.randperm seeded from lightning.seed, which does not
reproduce Lightning's draws; per-image outputs do not depend on the order, the epoch correlation does, through the batch grouping), the
interactive batch-size prompt (one line on stderr instead), the vis figure and hparams.yaml.
"""
from __future__ import annotations

import csv
import ctypes as C
import functools
import os
import sys
from datetime import datetime
from pathlib import Path
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, parallel, pooling, scoring
from .config import load_config, this_main_choice
from .data import EMPTY, metric_mode
from .model import U8Batch
from .nvs import NvsItems, random_order

METRIC_KEYS = ("test/loss", "test/loss_cross", "test/corr_cross", "test/psnr_cross")
CSV_COLUMNS = sorted(METRIC_KEYS + ("epoch", "step"))  # CSVLogger sorts its keys
BATCH_COLUMNS = ("batch_idx", "rank", "batch_size", "loss", "corr", "psnr")
GT_METRIC_MAPS = ("files", "compute")


def gt_metric_maps_choice(cfg) -> str:
    """this_main.gt_metric_maps (this build's key): files (default) | compute."""
    return this_main_choice(cfg, "gt_metric_maps", GT_METRIC_MAPS)


def gt_map_kind(metric_type: str) -> int:
    """The cs_op_gt_metric_map_u8 kind behind a metric type, as nvs.metric_load_dir picks the directory: MSE is the MAE map squared."""
    if metric_type == "ssim":
        return _lib.GTMAP_SSIM
    if metric_type in ("mae", "mse"):
        return _lib.GTMAP_MAE
    raise ValueError(f"Invalid metric type {metric_type}")


def next_version(root: Path) -> int:
    """CSVLogger._get_next_version: one past the largest version_<n> under root, 0 when there is none."""
    ns = []
    if root.is_dir():
        for d in os.listdir(root):
            if d.startswith("version_") and (root / d).is_dir():
                try:
                    ns.append(int(d.split("_")[1]))
                except ValueError:
                    pass
    return max(ns) + 1 if ns else 0


def resolve_dirs(cfg, now: Optional[str] = None):
    """task/test.py:48-64: (version dir holding metrics.csv, out_dir).  The log dir is ckpt.parents[1]/test, or log/<now>/test_empty_ckpt
    without a checkpoint; out_dir is f"{version_dir}_{alias}" (a trailing "_" when alias is "") unless logger.test.out_dir is set."""
    if cfg.trainer.ckpt_path_to_load is None:
        now = now or datetime.now().strftime("%Y%m%d_%H%M%S.%f")
        log_dir, name = Path("log") / now, "test_empty_ckpt"
    else:
        log_dir, name = Path(cfg.trainer.ckpt_path_to_load).parents[1], "test"
    root = log_dir / name
    version_dir = root / f"version_{next_version(root)}"
    out_dir = cfg.logger.test.out_dir
    if out_dir is None:
        out_dir = f"{version_dir}_{cfg.alias}"
    return str(version_dir), str(out_dir)


def limit_batches(n: int, limit) -> int:
    """trainer.limit_test_batches as Lightning reads it: an int is a count, a float a fraction of the batches."""
    if isinstance(limit, bool) or not isinstance(limit, (int, float)) or limit < 0:
        raise ValueError(f"limit_test_batches must be a non-negative int or float, got {limit!r}")
    if isinstance(limit, int):
        return min(n, limit)
    if limit > 1.0:
        raise ValueError(f"limit_test_batches {limit} is a float above 1.0")
    k = int(n * limit)
    if k == 0 and limit > 0 and n > 0:
        raise ValueError(f"limit_test_batches={limit} of {n} batches selects none")
    return k


def batch_metrics(stats: np.ndarray, pixels_per_image: int) -> Dict[str, float]:
    """Per-batch values from the (B, 6) fp64 sums of cs_op_score_gt_stats: the L1 loss (the mean over the batch's pixels, task/core.py:282-285),
    the Pearson correlation of the batch's flattened pixels (utils/evaluation/metric.py:26-30: the whole batch, not per image) from the
    pooled sums, and abs2psnr of the loss (core.py:181)."""
    s = np.asarray(stats, dtype=np.float64).reshape(-1, 6).sum(axis=0)
    n = float(stats.shape[0]) * float(pixels_per_image)
    with np.errstate(all="ignore"):
        loss = s[0] / n
        cov = n * s[5] - s[1] * s[2]
        var = (n * s[3] - s[1] * s[1]) * (n * s[4] - s[2] * s[2])
        corr = cov / np.sqrt(var) if var > 0 else float("nan")
        psnr = -10.0 * np.log10(loss * loss)
    return {"loss": float(loss), "corr": float(corr), "psnr": float(psnr)}


def weighted_sums(rows: Sequence[Dict[str, float]]) -> List[float]:
    """(sum bs * loss, sum bs * corr, sum bs * psnr, sum bs) of a rank's batch rows."""
    return [sum(r["batch_size"] * r[k] for r in rows) for k in ("loss", "corr", "psnr")] + [float(sum(r["batch_size"] for r in rows))]


def epoch_metrics(sums: Sequence[float]) -> Dict[str, float]:
    """The epoch values from the (rank-summed) weighted_sums: see the module docstring."""
    loss, corr, psnr, w = sums
    with np.errstate(all="ignore"):
        m = [float(np.float64(v) / np.float64(w)) if w > 0 else float("nan") for v in (loss, corr, psnr)]
    return {"test/loss": m[0], "test/loss_cross": m[0], "test/corr_cross": m[1], "test/psnr_cross": m[2]}


def write_metrics_csv(version_dir: str, metrics: Dict[str, float], epoch: int = 0, step: int = 0) -> str:
    Path(version_dir).mkdir(parents=True, exist_ok=True)
    path = os.path.join(version_dir, "metrics.csv")
    row = dict(metrics, epoch=epoch, step=step)
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(CSV_COLUMNS)
        w.writerow([repr(float(row[k])) if k in METRIC_KEYS else row[k] for k in CSV_COLUMNS])
    return path


def write_batches_csv(out_dir: str, rows: Sequence[Dict[str, float]]) -> str:
    path = os.path.join(out_dir, "test_batches.csv")
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(BATCH_COLUMNS)
        for r in sorted(rows, key=lambda r: (r["rank"], r["batch_idx"])):
            w.writerow([r["batch_idx"], r["rank"], r["batch_size"], repr(r["loss"]), repr(r["corr"]), repr(r["psnr"])])
    return path


def gt_file(item, compute_gt: bool):
    """The [(path, gray16)] of an item's ground truth beside its images (scoring.score's extra_files): the 16-bit metric map (none for
    "empty_image"), in compute mode the captured image ("query/gt")."""
    if compute_gt:
        return [(item["query/gt"], False)]
    return [] if item["query/score_map"] == EMPTY else [(item["query/score_map"], True)]


def gt_inputs(decoded, items, compute_gt: bool) -> list:
    """Per item what gt_file named, out of the batch's decoded files (host arrays, or the decode window's device tensors); None for "empty_image"."""
    files = [gt_file(it, compute_gt) for it in items]
    return [decoded[f[0][0]] if f else None for f in files]


def evaluate(cfg, state_dict: Optional[Dict[str, torch.Tensor]] = None, now: Optional[str] = None,
             capture: Optional[list] = None) -> Dict[str, object]:
    """Runs the test loop; returns {"version_dir", "out_dir", "metrics", "batches", "files", "query_images_per_sec", "input_stage", "png_encoder", "png_compression",
    "png_files", "gt_metric_maps", "png_decoder", "png_decoded", "jpeg_decoder", "jpeg_decoded", "jpeg_progressive", "jpeg_progressive_decoded",
    "score_pool", "vis_sheet", "vis_sheets"} and, with this_main.score_pool, "score_pool_correlation": per pooled value the Pearson coefficient of its pred_ column against
    its gt_ column over this rank's rows whose ground truth is no placeholder.
    capture (tests, tools): a list that receives per batch {"batch_idx", "item_paths", "score", "gt", "stats"} (host copies)."""
    opts = scoring.options(cfg, "test")
    compute_gt = gt_metric_maps_choice(cfg) == "compute"  # this_main.gt_metric_maps: files (default) | compute
    scoring.start(cfg, opts)
    rank, device = opts.rank, opts.device
    bs = int(cfg.data.loader.validation.batch_size)
    crop_mode = cfg.this_main.crop_mode
    if not cfg.this_main.get("force_batch_size", False) and bs > 8 and crop_mode in (None, "integer_patches"):
        # task/test.py:27-45 asks on stdin whether to go on; a batch job cannot answer
        print(f"[crossscore_amd.evaluate] testing full image resolution in a large batch size {bs}", file=sys.stderr)
    version_dir, out_dir = parallel.gather_objects(resolve_dirs(cfg, now))[0]  # rank 0's names on every rank
    cfg.logger.test.out_dir = out_dir
    Path(out_dir).mkdir(parents=True, exist_ok=True)

    stage = scoring.nvs_input_stage(cfg, device)
    mode = metric_mode(cfg.model.predict.metric.type, cfg.model.predict.metric.min)
    if cfg.model.loss.fn != "l1":
        raise NotImplementedError(f"loss fn {cfg.model.loss.fn} (task/core.py:183-187 knows l1)")
    items = NvsItems.from_config(cfg, compute_gt)
    gt_kind = gt_map_kind(cfg.model.predict.metric.type)
    patch = int(cfg.model.patch_size)

    order = random_order(len(items), int(cfg.lightning.seed)) if cfg.data.loader.validation.shuffle else list(range(len(items)))
    lo, hi = parallel.shard_bounds(len(order), opts.world, rank)
    batches = [[items[order[i]] for i in range(start, min(start + bs, hi))] for start in range(lo, hi, bs)]
    batches = batches[:limit_batches(len(batches), cfg.trainer.limit_test_batches)]
    lib = _lib.load()
    rows: List[Dict[str, float]] = []
    gt_pool: list = []  # this_main.score_pool: the pooling.ScorePool of the ground-truth maps, built with the first batch
    pool_names = pooling.value_names(pooling.PERMILLE, opts.score_pool_window)
    pool_signed = pooling.signed_range_of(cfg.model.predict.metric.type)  # cs_op_score_gt_stats' tensor, the range the writer stores it over

    def gt_and_stats(ticket, its, decoded, size, batch):
        """GT stage + statistics kernel on the forward's stream, behind its score map; returns (gt, stats, event, the score pool's ticket)."""
        s = ticket.stream if ticket.stream is not None else torch.cuda.current_stream(device)
        oh, ow = size
        B = len(its)
        maps = gt_inputs(decoded, its, compute_gt)
        if compute_gt:  # `maps` holds the captured images
            for it, g in zip(its, maps):
                r = decoded[it["query/img"]]
                if r.shape != g.shape:
                    raise ValueError(f"{it['query/img']} is {r.shape[0]}x{r.shape[1]} and {it['query/gt']} is {g.shape[0]}x{g.shape[1]}: a render "
                                     "and the captured image of its view must have one size")
        with torch.cuda.stream(s):
            gt = torch.empty((B, oh, ow), dtype=torch.float32, device=device)
            if compute_gt:
                # the render bytes the one-pass input stage already holds on the device, else the decoded host arrays
                on_device = isinstance(batch["query/img"], U8Batch)
                renders = [im.data for im in batch["query/img"].images] if on_device else [decoded[it["query/img"]] for it in its]
                maps = stage.gt_metric_maps(renders, maps, gt_kind)
            stage.metric_maps(maps, [decoded[it["query/img"]].shape[:2] for it in its], mode, gt)
            score = ticket.out["score_map_ref_cross"]
            if tuple(score.shape) != (B, oh, ow):
                raise ValueError(f"score map {tuple(score.shape)} and GT maps {(B, oh, ow)} differ in shape")
            stats = torch.empty((B, 6), dtype=torch.float64, device=device)
            scratch = torch.empty((lib.cs_score_gt_workspace_bytes(B, oh, ow),), dtype=torch.uint8, device=device)
            _lib.check(lib.cs_op_score_gt_stats(C.c_void_p(score.data_ptr()), C.c_void_p(gt.data_ptr()), B, oh, ow, C.c_void_p(stats.data_ptr()),
                                                C.c_void_p(scratch.data_ptr()), C.c_void_p(s.cuda_stream)))
            ev = torch.cuda.Event()
            ev.record(s)
        pooled = None
        if opts.score_pool:  # the ground-truth maps pooled as the score maps are (pooling.py), behind the statistics kernel on the same stream
            if not gt_pool:
                gt_pool.append(pooling.ScorePool(device, opts.depth, pooling.PERMILLE, opts.score_pool_window))
            placeholder = [not compute_gt and it["query/score_map"] == EMPTY for it in its]
            pooled = (gt_pool[0].queue(gt, s, pool_signed), placeholder)
        return gt, stats, ev, pooled

    def check_size(size):
        if crop_mode is None and (size[0] % patch or size[1] % patch):
            raise ValueError(f"crop_mode null: a {size[0]}x{size[1]} image is no whole number of {patch}-pixel patches (the reference "
                             "fails in the L1 loss' broadcast); use crop_mode=integer_patches")

    def batch_stats(idx, batch, out, state):
        gt, stats, ev, pooled = state
        if pooled is not None:  # the gt_ fields of the batch's score-pool rows; a placeholder ground truth reads nan in every one
            values = gt_pool[0].rows(pooled[0])
            batch["score_pool/extra"] = [pooling.format_fields(None if ph else v, pool_names) for v, ph in zip(values, pooled[1])]
        cur = torch.cuda.current_stream(device)
        cur.wait_event(ev)
        gt.record_stream(cur)
        st = stats.cpu().numpy()  # B x 6 doubles: the one host wait of the batch
        m = batch_metrics(st, gt.shape[1] * gt.shape[2])
        rows.append(dict(m, batch_idx=idx, rank=rank, batch_size=int(gt.shape[0])))
        batch["query/score_map"] = gt
        if opts.vis_sheet:  # item 0's ground-truth mean and L1 for its preview sheet, from the sums read above
            n = float(gt.shape[1] * gt.shape[2])
            batch["vis_sheet/extra"] = (float(st[0][2]) / n, float(st[0][0]) / n)
        if capture is not None:
            capture.append({"batch_idx": idx, "item_paths": batch["item_paths"], "score": out["score_map_ref_cross"].cpu().numpy(),
                            "gt": gt.cpu().numpy(), "stats": st})

    run = scoring.score(cfg, opts, stage, batches, state_dict, batches[0][0]["query/img"] if batches else None,
                        calibrate=False,  # inherited: the test loop has never calibrated its batches in flight
                        extra_files=functools.partial(gt_file, compute_gt=compute_gt),
                        check_size=check_size, after_submit=gt_and_stats, on_consume=batch_stats,
                        reference_groups=items.groups if items.candidates else None)  # neighbour strategy similar: each scene's candidate lists
    # one collective that carries the metrics and any failure of a rank's output stage (a rank that raised on its own before it would leave
    # the others waiting in it): the failure is re-raised behind the collective, as in predict.py
    failure, files = run.failure, run.files
    tot = parallel.sum_over_ranks(weighted_sums(rows) + [1.0 if failure is not None else 0.0, float(run.nonfinite)], device)
    all_rows = [r for rr in parallel.gather_objects(rows) for r in rr]
    parallel.barrier()
    if failure is not None:
        raise failure
    if tot[4] > 0:
        raise RuntimeError(f"another rank failed while finishing its outputs (see its traceback); this rank's outputs are under {out_dir}")
    if tot[5] > 0:
        raise FloatingPointError(f"{int(tot[5])} non-finite score-map values with {run.operand_dtype} MFMA operands: run with "
                                 f"trainer.precision=bf16-mixed (model.backbone.operand_dtype=bf16); the outputs written are under {out_dir}")
    metrics = epoch_metrics(tot[:4])
    if rank == 0:
        files.append(write_metrics_csv(version_dir, metrics))
        files.append(write_batches_csv(out_dir, all_rows))
    return {"version_dir": version_dir, "out_dir": out_dir, "metrics": metrics, "batches": sorted(rows, key=lambda r: r["batch_idx"]),
            "files": files, "gt_metric_maps": "compute" if compute_gt else "files", **run.result,
            **({"score_pool_correlation": pooling.pool_correlation(run.pool_rows, run.pool_columns)} if opts.score_pool else {})}


def main(argv: Optional[Iterable[str]] = None) -> int:
    overrides = list(sys.argv[1:] if argv is None else argv)
    from . import configure_runtime
    configure_runtime()
    cfg = load_config("default_test", overrides)
    with torch.no_grad():
        res = evaluate(cfg)
    m = res["metrics"]
    print(f"[crossscore_amd.evaluate] {sum(r['batch_size'] for r in res['batches'])} query images: test/loss {m['test/loss']:.6f} "
          f"test/corr_cross {m['test/corr_cross']:.6f} test/psnr_cross {m['test/psnr_cross']:.4f} (png_decoder {res['png_decoder']}, jpeg_decoder {res['jpeg_decoder']}); metrics under {res['version_dir']}, outputs "
          f"under {res['out_dir']}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
