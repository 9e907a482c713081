"""`task/predict.py`-compatible driver for the MI355X path.

    python -m crossscore_amd.predict trainer.ckpt_path_to_load=ckpt/CrossScore-v1.0.0.ckpt \\
        data.dataset.query_dir=<dir> data.dataset.reference_dir=<dir> [any a.b=c override of config/default_predict.yaml]

Same key tree and defaults as the reference's Hydra config (crossscore_amd/config/), same output tree:
  out_dir naming                        task/predict.py:47-65
  dataset / sampling / transforms       task/predict.py:67-108 -> crossscore_amd/data.py (GPU input stage)
  model + checkpoint                    task/predict.py:120-141, task/core.py:173 -> crossscore_amd/model.py (state_dict keys "model.*")
  per-batch writers, end-of-run CSV     task/core.py:214-225,419-441,483-484 -> crossscore_amd/writers.py
What is not reproduced: Lightning's Trainer (one process per GPU is launched with torchrun instead of DDPStrategy; ranks take
contiguous shards of the query list), DataLoader worker processes (so with `neighbour_config.deterministic=False` the random
reference choice follows numpy's global RNG seeded with `lightning.seed` in this process, not Lightning's per-worker seeds), and the
composite matplotlib "vis" figure.
"""
from __future__ import annotations

import sys
from datetime import datetime
from pathlib import Path
from typing import Dict, Iterable, Optional

import torch

from . import parallel, scoring
from .config import load_config
from .data import InputStage, SimpleReferenceItems
from .scoring import seed_everything  # noqa: F401 -- its name here is part of this module's interface


def resolve_out_dir(cfg, now: Optional[str] = None) -> str:
    """task/predict.py:47-65."""
    now = now or datetime.now().strftime("%Y%m%d_%H%M%S.%f")
    if cfg.trainer.ckpt_path_to_load is None:
        log_dir, test_dir_name = Path("log") / now, "predict_empty_ckpt"
    else:
        log_dir, test_dir_name = Path(cfg.trainer.ckpt_path_to_load).parents[1], "predict"
    log_dir = log_dir / test_dir_name
    log_dir.mkdir(parents=True, exist_ok=True)
    out_dir = cfg.logger.predict.out_dir
    if out_dir is None:
        out_dir = f"{log_dir}/{now}"
    if cfg.alias != "":
        out_dir += f"_{cfg.alias}"
    return out_dir


def predict(cfg, state_dict: Optional[Dict[str, torch.Tensor]] = None, now: Optional[str] = None) -> Dict[str, object]:
    """Runs the predict loop; returns {"out_dir", "files", "rows", "input_stage", "png_encoder", "png_compression", "png_files", "png_decoder", "png_decoded",
    "jpeg_decoder", "jpeg_decoded", "jpeg_progressive", "jpeg_progressive_decoded", "reference_strategy", "reference_use", "query_images_per_sec"}."""
    opts = scoring.options(cfg, "predict")
    scoring.start(cfg, opts)
    device = opts.device
    cfg.logger.predict.out_dir = resolve_out_dir(cfg, now)
    Path(cfg.logger.predict.out_dir).mkdir(parents=True, exist_ok=True)

    if cfg.this_main.crop_mode not in (None, "dataset_default"):
        raise ValueError(f"crop_mode {cfg.this_main.crop_mode} not supported (task/predict.py:76-86 knows null and dataset_default)")
    stage = InputStage(device, resize_short_side=int(cfg.this_main.resize_short_side),
                       crop_size=int(cfg.data.transforms.crop_size) if cfg.this_main.crop_mode == "dataset_default" else None)
    items = SimpleReferenceItems(cfg.data.dataset.query_dir, cfg.data.dataset.reference_dir, cfg.data.neighbour_config)
    lo, hi = parallel.shard_bounds(len(items), opts.world, opts.rank)
    bs = int(cfg.data.loader.validation.batch_size)
    # the file lists of all batches are fixed up front (sampling order = item order, like a shuffle=False DataLoader)
    batches = [[items[i] for i in range(start, min(start + bs, hi))] for start in range(lo, hi, bs)]
    # a long run (>= 16 batches) calibrates at its first batch: the batches in flight, or at depth 1 the forward's lanes, must really overlap
    run = scoring.score(cfg, opts, stage, batches, state_dict, items.query_paths[lo] if len(items) > lo else None, calibrate=True,
                        reference_paths=items.reference_paths)
    # A rank whose output stage raised still takes part in the collective below, or the other ranks wait in it forever: the
    # failure travels with the overflow count (one max-reduction: value = count + 1e12 for a failed rank) and is re-raised behind the
    # barrier -- on the failing rank as it was, on the others as a RuntimeError naming the situation.
    failure, bad = run.failure, run.nonfinite
    FAILED = 1.0e12
    worst = parallel.max_over_ranks(float(bad) + (FAILED if failure is not None else 0.0), device)  # every rank learns about ANY rank
    parallel.barrier()
    if failure is not None:
        raise failure
    if worst >= FAILED:
        raise RuntimeError("another rank failed while finishing its outputs (see its traceback); this rank's outputs are under "
                           f"{cfg.logger.predict.out_dir}")
    bad_any = int(worst)
    if bad_any:  # an activation left the range of the 16-bit operand type somewhere upstream (fp16: |x| > 65504)
        raise FloatingPointError(f"{bad} non-finite score-map values on this rank (up to {bad_any} on one rank) with {run.operand_dtype} MFMA operands: "
                                 "run with trainer.precision=bf16-mixed (model.backbone.operand_dtype=bf16); the outputs written are under "
                                 f"{cfg.logger.predict.out_dir}")
    return {"out_dir": cfg.logger.predict.out_dir, "files": run.files, "rows": run.rows, **run.result}


def main(argv: Optional[Iterable[str]] = None) -> int:
    overrides = list(sys.argv[1:] if argv is None else argv)
    from . import configure_runtime
    configure_runtime()  # hardware queues for the batches in flight; before the first HIP call (a no-op afterwards)
    cfg = load_config("default_predict", overrides)
    if cfg.data.dataset.query_dir is None or cfg.data.dataset.reference_dir is None:
        print("usage: python -m crossscore_amd.predict data.dataset.query_dir=<dir> data.dataset.reference_dir=<dir> "
              "[trainer.ckpt_path_to_load=<ckpt>] [a.b=c ...]", file=sys.stderr)
        return 2
    with torch.no_grad():
        res = predict(cfg)
    print(f"[crossscore_amd.predict] {len(res['rows'])} query images, {res['query_images_per_sec']:.1f} query-images/s through the scoring loop "
          f"(png_decoder {res['png_decoder']}, jpeg_decoder {res['jpeg_decoder']}: {res['jpeg_decoded']['jpeg_decoded_gpu']} files on the device), outputs under {res['out_dir']}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
