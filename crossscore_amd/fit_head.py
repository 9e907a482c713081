"""python -m crossscore_amd.fit_head: fits the regression head on the device, or with this_main.fit_scope=tail the decoder's
tail: the last decoder layer's linear1, linear2 and norm3 together with the head, ten tensors (CrossScoreNet.fit_tail_step),
or with this_main.fit_scope=cross that layer's cross-attention as well: its in_proj, out_proj and norm2, sixteen tensors (DESIGN.md 6, f17;
CrossScoreNet.fit_cross_step), or with this_main.fit_scope=layer the whole last decoder layer: its self-attention and norm1 too, twenty-two tensors
(CrossScoreNet.fit_layer_step; needs model.decoder_do_self_attn=True).  The default scope is head; the gradient of the tail
stops at the last layer's norm2 output, that of the cross scope at the rows and the reference tokens that enter the cross-attention and that of
the layer scope at the rows that enter the layer, so everything below stays frozen in every scope.

Walks the nvs.NvsItems of this_main.data_split (default train) with the host loaders and the GT stage of crossscore_amd.evaluate
(InputStage.metric_maps over the metric-map files, or this_main.gt_metric_maps=compute on a bare tree), geometry as evaluate's, one handle, one
batch at a time: CrossScoreNet.fit_head_step = forward + cs_head_backward + cs_op_adamw + cs_set_head_weights.  The encoder, the decoder and
the positional tables stay as the checkpoint has them (the encoder is frozen in the reference too, task/core.py:494).

Hyperparameters are the reference's keys (config/default.yaml): trainer.optimizer.lr, trainer.lr_scheduler.{step_size, gamma, step_interval}
(StepLR), trainer.max_epochs, max_steps, limit_train_batches, lightning.seed.  Outputs under logger.train.out_dir: fit_head.csv (epoch, step,
lr, loss), checkpoints/last.ckpt (the whole state dict; load_lightning_checkpoint and both drivers read it) and the returned run summary
(with fit_scope).  Not built: random crops and
augmentation, a validation loop, more than one device, and the one-pass (uint8) input stage and the device decoders in this driver: the queries
take the fp32 input path; the references go through evaluate's token cache (this_main.cache_reference_tokens, default True), so each reference
image is encoded once per run and every step after that is a forward_cached."""
from __future__ import annotations

import csv
import functools
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from datetime import datetime
from pathlib import Path
from typing import Dict, Iterable, Optional

import torch

from .config import load_config
from .data import EMPTY, ReferenceTokenCache, decode_items, load_batch, metric_mode
from .evaluate import gt_file, gt_inputs, gt_map_kind, gt_metric_maps_choice, limit_batches
from .model import FIT_SCOPES as SCOPE_TABLE, HeadFitState, arch_from_cfg, check_fit_supported, save_lightning_checkpoint
from .nvs import NvsItems, random_order
from .scoring import build_net, nvs_input_stage, seed_everything


def step_lr(lr0: float, step_size: int, gamma: float, n: int) -> float:
    """torch.optim.lr_scheduler.StepLR: the rate in force after n scheduler steps"""
    return lr0 * gamma ** (n // step_size)


FIT_SCOPES = tuple(SCOPE_TABLE)  # head, tail, cross, layer: the names of model.FIT_SCOPES


def fit_scope(cfg) -> str:
    """this_main.fit_scope: head (default; ref_cross.head.{0,2}), tail (the last decoder layer's feed-forward block and norm3 as well) or cross
    (that layer's cross-attention and norm2 as well) or layer (its self-attention and norm1 as well: the whole last decoder layer)"""
    scope = str(cfg.this_main.get("fit_scope", "head"))
    if scope not in FIT_SCOPES:
        raise ValueError(f"this_main.fit_scope={scope}: " + " | ".join(FIT_SCOPES))
    return scope


def check_config(cfg) -> None:
    fit_scope(cfg)
    devices = cfg.trainer.devices
    if (isinstance(devices, (list, tuple)) and len(devices) != 1) or (isinstance(devices, int) and devices != 1):
        raise ValueError(f"trainer.devices={devices}: the head fit runs on one device (gradients are not reduced across GPUs)")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("the head fit runs as one process (gradients are not reduced across GPUs)")
    if not bool(cfg.model.do_reference_cross):
        raise ValueError("model.do_reference_cross=False: there is no regression head to fit")
    if cfg.model.loss.fn != "l1":
        raise ValueError(f"model.loss.fn={cfg.model.loss.fn}: the head fit is built for l1 (task/core.py:283-285)")
    if str(cfg.trainer.optimizer.type) != "AdamW" or str(cfg.trainer.lr_scheduler.type) != "StepLR":
        raise ValueError("the head fit is built for trainer.optimizer.type=AdamW and trainer.lr_scheduler.type=StepLR")
    if str(cfg.trainer.lr_scheduler.step_interval) not in ("epoch", "step"):
        raise ValueError(f"trainer.lr_scheduler.step_interval={cfg.trainer.lr_scheduler.step_interval}: epoch | step")
    if cfg.this_main.crop_mode not in (None, "integer_patches", "dataset_default"):
        raise ValueError(f"crop_mode {cfg.this_main.crop_mode} not supported (null, integer_patches, dataset_default)")


def fit_head(cfg, state_dict: Optional[Dict[str, torch.Tensor]] = None, now: Optional[str] = None) -> Dict[str, object]:
    """Runs the fit; returns {"out_dir", "csv", "checkpoint", "steps", "epochs", "first_loss", "last_loss", "losses", "gt_metric_maps", "fit_scope"}."""
    check_config(cfg)
    if not torch.cuda.is_available():
        raise RuntimeError("crossscore_amd.fit_head needs a GPU: the head fit has no CPU fallback")
    compute_gt = gt_metric_maps_choice(cfg) == "compute"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    seed_everything(int(cfg.lightning.seed))
    scope = fit_scope(cfg)
    check_fit_supported(arch_from_cfg(cfg), scope)  # (before the weights: they would not fit another patch size either)
    net = build_net(cfg, device, state_dict, "fit_head")
    fit_step = getattr(net, f"fit_{scope}_step")

    out_dir = cfg.logger.train.out_dir
    if out_dir is None:
        ckpt = cfg.trainer.ckpt_path_to_load
        out_dir = os.path.join("log", now or datetime.now().strftime("%Y%m%d_%H%M%S.%f"),
                               "fit_head_" + (Path(ckpt).stem if ckpt is not None else "empty_ckpt"))
    Path(out_dir, "checkpoints").mkdir(parents=True, exist_ok=True)

    stage = nvs_input_stage(cfg, device)
    mode = metric_mode(cfg.model.predict.metric.type, cfg.model.predict.metric.min)
    gt_kind = gt_map_kind(cfg.model.predict.metric.type)
    items = NvsItems.from_config(cfg, compute_gt)
    if not compute_gt:
        # (not items[i]: building an item draws its references from the seeded generator, and the run must draw the same numbers whichever
        #  way its ground truth comes)
        for query, score_map in items.ground_truth_files():
            if score_map == EMPTY:
                raise ValueError(f"{query} has no ground-truth metric map (a placeholder cannot be fitted): write the maps with "
                                 "python -m crossscore_amd.metric_maps, or run with this_main.gt_metric_maps=compute")
    loader = cfg.data.loader.train
    bs, zero_ref = int(loader.batch_size), bool(cfg.data.dataset.zero_reference)
    sched = cfg.trainer.lr_scheduler
    lr0, step_size, gamma, per_step = float(cfg.trainer.optimizer.lr), int(sched.step_size), float(sched.gamma), str(sched.step_interval) == "step"
    max_epochs, max_steps = int(cfg.trainer.max_epochs), int(cfg.trainer.max_steps)
    state = HeadFitState(lr=lr0)
    cache = (ReferenceTokenCache(net, stage, keep_images=False, max_images=int(cfg.this_main.get("reference_cache_max_images", 4096)))
             if bool(cfg.this_main.get("cache_reference_tokens", True)) else None)
    pool = ThreadPoolExecutor(max_workers=max(1, int(loader.num_workers)))
    gt_files = functools.partial(gt_file, compute_gt=compute_gt)
    rows, losses = [], []
    try:
        for epoch in range(max_epochs):
            order = random_order(len(items), int(cfg.lightning.seed) + epoch) if loader.shuffle else list(range(len(items)))
            batches = [[items[i] for i in order[s:s + bs]] for s in range(0, len(order), bs)]
            batches = batches[:limit_batches(len(batches), cfg.trainer.limit_train_batches)]
            for its in batches:
                if 0 <= max_steps <= state.step:
                    break
                decoded = decode_items(its, zero_ref, pool, {k[0] for k in cache.tokens} if cache is not None else (), gt_files)
                maps = gt_inputs(decoded, its, compute_gt)
                batch, size = load_batch(its, stage, decoded, False, references=cache is None, zero_reference=zero_ref)
                if size[0] % net.arch.patch or size[1] % net.arch.patch:
                    raise ValueError(f"a {size[0]}x{size[1]} image is no whole number of {net.arch.patch}-pixel patches; use crop_mode=integer_patches")
                if compute_gt:
                    maps = stage.gt_metric_maps([decoded[it["query/img"]] for it in its], maps, gt_kind)
                gt = torch.empty((len(its), size[0], size[1]), dtype=torch.float32, device=device)
                stage.metric_maps(maps, [decoded[it["query/img"]].shape[:2] for it in its], mode, gt)
                state.lr = step_lr(lr0, step_size, gamma, state.step if per_step else epoch)
                if cache is not None:
                    # the encoder is frozen, so a reference's tokens never change: each image of the split is encoded once per run
                    tokens, _ = cache.gather([it["reference/cross/imgs"] for it in its], decoded, size, zero_ref)
                    losses.append(fit_step(batch["query/img"], None, gt, state, ref_tokens=tokens))
                else:
                    losses.append(fit_step(batch["query/img"], batch["reference/cross/imgs"], gt, state))
                rows.append((epoch, state.step, state.lr))
    finally:
        pool.shutdown()
    host = torch.stack(losses).cpu().tolist() if losses else []  # the one host wait of the run
    if any(v != v for v in host):
        raise FloatingPointError("the loss turned NaN: a ground-truth map holds NaN (MAE / MSE placeholders), or the activations left the half "
                                 "range (trainer.precision=bf16-mixed)")
    csv_path = os.path.join(out_dir, "fit_head.csv")
    with open(csv_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["epoch", "step", "lr", "loss"])
        for (epoch, step, lr), loss in zip(rows, host):
            w.writerow([epoch, step, repr(lr), "%.6f" % loss])
    ckpt_path = os.path.join(out_dir, "checkpoints", "last.ckpt")
    save_lightning_checkpoint(ckpt_path, net)
    return {"out_dir": out_dir, "csv": csv_path, "checkpoint": ckpt_path, "steps": state.step, "epochs": max_epochs, "losses": host,
            "first_loss": host[0] if host else None, "last_loss": host[-1] if host else None, "gt_metric_maps": "compute" if compute_gt else "files",
            "cache_reference_tokens": cache is not None, "fit_scope": scope}


def main(argv: Optional[Iterable[str]] = None) -> int:
    overrides = list(sys.argv[1:] if argv is None else argv)
    from . import configure_runtime
    configure_runtime()
    res = fit_head(load_config("default_fit_head", overrides))
    print(f"[crossscore_amd.fit_head] {res['steps']} steps: loss {res['first_loss']:.6f} -> {res['last_loss']:.6f}; {res['csv']}, {res['checkpoint']}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
