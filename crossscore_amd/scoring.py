"""The scoring run predict.py and evaluate.py share: this build's options, device, net and weights, writers, the input-stage decision, the
reference-token cache, the decode window and the batch loop with its batches in flight.

    opts = options(cfg, "predict")          # this_main.* keys, validated before anything is created or the device is touched
    start(cfg, opts)                        # seeds, process group, device
    ... the driver's own directories, InputStage, items and batch lists ...
    run = score(cfg, opts, stage, batches, ...)
    ... the driver's collective over the ranks, which re-raises run.failure behind it ...

A driver adds what differs as plain arguments and two hooks: after_submit (right after a batch's forward is queued) and on_consume (when its
outputs are taken, depth - 1 submits later).
"""
from __future__ import annotations

import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from . import parallel, pooling, synth, vis
from .data import EMPTY, STRATEGIES, InputStage, ReferenceBank, ReferenceTokenCache, decode_items, load_batch, plan_decodes
from .decode import DecodeWindow, ImageDecoder, jpeg_decoder_choice, jpeg_progressive_choice, png_decode_window_choice, png_decoder_choice, read_image_u8
from .model import CrossScoreNet, U8Image, load_lightning_checkpoint
from .pipeline import ForwardPipeline
from .writers import BatchWriter, ScoreSummariser, png_compression_choice, png_encoder_choice

DRIVER = {"predict": "predict", "test": "evaluate"}  # cfg.logger.<phase> -> the module that runs it


def seed_everything(seed: int) -> None:
    """lightning.seed_everything (task/predict.py:23): python, numpy and torch global generators."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def options(cfg, phase: str) -> SimpleNamespace:
    """This build's this_main.* keys of a scoring run; an unknown value raises ValueError here."""
    if not torch.cuda.is_available():
        raise RuntimeError(f"crossscore_amd.{DRIVER[phase]} needs a GPU: the scoring path has no CPU fallback")
    o = SimpleNamespace(phase=phase)
    # this_main.png_encoder (default "host"): who compresses the PNG outputs -- PIL on the writer's threads, or the device
    # (writers.PngEncoder: conversion, de-normalisation and compression queued behind the forward; pixel-exact, not byte-equal)
    o.png_encoder = png_encoder_choice(cfg)
    # this_main.png_compression (default "fast"): the device encoder's form -- fast (Sub filter, fixed-Huffman / stored blocks)
    # or compact (per-row adaptive filter, dynamic-Huffman blocks); ignored with png_encoder=host
    o.png_compression = png_compression_choice(cfg)
    # this_main.png_decoder (default "host"): who decodes the PNG inputs -- PIL on the loader's threads, or the device
    # (decode.ImageDecoder: the compressed bytes go up, a window of this_main.png_decode_window upcoming files is decoded beside earlier forwards;
    # the same pixels, bit for bit; files the device decoder does not take still go through PIL).  In evaluate the window also holds the 16-bit
    # metric maps (gt_metric_maps=files) or the captured images (compute)
    o.png_decoder, o.decode_window = png_decoder_choice(cfg), png_decode_window_choice(cfg)
    # this_main.jpeg_decoder (default "host"): the same choice for baseline JPEG inputs (cs_op_jpeg_decode); either key set to gpu
    # builds the decoder and its window, and each format goes to the device only under its own key
    o.jpeg_decoder = jpeg_decoder_choice(cfg)
    # this_main.jpeg_progressive (default "host"): with jpeg_decoder=gpu, complete progressive files join the device decoder's calls
    # (cs_op_jpeg_decode_ex); gpu without jpeg_decoder=gpu is a ValueError
    o.jpeg_progressive = jpeg_progressive_choice(cfg)
    # this_main.cache_reference_tokens (default on): every reference image goes through the encoder once per run
    # instead of once per query that samples it; the score maps are bit-identical
    o.use_cache = bool(cfg.this_main.get("cache_reference_tokens", True)) and int(cfg.data.neighbour_config.cross) > 0
    o.cache_max_images = int(cfg.this_main.get("reference_cache_max_images", 4096))
    # this_main.batches_in_flight (default 3: with cached reference tokens a batch is 1/3 decoder, measured 2837 /
    # 4152 / 4473 query-images/s with 1 / 2 / 3 in flight): the batch loop keeps that many forwards queued on replicas of the
    # module (pipeline.py), so one batch's decoder runs beside the next batch's encoder; outputs are consumed depth-1 submits later,
    # in batch order, bit-identical to the one-at-a-time loop
    o.depth = max(1, int(cfg.this_main.get("batches_in_flight", 3)))
    # this_main.fused_input_stage (default "auto"): uint8 in, tokens out -- the resize / crop / normalise of the
    # input stage happens inside the patch-embedding launch and no processed fp32 image is written.  The writers' image_query / image_reference
    # outputs (on by default, as in the reference's config) ARE that processed image, so "auto" takes the one-pass form only when neither is
    # written, and only for geometries it holds (cs_u8_input_supported); True insists, False never.  Results are bit-identical either way.
    o.fused = cfg.this_main.get("fused_input_stage", "auto")
    # data.neighbour_config.strategy: random (the reference's sampler) | similar (this build): each query is scored against the
    # neighbour_config.cross candidates whose pooled DINOv2 descriptor is most similar to its own, chosen on the device from the tokens of ALL
    # candidates (data.ReferenceBank).  predict: the files of reference_dir; evaluate: per query the captured images of the other split of its
    # own scene and iteration (the list random draws from), a list shorter than cross padded with "empty_image" as the reference's sampler pads.
    # this_main.similar_exclude_self (default on): a query never takes the candidate that is itself (same real path), e.g. with
    # query_dir == reference_dir.
    o.strategy = str(cfg.data.neighbour_config.strategy)
    o.exclude_self = bool(cfg.this_main.get("similar_exclude_self", True))
    if o.strategy == "similar":
        if bool(cfg.data.dataset.zero_reference):
            raise ValueError("data.neighbour_config.strategy=similar with data.dataset.zero_reference=True: there is nothing to choose between")
        if not bool(cfg.this_main.get("cache_reference_tokens", True)):
            raise ValueError("data.neighbour_config.strategy=similar chooses from the cached reference tokens: this_main.cache_reference_tokens=False is not possible with it")
        if int(cfg.data.neighbour_config.cross) < 1:
            raise ValueError("data.neighbour_config.strategy=similar needs data.neighbour_config.cross >= 1")
    elif o.strategy not in STRATEGIES:
        raise NotImplementedError(f"neighbour strategy {o.strategy} (sampler.py:60-66 knows 'random'; this build adds 'similar')")
    # this_main.reference_use (default off): every batch is scored with need_reference_use and the run writes
    # reference_use.csv -- per query the references it was scored against, the share of its patches' last-layer cross-attention each one took,
    # the mean peak probability inside it, and how focused the attention was.  this_main.reference_use_images (default off) also writes the
    # share maps and the focus map of every query as PNG files under batch/reference_use; it needs reference_use and the batch writer.
    o.reference_use = bool(cfg.this_main.get("reference_use", False))
    o.reference_use_images = bool(cfg.this_main.get("reference_use_images", False))
    if o.reference_use and int(cfg.data.neighbour_config.cross) < 1:
        raise ValueError("this_main.reference_use=True needs data.neighbour_config.cross >= 1: without reference views there is nothing to report")
    if o.reference_use_images and not (o.reference_use and bool(cfg.logger[phase].write.flag.batch)):
        raise ValueError(f"this_main.reference_use_images=True needs this_main.reference_use=True and logger.{phase}.write.flag.batch=True")
    # this_main.score_pool (default off): behind every batch's forward the device pools its score maps -- per image the 16-bit
    # mean, the 1 / 5 / 10 / 25 / 50 % quantiles, the means of the worst 1 / 5 / 10 / 25 / 50 % of the pixels and the worst window of
    # this_main.score_pool_window pixels a side (default 56; 0: no window; only given with score_pool) -- and the run writes
    # score_pool/<dataset>/<method>.csv beside the score summary (pooling.py).  evaluate pools the ground-truth maps the same way (gt_ columns).
    o.score_pool, o.score_pool_window = pooling.pool_options(cfg)
    # this_main.vis_sheet (default off): every logger.<phase>.write.config.vis_img_every_n_steps-th batch writes the preview
    # sheet of its item 0 to vis/r<rank>_B<batch>_b0.png (vis.py), whatever write.flag.batch says, as in the reference.  The sheet is built from
    # the processed images: like image_query it keeps fused_input_stage=auto on the two-launch stage and is refused with fused_input_stage=True.
    o.vis_sheet, o.vis_every = vis.sheet_options(cfg, phase)
    return o


def start(cfg, o: SimpleNamespace) -> None:
    """Seeds, process group and device of the run: o.rank, o.local_rank, o.world, o.device.  The seeding comes before the driver indexes its
    items: with neighbour_config.deterministic=False they draw their references from numpy's global generator as the batch lists are formed."""
    seed_everything(int(cfg.lightning.seed))
    o.rank, o.local_rank, o.world = parallel.init_from_env()
    o.device = torch.device("cuda", o.local_rank if o.world > 1 else 0)
    torch.cuda.set_device(o.device)


def build_net(cfg, device, state_dict, who: str) -> CrossScoreNet:
    """The run's module on `device` with its weights: state_dict, else the checkpoint of trainer.ckpt_path_to_load, else seeded synthetic
    weights and a warning in the name of the driver `who`."""
    net = CrossScoreNet(cfg)
    # trainer.precision (config/default_predict.yaml:25, the reference's own key; Lightning names): "16-mixed" (default) / "16" -> IEEE
    # half MFMA operands, "bf16-mixed" / "bf16" -> bfloat16 operands (fp32's range: for checkpoints whose activations leave the half
    # range).  "32" / "32-true" have no counterpart here (the MFMA operands are 16 bits wide; everything else is fp32 already) and
    # select the more accurate of the two, half.  An explicit model.backbone.operand_dtype wins.
    if "operand_dtype" not in cfg.model.backbone:
        net.operand_dtype = "bf16" if str(cfg.trainer.precision).startswith("bf16") else "fp16"
    if state_dict is None:
        if cfg.trainer.ckpt_path_to_load is not None:
            state_dict = load_lightning_checkpoint(cfg.trainer.ckpt_path_to_load)
        else:  # the reference would start from the hub's DINOv2 weights + a random decoder; there is no hub here
            print(f"[crossscore_amd.{who}] no checkpoint: seeded synthetic weights (scores are meaningless)", file=sys.stderr)
            state_dict = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(net.arch, int(cfg.lightning.seed)).items()}
    net.load_state_dict(state_dict, strict=True)
    return net.to(device)


def nvs_input_stage(cfg, device) -> InputStage:
    """The input stage of the drivers that walk an NvsDataset tree (evaluate, fit_head), from this_main.crop_mode."""
    crop_mode = cfg.this_main.crop_mode
    if crop_mode not in (None, "integer_patches", "dataset_default"):
        raise ValueError(f"crop_mode {crop_mode} not supported (task/test.py:75-91 knows null, integer_patches and dataset_default)")
    return InputStage(device, resize_short_side=int(cfg.this_main.resize_short_side),
                      crop_size=int(cfg.data.transforms.crop_size) if crop_mode == "dataset_default" else None,
                      integer_patches=crop_mode == "integer_patches")


def write_reference_selection(out_dir: str, selection, path_parts: int = 1) -> str:
    """reference_selection.csv of a run with neighbour strategy similar: per query its file name, then the chosen references' file names in the
    order chosen, then their similarities as %.4f.  path_parts: how many trailing parts of a path name a file, joined with "/" -- 1 for predict's
    two directories, 5 for evaluate (<scene>/<split>/<name>_<iter>/<kind>/<file>: base names repeat across scenes).  A padded place (a query
    whose candidate list is shorter than the views it takes) is written as empty_image with an empty similarity."""
    import csv
    import os
    from pathlib import Path

    def name(p):
        return EMPTY if p == EMPTY else "/".join(Path(p).parts[-path_parts:])

    path = os.path.join(str(out_dir), "reference_selection.csv")
    n = len(selection[0][1]) if selection else 0
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["query"] + [f"reference_{k}" for k in range(n)] + [f"similarity_{k}" for k in range(n)])
        for query, refs, sims in selection:
            w.writerow([name(query)] + [name(p) for p in refs] + ["" if p == EMPTY else "%.4f" % v for p, v in zip(refs, sims)])
    return path


USE_KEYS = ("ref_use_share", "ref_use_peak_prob", "ref_use_peak_index", "ref_use_entropy")


def reference_use_row(share, peak_prob, entropy):
    """One query's line of reference_use.csv from its outputs (share, peak_prob (N, h, w), entropy (h, w); host tensors), formed in fp64:
    -> (mean share per reference, mean peak probability per reference, focus = 1 - mean(entropy) / log2(N h w))"""
    N, h, w = (int(v) for v in share.shape)
    shares = share.double().mean(dim=(1, 2)).tolist()
    peaks = peak_prob.double().mean(dim=(1, 2)).tolist()
    bits = float(np.log2(float(N * h * w)))
    focus = 1.0 - float(entropy.double().mean()) / bits if bits > 0 else 1.0  # (one key in all: nothing to spread over)
    return shares, peaks, focus


def write_reference_use(out_dir: str, rows, path_parts: int = 1) -> str:
    """reference_use.csv of a run with this_main.reference_use: per query its file name, the file names of the references it was scored against
    (formed as write_reference_selection forms them: path_parts, empty_image for a padded place), then per reference share_k and peak_k, then
    focus, all as %.4f.  rows: (query path, reference paths, shares, peaks, focus)."""
    import csv
    import os
    from pathlib import Path

    def name(p):
        return EMPTY if p == EMPTY else "/".join(Path(p).parts[-path_parts:])

    path = os.path.join(str(out_dir), "reference_use.csv")
    n = len(rows[0][1]) if rows else 0
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["query"] + [f"reference_{k}" for k in range(n)] + [f"share_{k}" for k in range(n)] + [f"peak_{k}" for k in range(n)] + ["focus"])
        for query, refs, shares, peaks, focus in rows:
            w.writerow([name(query)] + [name(p) for p in refs] + ["%.4f" % v for v in shares] + ["%.4f" % v for v in peaks] + ["%.4f" % focus])
    return path


class Scored(NamedTuple):
    result: Dict[str, object]  # the result keys both drivers report
    files: list                # what the writers and the summariser wrote
    rows: list                 # the summariser's per-image rows
    failure: Optional[BaseException]  # what this rank's output stage raised: the driver re-raises it behind its collective
    nonfinite: int             # non-finite score-map values over the replicas
    operand_dtype: str
    pool_rows: list = []       # this_main.score_pool: per image [scene_name, rendered_dir, image_name, fields ...] as the CSV holds them
    pool_columns: list = []    # ... and the names of the fields


def score(cfg, o: SimpleNamespace, stage, batches, state_dict=None, probe_path: Optional[str] = None, *, calibrate: bool = False,
          extra_files=None, check_size=None, after_submit=None, on_consume=None,
          reference_paths=None, reference_groups=None) -> Scored:
    """Scores `batches` (lists of item dictionaries; cfg.logger.<phase>.out_dir exists) and finishes the outputs.

    probe_path: the first query of this rank, whose geometry decides about the one-pass input stage (None: no image to look at).
    calibrate: at batch 0 of a run of >= 16 batches, make sure the batches in flight (at depth 1 the forward's lanes) really overlap.
    extra_files(item) -> [(path, gray16)]: files the loader reads beside the item's images, into the same `decoded`.
    check_size(size) may refuse a batch's processed size before anything of it is queued.
    reference_paths: the files of reference_dir, in the driver's order: the candidates of neighbour strategy similar.
    reference_groups (instead): candidate lists, of which each item names its own by "reference/cross/group" (nvs.NvsItems.groups).
    after_submit(ticket, items, decoded, size, batch) -> state; on_consume(idx, batch, out, state) runs before the summariser and writer;
    with this_main.score_pool it may leave per image the fields of its own score-pool columns in batch["score_pool/extra"] (evaluate: gt_*),
    with this_main.vis_sheet item 0's ground-truth mean and L1 in batch["vis_sheet/extra"]."""
    phase, device = o.phase, o.device
    log = cfg.logger[phase]
    net = build_net(cfg, device, state_dict, DRIVER[phase])

    writer = (BatchWriter(cfg, phase, net.img_mean_std, device, workers=max(1, int(cfg.data.loader.validation.num_workers) // 2),
                          png_encoder=o.png_encoder, png_compression=o.png_compression)
              if log.write.flag.batch else None)
    sheets = (vis.SheetWriter(cfg, phase, net.img_mean_std, device, png_encoder=o.png_encoder, png_compression=o.png_compression)
              if o.vis_sheet and o.vis_every > 0 else None)
    summariser = ScoreSummariser(cfg.model.predict.metric.type, cfg.model.predict.metric.min, log.out_dir)
    zero_ref = bool(cfg.data.dataset.zero_reference)
    # Host side of the loader: the file lists of all batches are fixed up front, images are decoded by `num_workers` threads, and the next
    # batch is decoded while the GPU scores this one.
    pool = ThreadPoolExecutor(max_workers=max(1, int(cfg.data.loader.validation.num_workers)))
    prefetch = ThreadPoolExecutor(max_workers=1)
    pipe = ForwardPipeline(net, depth=o.depth)
    want_imgs = (writer is not None and bool(log.write.flag.image_query or log.write.flag.image_reference)) or sheets is not None
    fused_in = False
    if o.fused not in (False, "false", "False", 0) and probe_path is not None and not want_imgs:
        probe = read_image_u8(probe_path)
        rs0, crop0 = stage.geometry(*probe.shape[:2])
        fused_in = net.u8_input_supported(U8Image(None, probe.shape[0], probe.shape[1], rs0, crop0[0], crop0[1]), crop0[2:], device)
    if o.fused in (True, "true", "True", 1) and not fused_in:
        raise ValueError("this_main.fused_input_stage=True, but " + (f"the writers need the processed images (logger.{phase}.write.flag.image_query / "
                         "image_reference)" if want_imgs else "this backbone / image geometry is not taken by the one-pass input stage"))
    similar = o.strategy == "similar"
    keep_ref_images = bool(writer is not None and log.write.flag.image_reference) or sheets is not None
    cache = ReferenceTokenCache(pipe, stage, keep_images=keep_ref_images,
                                max_images=o.cache_max_images, from_u8=fused_in) if o.use_cache and not similar else None
    bank = None  # neighbour strategy similar: data.ReferenceBank, built when the first batch tells the processed size
    grouped = similar and reference_groups is not None
    # ... from the candidate lists THIS rank's batches name, in their order: bank_group maps an item's "reference/cross/group" to the bank's
    bank_group = {g: k for k, g in enumerate(sorted({it["reference/cross/group"] for its in batches for it in its}))} if grouped else None
    selection = []  # ... and per query (path, chosen reference paths, their similarities), in consumption order
    use_rows = []   # this_main.reference_use: per query (path, reference paths, shares, peaks, focus), in consumption order
    pool_rows = []  # this_main.score_pool: per query its key columns and fields, in consumption order
    pool_names = pooling.value_names(pooling.PERMILLE, o.score_pool_window)
    pool_columns = [f"pred_{k}" for k in pool_names] + ([f"gt_{k}" for k in pool_names] if phase == "test" else [])
    pool_signed = pooling.signed_range_of(cfg.model.predict.metric.type)  # the range the gray16 writer stores this metric over
    score_pool = None  # pooling.ScorePool, built with the first batch
    decoder = ImageDecoder(device, pool, png=o.png_decoder == "gpu", jpeg=o.jpeg_decoder == "gpu",
                         progressive=o.jpeg_progressive == "gpu") if "gpu" in (o.png_decoder, o.jpeg_decoder) else None
    window = DecodeWindow(decoder, plan_decodes(batches, zero_ref, cache is not None, extra_files), o.decode_window) if decoder is not None else None
    n_cross = int(cfg.data.neighbour_config.cross)

    def decode(i, skip):
        """the decoded files of batch i, on the loader's thread: {path: device tensor} from the decode window, else {path: host array}"""
        return window.fetch(i) if window is not None else decode_items(batches[i], zero_ref, pool, skip, extra_files)

    def submit_decode(i):
        if i >= len(batches):
            return None
        return prefetch.submit(decode, i, {k[0] for k in cache.tokens} if cache is not None else ())  # (skip: the paths cached by now)

    need_w, head_id = bool(cfg.model.need_attn_weights), int(cfg.model.need_attn_weights_head_id)
    use_kw = {"need_reference_use": True} if o.reference_use else {}
    files, n_done = [], 0

    def stage_reference_use(ticket):
        """the four reference-use outputs on their way to pinned memory, queued behind the batch's forward on its stream: read in consume"""
        if not o.reference_use:
            return None
        s = ticket.stream if ticket.stream is not None else torch.cuda.current_stream(device)
        with torch.cuda.stream(s):
            host = {k: torch.empty(ticket.out[k].shape, dtype=ticket.out[k].dtype, pin_memory=True) for k in USE_KEYS}
            for k in USE_KEYS:
                host[k].copy_(ticket.out[k], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(s)
        return host, ev

    def stage_score_pool(ticket):
        """the pooling of the batch's score maps and the copy of its words to pinned memory, queued behind the forward on its stream: read in consume"""
        nonlocal score_pool
        if not o.score_pool:
            return None
        if score_pool is None:
            score_pool = pooling.ScorePool(device, pipe.depth, pooling.PERMILLE, o.score_pool_window)
        return score_pool.queue(ticket.out["score_map_ref_cross"], ticket.stream, pool_signed)

    def check(size):
        if check_size is not None:
            check_size(size)
        if o.score_pool:
            pooling.check_window(o.score_pool_window, size)

    def consume(entry):
        ticket, batch, idx, state, use, pooled = entry
        out = pipe.result(ticket)
        if window is not None:
            window.check(idx)  # the status words of the files this batch read: a rejected file raises here, naming its path
        if similar:
            # the views this batch was scored against, read now that the batch is taken anyway: paths for the item-path JSON, the reference PNGs'
            # and the attention images' names; the processed images from the bank where they are written
            # (a grouped bank: -1, a place the query's candidate list could not fill, is "empty_image" and the bank's placeholder row)
            index = out["reference_index"].cpu()
            sims = out["reference_similarity"].cpu().numpy()
            chosen = [[bank.paths[int(i)] if i >= 0 else EMPTY for i in row] for row in index.tolist()]
            batch["item_paths"]["reference/cross/imgs"] = [[row[n] for row in chosen] for n in range(n_cross)]
            if bank.images is not None:
                rows = index.to(device=device, dtype=torch.int64)
                batch["reference/cross/imgs"] = bank.images[torch.where(rows < 0, bank.bank.blank_row, rows) if grouped else rows]
            selection.extend(zip(batch["item_paths"]["query/img"], chosen, sims.tolist()))
        if use is not None:
            host, ev = use
            ev.synchronize()
            ref_lists = batch["item_paths"]["reference/cross/imgs"]  # N lists of B paths
            for b, query in enumerate(batch["item_paths"]["query/img"]):
                use_rows.append((query, [ref_lists[n][b] for n in range(len(ref_lists))]) +
                                reference_use_row(host["ref_use_share"][b], host["ref_use_peak_prob"][b], host["ref_use_entropy"][b]))
        if on_consume is not None:
            on_consume(idx, batch, out, state)
        summariser.update(batch, out, means=out.get("score_mean_ref_cross"))  # the per-image means the head launch left (score_summariser.py:180-192)
        worst = None  # item 0's worst window (y, x, S), for its sheet
        if pooled is not None:
            values = score_pool.rows(pooled)  # waits for the pool's event: its words are in pinned memory
            extra = batch.get("score_pool/extra")
            for b, (key, v) in enumerate(zip(summariser.rows[-len(values):], values)):  # (the summariser's key columns of the same images)
                pool_rows.append(list(key[:3]) + pooling.format_fields(v, pool_names) + (list(extra[b]) if extra is not None else []))
            if o.score_pool_window:
                worst = (values[0]["window_y"], values[0]["window_x"], o.score_pool_window)
        if sheets is not None and vis.sheet_due(idx, o.vis_every):
            # (the number on the sheet is the score summary's: the mean as its CSV holds it, four digits)
            mean0 = float("%.4f" % summariser.rows[-len(batch["item_paths"]["query/img"])][3])
            files.extend(sheets.write(batch, out, o.local_rank, idx, mean0, worst, batch.get("vis_sheet/extra")))
        if writer is not None:
            files.extend(writer.write_out(batch, out, o.local_rank, idx))
            if o.reference_use_images:
                files.extend(writer.write_reference_use(batch, out, o.local_rank, idx))

    long_run = calibrate and len(batches) >= 16
    pending = submit_decode(0)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    queued = []  # batches submitted and not yet consumed, oldest first: depth of them stay in flight
    for batch_idx, its in enumerate(batches):
        decoded = pending.result()
        if similar:
            batch, size = load_batch(its, stage, decoded, fused_in, references=False)
            check(size)
            if bank is None:
                bank = ReferenceBank(pipe, stage, reference_paths, tuple(size), n_cross, keep_images=keep_ref_images, max_images=o.cache_max_images,
                                     from_u8=fused_in, decoder=decoder, pool=pool, window=o.decode_window,
                                     groups=[reference_groups[g] for g in bank_group] if grouped else None)
                bank_size = tuple(size)
            if tuple(bank.bank.tokens.shape[1:2]) != ((size[0] // net.arch.patch) * (size[1] // net.arch.patch),) or (grouped and tuple(size) != bank_size):
                raise ValueError(f"neighbour strategy similar: this batch's processed size {size[0]}x{size[1]} differs from the reference bank's" +
                                 (f" {bank_size[0]}x{bank_size[1]}: one bank has one patch grid; this_main.crop_mode=dataset_default gives the images of "
                                  "every scene one size" if grouped else ""))
            pending = submit_decode(batch_idx + 1)  # (behind the bank's own decodes: the decoder serves one thread at a time)
            exclude = None
            if o.exclude_self:
                ex = [bank.index_of(it["query/img"], bank_group[it["reference/cross/group"]] if grouped else None) for it in its]
                if any(e >= 0 for e in ex):  # (an array makes every query of the call count as carrying an exclusion: cs_forward_select)
                    exclude = torch.tensor(ex, dtype=torch.int32).to(device)
            group = np.array([bank_group[it["reference/cross/group"]] for it in its], dtype=np.int32) if grouped else None
            ticket = pipe.submit_select(batch["query/img"], bank.bank, exclude, need_w, head_id, True, group=group, **use_kw)
        elif cache is None:
            pending = submit_decode(batch_idx + 1)
            batch, size = load_batch(its, stage, decoded, fused_in, zero_reference=zero_ref)
            check(size)
            refs = batch["reference/cross/imgs"]
            if batch_idx == 0 and long_run:  # make sure the batches in flight really overlap (pipeline.py)
                pipe.calibrate(batch["query/img"], refs)
                if pipe.depth == 1 and not fused_in:  # one batch at a time: then it is the forward's two lanes that have to overlap (model.py)
                    net.calibrate_lanes(batch["query/img"], refs)
            ticket = pipe.submit(batch["query/img"], refs, need_w, head_id, return_mean=True, **use_kw)
        else:
            batch, size = load_batch(its, stage, decoded, fused_in, references=False)
            check(size)
            tokens, batch["reference/cross/imgs"] = cache.gather([it["reference/cross/imgs"] for it in its], decoded, size, zero_ref)
            # (submitted after gather so that the set of cached paths is current; decoding overlaps the forward below)
            pending = submit_decode(batch_idx + 1)
            if batch_idx == 0 and long_run:  # the same check for the (default) cached mode
                pipe.calibrate(batch["query/img"], tokens, cached=True)
            ticket = pipe.submit_cached(batch["query/img"], tokens, need_w, head_id, True, **use_kw)
        pooled = stage_score_pool(ticket)
        state = after_submit(ticket, its, decoded, tuple(size), batch) if after_submit is not None else None
        n_done += len(its)
        queued.append((ticket, batch, batch_idx, state, stage_reference_use(ticket), pooled))
        while len(queued) >= pipe.depth:
            consume(queued.pop(0))
    while queued:
        consume(queued.pop(0))
    torch.cuda.synchronize(device)
    t_loop = time.perf_counter() - t0
    # Finish the outputs and the pools first; the driver then decides together with the other ranks.  A rank whose output stage raises must
    # still take part in the driver's collective, or the other ranks wait in it forever: the exception is kept and the driver
    # re-raises it behind the collective, and the files written so far are worth keeping either way.
    failure: Optional[BaseException] = None
    try:
        if writer is not None:
            writer.finish()
        if sheets is not None:
            sheets.finish()
        files += summariser.summarise()
        if similar:
            files.append(write_reference_selection(log.out_dir, selection, 5 if grouped else 1))
        if o.reference_use:
            files.append(write_reference_use(log.out_dir, use_rows, 5 if phase == "test" else 1))
        if o.score_pool:
            files += pooling.write_pool_csvs(log.out_dir, pool_rows, pool_columns)
    except BaseException as exc:  # noqa: BLE001 -- re-raised by the driver, behind its collective
        failure = exc
    finally:
        prefetch.shutdown()
        pool.shutdown()
    result = {"input_stage": "one-pass (uint8 in, tokens out)" if fused_in else "two-launch (uint8 -> fp32 image -> tokens)",
              "png_encoder": o.png_encoder, "png_compression": o.png_compression,
              "png_files": writer.stats() if writer is not None else {"png_gpu_files": 0, "png_host_files": 0},
              "png_decoder": o.png_decoder, "png_decoded": decoder.stats() if o.png_decoder == "gpu" else {"png_decoded_gpu": 0, "png_decoded_host": 0},
              "jpeg_decoder": o.jpeg_decoder, "jpeg_decoded": decoder.jpeg_stats() if o.jpeg_decoder == "gpu" else {"jpeg_decoded_gpu": 0, "jpeg_decoded_host": 0},
              "jpeg_progressive": o.jpeg_progressive,
              "jpeg_progressive_decoded": decoder.progressive_stats() if o.jpeg_progressive == "gpu" else {"jpeg_progressive_gpu": 0, "jpeg_progressive_host": 0},
              "reference_strategy": o.strategy, "reference_use": o.reference_use, "score_pool": o.score_pool,
              "vis_sheet": o.vis_sheet, "vis_sheets": sheets.sheets if sheets is not None else 0,
              "query_images_per_sec": n_done / t_loop if t_loop > 0 else 0.0}  # the whole scoring loop: input stage, forwards, output stage
    return Scored(result, files, summariser.rows, failure, pipe.nonfinite_count(), net.operand_dtype, pool_rows, pool_columns)
