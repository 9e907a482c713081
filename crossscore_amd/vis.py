"""The preview sheet: this build's form of the reference's composite figure <out_dir>/vis/r<rank>_B<batch>_b0.png
(task/core.py:397-409, 422-434, utils/plot/batch_visualiser.py) -- item 0 of a batch: the processed query with the turbo colour bar, beside it a
column of half-size panels (the score map with its mean, the score map laid over the query; in the test phase also the ground-truth map with its
mean and |score - gt| with the item's L1), below them the references as thumbnails, five to a row.  With score pooling the worst window is
outlined on the score-map and overlay panels.  The matplotlib figure itself (fonts, layout engine) is not reproduced: the sheet is an integer image
composed on the device by cs_op_sheet_compose (include/crossscore_hip.h states the definition) from the integer images the writers form.

    sheet_layout(H, W, n_ref, has_gt, has_window) -> (canvas_h, canvas_w, [Panel])    pure host arithmetic; sources and numbers by name
    compose(panels, canvas_h, canvas_w)                                                 bound panels -> the canvas, one launch
    SheetWriter                                                                         the drivers' writer, called in scoring.score's consume
this_main.vis_sheet (default off) switches it on; logger.<phase>.write.config.vis_img_every_n_steps = n > 0 writes batches with idx % n == 0.
"""
from __future__ import annotations

import ctypes as C
import math
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, replace
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib

FILL, IMAGE, BLEND, RAMP, FRAME, TEXT = (_lib.SHEET_FILL, _lib.SHEET_IMAGE, _lib.SHEET_BLEND, _lib.SHEET_RAMP, _lib.SHEET_FRAME, _lib.SHEET_TEXT)
CHARS = "0123456789.- "

# the layout's constants
MARGIN = 8                  # around the sheet
GAP = 8                     # between panels
BAR_WIDTH = 12              # the colour bar beside the query
TEXT_SCALE = 1              # the 5 x 7 font at its own size
TEXT_CHARS = 6              # a number's field: "%.3f" right-aligned, "-0.123"
TEXT_GAP = 3                # between a panel and the number under it
REFS_PER_ROW = 5            # make_grid(nrow=5)
BACKGROUND = (48, 48, 48)
TEXT_COLOUR = (255, 255, 255)
WINDOW_COLOUR = (255, 0, 255)  # magenta, the reference's rectangle colour
FRAME_THICKNESS = 1
TEXT_H, TEXT_W = 7 * TEXT_SCALE, (6 * TEXT_CHARS - 1) * TEXT_SCALE


@dataclass(frozen=True)
class Panel:
    """One panel.  role names it ("background", "query", "colour_bar", "score", "score_mean", "overlay", "gt", "gt_mean", "diff", "l1",
    "window_score", "window_overlay", "ref<k>").  In a layout src / src2 name the image a panel reads ("query", "query_on_map": the part of the
    query the score map covers, its top-left whole patches; "score", "gt", "diff", "turbo", "ref<k>"), text names the number (the role) and a
    window frame holds the rectangle of the panel it lies in; bind() replaces them."""
    kind: int
    role: str
    y: int
    x: int
    h: int
    w: int
    src: object = None
    src2: object = None
    rgb: Tuple[int, int, int] = (0, 0, 0)
    param: int = 0
    text: str = ""


def sheet_layout(H: int, W: int, n_ref: int, has_gt: bool, has_window: bool) -> Tuple[int, int, List[Panel]]:
    """The sheet of an H x W processed query with n_ref references (the maps may be smaller, the whole patches of it: they are resampled into
    their panels whatever their size): (canvas_h, canvas_w, panels in painting order).  ValueError for a canvas above 4096 a side or more than
    48 panels."""
    H, W, n_ref = int(H), int(W), int(n_ref)
    if H < 1 or W < 1 or n_ref < 0:
        raise ValueError(f"sheet_layout: a {H}x{W} query with {n_ref} references")
    hh, hw = max(1, H // 2), max(1, W // 2)  # the half-size panels and thumbnails
    col_w = max(hw, TEXT_W)
    col_x = MARGIN + W + GAP + BAR_WIDTH + GAP
    panels = [None,  # (the background, once the canvas is known)
              Panel(IMAGE, "query", MARGIN, MARGIN, H, W, src="query"),
              Panel(RAMP, "colour_bar", MARGIN, MARGIN + W + GAP, H, BAR_WIDTH, src="turbo")]
    frames = []
    y = MARGIN

    def numbered(kind, role, number, **kw):
        nonlocal y
        panels.append(Panel(kind, role, y, col_x, hh, hw, **kw))
        if has_window and role in ("score", "overlay"):
            frames.append(Panel(FRAME, f"window_{role}", y, col_x, hh, hw, rgb=WINDOW_COLOUR, param=FRAME_THICKNESS))
        y += hh
        if number is not None:
            panels.append(Panel(TEXT, number, y + TEXT_GAP, col_x, TEXT_H, TEXT_W, rgb=TEXT_COLOUR, param=TEXT_SCALE, text=number))
            y += TEXT_GAP + TEXT_H
        y += GAP

    numbered(IMAGE, "score", "score_mean", src="score")
    numbered(BLEND, "overlay", None, src="query_on_map", src2="score")
    if has_gt:
        numbered(IMAGE, "gt", "gt_mean", src="gt")
        numbered(IMAGE, "diff", "l1", src="diff")
    top_h = max(H, y - GAP - MARGIN)
    y = MARGIN + top_h + GAP
    for k in range(n_ref):
        r, c = divmod(k, REFS_PER_ROW)
        panels.append(Panel(IMAGE, f"ref{k}", y + r * (hh + GAP), MARGIN + c * (hw + GAP), hh, hw, src=f"ref{k}"))
    rows = (n_ref + REFS_PER_ROW - 1) // REFS_PER_ROW
    canvas_h = MARGIN + top_h + (rows * (GAP + hh) if rows else 0) + MARGIN
    canvas_w = max(col_x + col_w, MARGIN + min(n_ref, REFS_PER_ROW) * (hw + GAP) - GAP) + MARGIN
    panels += frames  # (painted last: over the panels they lie in)
    panels[0] = Panel(FILL, "background", 0, 0, canvas_h, canvas_w, rgb=BACKGROUND)
    if canvas_h > _lib.SHEET_MAX_SIDE or canvas_w > _lib.SHEET_MAX_SIDE:
        raise ValueError(f"sheet_layout: the sheet of a {H}x{W} query with {n_ref} references is {canvas_h}x{canvas_w}, above {_lib.SHEET_MAX_SIDE} a side")
    if len(panels) > _lib.SHEET_MAX_PANELS:
        raise ValueError(f"sheet_layout: {n_ref} references make {len(panels)} panels, more than {_lib.SHEET_MAX_PANELS}")
    return canvas_h, canvas_w, panels


def number_text(v: Optional[float]) -> str:
    """a number's field: "%.3f" right-aligned in TEXT_CHARS characters (cut to them); "-" for None or a non-finite value"""
    s = "-" if v is None or not math.isfinite(v) else ("%.3f" % v)[:TEXT_CHARS]
    return s.rjust(TEXT_CHARS)


def window_rect(panel: Panel, H: int, W: int, wy: int, wx: int, S: int) -> Tuple[int, int, int, int]:
    """the S x S window at (wy, wx) of the H x W map inside the panel that shows the map: corner and side scaled by floor, at least one pixel,
    kept inside the panel -> (y, x, h, w)"""
    fy, fx = (wy * panel.h) // H, (wx * panel.w) // W
    fh, fw = max(1, (S * panel.h) // H), max(1, (S * panel.w) // W)
    return panel.y + fy, panel.x + fx, min(fh, panel.h - fy), min(fw, panel.w - fx)


def bind(panels: Sequence[Panel], images: Dict[str, object], numbers: Dict[str, Optional[float]], size: Tuple[int, int],
         window: Optional[Tuple[int, int, int]] = None) -> List[Panel]:
    """A layout's panels with their names resolved: images by name, numbers through number_text, the window frames placed (window: y, x, S in the
    size = (H, W) map; without one the frames are left out)."""
    out = []
    for p in panels:
        if p.kind == FRAME and p.role.startswith("window_"):
            if window is None:
                continue
            y, x, h, w = window_rect(p, size[0], size[1], *window)
            out.append(replace(p, y=y, x=x, h=h, w=w))
        elif p.kind == TEXT:
            out.append(replace(p, text=number_text(numbers.get(p.text))))
        elif p.kind in (IMAGE, BLEND, RAMP):
            out.append(replace(p, src=images[p.src], src2=images[p.src2] if p.src2 is not None else None))
        else:
            out.append(p)
    return out


def _source(t: torch.Tensor, what: str):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3 and t.stride(2) == 1
            and t.stride(1) == 3):
        raise ValueError(f"compose: {what} must be an (h, w, 3) uint8 CUDA tensor with dense pixels")
    return C.c_void_p(t.data_ptr()), int(t.shape[0]), int(t.shape[1]), int(t.stride(0)) if t.shape[0] > 1 else 3 * int(t.shape[1])


def panel_struct(p: Panel) -> _lib.CsSheetPanel:
    """a bound panel as cs_op_sheet_compose takes it"""
    s = _lib.CsSheetPanel(kind=int(p.kind), dst_y=int(p.y), dst_x=int(p.x), dst_h=int(p.h), dst_w=int(p.w), param=int(p.param))
    s.rgb[0], s.rgb[1], s.rgb[2] = (int(v) for v in p.rgb)
    if p.kind in (IMAGE, BLEND):
        s.src, s.src_h, s.src_w, s.src_row_bytes = _source(p.src, f"the source of {p.role}")
    if p.kind == BLEND:
        s.src2, s.src2_h, s.src2_w, s.src2_row_bytes = _source(p.src2, f"the second source of {p.role}")
    if p.kind == RAMP:
        if not (isinstance(p.src, torch.Tensor) and p.src.is_cuda and p.src.dtype == torch.uint8 and p.src.numel() == 768 and p.src.is_contiguous()):
            raise ValueError("compose: a ramp reads a contiguous 256 x 3 uint8 CUDA table")
        s.src = C.c_void_p(p.src.data_ptr())
    if p.kind == TEXT:
        s.text = p.text.encode("ascii")
    return s


def compose(panels: Sequence[Panel], canvas_h: int, canvas_w: int, out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """cs_op_sheet_compose on the current stream: bound panels -> the (canvas_h, canvas_w, 3) uint8 canvas (out, or a new tensor); nothing waits"""
    if out is None:
        out = torch.empty((int(canvas_h), int(canvas_w), 3), dtype=torch.uint8, device=device if device is not None else "cuda")
    if not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (int(canvas_h), int(canvas_w), 3) and out.is_contiguous()):
        raise ValueError("compose: the canvas must be a contiguous (canvas_h, canvas_w, 3) uint8 CUDA tensor")
    arr = (_lib.CsSheetPanel * max(1, len(panels)))(*[panel_struct(p) for p in panels])
    _lib.check(_lib.load().cs_op_sheet_compose(arr, len(panels), C.c_void_p(out.data_ptr()), int(canvas_h), int(canvas_w),
                                               C.c_void_p(torch.cuda.current_stream(out.device).cuda_stream)))
    return out


def sheet_options(cfg, phase: str) -> Tuple[bool, int]:
    """(this_main.vis_sheet, logger.<phase>.write.config.vis_img_every_n_steps), checked.  The sheet is built from the processed images, so with
    the key on this_main.fused_input_stage=True (which writes none) is refused."""
    on = cfg.this_main.get("vis_sheet", False)
    if not isinstance(on, bool):
        raise ValueError(f"this_main.vis_sheet={on!r} is neither True nor False")
    if not on:
        return False, 0  # (the cadence key is carried from the reference's configs and not looked at without the sheet)
    every = cfg.logger[phase].write.config.get("vis_img_every_n_steps", 1)
    if isinstance(every, bool) or not isinstance(every, int) or every < 0:
        raise ValueError(f"logger.{phase}.write.config.vis_img_every_n_steps={every!r} is no integer >= 0 (0: no sheets)")
    if cfg.this_main.get("fused_input_stage", "auto") in (True, "true", "True", 1):
        raise ValueError("this_main.fused_input_stage=True, but the preview sheet needs the processed images (this_main.vis_sheet)")
    return on, int(every)


def sheet_due(batch_idx: int, every: int) -> bool:
    """whether batch batch_idx gets a sheet: every n-th from batch 0 on, none with n = 0"""
    return every > 0 and batch_idx % every == 0


def _save_host(path, event, host: torch.Tensor) -> None:
    from .writers import save_png

    event.synchronize()
    save_png(path, host.numpy())


class SheetWriter:
    """write() builds item 0's integer images with the writers' ops, composes one sheet and queues its file; nothing waits on the device.  With
    png_encoder "gpu" the canvas goes through PngEncoder.encode_async, with "host" through a pinned copy and PIL, on this writer's thread either way;
    both give equal pixels.  finish() joins the files."""

    def __init__(self, cfg, phase: str, img_mean_std: torch.Tensor, device: torch.device, png_encoder: str = "host", png_compression: str = "fast"):
        from .writers import PngEncoder, ScoreMapEncoder, colormap_table

        self.phase = phase
        self.device = device
        self.dir = Path(cfg.logger[phase].out_dir) / "vis"
        self.dir.mkdir(parents=True, exist_ok=True)
        self.img_mean_std = img_mean_std.detach().float().cpu()
        m = cfg.model.predict.metric
        self._colour = ScoreMapEncoder(m.type, m.min, m.max, "rgb", device)  # the rgb writer's colours over [metric.min, metric.max]
        self._turbo = torch.from_numpy(colormap_table("turbo").reshape(-1)).to(device)
        self._png = PngEncoder(png_compression) if png_encoder == "gpu" else None
        self._pool = ThreadPoolExecutor(max_workers=1)
        self._pending = []
        self._layouts = {}
        self.sheets = 0

    def write(self, batch, out, local_rank: int, batch_idx: int, mean: Optional[float], window: Optional[Tuple[int, int, int]] = None,
              gt_numbers: Optional[Tuple[float, float]] = None) -> List[str]:
        """mean: item 0's score mean as the score summary holds it; window: (y, x, S) of item 0's worst window; gt_numbers (test phase): item 0's
        ground-truth mean and L1."""
        from .writers import denorm_to_rgb8, save_png_bytes, unit_to_rgb8

        score = out["score_map_ref_cross"][:1]
        query = denorm_to_rgb8(batch["query/img"][:1], self.img_mean_std)[0]
        H, W = int(query.shape[0]), int(query.shape[1])
        map_h, map_w = int(score.shape[1]), int(score.shape[2])  # the whole patches of the query: its top-left map_h x map_w pixels
        refs = batch.get("reference/cross/imgs")
        n_ref = int(refs.shape[1]) if isinstance(refs, torch.Tensor) and refs.dim() == 5 else 0
        has_gt = self.phase == "test"
        key = (H, W, n_ref, has_gt, window is not None)
        if key not in self._layouts:
            self._layouts[key] = sheet_layout(*key)
        canvas_h, canvas_w, panels = self._layouts[key]
        images = {"turbo": self._turbo, "query": query, "query_on_map": query[:map_h, :map_w], "score": self._colour.device_image(score)[0]}
        if n_ref:
            thumbs = denorm_to_rgb8(refs[0], self.img_mean_std)
            images.update({f"ref{k}": thumbs[k] for k in range(n_ref)})
        numbers = {"score_mean": mean}
        if has_gt:
            gt = batch["query/score_map"][:1]
            images["gt"] = self._colour.device_image(gt)[0]
            images["diff"] = unit_to_rgb8(torch.abs(score - gt), self._turbo)[0]
            numbers["gt_mean"], numbers["l1"] = gt_numbers if gt_numbers is not None else (None, None)
        canvas = compose(bind(panels, images, numbers, (map_h, map_w), window), canvas_h, canvas_w, device=score.device)
        path = self.dir / f"r{local_rank}_B{batch_idx:04}_b0.png"
        if self._png is not None:
            self._pending.append(self._pool.submit(save_png_bytes, path, self._png.encode_async(canvas[None]), 0))
        else:
            host = torch.empty(tuple(canvas.shape), dtype=torch.uint8, pin_memory=True)
            host.copy_(canvas, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(score.device))
            self._pending.append(self._pool.submit(_save_host, path, ev, host))
        self.sheets += 1
        return [str(path)]

    def finish(self) -> None:
        """Waits for every queued file (re-raises the first failure)."""
        pending, self._pending = self._pending, []
        for f in pending:
            f.result()
