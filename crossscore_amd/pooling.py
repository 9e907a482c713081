"""Score pooling: per image the order statistics, worst-tail means and the worst S x S window of the 16-bit codes the gray16
writer stores, computed on the device behind each batch's forward (cs_op_score_pool_f32 / cs_op_score_pool_u16; include/crossscore_hip.h states the
definition) and written to <run>/score_pool/<dataset>/<method>.csv, which crossscore_amd.summary reads like a score summary.

The device returns integers only.  The rank and count formulas, the conversion to the units of the written map and the CSV's columns live here once:
    quantile_index(q, n) = (q (n - 1)) // 1000      tail_count(q, n) = max(1, (q n) // 1000)
    code_value(c, signed_range) = c / 65535, or c / 32767 - 1                                   (fp64)
    pooled_values(...)  one image's words -> {"mean16", "q010", ..., "low010", ..., "window", "window_y", "window_x"}
this_main.score_pool (default off) switches it on in predict and evaluate; this_main.score_pool_window (default 56; 0: no window) is S.
"""
from __future__ import annotations

import csv
import ctypes as C
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

PERMILLE = (10, 50, 100, 250, 500)  # the drivers' request: the worst 1 %, 5 %, 10 %, 25 % and the lower median
DEFAULT_WINDOW = 56
MAX_WINDOW = 255
KEY_COLUMNS = ("scene_name", "rendered_dir", "image_name")


def quantile_index(q: int, n: int) -> int:
    """index into the sorted codes of the q-permille quantile of n codes: 0 the minimum, 1000 the maximum, 500 the lower median"""
    return (int(q) * (int(n) - 1)) // 1000


def tail_count(q: int, n: int) -> int:
    """how many of the smallest codes the q-permille tail takes: at least one"""
    return max(1, (int(q) * int(n)) // 1000)


def code_value(c, signed_range: bool) -> float:
    """a 16-bit code (or a mean of codes) in the units of the written map: c / 65535 for the [0, 1] range, c / 32767 - 1 for [-1, 1]; fp64"""
    c = np.float64(c)
    return float(c / np.float64(32767.0) - np.float64(1.0)) if signed_range else float(c / np.float64(65535.0))


def value_names(permille: Sequence[int] = PERMILLE, window: int = DEFAULT_WINDOW) -> List[str]:
    """the CSV's value columns without their prefix, in file order"""
    names = ["mean16"] + [f"q{int(q):03d}" for q in permille] + [f"low{int(q):03d}" for q in permille]
    return names + (["window", "window_y", "window_x"] if window else [])


def pooled_values(total: int, quant: Sequence[int], tail: Sequence[int], window: Optional[Sequence[int]], n: int, permille: Sequence[int],
                  S: int, signed_range: bool) -> Dict[str, object]:
    """One image's integer words -> its values by column name (value_names): fp64 in the written map's units, the window's corner as integers.
    Integer ratios are formed in fp64 from the exact integers (sums stay below 2^53)."""
    v: Dict[str, object] = {"mean16": code_value(np.float64(int(total)) / np.float64(n), signed_range)}
    for q, c in zip(permille, quant):
        v[f"q{int(q):03d}"] = code_value(int(c), signed_range)
    for q, t in zip(permille, tail):
        v[f"low{int(q):03d}"] = code_value(np.float64(int(t)) / np.float64(tail_count(q, n)), signed_range)
    if S and window is not None:
        v["window"] = code_value(np.float64(int(window[0])) / np.float64(S * S), signed_range)
        v["window_y"], v["window_x"] = int(window[1]), int(window[2])
    return v


def format_fields(values: Optional[Dict[str, object]], names: Sequence[str]) -> List[str]:
    """the CSV fields of one image: %.6f, the window's corner as integers; None (a placeholder ground truth) gives nan everywhere"""
    if values is None:
        return ["nan"] * len(names)
    return [str(int(values[k])) if k in ("window_y", "window_x") else "%.6f" % values[k] for k in names]


def pool_options(cfg) -> Tuple[bool, int]:
    """(this_main.score_pool, this_main.score_pool_window), checked: the window is an integer in 0 .. 255 and only given with score_pool"""
    on = cfg.this_main.get("score_pool", False)
    if not isinstance(on, bool):
        raise ValueError(f"this_main.score_pool={on!r} is neither True nor False")
    given = "score_pool_window" in cfg.this_main
    w = cfg.this_main.get("score_pool_window", DEFAULT_WINDOW)
    if isinstance(w, bool) or not isinstance(w, int) or w < 0 or w > MAX_WINDOW:
        raise ValueError(f"this_main.score_pool_window={w!r} is no integer in 0 .. {MAX_WINDOW} (0: no window)")
    if given and not on:
        raise ValueError("this_main.score_pool_window needs this_main.score_pool=True")
    return on, int(w)


def check_window(window: int, size) -> None:
    """the window against a batch's map size, known with the first batch"""
    if window > min(int(size[0]), int(size[1])):
        raise ValueError(f"this_main.score_pool_window={window} is larger than the shorter side of the {int(size[0])}x{int(size[1])} score map")


def signed_range_of(metric_type: str) -> bool:
    """the gray16 writer's decision (writers.get_vrange): SSIM maps are stored over [-1, 1], MAE / MSE maps over [0, 1]"""
    from .writers import get_vrange

    return get_vrange(metric_type, 0, 1)[0] == [-1, 1]


class _Slot:
    def __init__(self):
        self.capacity = (0, 0, 0)
        self.scratch = self.dev = self.host = self.event = None
        self.shape = None   # (B, H, W) of the call in flight
        self.signed = False
        self.busy = False


class ScorePool:
    """Queues the pooling of a batch of maps behind whatever produced them and hands the values out later.

    slots: how many calls may be in flight (the run's batches in flight); each slot owns its scratch, its device outputs (one block: sum, tail,
    window as 64-bit words, quant as 32-bit words behind them) and the pinned host copy of that block.
    queue(map, stream, signed_range) -> ticket: the op and one non-blocking copy on `stream`, then an event; nothing waits.
    rows(ticket) -> per image the values of pooled_values, after waiting for that event."""

    def __init__(self, device: torch.device, slots: int, permille: Sequence[int] = PERMILLE, window: int = DEFAULT_WINDOW):
        self.device = device
        self.permille = tuple(int(q) for q in permille)
        if not 1 <= len(self.permille) <= 16 or any(q < 0 or q > 1000 for q in self.permille):
            raise ValueError(f"ScorePool: 1 .. 16 permille values in 0 .. 1000, not {self.permille}")
        self.window = int(window)
        self._permille = (C.c_int32 * len(self.permille))(*self.permille)
        self._slots = [_Slot() for _ in range(max(1, int(slots)))]
        self._next = 0
        self.calls = 0

    def _words(self, B: int) -> Tuple[int, int, int, int]:
        """offsets (in 64-bit words) of tail, window and quant inside a slot's block of B images, and the block's length"""
        Q = len(self.permille)
        tail, window = B, B + B * Q
        quant = window + 3 * B
        return tail, window, quant, quant + (B * Q + 1) // 2

    def queue(self, maps: torch.Tensor, stream, signed_range: bool) -> int:
        lib = _lib.load()
        if not maps.is_cuda or maps.dim() != 3 or not maps.is_contiguous():
            raise ValueError("ScorePool.queue takes a contiguous (B, H, W) CUDA tensor")
        sixteen = (torch.int16, getattr(torch, "uint16", torch.int16))
        if maps.dtype != torch.float32 and maps.dtype not in sixteen:
            raise ValueError(f"ScorePool.queue takes fp32 score maps or 16-bit codes, not {maps.dtype}")
        B, H, W = (int(v) for v in maps.shape)
        Q = len(self.permille)
        check_window(self.window, (H, W))
        idx = self._next
        slot = self._slots[idx]
        if slot.busy:
            raise RuntimeError("ScorePool: every slot is in flight: read rows() of the oldest ticket first")
        self._next = (idx + 1) % len(self._slots)
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(s):
            if B > slot.capacity[0] or H * W > slot.capacity[1] * slot.capacity[2]:
                nbytes = int(lib.cs_score_pool_workspace_bytes(B, H, W, Q))
                if nbytes == 0:
                    raise NotImplementedError(f"ScorePool: {B} maps of {H} x {W} are more than the op takes (1024 of 4096 x 4096)")
                slot.scratch = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
                words = self._words(B)[3]
                slot.dev = torch.empty((words,), dtype=torch.int64, device=self.device)
                slot.host = torch.empty((words,), dtype=torch.int64, pin_memory=True)
                slot.capacity = (B, H, W)
            tail, window, quant, words = self._words(B)
            base = slot.dev.data_ptr()
            args = (self._permille, Q, self.window, C.c_void_p(base), C.c_void_p(base + 8 * quant), C.c_void_p(base + 8 * tail),
                    C.c_void_p(base + 8 * window) if self.window else None, C.c_void_p(slot.scratch.data_ptr()), C.c_void_p(s.cuda_stream))
            if maps.dtype == torch.float32:
                _lib.check(lib.cs_op_score_pool_f32(C.c_void_p(maps.data_ptr()), B, H, W, 1 if signed_range else 0, *args))
            else:
                _lib.check(lib.cs_op_score_pool_u16(C.c_void_p(maps.data_ptr()), B, H, W, W, H * W, *args))
            slot.host[:words].copy_(slot.dev[:words], non_blocking=True)
            slot.event = torch.cuda.Event()
            slot.event.record(s)
        slot.shape, slot.signed, slot.busy = (B, H, W), bool(signed_range), True
        self.calls += 1
        return idx

    def words(self, ticket: int) -> Dict[str, np.ndarray]:
        """the integer words of a ticket's images: {"sum" (B), "quant" (B, Q), "tail" (B, Q), "window" (B, 3) or None}; frees the slot"""
        slot = self._slots[ticket]
        if not slot.busy:
            raise RuntimeError("ScorePool: this ticket has been read already")
        slot.event.synchronize()
        B, Q = slot.shape[0], len(self.permille)
        tail, window, quant, words = self._words(B)
        h = slot.host[:words].numpy().view(np.uint64).copy()
        slot.busy = False
        return {"sum": h[:B], "tail": h[tail:tail + B * Q].reshape(B, Q),
                "window": h[window:window + 3 * B].reshape(B, 3) if self.window else None,
                "quant": h[quant:].view(np.uint32)[:B * Q].reshape(B, Q)}

    def rows(self, ticket: int) -> List[Dict[str, object]]:
        slot = self._slots[ticket]
        shape, signed = slot.shape, slot.signed
        w = self.words(ticket)
        n = shape[1] * shape[2]
        return [pooled_values(int(w["sum"][b]), w["quant"][b], w["tail"][b], w["window"][b] if self.window else None, n, self.permille,
                              self.window, signed) for b in range(shape[0])]


def write_pool_csvs(dir_out, rows: Sequence[Sequence[str]], columns: Sequence[str]) -> List[str]:
    """<dir_out>/score_pool/<dataset>/<method>.csv, grouped and ordered as the score summary's files are (writers.group_summary_rows).
    rows: per image [scene_name, rendered_dir, image_name, field strings ...] in the order the images were scored."""
    from .writers import group_summary_rows

    root = Path(dir_out).expanduser() / "score_pool"
    written = []
    for dataset, method, group in group_summary_rows(rows):
        out_dir = root / dataset
        out_dir.mkdir(parents=True, exist_ok=True)
        path = out_dir / f"{method}.csv"
        with open(path, "w", newline="") as f:
            w = csv.writer(f, lineterminator="\n")
            w.writerow(list(KEY_COLUMNS) + list(columns))
            for r in group:
                w.writerow(list(r))
        written.append(str(path))
    return written


def pool_correlation(rows: Sequence[Sequence[str]], columns: Sequence[str]) -> Dict[str, float]:
    """Per value column the Pearson coefficient (summary.pearson) of pred_<name> against gt_<name>, from the fields as the CSV holds them, over the
    rows whose ground truth is no placeholder (nan), taken in the order the files hold them."""
    from .summary import pearson
    from .writers import group_summary_rows

    rows = [r for _, _, group in group_summary_rows(rows) for r in group]
    cols = list(columns)
    out: Dict[str, float] = {}
    for name in [c[len("pred_"):] for c in cols if c.startswith("pred_")]:
        if f"gt_{name}" not in cols:
            continue
        ip, ig = 3 + cols.index(f"pred_{name}"), 3 + cols.index(f"gt_{name}")
        pairs = [(float(r[ip]), float(r[ig])) for r in rows if r[ig] != "nan"]
        out[name] = pearson([p for p, _ in pairs], [g for _, g in pairs])
    return out
