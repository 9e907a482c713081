"""Plain numpy statement of the score pool (include/crossscore_hip.h, cs_op_score_pool_u16): np.sort, cumulative sums and a brute-force window
minimum over (H, W) uint16 codes.  Its rank and count formulas are written out here, not imported from crossscore_amd.pooling, so the tests compare two
statements of the definition.  Also the gray16 conversion of fp32 scores as numpy does it, and a reader of the CSVs the drivers write."""
import csv

import numpy as np


def gray16(score, signed_range):
    """metric_map_write (utils/io/images.py:49-63) in numpy: fp32 multiply, astype(int32) on finite values in range, clipped.  NaN, +-Inf and values
    whose product leaves int32 are set by rule (NaN -> 0, saturation), as the device's conversion does."""
    m = np.asarray(score, dtype=np.float32)
    with np.errstate(all="ignore"):
        v = (m + np.float32(1.0)) * np.float32(32767.0) if signed_range else m * np.float32(65535.0)
    out = np.zeros(v.shape, dtype=np.int64)
    fin = np.isfinite(v)
    out[fin] = np.clip(np.trunc(v[fin].astype(np.float64)), 0, 65535).astype(np.int64)
    out[np.isposinf(v)] = 65535
    return out.astype(np.uint16)


def window_min(codes, S):
    """(smallest S x S window sum, y, x): every window by a 2-D cumulative sum in Python integers' range (int64), ties to the smallest y, then x"""
    c = np.asarray(codes, dtype=np.int64)
    H, W = c.shape
    P = np.zeros((H + 1, W + 1), dtype=np.int64)
    P[1:, 1:] = c.cumsum(axis=0).cumsum(axis=1)
    sums = P[S:, S:] - P[:-S, S:] - P[S:, :-S] + P[:-S, :-S]  # (H - S + 1, W - S + 1)
    flat = int(np.argmin(sums.reshape(-1)))  # the first smallest in row-major order: smallest y, then smallest x
    y, x = divmod(flat, sums.shape[1])
    return int(sums[y, x]), y, x


def window_min_brute(codes, S):
    """the same by looking at every window in turn (small maps only)"""
    c = np.asarray(codes, dtype=np.int64)
    H, W = c.shape
    best = None
    for y in range(H - S + 1):
        for x in range(W - S + 1):
            s = int(c[y:y + S, x:x + S].sum())
            if best is None or s < best[0]:
                best = (s, y, x)
    return best


def pool(codes, permille, S=0):
    """one (H, W) map of codes -> {"sum", "quant" [Q], "tail" [Q], "window" (sum, y, x) or None}, Python integers"""
    c = np.asarray(codes).astype(np.int64)
    n = c.size
    s = np.sort(c.reshape(-1))
    cum = np.cumsum(s)
    quant = [int(s[(q * (n - 1)) // 1000]) for q in permille]
    tail = [int(cum[max(1, (q * n) // 1000) - 1]) for q in permille]
    return {"sum": int(cum[-1]), "quant": quant, "tail": tail, "window": window_min(c, S) if S else None}


def unit(c, signed_range):
    """a code or a mean of codes in the written map's units, fp64"""
    return float(np.float64(c) / np.float64(32767.0) - np.float64(1.0)) if signed_range else float(np.float64(c) / np.float64(65535.0))


def fields(codes, permille, S, signed_range):
    """the CSV fields of one map, as strings: mean16, the quantiles, the tail means, then the window's mean and corner"""
    p = pool(codes, permille, S)
    n = int(np.asarray(codes).size)
    out = ["%.6f" % unit(np.float64(p["sum"]) / np.float64(n), signed_range)]
    out += ["%.6f" % unit(q, signed_range) for q in p["quant"]]
    out += ["%.6f" % unit(np.float64(t) / np.float64(max(1, (q * n) // 1000)), signed_range) for q, t in zip(permille, p["tail"])]
    if S:
        out += ["%.6f" % unit(np.float64(p["window"][0]) / np.float64(S * S), signed_range), str(p["window"][1]), str(p["window"][2])]
    return out


def read_rows(path):
    """a CSV as (header, rows of strings)"""
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]
