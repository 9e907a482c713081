"""The antialiased resize's filter tables against ATen, bit for bit.

F.interpolate(mode="bilinear", antialias=True) applied to an identity matrix along one axis returns the weight matrix ATen uses: every other
term of each dot product is 0 * w, so out[a'][b'] = W[b'][a'] exactly.  The CPU tests hold the oracle (oracle/preprocess_oracle.py, the
yardstick of every preprocessing test) to that matrix over a sweep of axis pairs and to F.interpolate's outputs over a 2-D sweep; the GPU tests
read the host-built tables of csrc/preprocess.hip (build_axis) back through cs_op_preprocess_u8 and cs_op_metric_map_u16 the same way, and
sweep cs_op_preprocess_u8's outputs against the oracle under a derived bound."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import preprocess_oracle as po  # noqa: E402

ULP1 = 2.0 ** -24  # one ulp of 1.0 downwards: the rounding unit of fp32 values in [0.5, 1]

# ------------------------------------------------------------------------------------------------------------------- CPU
AXIS_IN = list(range(1, 70)) + [97, 98, 100, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 540, 720, 777, 1000, 1036, 2100]
AXIS_OUT = list(range(1, 70)) + [70, 84, 98, 112, 255, 256, 257, 518, 686, 690]
# pairs the double-precision bounds / filter arguments got wrong (the smallest of the 927 of this sweep)
WRONG_BEFORE = [(5, 3), (9, 5), (9, 7), (10, 3), (11, 7), (13, 9), (17, 11), (20, 12)]


def aten_axis_matrix(a, b):
    """W[b][a]: the weights ATen applies along an axis of a samples resized to b"""
    return F.interpolate(torch.eye(a)[None, None], (a, b), mode="bilinear", align_corners=False, antialias=True)[0, 0].T.contiguous().numpy()


def dense(table, a):
    xmin, xsize, w = table
    m = np.zeros((len(xmin), a), np.float32)
    for i in range(len(xmin)):
        m[i, xmin[i]:xmin[i] + xsize[i]] = w[i, :xsize[i]]
    return m


def test_oracle_axis_tables_are_atens_bit_for_bit():
    """6 879 axis pairs (a != b): every scale class (up, down, near 1, > 70 x), every size up to 69 on both sides, the workload's sizes.
    The tables formed with double-precision bounds and filter arguments differed at 927 of them (another tap set at 479, worst weight 1.46e-6)."""
    assert all(a in AXIS_IN and b in AXIS_OUT for a, b in WRONG_BEFORE)
    bad, n = [], 0
    for a in AXIS_IN:
        for b in AXIS_OUT:
            if a == b:
                continue
            n += 1
            xmin, xsize, w = po.aa_axis_table(a, b)
            assert (xsize >= 1).all() and (xmin >= 0).all() and (xmin + xsize <= a).all() and (xsize <= w.shape[1]).all(), (a, b)
            if not np.array_equal(dense((xmin, xsize, w), a), aten_axis_matrix(a, b)):
                bad.append((a, b))
    assert n == 6879
    assert not bad, f"{len(bad)} of {n} axis pairs differ from ATen, first {bad[:12]}"


def _geometries_2d():
    """(h, w) -> (oh, ow) with w = round(1.5 h), ow = round(1.5 oh): both axes change, by slightly different scales"""
    hs = list(range(1, 40)) + [63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 511, 1000]
    ohs = list(range(1, 40)) + [49, 56, 63, 64, 65, 70, 98, 255, 256, 257, 518]
    geo = [((h, round(1.5 * h)), (oh, round(1.5 * oh))) for h in hs for oh in ohs if h != oh]
    assert ((511, 766), (257, 386)) in geo  # among the worst geometries of the double-precision tables
    return geo


OUTPUT_TOL = 4 * ULP1  # measured 3 * 2^-24 = 1.79e-7 (below), + one ulp of 1.0 for a torch build that vectorises the sums differently


def test_oracle_resize_matches_interpolate_over_geometries():
    """resize_bilinear_aa against F.interpolate on random fp32 images in [0, 1] over 2 505 2-D geometries.  With ATen's tables the two differ by
    summation order only (the oracle adds tap by tap, ATen's vectorised kernel in another order).  Measured with torch 2.10 on the CPU: worst
    difference 1.79e-7 = 3 * 2^-24 (first reached at 24x36 -> 22x33); the bound is that plus 2^-24 = 2.38e-7 and has to stay below 1e-6.  With the
    double-precision tables the worst was 3.40e-6 (at 257x386 -> 255x382; above 2e-6 at 511x766 -> 257x386 too)."""
    assert OUTPUT_TOL < 1e-6
    rng = np.random.Generator(np.random.PCG64(2024))
    worst, where = 0.0, None
    for (h, w), (oh, ow) in _geometries_2d():
        img = rng.random((1, h, w), dtype=np.float32)
        ref = F.interpolate(torch.from_numpy(img)[None], (oh, ow), mode="bilinear", align_corners=False, antialias=True)[0].numpy()
        got = po.resize_bilinear_aa(img, oh, ow)
        assert got.shape == ref.shape and got.dtype == np.float32
        d = float(np.abs(got - ref).max())
        if d > worst:
            worst, where = d, ((h, w), (oh, ow))
    print(f"oracle vs F.interpolate: worst {worst:.3e} at {where}, bound {OUTPUT_TOL:.3e}")
    assert worst <= OUTPUT_TOL, (worst, where)


# ------------------------------------------------------------------------------------------------------------------- GPU
PROBE_PAIRS = [
    (5, 3), (9, 5), (9, 7), (10, 3), (13, 9), (17, 11), (20, 12),   # wrong with double-precision bounds / filter arguments
    (1, 7), (7, 1), (2, 1), (1, 2),                                 # degenerate
    (20, 28), (45, 98),                                             # up-scale
    (257, 255), (255, 256), (256, 257),                             # scale near 1, around the 256-thread block
    (64, 9), (300, 37),                                             # more than 8 taps
    (777, 518), (720, 690), (2100, 518),                            # workload geometries
    (1000, 14),                                                     # 71 x down-scale, 145 taps
]
METRIC_PROBE_PAIRS = [(5, 3), (9, 7), (1, 7), (7, 1), (45, 98), (257, 255), (64, 9), (777, 518), (1000, 14)]


@functools.lru_cache(maxsize=None)
def _aten_matrix_shared(a, b):
    m = aten_axis_matrix(a, b)
    m.setflags(write=False)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("a,b", PROBE_PAIRS)
def test_preprocess_u8_filter_tables_are_atens_bit_for_bit(a, b):
    """An a x a uint8 image with 255 on the diagonal, mean 0, std 1: 255 / 255 is 1.0, a one-term dot product is exact and the axis that keeps
    its size has the identity table (weights 1 and 0), so rs = (a, b) returns wx as out[c][y][x'] and rs = (b, a) returns wy as out[c][y'][x]."""
    import hip_helpers as hh

    want = _aten_matrix_shared(a, b)  # [b][a]
    buf = np.full((a, a * 3 + 5), 77, np.uint8)  # (the row padding is not read)
    buf[:, :a * 3] = np.repeat(np.eye(a, dtype=np.uint8) * 255, 3, axis=1)
    img = torch.from_numpy(buf).cuda()
    zero, one = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    wx = hh.preprocess_u8(img, a, (a, b), (0, 0), (a, b), zero, one).cpu().numpy()
    wy = hh.preprocess_u8(img, a, (b, a), (0, 0), (b, a), zero, one).cpu().numpy()
    for c in range(3):
        assert np.array_equal(wx[c].T, want), ("wx", c, float(np.abs(wx[c].T - want).max()))
        assert np.array_equal(wy[c], want), ("wy", c, float(np.abs(wy[c] - want).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("a,b", METRIC_PROBE_PAIRS)
def test_metric_map_u16_filter_tables_are_atens_bit_for_bit(a, b):
    """The same probe through the ground-truth map's resize: 65535 / 65535 is 1.0 in CS_METRIC_MAE; two maps per launch with the diagonal
    shifted differently, rows of a + 3 samples."""
    import hip_helpers as hh
    from crossscore_amd import _lib

    want = _aten_matrix_shared(a, b)
    shifts = (1 % a, 3 % a)
    buf = np.full((2, a, a + 3), 12345, np.uint16)
    for k, s in enumerate(shifts):
        buf[k, :, :a] = np.roll(np.eye(a, dtype=np.uint16) * 65535, s, axis=1)  # map k: 1.0 at (y, (y + s) % a)
    maps = torch.from_numpy(buf.view(np.int16)).cuda()[:, :, :a]
    wx = hh.metric_map_u16(maps, 2, a, a, _lib.METRIC_MAE, (a, b), (0, 0), (a, b)).cpu().numpy()  # [k][y][x'] = W[x'][(y + s) % a]
    wy = hh.metric_map_u16(maps, 2, a, a, _lib.METRIC_MAE, (b, a), (0, 0), (b, a)).cpu().numpy()  # [k][y'][x] = W[y'][(x - s) % a]
    for k, s in enumerate(shifts):
        assert np.array_equal(np.roll(wx[k], s, axis=0).T, want), ("wx", k)
        assert np.array_equal(np.roll(wy[k], -s, axis=1), want), ("wy", k)


def _sweep_cases():
    """(h, w, rs_h, rs_w): the probe list's scales, one pair on each axis; small on the axis whose partner is large"""
    small = [(5, 3), (9, 5), (9, 7), (10, 3), (13, 9), (17, 11), (20, 12), (1, 7), (7, 1), (2, 1), (1, 2), (20, 28), (45, 98), (64, 9)]
    wide = [(257, 255), (255, 256), (256, 257), (300, 37), (777, 518), (720, 690), (2100, 518), (1000, 14)]
    cases = []
    for k, (a, b) in enumerate(wide):            # wide pair along x (the windows of 255 / 256 / 257 columns), then along y
        (c, d), (e, f) = small[k], small[k + 5]
        cases.append((c, a, d, b))
        cases.append((a, e, b, f))
    for k, (a, b) in enumerate(small):           # small pairs on both axes
        c, d = small[(k + 3) % len(small)]
        cases.append((a, c, b, d))
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("k,h,w,rs_h,rs_w", [(k,) + c for k, c in enumerate(_sweep_cases())])
def test_preprocess_u8_resize_sweep_within_derived_bound(k, h, w, rs_h, rs_w):
    """cs_op_preprocess_u8 against the oracle on random images, windows at the four corners of the resized image (the clamped first and last
    taps), padded rows, windows of 255 / 256 / 257 columns where the resized image has them.  The bound is derived: a dot product of n values
    in [0, 1] with non-negative weights of sum 1, accumulated in fp32, is off by at most n * 2^-24 whether by fma (kernel) or multiply and add
    (oracle); the width pass's difference goes through the height pass's weights (sum 1) unamplified, so the resized values differ by at most
    2 (nx + ny) * 2^-24, and the subtraction and the division of the normalisation round once more on each side (4 * 2^-24 before the
    division covers both), all divided by the smallest std.  An indexing error is a thousand times that."""
    import hip_helpers as hh

    rng = np.random.Generator(np.random.PCG64(100 + k))
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    pad = (0, 1, 5)[k % 3]
    buf = np.full((h, w * 3 + pad), 255, np.uint8)
    buf[:, :w * 3] = img.reshape(h, w * 3)
    d_img = torch.from_numpy(buf).cuda()
    ref = po.preprocess_u8(img, (rs_h, rs_w))
    nx, ny = int(po.aa_axis_table(w, rs_w)[1].max()), int(po.aa_axis_table(h, rs_h)[1].max())
    bound = (2 * (nx + ny) + 4) * ULP1 / min(po.IMAGENET_STD)
    ow = min(rs_w, (255, 256, 257)[k % 3]) if rs_w >= 255 else max(1, rs_w - 1)
    oh = max(1, (rs_h * 3 + 3) // 4)
    worst = 0.0
    for y0 in sorted({0, rs_h - oh}):
        for x0 in sorted({0, rs_w - ow}):
            got = hh.preprocess_u8(d_img, w, (rs_h, rs_w), (y0, x0), (oh, ow), po.IMAGENET_MEAN, po.IMAGENET_STD).cpu().numpy()
            worst = max(worst, float(np.abs(got - ref[:, y0:y0 + oh, x0:x0 + ow]).max()))
    print(f"sweep {h}x{w} -> {rs_h}x{rs_w} window {oh}x{ow} pad {pad}: worst {worst:.3e} bound {bound:.3e} (nx {nx}, ny {ny})")
    assert worst <= bound, (worst, bound)
