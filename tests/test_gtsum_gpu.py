"""The frame-sum kernels of the ground-truth score summary (cs_op_metric_map_sums_u16, cs_op_gt_metric_sums_u8).

The ops return four unsigned 64-bit integer sums per frame, so every comparison here is integer equality, without a tolerance: the u16 op
against numpy int64 (Python integers where a sum passes 2^53), the fused u8 op against the u16 op on the two maps cs_op_gt_metric_map_u8
writes for the same pairs.  Padding, the samples ahead of a row and the guard bands (tests/guard.py) hold 0xFFFF / 255, so any read outside
[row, row + W) changes a sum."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from guard import guarded, poisoned_in  # noqa: E402

torch = pytest.importorskip("torch")
SHAPES = [(1, 1), (1, 7), (3, 5), (2, 8), (5, 9), (60, 84), (33, 257)]


def _p(t):
    return C.c_void_p(t.data_ptr())


def _lib_():
    from crossscore_amd import _lib

    return _lib, _lib.load()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def np_sums(ssim, mae):
    """(B, 4) Python integers from (B, H, W) uint16 maps"""
    out = []
    for cs, cm in zip(ssim.astype(np.int64), mae.astype(np.int64)):
        out.append([int(cs.sum()), int(np.clip(cs, 32767, 65534).sum()), int(cm.sum()), sum(int(v) for v in (cm * cm).sum(axis=1))])
    return out


def placed(maps, pad=0, off=0):
    """maps (B, H, W) uint16 inside poison: `off` samples of 0xFFFF ahead of every row (so the rows start `off` samples past where the view does,
    which is 16-byte aligned), `pad` behind, guard bands around -> (keep-alive, address of the first sample, row_elems, image stride)"""
    B, H, W = maps.shape
    wide = np.full((B, H, W + off), 0xFFFF, dtype=np.uint16)
    wide[:, :, off:] = maps
    v = poisoned_in(torch.from_numpy(wide.view(np.int16)).cuda(), ld=W + off + pad)
    return v, v.data_ptr() + 2 * off, W + off + pad, H * (W + off + pad)


def sums_u16(ssim, mae, pad=0, off_s=0, off_m=0, out=None):
    """the op on host maps; ssim and mae share row_elems and the stride, so their offsets must leave both the same row length"""
    _lib, lib = _lib_()
    B, H, W = ssim.shape
    ks, ps, ld, stride = placed(ssim, pad + (off_m - off_s if off_m > off_s else 0), off_s)
    km, pm, ld_m, _ = placed(mae, pad + (off_s - off_m if off_s > off_m else 0), off_m)
    assert ld == ld_m
    g = out if out is not None else guarded((B, 4), torch.int64, guard_rows=4)
    _lib.check(lib.cs_op_metric_map_sums_u16(C.c_void_p(ps), C.c_void_p(pm), B, H, W, ld, stride, _p(g.view), _st()))
    torch.cuda.synchronize()
    g.check("sums")
    return [[int(v) for v in row] for row in g.view.cpu().numpy().view(np.uint64)]


def random_maps(rng, B, H, W):
    m = rng.integers(0, 65536, (B, H, W), dtype=np.uint16)
    m.reshape(B, -1)[:, :4] = np.array([0, 65535, 32767, 65534], dtype=np.uint16)[:min(4, H * W)]
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", SHAPES)
def test_sums_u16_equal_numpy_at_every_layout(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    for B in (1, 3):
        ssim, mae = random_maps(rng, B, h, w), random_maps(rng, B, h, w)
        want = np_sums(ssim, mae)
        for pad in (0, 3):
            for off_s, off_m in ((0, 0), (1, 1), (3, 1), (0, 5), (7, 7)):
                assert sums_u16(ssim, mae, pad, off_s, off_m) == want, (B, pad, off_s, off_m)


@pytest.mark.gpu
def test_sums_accumulate_in_64_bits():
    _lib, lib = _lib_()
    h, w = 1200, 1800
    rng = np.random.default_rng(1)
    full = np.full((1, h, w), 65535, dtype=np.uint16)
    rnd = rng.integers(0, 65536, (1, h, w), dtype=np.uint16)
    dent = full.copy()
    dent[0, 700, 901] = 65534  # makes S4 odd: above 2^53 no double holds it
    for ssim, mae in ((full, full), (rnd, full), (full, rnd), (rnd, dent)):
        a, b = torch.from_numpy(ssim.view(np.int16)).cuda(), torch.from_numpy(mae.view(np.int16)).cuda()
        g = guarded((1, 4), torch.int64, guard_rows=4)
        _lib.check(lib.cs_op_metric_map_sums_u16(_p(a), _p(b), 1, h, w, w, h * w, _p(g.view), _st()))
        torch.cuda.synchronize()
        g.check("sums")
        got = [int(v) for v in g.view.cpu().numpy().view(np.uint64)[0]]
        assert got == np_sums(ssim, mae)[0]
    n = h * w
    want = [65535 * n, 65534 * n, 65535 * n, 65535 * 65535 * n]
    assert np_sums(full, full)[0] == want and want[3] > 2 ** 53
    odd = np_sums(rnd, dent)[0][3]
    assert odd == want[3] - 65535 ** 2 + 65534 ** 2 and odd % 2 == 1 and float(odd) != odd


@pytest.mark.gpu
def test_a_frame_has_the_same_sums_alone_and_in_a_batch():
    rng = np.random.default_rng(2)
    ssim, mae = random_maps(rng, 3, 60, 84), random_maps(rng, 3, 60, 84)
    batch = sums_u16(ssim, mae, pad=3, off_s=1, off_m=1)
    assert len({tuple(r) for r in batch}) == 3
    for i in range(3):
        assert sums_u16(ssim[i:i + 1], mae[i:i + 1]) == [batch[i]], i


@pytest.mark.gpu
def test_inputs_stay_intact_and_the_op_zeroes_the_sums():
    _lib, lib = _lib_()
    rng = np.random.default_rng(3)
    B, H, W = 3, 33, 257
    ssim, mae = random_maps(rng, B, H, W), random_maps(rng, B, H, W)
    ks, ps, ld, stride = placed(ssim, 3, 1)
    km, pm, _, _ = placed(mae, 3, 1)
    bases = [k._base if k._base is not None else k for k in (ks, km)]
    before = [b.clone() for b in bases]
    g = guarded((B, 4), torch.int64, guard_rows=4)  # the view holds the sentinel: an op that only added would keep it in the sums
    runs = []
    for _ in range(2):
        _lib.check(lib.cs_op_metric_map_sums_u16(C.c_void_p(ps), C.c_void_p(pm), B, H, W, ld, stride, _p(g.view), _st()))
        torch.cuda.synchronize()
        g.check("sums")
        runs.append([[int(v) for v in row] for row in g.view.cpu().numpy().view(np.uint64)])
    assert runs[0] == runs[1] == np_sums(ssim, mae)
    assert all(torch.equal(b, c) for b, c in zip(bases, before))


# ------------------------------------------------------------------------------------------------------------------ the fused op
def pairs(rng, B, h, w):
    a = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)
    if B > 1:
        b[1] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)  # unrelated images: SSIM codes on both sides of 32767
    return a, b


def offset_images(src, off, gap=5):
    """(B, h, w, 3) uint8 -> a device buffer of 255s holding the images `off` bytes in and h*w*3 + gap apart: (buffer, address, stride)"""
    B = src.shape[0]
    n = src[0].size
    stride = n + gap
    buf = torch.full((4096 + off + B * stride + 4096,), 255, dtype=torch.uint8, device="cuda")
    for i in range(B):
        buf[4096 + off + i * stride: 4096 + off + i * stride + n] = torch.from_numpy(src[i].reshape(-1)).cuda()
    return buf, buf.data_ptr() + 4096 + off, stride


def fused_and_two_step(a, b, off=0):
    """-> (sums of cs_op_gt_metric_sums_u8, sums of cs_op_metric_map_sums_u16 on the maps of cs_op_gt_metric_map_u8), same pairs"""
    _lib, lib = _lib_()
    B, h, w, _ = a.shape
    ba, pa, stride = offset_images(a, off)
    bb, pb, _ = offset_images(b, off)
    before = (ba.clone(), bb.clone())
    maps = torch.empty((2, B, h, w), dtype=torch.int16, device="cuda")
    for kind in (0, 1):
        _lib.check(lib.cs_op_gt_metric_map_u8(C.c_void_p(pa), C.c_void_p(pb), B, h, w, stride, kind, _p(maps[kind]), w, _st()))
    two = guarded((B, 4), torch.int64, guard_rows=4)
    _lib.check(lib.cs_op_metric_map_sums_u16(_p(maps[0]), _p(maps[1]), B, h, w, w, h * w, _p(two.view), _st()))
    one = guarded((B, 4), torch.int64, guard_rows=4)
    _lib.check(lib.cs_op_gt_metric_sums_u8(C.c_void_p(pa), C.c_void_p(pb), B, h, w, stride, _p(one.view), _st()))
    torch.cuda.synchronize()
    one.check("fused sums")
    two.check("sums")
    assert torch.equal(ba, before[0]) and torch.equal(bb, before[1])
    as_int = lambda g: [[int(v) for v in row] for row in g.view.cpu().numpy().view(np.uint64)]  # noqa: E731
    m = maps.cpu().numpy().view(np.uint16)
    assert as_int(two) == np_sums(m[0], m[1])
    return as_int(one), as_int(two)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(11, 11), (16, 64), (17, 65), (60, 84), (45, 130)])
def test_fused_sums_equal_the_sums_of_the_maps(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    a, b = pairs(rng, 3, h, w)
    for off in (0, 1, 2, 3):
        one, two = fused_and_two_step(a, b, off)
        assert one == two, off
    assert len({tuple(r) for r in one}) == 3
    alone, _ = fused_and_two_step(a[2:3], b[2:3], 1)  # a pair's sums alone = its row in the batch
    assert alone == [one[2]]


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(11, 11), (17, 65), (60, 84)])
def test_fused_sums_of_identical_images(h, w):
    rng = np.random.default_rng(7)
    a, _ = pairs(rng, 3, h, w)
    a[1] = 0
    one, two = fused_and_two_step(a, a.copy())
    n = h * w
    assert one == two == [[65534 * n, 65534 * n, 0, 0]] * 3


@pytest.mark.gpu
def test_bad_arguments_leave_the_sums_untouched():
    _lib, lib = _lib_()
    BAD, UNS = _lib.CS_ERR_BAD_ARG, _lib.CS_ERR_UNSUPPORTED
    m = torch.zeros((2, 8, 16), dtype=torch.int16, device="cuda")
    im = torch.zeros((2, 8, 16, 3), dtype=torch.uint8, device="cuda")
    g = guarded((2, 4), torch.int64, guard_rows=4)
    s, st = _p(g.view), _st()
    u16 = lib.cs_op_metric_map_sums_u16
    u8 = lib.cs_op_gt_metric_sums_u8
    odd = C.c_void_p(m.data_ptr() + 1)
    cases = [
        (u16(None, _p(m), 2, 8, 16, 16, 128, s, st), BAD), (u16(_p(m), None, 2, 8, 16, 16, 128, s, st), BAD),
        (u16(_p(m), _p(m), 2, 8, 16, 16, 128, None, st), BAD),
        (u16(_p(m), _p(m), 0, 8, 16, 16, 128, s, st), BAD), (u16(_p(m), _p(m), 2, 0, 16, 16, 128, s, st), BAD),
        (u16(_p(m), _p(m), 2, 8, -1, 16, 128, s, st), BAD),
        (u16(_p(m), _p(m), 2, 8, 16, 15, 128, s, st), BAD),   # row_elems < W
        (u16(_p(m), _p(m), 2, 8, 16, 16, 127, s, st), BAD),   # frames would overlap
        (u16(odd, _p(m), 2, 8, 16, 16, 128, s, st), BAD),     # samples not 2-byte aligned
        (u16(_p(m), _p(m), 1, 65536, 1, 1, 65536, s, st), UNS), (u16(_p(m), _p(m), 1, 1, 65536, 65536, 65536, s, st), UNS),
        (u8(None, _p(im), 2, 8, 16, 384, s, st), BAD), (u8(_p(im), None, 2, 8, 16, 384, s, st), BAD),
        (u8(_p(im), _p(im), 2, 8, 16, 384, None, st), BAD),
        (u8(_p(im), _p(im), 0, 8, 16, 384, s, st), BAD), (u8(_p(im), _p(im), 2, 8, 0, 384, s, st), BAD),
        (u8(_p(im), _p(im), 2, 8, 16, 383, s, st), BAD),      # stride below the image
        (u8(_p(im), _p(im), 1, 65536, 1, 65536 * 3, s, st), UNS),
    ]
    for i, (rc, want) in enumerate(cases):
        assert rc == want, i
    torch.cuda.synchronize()
    g.check("sums")
    sentinel = g.sentinel
    assert bool((g.view == sentinel).all())  # nothing was queued: not even the zeroing
    with pytest.raises(NotImplementedError):
        _lib.check(u8(_p(im), _p(im), 1, 1, 65536, 65536 * 3, s, st))
    with pytest.raises(ValueError):
        _lib.check(u16(_p(m), _p(m), 2, 8, 16, 15, 128, s, st))
