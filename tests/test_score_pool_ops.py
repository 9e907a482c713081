"""The score-pool ops (cs_op_score_pool_u16, cs_op_score_pool_f32) against the numpy statement of
tests/score_pool_oracle.py.  The ops return unsigned integers, so every comparison is integer equality.  Each call pools a batch whose images
are the contents under test side by side, which also puts every content at a position of its own in a batch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import score_pool_oracle as oracle  # noqa: E402
from guard import guarded, poisoned_in  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (14, 14), (37, 53), (130, 70), (266, 266), (518, 518)]
PERMILLES = [(0,), (1000,), (10, 50, 100, 250, 500), (1000, 999, 750, 500, 500, 250, 250, 100, 50, 50, 10, 1, 1, 0, 0, 500)]
WINDOWS = (1, 2, 14, 56)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _lib_():
    from crossscore_amd import _lib

    return _lib, _lib.load()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Outputs:
    """the four outputs and the scratch of a call inside guard bands (the scratch only while it is small: its mask costs eight times its size)"""

    def __init__(self, B, H, W, Q):
        _, lib = _lib_()
        self.B, self.Q = B, Q
        self.sum = guarded((B,), torch.int64, guard_rows=4)
        self.quant = guarded((B, Q), torch.int32, guard_rows=4)
        self.tail = guarded((B, Q), torch.int64, guard_rows=4)
        self.window = guarded((B, 3), torch.int64, guard_rows=4)
        nbytes = int(lib.cs_score_pool_workspace_bytes(B, H, W, Q))
        assert nbytes > 0
        self.scratch = guarded((nbytes,), torch.uint8, guard_rows=1) if nbytes <= (4 << 20) else None
        self.scratch_view = self.scratch.view if self.scratch is not None else torch.empty((nbytes,), dtype=torch.uint8, device="cuda")

    def tail_args(self, permille, S, window=True):
        arr = (C.c_int32 * len(permille))(*permille)
        return (arr, len(permille), S, _p(self.sum.view), _p(self.quant.view), _p(self.tail.view), _p(self.window.view) if window else None,
                _p(self.scratch_view), _st())

    def check(self):
        torch.cuda.synchronize()
        for g, what in ((self.sum, "sum"), (self.quant, "quant"), (self.tail, "tail"), (self.window, "window"), (self.scratch, "scratch")):
            if g is not None:
                g.check(what)

    def untouched(self, g):
        torch.cuda.synchronize()
        return bool((g.ibase == g.sentinel).all())

    def words(self, window=True):
        self.check()
        return {"sum": [int(v) for v in self.sum.view.cpu().numpy().view(np.uint64)],
                "quant": self.quant.view.cpu().numpy().view(np.uint32).astype(np.int64).tolist(),
                "tail": [[int(v) for v in r] for r in self.tail.view.cpu().numpy().view(np.uint64)],
                "window": [tuple(int(v) for v in r) for r in self.window.view.cpu().numpy().view(np.uint64)] if window else None}


def pool_u16(maps, permille, S=0, out=None, window=True):
    """the u16 entry on host maps (B, H, W) uint16, contiguous on the device"""
    _lib, lib = _lib_()
    B, H, W = maps.shape
    dev = torch.from_numpy(np.ascontiguousarray(maps).view(np.int16)).cuda()
    out = out or Outputs(B, H, W, len(permille))
    _lib.check(lib.cs_op_score_pool_u16(_p(dev), B, H, W, W, H * W, *out.tail_args(permille, S, window)))
    return out.words(window and S > 0)


def pool_f32(scores, signed, permille, S=0, out=None, window=True):
    _lib, lib = _lib_()
    B, H, W = scores.shape
    dev = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).cuda()
    out = out or Outputs(B, H, W, len(permille))
    _lib.check(lib.cs_op_score_pool_f32(_p(dev), B, H, W, 1 if signed else 0, *out.tail_args(permille, S, window)))
    return out.words(window and S > 0)


def want(maps, permille, S=0):
    ps = [oracle.pool(m, permille, S) for m in maps]
    return {"sum": [p["sum"] for p in ps], "quant": [p["quant"] for p in ps], "tail": [p["tail"] for p in ps],
            "window": [p["window"] for p in ps] if S else None}


def scores_of(codes):
    """fp32 scores whose codes over the [0, 1] range are `codes`: the middle of each code's interval"""
    s = ((codes.astype(np.float64) + 0.5) / 65535.0).astype(np.float32)
    assert np.array_equal(oracle.gray16(s, False), codes)
    return s


def two_valued(rng, h, w, low):
    m = np.full(h * w, 40000, dtype=np.uint16)
    m[:max(0, min(h * w, low))] = 4095  # (the last code of a coarse bin)
    return rng.permutation(m).reshape(h, w)


def contents(rng, h, w):
    n = h * w
    r = 250 * (n - 1) // 1000  # the index the 250-permille quantile reads
    maps = [rng.integers(0, 65536, (h, w), dtype=np.uint16), np.zeros((h, w), np.uint16), np.full((h, w), 65535, np.uint16),
            np.full((h, w), 32767, np.uint16)]
    maps += [two_valued(rng, h, w, low) for low in (r, r + 1, r + 2)]  # s[r] is the first high code, the last low one, a low one
    maps.append((4088 + rng.integers(0, 17, (h, w))).astype(np.uint16))  # 17 neighbours across the edge of coarse bin 255 | 256
    return np.stack(maps)


@pytest.mark.parametrize("h,w", SHAPES)
def test_order_statistics_and_tails_equal_numpy(h, w):
    rng = np.random.default_rng(1000 * h + w)
    maps = contents(rng, h, w)
    for permille in PERMILLES:
        exp = want(maps, permille)
        got = pool_u16(maps, permille)
        assert got == exp, ("u16", permille)
        got = pool_f32(scores_of(maps), False, permille)
        assert got == exp, ("f32", permille)


def test_every_code_once():
    rng = np.random.default_rng(65536)
    maps = rng.permutation(65536).astype(np.uint16).reshape(1, 256, 256)
    permille = tuple(range(0, 1001, 67))  # 15 values, every quantile another code
    exp = want(maps, permille)
    assert len(set(exp["quant"][0])) == len(permille) and exp["quant"][0] == [q * 65535 // 1000 for q in permille]
    assert pool_u16(maps, permille) == exp
    assert pool_f32(scores_of(maps), False, permille) == exp


def window_contents(rng, h, w, S):
    maps = [rng.integers(0, 65536, (h, w), dtype=np.uint16), np.full((h, w), 777, np.uint16)]
    for y, x in ((h - S, (w - S) // 2), ((h - S) // 2, w - S)):  # the unique minimum in the last row, in the last column
        m = rng.integers(1000, 65536, (h, w), dtype=np.uint16)
        m[y:y + S, x:x + S] = 0
        maps.append(m)
    m = np.full((h, w), 1000, np.uint16)  # two equal minima in one row
    m[h - 1, 0] = m[h - 1, w - 1] = 0
    maps.append(m)
    m = np.full((h, w), 1000, np.uint16)  # ... and in one column
    m[0, w - 1] = m[h - 1, w - 1] = 0
    maps.append(m)
    return np.stack(maps)


@pytest.mark.parametrize("h,w", SHAPES)
def test_worst_window_equals_numpy(h, w):
    rng = np.random.default_rng(2000 * h + w)
    for S in sorted({s for s in WINDOWS + (min(h, w),) if s <= min(h, w, 255)}):
        maps = window_contents(rng, h, w, S)
        exp = want(maps, (500,), S)
        assert exp["window"][1] == (777 * S * S, 0, 0)  # a constant map: the first corner
        assert pool_u16(maps, (500,), S) == exp, ("u16", S)
        assert pool_f32(scores_of(maps), False, (500,), S) == exp, ("f32", S)


def test_largest_window_sum_and_no_window():
    maps = np.full((1, 255, 256), 65535, np.uint16)
    got = pool_u16(maps, (1000,), 255)
    assert got["window"] == [(4261413375, 0, 0)] and got["sum"] == [255 * 256 * 65535] == got["tail"][0]
    assert pool_f32(np.ones((1, 255, 256), np.float32), False, (1000,), 255) == got
    # S = 0, and a null window: no window launch; a window buffer that was handed over stays as it was
    rng = np.random.default_rng(9)
    maps = rng.integers(0, 65536, (2, 37, 53), dtype=np.uint16)
    out = Outputs(2, 37, 53, 1)
    assert pool_u16(maps, (500,), 0, out=out) == want(maps, (500,))
    assert out.untouched(out.window)
    assert pool_u16(maps, (500,), 14, out=out, window=False) == want(maps, (500,))
    assert out.untouched(out.window)


def specials(signed):
    ks = np.array([0, 1, 2, 255, 4095, 4096, 32766, 32767, 32768, 65534, 65535], dtype=np.float64)
    base = (ks / 32767.0 - 1.0 if signed else ks / 65535.0).astype(np.float32)
    near = np.concatenate([base, np.nextafter(base, np.float32(-4)), np.nextafter(base, np.float32(4))])
    odd = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -0.5, -1.0, -1.0000001, -2.0, 1.0, 1.0000001, 1.5, 2.0, 3.0e38, -3.0e38, 1e-45, -1e-45, 7e4, -7e4],
                   dtype=np.float32)
    return np.concatenate([near, odd])


@pytest.mark.parametrize("signed", [False, True])
def test_fp32_entry_is_the_gray16_op_then_the_u16_entry(signed):
    _lib, lib = _lib_()
    rng = np.random.default_rng(77 + signed)
    h, w = 37, 53
    s = rng.uniform(-1.2, 1.2, (2, h * w)).astype(np.float32)
    sp = specials(signed)
    s[0, :sp.size] = sp
    s[1] = rng.permutation(s[0])
    s = s.reshape(2, h, w)
    dev = torch.from_numpy(s).cuda()
    codes = torch.empty((2, h, w), dtype=torch.int16, device="cuda")
    _lib.check(lib.cs_op_score_to_gray16(_p(dev), dev.numel(), 1 if signed else 0, _p(codes), _st()))
    codes = codes.cpu().numpy().view(np.uint16)
    assert np.array_equal(codes, oracle.gray16(s, signed))  # the op's codes are numpy's, the odd values included
    for permille, S in (((0, 1000, 10, 50, 100, 250, 500), 14), (PERMILLES[3], 1)):
        a = pool_f32(s, signed, permille, S)
        assert a == pool_u16(codes, permille, S) == want(codes, permille, S)


def test_strided_u16_maps_read_only_their_own_samples():
    _lib, lib = _lib_()
    rng = np.random.default_rng(4)
    B, h, w, pad, extra = 3, 37, 53, 11, 3
    maps = rng.integers(0, 65000, (B, h, w), dtype=np.uint16)  # (no 0xFFFF of their own: one read of the poison moves the maximum and the sum)
    tall = np.full((B, h + extra, w), 0xFFFF, dtype=np.uint16)  # rows of 0xFFFF behind every image: the image stride lies beyond the image
    tall[:, :h] = maps
    v = poisoned_in(torch.from_numpy(tall.view(np.int16)).cuda(), ld=w + pad)  # 0xFFFF behind every row and around the whole
    permille = (0, 10, 500, 1000)
    out = Outputs(B, h, w, len(permille))
    _lib.check(lib.cs_op_score_pool_u16(_p(v), B, h, w, w + pad, (h + extra) * (w + pad), *out.tail_args(permille, 14)))
    assert out.words() == want(maps, permille, 14)


def test_an_image_has_the_same_words_alone_and_anywhere_in_a_batch():
    rng = np.random.default_rng(12)
    h, w = 130, 70
    img = rng.integers(0, 65536, (h, w), dtype=np.uint16)
    others = rng.integers(0, 65536, (8, h, w), dtype=np.uint16)
    permille = PERMILLES[2]
    alone = pool_u16(img[None], permille, 14)
    alone_f = pool_f32(scores_of(img[None]), False, permille, 14)
    assert alone == alone_f == want(img[None], permille, 14)
    for pos in (0, 3, 7):
        batch = others.copy()
        batch[pos] = img
        for got in (pool_u16(batch, permille, 14), pool_f32(scores_of(batch), False, permille, 14)):
            assert {k: [v[pos]] for k, v in got.items()} == alone, pos


def test_guard_bands_hold_over_two_runs_on_the_same_buffers():
    rng = np.random.default_rng(21)
    B, h, w = 3, 130, 70
    permille = PERMILLES[3]
    out = Outputs(B, h, w, len(permille))
    assert out.scratch is not None  # the scratch of this size stands inside guard bands too
    first = rng.integers(0, 65536, (B, h, w), dtype=np.uint16)
    second = np.stack([np.full((h, w), 65535, np.uint16), np.zeros((h, w), np.uint16), rng.integers(0, 300, (h, w)).astype(np.uint16)])
    assert pool_u16(first, permille, 56, out=out) == want(first, permille, 56)
    assert pool_u16(second, permille, 56, out=out) == want(second, permille, 56)  # the ops start their accumulators afresh
    assert pool_f32(scores_of(first), False, permille, 2, out=out) == want(first, permille, 2)
    assert pool_f32(scores_of(second), False, permille, 70, out=out) == want(second, permille, 70)


def test_bad_arguments_are_rejected_before_anything_is_queued():
    _lib, lib = _lib_()
    B, h, w = 2, 20, 30
    u16 = torch.zeros((B, h, w), dtype=torch.int16, device="cuda")
    f32 = torch.zeros((B, h, w), dtype=torch.float32, device="cuda")
    out = Outputs(B, h, w, 16)
    BAD, UNS = _lib.CS_ERR_BAD_ARG, _lib.CS_ERR_UNSUPPORTED

    def call(entry="u16", m="map", b=B, hh=h, ww=w, ld=w, stride=h * w, signed=0, permille=(500,), q=None, S=5, null=()):
        arr = (C.c_int32 * max(1, len(permille)))(*permille)
        q = len(permille) if q is None else q
        ptr = {k: (None if k in null else _p(g.view)) for k, g in (("sum", out.sum), ("quant", out.quant), ("tail", out.tail), ("window", out.window))}
        scratch = None if "scratch" in null else _p(out.scratch_view)
        per = None if "permille" in null else arr
        tail = (per, q, S, ptr["sum"], ptr["quant"], ptr["tail"], ptr["window"], scratch, _st())
        if entry == "u16":
            return lib.cs_op_score_pool_u16(None if m is None else _p(u16), b, hh, ww, ld, stride, *tail)
        return lib.cs_op_score_pool_f32(None if m is None else _p(f32), b, hh, ww, signed, *tail)

    cases = [(dict(b=0), BAD), (dict(hh=0), BAD), (dict(ww=0), BAD), (dict(b=1025), UNS), (dict(hh=4097, stride=4097 * w), UNS),
             (dict(ww=4097, ld=4097, stride=4097 * h), UNS), (dict(S=21), BAD), (dict(S=256), BAD), (dict(S=-1), BAD), (dict(q=0), BAD),
             (dict(q=17), BAD), (dict(permille=(500, 1001)), BAD), (dict(permille=(-1,)), BAD), (dict(ld=w - 1), BAD), (dict(stride=h * w - 1), BAD),
             (dict(m=None), BAD), (dict(null=("sum",)), BAD), (dict(null=("quant",)), BAD), (dict(null=("tail",)), BAD), (dict(null=("scratch",)), BAD),
             (dict(null=("permille",)), BAD)]
    for kw, code in cases:
        assert call("u16", **kw) == code, kw
        assert _lib.last_error(), kw
    for kw, code in [(dict(signed=2), BAD), (dict(b=1025), UNS), (dict(hh=4097), UNS), (dict(S=21), BAD), (dict(q=17), BAD), (dict(permille=(1001,)), BAD),
                     (dict(m=None), BAD), (dict(null=("tail",)), BAD)]:
        assert call("f32", **kw) == code, kw
    for g in (out.sum, out.quant, out.tail, out.window):
        assert out.untouched(g)
    if out.scratch is not None:
        assert out.untouched(out.scratch)
    with pytest.raises(ValueError, match="permille"):
        _lib.check(call("u16", permille=(2000,)))
    assert call("u16") == 0 and call("f32") == 0  # and the same buffers take a good call
    out.check()
