"""Operand data and a host model of the persistent tile walk for the GEMM walk tests (numpy only: tests/test_gemm_walk_host.py proves on the CPU
what tests/test_hip_gemm_walk.py relies on on the GPU).

The data: small integers drawn from a 64-bit mix of (row, column, seed).  Nothing in it is periodic in m, n or k, so the operands of two row
panels, two column tiles, two K slices or two 16-row epilogue steps never coincide, and a kernel that reads any of them from the wrong tile, the
wrong ring slot or a stale register set produces other integers than the reference.  A holds -2..2, W holds -1, 0, 1 at a density chosen so that
every expected 16-bit output is an integer the type holds (|y| <= 2048 in fp16, <= 256 in bf16: asserted, not assumed), all products and fp32
sums are exact (far below 2^24).

The walk: both kernels number their blocks b = 8 * slot + xcd; XCD x owns the row panels x, x + 8, ..; its blocks walk that list of tiles
n-fastest, block `slot` taking tiles slot, slot + slots, ..  (gemm.hip / gemm256.hip `tile_of`)."""
import numpy as np

U64 = np.uint64


def _mix(i, j, seed):
    """splitmix64-style mix of the index pair (broadcast) and a seed -> uint64"""
    with np.errstate(over="ignore"):
        x = (np.asarray(i, dtype=U64) * U64(0x9E3779B97F4A7C15) + np.asarray(j, dtype=U64) * U64(0xC2B2AE3D27D4EB4F)
             + U64(seed) * U64(0x165667B19E3779F9) + U64(0x632BE59BD9B4E019))
        x ^= x >> U64(30)
        x *= U64(0xBF58476D1CE4E5B9)
        x ^= x >> U64(27)
        x *= U64(0x94D049BB133111EB)
        x ^= x >> U64(31)
    return x


def ints(rows, cols, seed, lo, hi, density=1.0):
    """(rows, cols) float32 integers in [lo, hi]; an entry is non-zero with probability `density` (times the chance of drawing a non-zero)"""
    h = _mix(np.arange(rows)[:, None], np.arange(cols)[None, :], seed)
    v = (h % U64(hi - lo + 1)).astype(np.int64) + lo
    keep = ((h >> U64(40)) % U64(1024)).astype(np.int64) < int(round(density * 1024))
    return np.where(keep, v, 0).astype(np.float32)


def operands(M, N, K, seed=0, w_density=0.5):
    """A (M, K) in -2..2, W (N, K) in {-1, 0, 1}, bias (N,) in -8..8, residual (M, N) in -64..64: all float32 integers"""
    return dict(A=ints(M, K, 11 + seed, -2, 2), W=ints(N, K, 23 + seed, -1, 1, w_density), b=ints(1, N, 37 + seed, -8, 8)[0],
                r=ints(M, N, 41 + seed, -64, 64))


def pos_rows(Np, N, seed=0):
    """(1 + Np, N) position rows, integers in -32..32"""
    return ints(1 + Np, N, 53 + seed, -32, 32)


def ln_rows(M, Cc, BM, seed=0):
    """(M, Cc) integer rows whose LayerNorm statistics differ strongly from row panel to row panel and from row to row: panel p has the offset
    4 * ((5 p) % 7 - 3) and row m the scale 1 + mix(m) % 3 on values in -2..2.  |x| <= 18: exact in fp16."""
    m = np.arange(M)
    off = 4.0 * ((5 * (m // BM)) % 7 - 3)
    scale = 1.0 + (_mix(m, 0, 67 + seed) % U64(3)).astype(np.float64)
    return (off[:, None] + scale[:, None] * ints(M, Cc, 71 + seed, -2, 2)).astype(np.float32)


def ln_weights(N, Cc, seed=0):
    """W' (N, Cc) multiples of 1/64 in [-1/16, 1/16] (exact in fp16 and bf16; projections of order 1), s = its row sums (exact in fp32),
    c (N,) multiples of 1/4 in [-2, 2]"""
    Wp = ints(N, Cc, 83 + seed, -4, 4) / np.float32(64)
    return Wp, Wp.astype(np.float64).sum(1).astype(np.float32), ints(1, N, 89 + seed, -8, 8)[0] / np.float32(4)


# ------------------------------------------------------------------------------------------------ the cases of tests/test_hip_gemm_walk.py
# (here, so that the host test can check the conditions on exactly the data the GPU tests use)
# rows: 300 = 3 panels (five XCDs own nothing), 1147 = 9 * 128 - 5 (XCD 0: a full panel, then a ragged one), 2176 = 17 * 128 (XCD 0 owns 3 panels,
# the others 2); columns: 136 (128-column tiles, full / ragged alternate), 384 (three 128-column tiles, or two of 192 for the 'wide' epilogues),
# 576 (three of 192), 1664 (above BIAS_MAX: the bias comes from memory on every tile)
HALF128 = [(2176, 136, K, e) for e in ("bias", "relu", "leaky", "gelu") for K in (64, 256, 320)] + [
    (300, 136, 64, "bias"), (1147, 384, 256, "bias"), (1147, 576, 320, "bias"), (300, 1664, 64, "bias"), (1147, 1664, 320, "bias"),
    (2176, 384, 64, "bias"), (1147, 576, 64, "relu"), (1147, 384, 320, "relu"), (1147, 1664, 256, "leaky"), (2176, 576, 256, "gelu"),
    (1147, 384, 64, "gelu")]
RESID128 = [(2176, 136, K, "inplace") for K in (64, 256, 320, 1536)] + [(1147, 384, K, "sep") for K in (64, 256, 320, 1536)] + [
    (2176, 384, 320, "ldr"), (2176, 384, 320, "inplace"), (2176, 384, 256, "inplace"), (1147, 576, 320, "none"), (1147, 576, 64, "none"),
    (300, 136, 320, "ldr"), (1147, 1664, 320, "inplace"), (1147, 576, 1536, "sep"), (300, 1664, 64, "ldr"), (2176, 576, 320, "sep"),
    (2176, 136, 256, "none")]
RESID_LN128 = [(M, Cc, K) for Cc, M in ((128, 2176), (384, 1147), (136, 2176)) for K in (64, 320)] + [(300, 384, 64), (2176, 384, 320)]
LN128 = [(M, Cc, N, e) for e in ("ln", "ln_gelu") for Cc, N, M in ((128, 200, 2176), (128, 576, 1147), (384, 384, 2176), (384, 200, 1147),
                                                                    (768, 576, 1147), (768, 384, 300), (384, 576, 2176), (768, 200, 2176),
                                                                    (128, 384, 1147))]
BF16_128 = {"bias": (2176, 136, 320), "relu": (2176, 136, 320), "resid": (2176, 136, 256), "resid-pipe": (1147, 384, 320),
            "resid-ln": (1147, 384, 320)}
# M = 1197: 10 row panels, image boundaries inside tiles; two full 192-column tiles, and 128 + 8 columns (ragged > full hand-overs)
PATCH128 = [dict(I=19, Np=63, Cc=384, K=640), dict(I=19, Np=63, Cc=136, K=128)]
HEAD128 = dict(B=19, gh=7, gw=9, Cc=128)           # the same 1197 rows
G256 = [(768, 512, 384, "bias"), (2301, 256, 512, "bias"), (2301, 512, 640, "bias"), (768, 3328, 384, "bias"), (2301, 512, 384, "resid-inplace"),
        (2301, 256, 640, "resid-sep"), (768, 3328, 512, "resid-inplace"), (2301, 512, 512, "resid-sep"), (2301, 512, 384, "gelu"),
        (768, 512, 640, "gelu"), (2301, 512, 384, "resid-ln"), (768, 256, 512, "resid-ln"), (2301, 256, 640, "resid-ln")]
LN256 = [(2301, 384, 512, "ln"), (2301, 512, 256, "ln_gelu"), (768, 640, 512, "ln_gelu"), (2301, 640, 256, "ln")]


# ------------------------------------------------------------------------------------------------ the walk
def bn128(N, kind="plain"):
    """column tile of the 128-row kernel (gemm.hip `launch`): kind 'plain' (bias / activation / RESID_F32 / head: narrow tile for N <= 384 that
    128 divides), 'wide' (RESID_F32_LN, PATCH_F32, the LayerNorm-folded consumers: 192 wherever it divides N)"""
    wide = N % 192 == 0 and not (kind == "plain" and N % 128 == 0 and N <= 384)
    return 192 if wide else 128


def grid_of(M, N, BM, BN, blocks):
    """the launchers' clamps: a multiple of 8, at most one block per tile of the fullest XCD, at least 8"""
    tiles_m, tiles_n = -(-M // BM), -(-N // BN)
    return max(8, min(blocks // 8 * 8, -(-tiles_m // 8) * tiles_n * 8))


def walk(M, N, BM, BN, blocks):
    """{block: [(m0, n0), ..]} in the order the block computes them (blocks that own nothing have an empty list)"""
    tiles_m, tiles_n = -(-M // BM), -(-N // BN)
    grid = grid_of(M, N, BM, BN, blocks)
    slots = grid // 8
    out = {}
    for b in range(grid):
        xcd, slot = b % 8, b // 8
        ntile_x = (tiles_m - xcd + 7) // 8 * tiles_n
        out[b] = [((idx // tiles_n * 8 + xcd) * BM, idx % tiles_n * BN) for idx in range(slot, ntile_x, slots)]
    return out


def is_full(tile, M, N, BM, BN):
    return tile[0] + BM <= M and tile[1] + BN <= N


def orders(M, N, BM, BN, blocks):
    """the set of (previous tile full?, next tile full?) hand-overs the walk contains, as strings 'full>ragged' .., and the set of
    'last-full' / 'last-ragged' for the last tile of each block that owns any"""
    seen, last = set(), set()
    nm = {True: "full", False: "ragged"}
    for tiles in walk(M, N, BM, BN, blocks).values():
        for a, b in zip(tiles, tiles[1:]):
            seen.add(nm[is_full(a, M, N, BM, BN)] + ">" + nm[is_full(b, M, N, BM, BN)])
        if tiles:
            last.add("last-" + nm[is_full(tiles[-1], M, N, BM, BN)])
    return seen, last


def region(tile, M, N, BM, BN):
    """(row slice, column slice) of a tile inside the (M, N) output"""
    return slice(tile[0], min(tile[0] + BM, M)), slice(tile[1], min(tile[1] + BN, N))


def take_from(dst, src, M, N, BM, BN, rows=None):
    """index arrays (dst rows, dst cols, src rows, src cols): each element of tile `dst` (or of its rows dst.m0 + rows) paired with the element
    at the same offset of tile `src`, clamped into the matrix as the kernels clamp their operand rows"""
    rs, cs = region(dst, M, N, BM, BN)
    dr = np.arange(rs.start, rs.stop)
    if rows is not None:
        dr = dr[(dr - dst[0] >= rows.start) & (dr - dst[0] < rows.stop)]
    dc = np.arange(cs.start, cs.stop)
    sr = np.minimum(dr - dst[0] + src[0], M - 1)
    sc = np.minimum(dc - dst[1] + src[1], N - 1)
    return dr, dc, sr, sc


def product(A, W, b):
    """fp64 A W^T + b of float32 integer operands"""
    return A.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)


def tile_product_with_slice_from(A, W, b, tiles, pos, kt, back, BM, BN, BK=32):
    """A W^T + b of tile tiles[pos] with its K slice kt (BK wide) replaced by the slice `back` places earlier in the block's slice stream (which
    runs through the block's tiles one after the other: the slice 3 back is the one that last used the same ring slot of a 3-slot ring).  Rows
    past M / N are clamped as the staging does.  -> (rows, cols) array of the tile's extent"""
    M, K = A.shape
    N = W.shape[0]
    nk = K // BK
    g = pos * nk + kt - back
    assert g >= 0
    src_tile, src_kt = tiles[g // nk], g % nk
    m0, n0 = tiles[pos]
    ar = np.minimum(m0 + np.arange(BM), M - 1)
    wr = np.minimum(n0 + np.arange(BN), N - 1)
    a, w = A[ar].astype(np.float64), W[wr].astype(np.float64)
    sa = np.minimum(src_tile[0] + np.arange(BM), M - 1)
    sw = np.minimum(src_tile[1] + np.arange(BN), N - 1)
    a[:, kt * BK:(kt + 1) * BK] = A[sa, src_kt * BK:(src_kt + 1) * BK]
    w[:, kt * BK:(kt + 1) * BK] = W[sw, src_kt * BK:(src_kt + 1) * BK]
    rs, cs = region(tiles[pos], M, N, BM, BN)
    y = a @ w.T + b[wr].astype(np.float64)
    return y[:rs.stop - rs.start, :cs.stop - cs.start]


def row_partials128(x, BN):
    """(M, 4 * column tiles, 2) fp64 (sum, sum of squares) over the columns each (column tile, wave) of the 128-row kernel owns"""
    M, Cc = x.shape
    tiles = -(-Cc // BN)
    wn = BN // 4
    out = np.zeros((M, 4 * tiles, 2))
    for t in range(tiles):
        for w in range(4):
            seg = x[:, t * BN + w * wn:min(t * BN + (w + 1) * wn, Cc)].astype(np.float64)
            out[:, 4 * t + w, 0] = seg.sum(1)
            out[:, 4 * t + w, 1] = (seg * seg).sum(1)
    return out


def ln_folded(x16, Wp, s, c, mu, rstd):
    """the folded LayerNorm projection in fp64: rstd (x16 W'^T - mu s) + c"""
    acc = x16.astype(np.float64) @ Wp.astype(np.float64).T
    return rstd[:, None] * (acc - mu[:, None] * s.astype(np.float64)[None, :]) + c.astype(np.float64)[None, :]


def ln_stats(part, K, eps):
    """(mu, rstd) in fp64 from (M, sp, 2) partial sums, as the consumer computes them"""
    s1, s2 = part[:, :, 0].sum(1), part[:, :, 1].sum(1)
    mu = s1 / K
    return mu, 1.0 / np.sqrt(np.maximum(s2 / K - mu * mu, 0.0) + eps)
