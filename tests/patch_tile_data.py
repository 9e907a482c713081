"""Operand data and a host model of the one-launch patch embedding for its tile-level tests (numpy only: tests/test_patch_tiles_host.py proves on
the CPU what tests/test_hip_patch_tiles.py relies on on the GPU).

The kernel (csrc/patch.hip, cs_patch_fused_kernel): one workgroup = one run of np <= 48 consecutive patches of one patch row; a patch row of gw
patches is cut into nsx = ceil(gw / 48) runs of near-equal length (the first gw % nsx runs one longer).  The run's centred 16-bit A tile is
[np][648] in LDS; behind it, at 37 * 1296 bytes when no run is longer than 37 patches and at 48 * 1296 otherwise, the four waves' epilogue
patches and the means.  Wave w owns columns 96 w .. 96 w + 95 of a 384-column pass as six 16-column tiles, 19 k-steps of 32; a weight fragment
holds, for lane l, the 8 contraction indices 32 s + 8 (l >> 4) .. + 7 of column 16 j + (l & 15).

Contract of both forms (`fused`, and `two` = im2col_rows_kernel + the CS_EPI_PATCH_F32 GEMM):
    mu[patch][ch] = fp32 sum of the 14 pixels of a row left to right, then of the 14 row sums top to bottom, divided once by 196
    a[patch][k]   = round16(fl32(v[patch][k] - mu[patch][ch(k)]))          round to nearest even, once
    out           = sum_k a W16[n][k] + bias[n] + pos[token][n] + sum_ch mu[ch] * wsum[ch][n]    in fp32, wsum = fp32 tap sums of the fp32 weights
"""
import numpy as np

P = 14
PP = P * P            # taps per channel
KK = 3 * PP           # 588 contraction indices
KS = 19               # k-steps of 32
MAXNP = 48            # patches per run
NCOL = 384            # columns per pass
PITCH = 1296          # bytes per A tile row
F32 = np.float32

# gw -> the runs the issue's geometry table names
GW_TABLE = {1: [1], 15: [15], 16: [16], 17: [17], 31: [31], 32: [32], 33: [33], 37: [37], 38: [38], 48: [48], 49: [25, 24], 97: [33, 32, 32]}


# ---- geometry, by the arithmetic of cs_patch_fused_launch and the kernel's block decoding ------------------------------------------------
def runs(gw):
    """patches per run of a patch row of gw patches"""
    nsx = (gw + MAXNP - 1) // MAXNP
    base, rem = gw // nsx, gw - (gw // nsx) * nsx
    return [base + (1 if sx < rem else 0) for sx in range(nsx)]


def run_starts(gw):
    nsx = (gw + MAXNP - 1) // MAXNP
    base, rem = gw // nsx, gw - (gw // nsx) * nsx
    return [sx * base + (sx if sx < rem else rem) for sx in range(nsx)]


def layout(gw):
    """(npmax, rows the A tile is laid out for, byte offset of the epilogue patches)"""
    nsx = (gw + MAXNP - 1) // MAXNP
    npmax = (gw + nsx - 1) // nsx
    rows = 37 if npmax <= 37 else MAXNP
    return npmax, rows, rows * PITCH


def row_tiles(np_):
    """16-row MFMA tiles of a run, dead rows of its last tile"""
    mt = (np_ + 15) >> 4
    return mt, 16 * mt - np_


def image_size(gh, gw, trail_rows=0, trail_cols=0):
    return gh * P + trail_rows, gw * P + trail_cols


# ---- im2col and the fp64 reference ------------------------------------------------------------------------------------------------------
def blocks(x, gh, gw):
    """(I, 3, H, W) -> (I, 3, gh, P, gw, P) view of the whole patches: [image, channel, patch row, dy, patch column, dx]"""
    I = x.shape[0]
    return x[:, :, :gh * P, :gw * P].reshape(I, 3, gh, P, gw, P)


def patches(x, gh, gw):
    """(I, gh gw, 588): row = patch (row-major over the grid), column k = ch * 196 + dy * 14 + dx; pixels past the last whole patch are not read"""
    I = x.shape[0]
    return np.ascontiguousarray(blocks(x, gh, gw).transpose(0, 2, 4, 1, 3, 5)).reshape(I, gh * gw, KK)


def conv64(x, w, b, pos, gh, gw):
    """the convolution + bias + position rows in fp64: (I, gh gw, C)"""
    return patches(x, gh, gw).astype(np.float64) @ w.reshape(w.shape[0], KK).astype(np.float64).T + b.astype(np.float64) + pos[None, 1:].astype(np.float64)


# ---- the 16-bit operand types and the kernel's mean ---------------------------------------------------------------------------------------
def round16(a, bf16, toward_zero=False):
    """fp32 -> operand type -> fp32.  Nearest even, as the kernel's packing; toward_zero is the fault the host test measures the sensitivity to."""
    a = np.ascontiguousarray(a, dtype=F32)
    if bf16:
        u = a.view(np.uint32).astype(np.uint64)
        if not toward_zero:
            u = u + 0x7FFF + ((u >> 16) & 1)
        return (u & 0xFFFF0000).astype(np.uint32).view(F32).reshape(a.shape)
    r = a.astype(np.float16).astype(F32)
    if toward_zero:
        over = np.abs(r) > np.abs(a)
        r = np.where(over, np.nextafter(r.astype(np.float16), np.float16(0)).astype(F32), r)
    return r


def mean_f32(x, gh, gw, order="kernel"):
    """(I, gh gw, 3) per-(patch, channel) means in fp32.  order "kernel": the 14 pixels of a row left to right, then the 14 rows top to bottom,
    one division by 196.  "columns" (columns first) is the other order the host test measures the sensitivity to."""
    b = blocks(x, gh, gw).astype(F32)
    if order == "columns":
        b = b.transpose(0, 1, 2, 5, 4, 3)
    rs = np.zeros(b.shape[:-1], F32)
    for dx in range(P):
        rs = rs + b[..., dx]
    s = np.zeros((b.shape[0], 3, gh, gw), F32)
    for dy in range(P):
        s = s + rs[:, :, :, dy, :]
    assert s.dtype == F32
    mu = s / F32(PP)
    return np.ascontiguousarray(mu.transpose(0, 2, 3, 1)).reshape(x.shape[0], gh * gw, 3)


def wsum_f32(w):
    """(3, C): fp32 sums of the taps of a channel, in tap order (patch_wsum_kernel)"""
    w3 = w.reshape(w.shape[0], 3, PP).astype(F32)
    s = np.zeros((w.shape[0], 3), F32)
    for t in range(PP):
        s = s + w3[:, :, t]
    return np.ascontiguousarray(s.T)


def emulate(x, w, b, pos, gh, gw, bf16, centred=True):
    """host model of the contract above, (I, gh gw, C) fp32.  The products are summed in fp64 and rounded once (the kernel's fp32 accumulation
    differs from that by its summation error only); everything else in fp32 in the kernel's order."""
    pt = patches(x, gh, gw).astype(F32)
    mu = mean_f32(x, gh, gw) if centred else np.zeros((x.shape[0], gh * gw, 3), F32)
    a = round16(pt - np.repeat(mu, PP, axis=2), bf16)
    w16 = round16(w.reshape(w.shape[0], KK), bf16)
    r = (a.astype(np.float64) @ w16.astype(np.float64).T).astype(F32)
    r = r + b.astype(F32)[None, None, :]
    r = r + pos[None, 1:].astype(F32)
    ws = wsum_f32(w)
    dc = mu[:, :, 0:1] * ws[0][None, None, :]
    dc = dc + mu[:, :, 1:2] * ws[1][None, None, :]
    dc = dc + mu[:, :, 2:3] * ws[2][None, None, :]
    assert r.dtype == F32 and dc.dtype == F32
    return r + dc


# ---- 1. exact integers --------------------------------------------------------------------------------------------------------------------
def integer_images(I, gh, gw, seed, trail_rows=5, trail_cols=2):
    """(I, 3, 14 gh + trail_rows, 14 gw + trail_cols) float32: integer pixels in [-13, 13] whose every (patch, channel) sum is a multiple of 49
    (start in [-12, 12]; the sum moves to the nearest multiple by +-1 on |d| <= 24 distinct taps), so that every patch mean is a multiple of
    1/4.  The pixels past the last whole patch are NaN."""
    g = np.random.Generator(np.random.PCG64(seed))
    blk = g.integers(-12, 13, size=(I, 3, gh, gw, PP))
    s = blk.sum(-1)
    d = 49 * np.floor_divide(2 * s + 49, 98) - s
    assert np.abs(d).max() <= 24
    rank = np.argsort(np.argsort(g.random(blk.shape), axis=-1), axis=-1)
    blk = blk + np.sign(d)[..., None] * (rank < np.abs(d)[..., None])
    H, W = image_size(gh, gw, trail_rows, trail_cols)
    x = np.full((I, 3, H, W), np.nan, F32)
    x[:, :, :gh * P, :gw * P] = blk.reshape(I, 3, gh, gw, P, P).transpose(0, 1, 2, 4, 3, 5).reshape(I, 3, gh * P, gw * P)
    return x


def integer_operands(C, T, seed):
    """weights (C, 3, 14, 14) dense integers in -2..2, bias (C,) multiples of 1/4 in [-4, 4], position table (T, C): pos[t][n] = (t C + n -
    T C // 2) / 4, a different value at every (token row, column)"""
    g = np.random.Generator(np.random.PCG64(seed))
    w = g.integers(-2, 3, size=(C, 3, P, P)).astype(F32)
    b = (g.integers(-16, 17, size=C) / 4.0).astype(F32)
    pos = ((np.arange(T)[:, None] * C + np.arange(C)[None, :] - (T * C) // 2) / 4.0).astype(F32)
    return w, b, pos


def largest_partial_sum(x, w, b, pos, gh, gw):
    """the bound on every partial sum a kernel can form on the way to one output element, whatever its order: sum_k |a W| + sum_ch |mu wsum| +
    |bias| + |pos|, with a = v - mu (exact for the integer images)"""
    pt = patches(x, gh, gw).astype(np.float64)
    mu = np.repeat(pt.reshape(pt.shape[0], pt.shape[1], 3, PP).mean(-1), PP, axis=2)
    wa = np.abs(w.reshape(w.shape[0], KK)).astype(np.float64)
    s = np.abs(pt - mu) @ wa.T + np.abs(mu) @ wa.T + np.abs(b.astype(np.float64)) + np.abs(pos[None, 1:].astype(np.float64))
    return float(s.max())


# ---- 2. one-hot weights -------------------------------------------------------------------------------------------------------------------
ONEHOT_B = {768: (0, 22, 11, 25), 384: (0, 14, 23, 5)}


def onehot_k(C, b):
    """the contraction index of column n's single 1.0"""
    return (37 * np.arange(C) + b) % KK


def onehot_weights(C, b):
    w = np.zeros((C, KK), F32)
    w[np.arange(C), onehot_k(C, b)] = 1.0
    return w.reshape(C, 3, P, P)


def onehot_coverage(C):
    """what the four maps of width C hit together: (contraction indices, (16-column tile, k-step) pairs, (n mod 16, k mod 32) fragment slots)"""
    ks, tiles, slots = set(), set(), set()
    for b in ONEHOT_B[C]:
        k = onehot_k(C, b)
        n = np.arange(C)
        ks |= set(k.tolist())
        tiles |= set(zip((n // 16).tolist(), (k // 32).tolist()))
        slots |= set(zip((n % 16).tolist(), (k % 32).tolist()))
    return ks, tiles, slots


def generic_images(I, gh, gw, seed):
    """a per-(patch, channel) base in [-2, 2.4] plus 0.3 N(0, 1): smooth-image-like patches, mostly their mean"""
    g = np.random.Generator(np.random.PCG64(seed))
    base = g.uniform(-2.0, 2.4, size=(I, 3, gh, 1, gw, 1))
    x = base + 0.3 * g.standard_normal((I, 3, gh, P, gw, P))
    return x.reshape(I, 3, gh * P, gw * P).astype(F32)


def onehot_expected(x, gh, gw, k, bf16, toward_zero=False, order="kernel", centred=True):
    """out[m][n] = fl32(round16(fl32(v[m][k[n]] - mu)) + mu), mu the mean of k[n]'s channel: (I, gh gw, C) fp32.  bias and position table zero."""
    pt = patches(x, gh, gw).astype(F32)
    mu = mean_f32(x, gh, gw, order)
    v, m = pt[:, :, k], mu[:, :, k // PP]
    if not centred:
        return round16(v, bf16, toward_zero)
    out = round16(v - m, bf16, toward_zero) + m
    assert out.dtype == F32
    return out


# ---- 3. constant patches ------------------------------------------------------------------------------------------------------------------
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def constant_images(I, gh, gw, seed):
    """every patch constant per channel, at what a normalised uint8 level looks like: ((l / 255) - mean) / std in fp32 for a random level l.
    -> (images (I, 3, 14 gh, 14 gw), constants (I, gh gw, 3))"""
    g = np.random.Generator(np.random.PCG64(seed))
    lv = g.integers(0, 256, size=(I, 3, gh, gw))
    c = ((lv.astype(F32) / F32(255.0)) - np.array(IMAGENET_MEAN, F32)[None, :, None, None]) / np.array(IMAGENET_STD, F32)[None, :, None, None]
    x = np.broadcast_to(c[:, :, :, None, :, None], (I, 3, gh, P, gw, P)).reshape(I, 3, gh * P, gw * P)
    return np.ascontiguousarray(x, dtype=F32), np.ascontiguousarray(c.transpose(0, 2, 3, 1)).reshape(I, gh * gw, 3)


def random_operands(C, T, seed):
    """weights N(0, 1) / sqrt(588), bias and position table N(0, 1), all fp32"""
    g = np.random.Generator(np.random.PCG64(seed))
    w = (g.standard_normal((C, 3, P, P)) / np.sqrt(KK)).astype(F32)
    return w, g.standard_normal(C).astype(F32), g.standard_normal((T, C)).astype(F32)


def constant_bound(c, w, b, pos):
    """256 * 2^-24 * (sum_k |W[n][k]| |c_ch(k)| + |b[n]| + |pos[token][n]|): (I, gh gw, C) fp64 -- the fp32 bound of two 196-term sums (the
    mean and the tap sum) plus the epilogue"""
    wa = np.abs(w.reshape(w.shape[0], 3, PP).astype(np.float64)).sum(-1)  # (C, 3)
    s = np.abs(c.astype(np.float64)) @ wa.T + np.abs(b.astype(np.float64)) + np.abs(pos[None, 1:].astype(np.float64))
    return 256.0 * 2.0 ** -24 * s


# ---- 4, 5. random data ---------------------------------------------------------------------------------------------------------------------
def normal_images(I, gh, gw, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((I, 3, gh * P, gw * P)).astype(F32)
