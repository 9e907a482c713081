"""cs_op_png_encode_ex: the device PNG encoder's opt-in forms (CS_PNG_DYNAMIC: dynamic-Huffman blocks chosen per segment among four exactly
priced forms; CS_PNG_ADAPTIVE_FILTER: the per-row minimum-sum-of-absolute-differences filter).  Host-side contract on the CPU, files on the GPU.

Every file goes through the validator of tests/png_files.py: its own chunk parser with CRCs, zlib.decompress over the concatenated IDAT payloads
(Adler-32 and every code table), the un-filter, and PIL's pixels."""
import ctypes as C
import functools
import heapq
import os
import re
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
from crossscore_amd import _lib  # noqa: E402
from crossscore_amd.config import load_config  # noqa: E402
from png_files import GRAY16, RGB8, check_png, contents, encode_raw, filtered_size, parse_chunks, row_bytes  # noqa: E402

DYNAMIC, ADAPTIVE = 1, 2
SEG = 16384
FILL = 0xA5
CONTENT_NAMES = ("constant", "ramp", "noise", "score map")


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_symbol_and_flags_declared_bound_and_exported():
    hdr = open(os.path.join(REPO, "include", "crossscore_hip.h")).read()
    declared = set(re.findall(r"\b(cs_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    assert "cs_op_png_encode_ex" in declared and "cs_op_png_encode_ex" in _lib.SYMBOLS and hasattr(lib, "cs_op_png_encode_ex")
    assert re.search(r"CS_PNG_DYNAMIC\s*=\s*1\b", hdr) and re.search(r"CS_PNG_ADAPTIVE_FILTER\s*=\s*2\b", hdr)
    assert (_lib.PNG_DYNAMIC, _lib.PNG_ADAPTIVE_FILTER) == (DYNAMIC, ADAPTIVE)


def _host_call(lib, p, kind, i, h, w, stride, slot, flags):
    return lib.cs_op_png_encode_ex(p, kind, i, h, w, stride, p, slot, p, p, None, flags)


def test_flags_outside_0_to_3_and_bad_arguments_are_rejected_on_the_host():
    """CS_ERR_BAD_ARG with a message before any device call (this runs without a GPU)."""
    lib = _lib.load()
    dummy = (C.c_uint8 * 64)()
    p = C.cast(dummy, C.c_void_p)
    bound = lib.cs_png_bound(RGB8, 16, 16)
    for flags in (-1, 4, 7, 1 << 20):
        assert _host_call(lib, p, RGB8, 1, 16, 16, 768, bound, flags) == _lib.CS_ERR_BAD_ARG, flags
        assert b"flags" in lib.cs_last_error(), lib.cs_last_error()
    for flags in (0, 1, 2, 3):
        for args, word in (((7, 1, 16, 16, 768, bound), b"kind"), ((RGB8, 1, 16, 0, 768, bound), b"sizes"), ((RGB8, 0, 16, 16, 768, bound), b"sizes"),
                           ((RGB8, 1, 16, 16, 768, bound - 1), b"bound"), ((RGB8, 1, 16, 16, 767, bound), b"stride"),
                           ((GRAY16, 1, 16, 16, 513, lib.cs_png_bound(GRAY16, 16, 16)), b"stride")):
            assert _host_call(lib, p, *args, flags) == _lib.CS_ERR_BAD_ARG, (args, flags)
            assert word in lib.cs_last_error(), (args, flags, lib.cs_last_error())
        assert _host_call(lib, p, RGB8, 1, 4097, 16, 4097 * 48, 1 << 30, flags) == _lib.CS_ERR_UNSUPPORTED
        assert lib.cs_op_png_encode_ex(None, RGB8, 1, 16, 16, 768, p, bound, p, p, None, flags) == _lib.CS_ERR_BAD_ARG


@pytest.mark.parametrize("kind", [GRAY16, RGB8])
@pytest.mark.parametrize("h,w", [(1, 1), (14, 14), (75, 91), (518, 518), (1036, 1036)])
def test_bound_and_workspace_serve_all_four_flag_values(kind, h, w):
    """The two size functions take no flags: the slot that is one byte short of the bound is refused, and the bound itself passes the size
    check, with every flags value alike (the next complaint is the null pixels pointer)."""
    lib = _lib.load()
    dummy = (C.c_uint8 * 64)()
    p = C.cast(dummy, C.c_void_p)
    bound, stride = lib.cs_png_bound(kind, h, w), h * row_bytes(kind, w)
    assert filtered_size(kind, h, w) <= bound and lib.cs_png_workspace_bytes(kind, 3, h, w) == 3 * lib.cs_png_workspace_bytes(kind, 1, h, w)
    for flags in (0, 1, 2, 3):
        assert _host_call(lib, p, kind, 1, h, w, stride, bound - 1, flags) == _lib.CS_ERR_BAD_ARG and b"bound" in lib.cs_last_error()
        assert lib.cs_op_png_encode_ex(None, kind, 1, h, w, stride, p, bound, p, p, None, flags) == _lib.CS_ERR_BAD_ARG
        assert b"null" in lib.cs_last_error()
    hdr = open(os.path.join(REPO, "include", "crossscore_hip.h")).read()
    assert "hold for every flags value" in hdr


def test_png_compression_key_is_validated():
    from crossscore_amd.writers import PNG_COMPRESSIONS, PngEncoder, png_compression_choice

    assert PNG_COMPRESSIONS == {"fast": 0, "compact": 3}
    for name in ("default_predict", "default_test"):
        assert png_compression_choice(load_config(name)) == "fast"
        assert png_compression_choice(load_config(name, ["this_main.png_compression=compact"])) == "compact"
        with pytest.raises(ValueError, match="fast | compact"):
            png_compression_choice(load_config(name, ["this_main.png_compression=best"]))
    cfg = load_config("default_predict")
    del cfg.this_main["png_compression"]  # a config file written before the key existed
    assert png_compression_choice(cfg) == "fast"
    assert PngEncoder().flags == 0 and PngEncoder("fast").flags == 0 and PngEncoder(compression="compact").flags == 3
    with pytest.raises(ValueError, match="fast | compact"):
        PngEncoder("best")


# ----------------------------------------------------------------------------------------------------------------- GPU
def _to_dev(imgs, kind):
    a = np.ascontiguousarray(imgs)
    return torch.from_numpy(a.view(np.int16) if kind == GRAY16 else a).cuda()


def _encode_ex(imgs: np.ndarray, kind: int, flags: int, extra_slot: int = 0):
    """cs_op_png_encode_ex itself on a (I, ...) host array: (files, lengths, bound, tails); the slots are pre-filled with FILL."""
    lib = _lib.load()
    pixels = _to_dev(imgs, kind)
    I, H, W = (int(v) for v in pixels.shape[:3])
    bound = lib.cs_png_bound(kind, H, W)
    slot = bound + extra_slot
    out = torch.full((I, slot), FILL, dtype=torch.uint8, device="cuda")
    lengths = torch.zeros((I,), dtype=torch.int32, device="cuda")
    work = torch.empty((lib.cs_png_workspace_bytes(kind, I, H, W),), dtype=torch.uint8, device="cuda")
    _lib.check(lib.cs_op_png_encode_ex(C.c_void_p(pixels.data_ptr()), kind, I, H, W, H * row_bytes(kind, W), C.c_void_p(out.data_ptr()), slot,
                                       C.c_void_p(lengths.data_ptr()), C.c_void_p(work.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream),
                                       flags))
    torch.cuda.synchronize()
    ln = lengths.cpu().numpy()
    o = out.cpu().numpy()
    assert (ln > 0).all(), ln
    return [o[i, :ln[i]].tobytes() for i in range(I)], ln, bound, [o[i, ln[i]:] for i in range(I)]


def _idat(data: bytes) -> bytes:
    return b"".join(p for t, p in parse_chunks(data) if t == b"IDAT")


def _stream(data: bytes) -> bytes:
    return zlib.decompress(_idat(data))


def _first_btype(data: bytes) -> int:
    """BTYPE of the first deflate block: bits 1-2 of the byte behind the two-byte zlib header."""
    return (_idat(data)[2] >> 1) & 3


@functools.lru_cache(maxsize=None)
def _images(kind, h, w):
    return contents(kind, h, w)


@functools.lru_cache(maxsize=None)
def _plain_lengths(kind, h, w):
    """Lengths of the flags-0 files of _images(kind, h, w), validated once."""
    files, ln, _, _ = _encode_ex(_images(kind, h, w), kind, 0)
    for i in range(4):
        check_png(files[i], _images(kind, h, w)[i], kind)
    return [len(f) for f in files]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [GRAY16, RGB8])
def test_flags_zero_is_the_old_encoder_byte_for_byte(kind):
    imgs = _images(kind, 75, 91)
    old, _, _ = encode_raw(_to_dev(imgs, kind), kind)
    new, _, _, _ = _encode_ex(imgs, kind, 0)
    assert old == new


SIZES = [(1, 1), (1, 7), (14, 14), (75, 91), (150, 201)]
CASES = [(k, h, w) for k in (GRAY16, RGB8) for h, w in SIZES] + [(GRAY16, 120, 91)]  # 120 x 91 gray16: 21 960 filtered bytes, a row across the boundary


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("kind,h,w", CASES)
def test_files_are_valid_pixel_exact_and_never_larger(kind, h, w, flags):
    imgs = _images(kind, h, w)
    files, ln, bound, tails = _encode_ex(imgs, kind, flags, extra_slot=37)  # an oversized, odd-sized slot
    plain = _plain_lengths(kind, h, w)
    print(f"kind {kind} {h}x{w} flags {flags}: bound {bound}, raw {h * row_bytes(kind, w)}, lengths {ln.tolist()}, flags 0 {plain}")
    for i, name in enumerate(CONTENT_NAMES):
        assert ln[i] <= bound, (name, ln[i], bound)
        assert (tails[i] == FILL).all(), name  # nothing written behind the file
        check_png(files[i], imgs[i], kind)
        if flags == DYNAMIC:  # Sub kept: the per-segment choice includes the flags-0 form, so this is a condition, not a measurement
            assert ln[i] <= plain[i], (name, ln[i], plain[i])


# ---- the filter rule, restated
def filter_choice(raw: np.ndarray, bpp: int) -> np.ndarray:
    """Filter type per row of (h, rb) raw bytes: the smallest sum of min(f, 256 - f) over the row's filtered bytes, ties to the lowest type."""
    h, rb = raw.shape
    out = np.zeros(h, np.int64)
    prev = np.zeros(rb, np.int64)
    for y in range(h):
        x = raw[y].astype(np.int64)
        a = np.concatenate([np.zeros(bpp, np.int64), x[:rb - bpp]])
        b = prev
        c = np.concatenate([np.zeros(bpp, np.int64), prev[:rb - bpp]])
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        scores = []
        for pred in (0, a, b, (a + b) >> 1, paeth):
            f = (x - pred) & 255
            scores.append(int(np.minimum(f, 256 - f).sum()))
        out[y] = int(np.argmin(scores))  # the first minimum
        prev = x
    return out


def _band_image(kind, h, w, seed):
    """Five bands of rows: sparse bytes, a ramp, one noise row repeated, two bands of smooth sinusoids with sigma-3 noise -> image, raw bytes."""
    rng = np.random.Generator(np.random.PCG64(seed))
    bpp = 2 if kind == GRAY16 else 3
    rb = w * bpp
    raw = np.zeros((h, rb), np.uint8)
    e = [h * k // 5 for k in range(6)]
    raw[e[0]:e[1]] = np.where(rng.random((e[1] - e[0], rb)) < 0.1, rng.integers(1, 4, size=(e[1] - e[0], rb)), 0)
    ys = np.arange(e[1], e[2])[:, None]
    raw[e[1]:e[2]] = ((np.arange(rb) // bpp) * 3 + (np.arange(rb) % bpp) * 31 + ys * 40) % 256  # 3 a pixel along the row, 40 a row
    raw[e[2]:e[3]] = rng.integers(0, 256, size=rb)
    yy, xx = np.mgrid[0:h, 0:rb]
    px, ch = xx // bpp, xx % bpp
    for (lo, hi), (amp, fx, fy) in (((e[3], e[4]), (60.0, 9.0, 2.5)), ((e[4], e[5]), (25.0, 45.0, 38.0))):
        s = 128 + amp * np.sin(px / fx + ch) * np.cos(yy / fy) + 0.5 * amp * np.sin((px + yy) / (fx + 4.0)) + rng.normal(0, 3, size=(h, rb))
        raw[lo:hi] = np.clip(np.round(s), 0, 255).astype(np.uint8)[lo:hi]
    img = raw.view(">u2").astype(np.uint16).reshape(h, w) if kind == GRAY16 else raw.reshape(h, w, 3)
    return np.ascontiguousarray(img), raw


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [2, 3])
@pytest.mark.parametrize("kind,h,w", [(RGB8, 75, 91), (GRAY16, 120, 91)])
def test_filter_type_of_every_row_follows_the_rule(kind, h, w, flags):
    img, raw = _band_image(kind, h, w, 5)
    want = filter_choice(raw, 2 if kind == GRAY16 else 3)
    counts = np.bincount(want, minlength=5)
    print(f"kind {kind} {h}x{w}: rows per filter type by the rule {counts.tolist()}")
    assert (counts > 0).all(), counts  # the inputs cover all five types
    files, _, _, _ = _encode_ex(img[None], kind, flags)
    check_png(files[0], img, kind)
    got = np.frombuffer(_stream(files[0]), np.uint8).reshape(h, 1 + raw.shape[1])[:, 0]
    assert np.array_equal(got, want), np.nonzero(got != want)[0]


# ---- code construction
def _huffman_depth(counts, deepest: bool):
    """Depth of an unrestricted Huffman tree of the positive counts; among equal weights the shallowest (or the deepest) subtrees merge first."""
    sign = -1 if deepest else 1
    heap = [(int(c), 0) for c in counts if c > 0]
    heapq.heapify(heap)
    while len(heap) > 1:
        (c1, d1), (c2, d2) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (c1 + c2, sign * (max(sign * d1, sign * d2) + 1)))
    return sign * heap[0][1]


@pytest.mark.gpu
def test_skewed_counts_need_the_length_limit():
    """Sub-filtered bytes with Fibonacci counts: the unrestricted Huffman tree is deeper than 15, the emitted code must still be complete
    (zlib's inflate rejects over-subscribed and incomplete literal/length codes).  The counts 1, 1, 2, 3, ... 6 765 (sum 17 710) are those of
    the segment's symbols: one of the 1s is the end-of-block symbol and the 34 is the filter byte of the 34 rows, the others are pixel values;
    the most frequent value is cut to the segment.  S(k) = c(0) + ... + c(k) = c(k + 2) - 1, so the merged node and the next leaf are always
    the two smallest weights: the tree is a chain whatever way equal weights are ordered."""
    h, w = 34, 160  # 34 * 481 = 16 354 filtered bytes: one segment
    n = h * w * 3
    rng = np.random.Generator(np.random.PCG64(9))
    fib = [1, 1]
    while fib[-1] < 6765:
        fib.append(fib[-1] + fib[-2])
    assert sum(fib) == 17710 and h in fib
    counts = [c for c in fib[1:] if c != h]
    counts[-1] += n - sum(counts)
    assert counts[-1] > counts[-2]
    values = rng.permutation(np.arange(2, 256))[:len(counts)]
    seq = rng.permutation(np.concatenate([np.full(c, v, np.uint8) for c, v in zip(counts, values)]))
    img = np.cumsum(seq.reshape(h, w, 3).astype(np.int64), axis=1).astype(np.uint8)  # prefix sums mod 256 per channel: Sub gives seq back
    files, _, _, _ = _encode_ex(img[None], RGB8, DYNAMIC)
    check_png(files[0], img, RGB8)
    stream = np.frombuffer(_stream(files[0]), np.uint8)
    assert np.array_equal(stream.reshape(h, 1 + 3 * w)[:, 1:].reshape(-1), seq)
    hist = list(np.bincount(stream, minlength=256)) + [1]  # with the end-of-block symbol
    shallow, deep = _huffman_depth(hist, False), _huffman_depth(hist, True)
    print(f"unrestricted Huffman depth of the segment's bytes {shallow} .. {deep}; file {len(files[0])} bytes of {len(stream)}")
    assert shallow > 15
    assert _first_btype(files[0]) == 2  # a dynamic block


def _long_match_images():
    rng = np.random.Generator(np.random.PCG64(33))
    a = rng.integers(0, 256, size=(40, 137, 3), dtype=np.uint8)
    a[33] = a[1]  # 32 rows of 412 filtered bytes back: distance 13 184
    b = rng.integers(0, 256, size=(2, 2731, 3), dtype=np.uint8)
    b[1] = b[0]   # one row of 8 194 filtered bytes back: the matcher's row candidate, length-258 matches all along the segment's second half
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_long_far_matches_between_rare_symbols(which):
    """Matches of length 258 at distances above 8 192 in a dynamic code: up to 48 bits per token."""
    img = _long_match_images()[which]
    plain, _, _, _ = _encode_ex(img[None], RGB8, 0)
    files, _, _, _ = _encode_ex(img[None], RGB8, DYNAMIC)
    check_png(plain[0], img, RGB8)
    check_png(files[0], img, RGB8)
    print(f"{img.shape}: flags 0 {len(plain[0])} bytes, flags 1 {len(files[0])} bytes")
    assert len(files[0]) < len(plain[0])


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("kind", [GRAY16, RGB8])
def test_degenerate_alphabets(kind, flags):
    bpp = 2 if kind == GRAY16 else 3

    def as_img(raw, h, w):
        raw = np.ascontiguousarray(raw.astype(np.uint8).reshape(h, w * bpp))
        return np.ascontiguousarray(raw.view(">u2").astype(np.uint16).reshape(h, w) if kind == GRAY16 else raw.reshape(h, w, 3))

    const = _images(kind, 75, 91)[0]                      # all matches, one distance code
    period = 2 if kind == RGB8 else 3                      # two byte values whose period does not divide the pixel
    alt = as_img(np.where(np.arange(75 * 91 * bpp) % period == 0, 0x11, 0xEE), 75, 91)
    one = as_img(np.array([7] * bpp), 1, 1)               # a 1 x 1 image: 1 + bpp filtered bytes
    zero = as_img(np.zeros(bpp), 1, 1)
    two = as_img(np.arange(2 * bpp) * 37 + 1, 1, 2)
    for name, img in (("constant", const), ("alternating", alt), ("1x1", one), ("1x1 zero", zero), ("1x2", two)):
        files, ln, bound, _ = _encode_ex(img[None], kind, flags)
        assert ln[0] <= bound, name
        check_png(files[0], img, kind)
        plain, _, _, _ = _encode_ex(img[None], kind, 0)
        if flags == DYNAMIC:
            assert len(files[0]) <= len(plain[0]), name
    files, _, _, _ = _encode_ex(const[None], kind, flags)
    assert len(files[0]) < filtered_size(kind, 75, 91) // 10  # the matches are really emitted


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [GRAY16, RGB8])
def test_bytes_do_not_depend_on_the_batch(kind):
    """Image k of a batch of 8 = the same image alone = the same image at another position among other images (flags 3)."""
    h, w = 75, 91
    parts = [_images(kind, h, w).copy(), _images(kind, h, w)[::-1].copy()]
    parts[1][0] = np.roll(parts[1][0], 5, axis=1)  # eight different images: the reversed contents are score map, noise, ramp, constant
    parts[1][1] = np.roll(parts[1][1], 7, axis=1)
    parts[1][2] = np.roll(parts[1][2], 9, axis=1)
    parts[1][3][10:20, 30:50] = ~parts[1][3][10:20, 30:50]
    imgs = np.concatenate(parts)
    assert len({imgs[k].tobytes() for k in range(8)}) == 8
    batch, _, _, _ = _encode_ex(imgs, kind, 3)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    shuffled, _, _, _ = _encode_ex(imgs[perm], kind, 3)
    for k in range(8):
        alone, _, _, _ = _encode_ex(imgs[k:k + 1], kind, 3)
        assert alone[0] == batch[k], k
        assert shuffled[perm.index(k)] == batch[k], k


# ---- size against an independent encoder
def _synthetic_photo(h, w, seed=17):
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = [128 + 70 * np.sin(xx / (31.0 + 9 * c) + c) * np.cos(yy / (27.0 - 5 * c)) + 35 * np.sin((xx + 2 * yy) / (53.0 + 7 * c)) for c in range(3)]
    return np.clip(np.round(np.stack(chans, -1) + rng.normal(0, 2.5, size=(h, w, 3))), 0, 255).astype(np.uint8)


HEADER_ALLOWANCE = 288  # bytes: a header that spells out all 316 code lengths without repeat symbols, 14 + 19 * 3 + 316 * 7 bits


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [1, 3])
@pytest.mark.parametrize("name", ["photo", "gray16 map", "turbo map"])
def test_size_against_huffman_only_zlib_per_segment(name, flags):
    """The bar is zlib itself, Huffman-only with memLevel 9, on the produced file's own filtered stream cut at the encoder's 16 384 bytes;
    the literals-only candidate with minimum-redundancy lengths meets it by construction, up to the header allowance."""
    h, w = 150, 201
    kind = GRAY16 if name == "gray16 map" else RGB8
    img = _synthetic_photo(h, w) if name == "photo" else _images(kind, h, w)[3]
    files, _, _, _ = _encode_ex(img[None], kind, flags)
    check_png(files[0], img, kind)
    stream = _stream(files[0])
    bar = 0
    pieces = [stream[o:o + SEG] for o in range(0, len(stream), SEG)]
    for piece in pieces:
        co = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        bar += len(co.compress(piece) + co.flush()) + 5 + HEADER_ALLOWANCE
    got = len(_idat(files[0]))
    plain, _, _, _ = _encode_ex(img[None], kind, 0)
    print(f"{name} flags {flags}: {len(pieces)} segments, raw {len(stream)}, IDAT payload {got}, bar {bar} (of it allowance {len(pieces) * (5 + HEADER_ALLOWANCE)}), "
          f"flags 0 payload {len(_idat(plain[0]))}")
    assert got <= bar
