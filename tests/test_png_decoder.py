"""The device PNG decoder (csrc/pngdec.hip, cs_png_probe / cs_op_png_decode, decode.ImageDecoder): every decoded image equals, bit for bit, what
read_image_u8 / read_metric_map_u16 make of PIL's array for the same bytes; hand-made streams are checked against zlib.decompress plus the
un-filter of tests/png_files.py.  No tolerances.  Malformed files end with their documented status beside good files that still decode."""
import ctypes as C
import io
import os
import re
import struct
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
from guard import guarded  # noqa: E402
from png_files import GRAY16, RGB8, SIGNATURE, chunk, encode_raw, ihdr, image_of, interlaced_png, pil_png, unfilter  # noqa: E402

NEW_SYMBOLS = ("cs_png_probe", "cs_png_decode_workspace_bytes", "cs_op_png_decode")
# (colour type, bit depth) -> (bytes per pixel, output kind)
FORMS = {"gray8": (0, 8, 1, RGB8), "gray16": (0, 16, 2, GRAY16), "rgb": (2, 8, 3, RGB8), "rgba": (6, 8, 4, RGB8)}
SIZES = [(1, 1), (1, 7), (7, 1), (14, 14), (75, 91)]


# ------------------------------------------------------------------------------------------------------------ a PNG writer
def split_at(data: bytes, cuts):
    """data cut at the byte positions `cuts` (sorted; repeated positions give empty pieces)"""
    pieces, a = [], 0
    for c in list(cuts) + [len(data)]:
        c = min(max(c, a), len(data))
        pieces.append(data[a:c])
        a = c
    return pieces


def png_file(h, w, form, zstream: bytes, cuts=(), front=()) -> bytes:
    ct, depth = FORMS[form][:2]
    out = SIGNATURE + ihdr(h, w, ct, depth) + b"".join(chunk(t, p) for t, p in front)
    out += b"".join(chunk(b"IDAT", p) for p in split_at(zstream, cuts))
    return out + chunk(b"IEND", b"")


def apply_filters(raw: np.ndarray, bpp: int, ftypes) -> bytes:
    """raw (h, rb) uint8 row bytes -> the filtered stream with filter type ftypes[y] on row y"""
    h, rb = raw.shape
    out = np.zeros((h, 1 + rb), np.uint8)
    z = np.zeros(rb, np.int64)
    for y in range(h):
        cur = raw[y].astype(np.int64)
        up = raw[y - 1].astype(np.int64) if y else z
        left = np.concatenate([np.zeros(min(bpp, rb), np.int64), cur[:-bpp]])[:rb] if rb > bpp else np.zeros(rb, np.int64)
        ul = np.concatenate([np.zeros(min(bpp, rb), np.int64), up[:-bpp]])[:rb] if rb > bpp else np.zeros(rb, np.int64)
        ft = int(ftypes[y])
        if ft == 0:
            pred = z
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (left + up) // 2
        else:
            p = left + up - ul
            pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
        out[y, 0] = ft
        out[y, 1:] = (cur - pred) & 255
    return out.tobytes()


def raw_rows(img: np.ndarray, form: str) -> np.ndarray:
    """the file's row bytes of an image: (h, w) uint8 / uint16, (h, w, 3) or (h, w, 4) uint8"""
    h = img.shape[0]
    if form == "gray16":
        return img.astype(">u2").view(np.uint8).reshape(h, -1)
    return np.ascontiguousarray(img).reshape(h, -1)


def deflate(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    return c.compress(data) + c.flush()


def write_png(img, form, ftypes=None, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, cuts=(), front=()) -> bytes:
    raw = raw_rows(img, form)
    h, w = img.shape[:2]
    ftypes = [0] * h if ftypes is None else ftypes
    return png_file(h, w, form, deflate(apply_filters(raw, FORMS[form][2], ftypes), level, strategy), cuts, front)


def expected(data: bytes, kind: int) -> np.ndarray:
    """the host readers' array for a file's bytes (they take anything PIL opens)"""
    from crossscore_amd.decode import read_image_u8, read_metric_map_u16

    return (read_metric_map_u16 if kind == GRAY16 else read_image_u8)(io.BytesIO(data))


def smooth_noise(rng, h, w):
    y, x = np.meshgrid(np.linspace(0, 3, h), np.linspace(0, 4, w), indexing="ij")
    base = np.stack([np.sin(y + c) * np.cos(x - c) for c in range(3)], axis=-1) * 100 + 128
    return np.clip(base + rng.normal(0, 8, size=(h, w, 3)), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------- fixed-Huffman tokens
class FixedBlock:
    """One final fixed-Huffman block from tokens, wrapped as a zlib stream (78 01 ... Adler-32 of `payload`)."""
    LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
    DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
    DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()
        self.bits(1, 1)  # BFINAL
        self.bits(1, 2)  # BTYPE = 01

    def bits(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):  # Huffman codes go in most significant bit first
        self.bits(int(format(c, f"0{n}b")[::-1], 2), n)

    def sym(self, s):
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def lit(self, b):
        self.sym(int(b))

    def match(self, length, dist):
        i = max(k for k in range(29) if self.LBASE[k] <= length) if length < 258 else 28
        self.sym(257 + i)
        self.bits(length - self.LBASE[i], self.LEXT[i])
        j = max(k for k in range(30) if self.DBASE[k] <= dist)
        self.code(j, 5)
        self.bits(dist - self.DBASE[j], self.DEXT[j])

    def finish(self, payload=None) -> bytes:
        self.sym(256)
        if self.n:
            self.bits(0, 8 - self.n)
        body = bytes(self.out)
        if payload is None:
            payload = zlib.decompressobj(-15).decompress(body)
        return b"\x78\x01" + body + struct.pack(">I", zlib.adler32(payload))


def block_types(deflate_pieces):
    """BTYPE of the first block of each byte-aligned piece of a raw deflate stream (each piece starts a block at its first bit)"""
    return [(p[0] >> 1) & 3 for p in deflate_pieces if p]


def mixed_block_stream(data: bytes):
    """One zlib stream whose pieces were compressed with different strategies and cut at Z_FULL_FLUSH points: stored, fixed and dynamic blocks."""
    n = len(data)
    parts = [(data[:n // 3], 0, zlib.Z_DEFAULT_STRATEGY), (data[n // 3:2 * n // 3], 6, zlib.Z_FIXED), (data[2 * n // 3:], 6, zlib.Z_DEFAULT_STRATEGY)]
    pieces = []
    for k, (d, level, strategy) in enumerate(parts):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        pieces.append(c.compress(d) + c.flush(zlib.Z_FINISH if k == len(parts) - 1 else zlib.Z_FULL_FLUSH))
    return b"\x78\x01" + b"".join(pieces) + struct.pack(">I", zlib.adler32(data)), pieces


# ----------------------------------------------------------------------------------------------------------------- CPU
def probe(data: bytes, max_spans=None):
    """(rc, info, spans) of cs_png_probe"""
    lib = _lib.load()
    info = _lib.CsPngInfo()
    rc = lib.cs_png_probe(data, len(data), C.byref(info), None, 0)
    if rc != _lib.CS_OK:
        return rc, info, None
    n = info.num_idat if max_spans is None else max_spans
    spans = np.zeros((max(n, 1), 2), dtype=np.uint32)
    rc = lib.cs_png_probe(data, len(data), C.byref(info), C.c_void_p(spans.ctypes.data), n)
    return rc, info, spans[:n]


def test_new_symbols_declared_listed_and_exported():
    hdr = open(os.path.join(REPO, "include", "crossscore_hip.h")).read()
    declared = set(re.findall(r"\b(cs_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "cs_png_info" in hdr and "cs_png_span" in hdr and "CS_PNGDEC_BAD_CRC" in hdr
    assert "pngdec.hip" in __import__("crossscore_amd.build", fromlist=["SOURCES"]).SOURCES


@pytest.mark.parametrize("n_idat", [1, 4, 300])
@pytest.mark.parametrize("form", list(FORMS))
def test_probe_reads_size_kind_and_spans(form, n_idat):
    rng = np.random.default_rng(1)
    img = image_of(rng, 40, 30, form)
    z = deflate(apply_filters(raw_rows(img, form), FORMS[form][2], [0] * 40), 0)
    assert len(z) > 300
    cuts = sorted(rng.choice(np.arange(1, len(z)), size=n_idat - 1, replace=False).tolist())
    front = [(b"gAMA", struct.pack(">I", 45455)), (b"pHYs", struct.pack(">IIB", 2835, 2835, 1)), (b"tEXt", b"Comment\0made by a test")]
    for fr in ((), front):
        data = png_file(40, 30, form, z, cuts, fr)
        rc, info, spans = probe(data)
        assert rc == _lib.CS_OK, _lib.last_error()
        assert (info.height, info.width, info.color_type, info.bit_depth, info.interlace) == (40, 30) + FORMS[form][:2] + (0,)
        assert info.kind == FORMS[form][3] and info.num_idat == n_idat and info.idat_bytes == len(z)
        assert b"".join(data[o:o + n] for o, n in spans.tolist()) == z
        for o, n in spans.tolist():
            assert data[o - 4:o] == b"IDAT" and o + n + 4 <= len(data)
        if n_idat > 1:  # a span table that is too short is refused, and the count is reported
            rc, info, _ = probe(data, max_spans=n_idat - 1)
            assert rc == _lib.CS_ERR_BAD_ARG and info.num_idat == n_idat


def test_probe_says_what_is_not_built():
    from PIL import Image

    rng = np.random.default_rng(2)
    rgb = image_of(rng, 12, 10, "rgb")
    good = pil_png(rgb)
    assert probe(good)[0] == _lib.CS_OK
    cases = {}
    inter = bytearray(good)
    inter[28] = 1  # IHDR's interlace byte (the CRC is the device's business, not the probe's)
    cases["interlaced"] = bytes(inter)
    buf = io.BytesIO()
    Image.fromarray(rgb).convert("P").save(buf, format="PNG")
    cases["palette"] = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(rgb).convert("LA").save(buf, format="PNG")
    cases["gray+alpha"] = buf.getvalue()
    z = deflate(b"\0" * (12 * (1 + 10 * 6)))
    cases["rgb16"] = SIGNATURE + ihdr(12, 10, 2, 16) + chunk(b"IDAT", z) + chunk(b"IEND", b"")
    buf = io.BytesIO()
    Image.fromarray(rgb).convert("1").save(buf, format="PNG")
    cases["1-bit"] = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG")
    cases["jpeg"] = buf.getvalue()
    cases["too large"] = SIGNATURE + ihdr(16, 4097, 2, 8) + chunk(b"IDAT", z) + chunk(b"IEND", b"")
    for name, data in cases.items():
        rc, info, _ = probe(data)
        assert rc == _lib.CS_ERR_UNSUPPORTED and info.kind == -1, (name, rc, _lib.last_error())
        assert len(_lib.last_error()) > 10
    # framing that runs past the end
    cut = bytearray(good)
    cut[33:37] = struct.pack(">I", len(good))  # the first chunk behind IHDR claims more bytes than the file has
    for name, data in (("chunk past the end", bytes(cut)), ("truncated signature", good[:5]), ("no IEND", good[:-12]), ("inside a chunk", good[:60])):
        rc, _, _ = probe(data)
        assert rc == _lib.CS_ERR_BAD_ARG, (name, rc, _lib.last_error())
        assert b"png_probe" in _lib.load().cs_last_error()


def test_workspace_is_host_arithmetic():
    lib = _lib.load()
    f = lib.cs_png_decode_workspace_bytes
    last = 0
    for i in (1, 2, 3, 8, 64, 65):
        cur = f(RGB8, i, 75, 91, 1000 * i)
        assert cur > last and cur >= i * 75 * (1 + 4 * 91) + 1000 * i
        last = cur
    assert f(RGB8, 4, 75, 91, 5000) > f(RGB8, 4, 75, 91, 4000)
    assert f(GRAY16, 1, 4096, 4096, 1) > 0
    for args in ((2, 1, 8, 8, 100), (-1, 1, 8, 8, 100), (RGB8, 1, 4097, 8, 100), (RGB8, 1, 8, 4097, 100), (RGB8, 0, 8, 8, 100), (RGB8, 1, 0, 8, 100)):
        assert f(*args) == 0, args


def test_png_decode_rejects_bad_arguments_on_the_host():
    """CS_ERR_BAD_ARG / CS_ERR_UNSUPPORTED with a message before any device call (this runs without a GPU)."""
    lib = _lib.load()
    dummy = (C.c_uint8 * 64)()
    p = C.cast(dummy, C.c_void_p)

    def call(kind=RGB8, i=1, h=16, w=16, stride=768, total=100, files=p, pixels=p, status=p, work=p, spans=p):
        return lib.cs_op_png_decode(files, p, p, spans, p, total, i, kind, h, w, pixels, stride, status, work, None)

    for kw, word in ((dict(kind=7), b"kind"), (dict(w=0), b"sizes"), (dict(i=0), b"sizes"), (dict(i=70000), b"sizes"), (dict(stride=767), b"stride"),
                     (dict(kind=GRAY16, stride=513), b"stride"), (dict(total=0), b"file bytes"), (dict(files=None), b"null"), (dict(pixels=None), b"null"),
                     (dict(status=None), b"null"), (dict(work=None), b"null"), (dict(spans=None), b"null")):
        assert call(**kw) == _lib.CS_ERR_BAD_ARG, kw
        assert word in lib.cs_last_error(), (kw, lib.cs_last_error())
    assert call(h=4097, stride=4097 * 48) == _lib.CS_ERR_UNSUPPORTED and b"4096" in lib.cs_last_error()
    odd = C.c_void_p(C.addressof(dummy) + 16 + 1)
    assert call(kind=GRAY16, stride=512, pixels=odd) == _lib.CS_ERR_BAD_ARG and b"aligned" in lib.cs_last_error()
    assert call(work=odd) == _lib.CS_ERR_BAD_ARG and b"aligned" in lib.cs_last_error()


def test_png_decoder_keys_are_validated():
    from crossscore_amd.decode import png_decode_window_choice, png_decoder_choice

    for name in ("default_predict", "default_test"):
        assert png_decoder_choice(load_config(name)) == "host"
        assert png_decode_window_choice(load_config(name)) == 64
        assert png_decoder_choice(load_config(name, ["this_main.png_decoder=gpu"])) == "gpu"
        assert png_decode_window_choice(load_config(name, ["this_main.png_decode_window=3"])) == 3
        with pytest.raises(ValueError):
            png_decoder_choice(load_config(name, ["this_main.png_decoder=pil"]))
        with pytest.raises(ValueError):
            png_decode_window_choice(load_config(name, ["this_main.png_decode_window=0"]))
        cfg = load_config(name)
        del cfg.this_main["png_decoder"]  # a config file written before the keys existed
        del cfg.this_main["png_decode_window"]
        assert png_decoder_choice(cfg) == "host" and png_decode_window_choice(cfg) == 64


def test_the_test_writers_agree_with_pil_and_zlib():
    """Guards the guard: the module's own PNG writer and token writer produce what PIL and zlib read back."""
    rng = np.random.default_rng(3)
    for form in FORMS:
        img = image_of(rng, 9, 11, form)
        data = write_png(img, form, ftypes=[y % 5 for y in range(9)], cuts=(1, 2, 3, 3, 40))
        want = img if form == "gray16" else np.repeat(img[:, :, None], 3, 2) if form == "gray8" else img[:, :, :3]
        assert np.array_equal(expected(data, FORMS[form][3]), want), form
    fb = FixedBlock()
    for b in b"abcabcabd":
        fb.lit(b)
    fb.match(258, 3)
    fb.match(5, 1)
    assert zlib.decompress(fb.finish()) == b"abcabcabd" + (b"abd" * 86) + b"ddddd"
    z, pieces = mixed_block_stream(bytes(rng.integers(0, 64, size=6000, dtype=np.uint8)))
    assert set(block_types(pieces)) == {0, 1, 2} and len(zlib.decompress(z)) == 6000


# ----------------------------------------------------------------------------------------------------------------- GPU
class Decode:
    """cs_op_png_decode on files of one size and kind, inside guard bands: pixels, status and workspace."""

    def __init__(self, files, kind, h, w, pad=0, work=None, spans_of=None):
        lib = _lib.load()
        n = len(files)
        tables = []
        for f in files:
            rc, info, spans = probe(f) if spans_of is None else spans_of(f)
            assert rc == _lib.CS_OK, _lib.last_error()
            tables.append(spans)
        lengths = np.array([len(f) for f in files], dtype=np.uint32)
        offsets = np.zeros(n, dtype=np.uint64)
        offsets[1:] = np.cumsum(lengths.astype(np.uint64))[:-1]
        span_off = np.zeros(n + 1, dtype=np.uint32)
        span_off[1:] = np.cumsum([len(t) for t in tables])
        total = int(lengths.sum())
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
        self.keep = [dev(np.frombuffer(b"".join(files), np.uint8)), dev(offsets), dev(lengths), dev(np.concatenate(tables)), dev(span_off)]
        es = 2 if kind == GRAY16 else 3
        self.stride = h * w * es + pad
        self.pix = guarded((n, h * w * es), torch.uint8, ld=self.stride, guard_rows=1)  # one image of sentinel before and behind
        self.status = guarded((n,), torch.int32, guard_rows=0)
        ws = lib.cs_png_decode_workspace_bytes(kind, n, h, w, total)
        assert ws > 0
        self.work = work if work is not None else guarded((ws,), torch.uint8, guard_rows=0)
        assert self.work.shape[0] >= ws
        _lib.check(lib.cs_op_png_decode(*(C.c_void_p(t.data_ptr()) for t in self.keep[:4]), C.c_void_p(self.keep[4].data_ptr()), total, n, kind, h, w,
                                        C.c_void_p(self.pix.view.data_ptr()), self.stride, C.c_void_p(self.status.view.data_ptr()),
                                        C.c_void_p(self.work.view.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        self.pix.check("pixels")
        self.status.check("status")
        self.work.check("workspace")
        self.st = self.status.view.cpu().numpy()
        raw = self.pix.view.cpu().numpy()
        self.images = [raw[i].view(np.uint16).reshape(h, w) if kind == GRAY16 else raw[i].reshape(h, w, 3) for i in range(n)]


def check_files(files, kind, h, w, names=None, want=None, **kw):
    """every file decodes with status 0 to the host readers' array (or to want[i])"""
    d = Decode(files, kind, h, w, **kw)
    for i, f in enumerate(files):
        name = names[i] if names else i
        assert d.st[i] == 0, (name, int(d.st[i]))
        ref = expected(f, kind) if want is None else want[i]
        assert d.images[i].dtype == ref.dtype and np.array_equal(d.images[i], ref), name
    return d


LEVELS = [("stored", 0, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED), ("level1", 1, zlib.Z_DEFAULT_STRATEGY), ("level6", 6, zlib.Z_DEFAULT_STRATEGY),
          ("level9", 9, zlib.Z_DEFAULT_STRATEGY), ("huffman", 6, zlib.Z_HUFFMAN_ONLY), ("rle", 6, zlib.Z_RLE), ("filtered", 6, zlib.Z_FILTERED)]


@pytest.mark.gpu
def test_block_types():
    """Stored, fixed and dynamic blocks from every zlib strategy, and one stream that holds all three."""
    rng = np.random.default_rng(10)
    h, w = 75, 91
    img = image_of(rng, h, w, "rgb")
    ft = [y % 5 for y in range(h)]
    files = [write_png(img, "rgb", ft, level, strategy) for _, level, strategy in LEVELS]
    names = [n for n, _, _ in LEVELS]
    z, pieces = mixed_block_stream(apply_filters(raw_rows(img, "rgb"), 3, ft))
    assert set(block_types(pieces)) == {0, 1, 2}
    files.append(png_file(h, w, "rgb", z))
    names.append("mixed")
    noise = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    files.append(write_png(noise, "rgb", [0] * h, 0))  # incompressible and stored
    names.append("stored noise")
    check_files(files, RGB8, h, w, names)


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("h,w", SIZES)
def test_filters(form, h, w):
    """Each filter type on every row, rows cycling 0-4, random types per row: one call per (form, size)."""
    rng = np.random.default_rng(h * 100 + w)
    img = image_of(rng, h, w, form)
    plans = [[t] * h for t in range(5)] + [[y % 5 for y in range(h)], rng.integers(0, 5, size=h).tolist(), rng.integers(0, 5, size=h).tolist()]
    files = [write_png(img, form, ft, 6 if k % 2 else 1) for k, ft in enumerate(plans)]
    kind = FORMS[form][3]
    d = check_files(files, kind, h, w, [str(p[:8]) for p in plans])
    # and against zlib + the encoder tests' un-filter, the reference of the hand-made streams
    bpp = FORMS[form][2]
    raw = unfilter(apply_filters(raw_rows(img, form), bpp, plans[6]), h, w * bpp, bpp)
    assert np.array_equal(raw, raw_rows(img, form))
    assert np.array_equal(d.images[6], expected(files[6], kind))


@pytest.mark.gpu
@pytest.mark.parametrize("optimize", [False, True])
def test_pil_written_content(optimize):
    rng = np.random.default_rng(20)
    h, w = 75, 91
    contents = {"constant": np.full((h, w, 3), 77, np.uint8),
                "ramp": np.broadcast_to((np.arange(w) * 255 // (w - 1)).astype(np.uint8)[None, :, None], (h, w, 3)).copy(),
                "noise": rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), "smooth+noise": smooth_noise(rng, h, w)}
    check_files([pil_png(v, optimize=optimize) for v in contents.values()], RGB8, h, w, list(contents))
    big = np.full((300, 300, 3), 9, np.uint8)  # 270 900 equal bytes: distance-1 runs of 258
    check_files([pil_png(big, optimize=optimize)], RGB8, 300, 300)
    maps = [rng.integers(0, 65536, size=(h, w)).astype(np.uint16), np.full((h, w), 65535, np.uint16),
            (np.arange(h * w).reshape(h, w) * 7 % 65536).astype(np.uint16)]
    check_files([pil_png(m, optimize=optimize) for m in maps], GRAY16, h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [GRAY16, RGB8])
@pytest.mark.parametrize("h,w", [(75, 91), (518, 686)])
def test_round_trip_with_the_device_encoder(kind, h, w):
    """cs_op_png_encode -> cs_op_png_decode: one IDAT chunk per 16-KiB segment, so this is also the many-chunk case."""

    rng = np.random.default_rng(30)
    if kind == GRAY16:
        imgs = np.stack([rng.integers(0, 65536, size=(h, w)).astype(np.uint16), (np.arange(h * w).reshape(h, w) % 65536).astype(np.uint16)])
        px = torch.from_numpy(imgs.view(np.int16)).cuda()
    else:
        imgs = np.stack([smooth_noise(rng, h, w), np.full((h, w, 3), 200, np.uint8)])
        px = torch.from_numpy(imgs).cuda()
    files, _, _ = encode_raw(px, kind)
    assert probe(files[0])[1].num_idat >= (h * w * (2 if kind == GRAY16 else 3)) // 16384
    check_files(files, kind, h, w, want=[imgs[0], imgs[1]])


@pytest.mark.gpu
def test_chunk_splits():
    """One dynamic-Huffman stream cut into IDAT chunks at awkward places; a stored stream cut inside LEN / NLEN."""
    rng = np.random.default_rng(40)
    h, w = 14, 14
    img = image_of(rng, h, w, "rgb")
    ft = [y % 5 for y in range(h)]
    z = deflate(apply_filters(raw_rows(img, "rgb"), 3, ft), 6)
    assert (z[2] >> 1) & 3 == 2  # a dynamic block
    z0 = deflate(apply_filters(raw_rows(img, "rgb"), 3, ft), 0)
    assert (z0[2] >> 1) & 3 == 0
    files = [png_file(h, w, "rgb", z, cuts) for cuts in (list(range(1, len(z))), [1], [2], [3], [1, 2, 3], [0, 0, 5, 5, 5, len(z), len(z)], [len(z) - 4], [len(z) - 1])]
    files += [png_file(h, w, "rgb", z0, cuts) for cuts in ([3], [4], [5], [6], [3, 4, 5, 6, 7], list(range(1, len(z0))))]
    assert probe(files[0])[1].num_idat == len(z)
    check_files(files, RGB8, h, w, want=[img] * len(files))


@pytest.mark.gpu
def test_window_of_32768_and_the_ring():
    """zlib never emits a distance above 32 506: a hand-made fixed-Huffman stream for a 127-wide, 260-high gray8 image (row pitch 128)."""
    rng = np.random.default_rng(50)
    h, w = 260, 127
    fb = FixedBlock()
    rows = rng.integers(0, 256, size=(256, 128), dtype=np.uint8)
    rows[:, 0] = 0  # filter type None
    for b in rows.reshape(-1):
        fb.lit(b)
    fb.match(100, 32768)  # row 256 = row 0, the farthest byte of the window
    fb.match(28, 32768)
    fb.lit(0)  # row 257: filter byte, then zeros to byte 2 of row 259 (distance 1, length 258)
    fb.match(258, 1)
    fb.match(125, 447)  # its source runs from byte 32 708 over 32 768: it wraps the ring
    z = fb.finish()
    stream = zlib.decompress(z)
    assert len(stream) == h * 128
    raw = unfilter(stream, h, w, 1)
    assert np.array_equal(raw[256], raw[0]) and not raw[257].any()
    want = np.repeat(raw[:, :, None], 3, 2)
    # a second file: matches of length 258 whose source wraps, at the largest distance, overlapping ones across the flush boundary
    fb2 = FixedBlock()
    for b in rows.reshape(-1)[:16300]:
        fb2.lit(b)
    pos, k = 16300, 0
    while pos + 258 <= h * 128:  # whole rows back, so that filter bytes stay filter bytes: overlapping, far, and the largest the position allows
        fb2.match(258, [128, 256, 384, 16256, min(pos // 128 * 128, 32768)][k % 5])
        pos, k = pos + 258, k + 1
    assert h * 128 - pos >= 3
    fb2.match(h * 128 - pos, 128)
    z2 = fb2.finish()
    stream2 = zlib.decompress(z2)
    assert len(stream2) == h * 128
    want2 = np.repeat(unfilter(stream2, h, w, 1)[:, :, None], 3, 2)
    check_files([png_file(h, w, "gray8", z), png_file(h, w, "gray8", z2, cuts=[7, 8, 9000])], RGB8, h, w, want=[want, want2])


@pytest.mark.gpu
def test_multi_window_image():
    """One PIL-written 518 x 686 smooth + noise image: about a megabyte of stream in 30-odd dynamic blocks."""
    rng = np.random.default_rng(60)
    data = pil_png(smooth_noise(rng, 518, 686))
    assert len(data) > 600_000
    check_files([data], RGB8, 518, 686)


def thirteen_files(rng, h, w):
    from PIL import Image

    rgb, rgba, gray = image_of(rng, h, w, "rgb"), image_of(rng, h, w, "rgba"), image_of(rng, h, w, "gray8")
    files = [pil_png(rgb), pil_png(rgba), pil_png(gray), pil_png(rgb, optimize=True), write_png(rgb, "rgb", [4] * h, 9), write_png(rgba, "rgba", [3] * h, 1),
             write_png(gray, "gray8", [y % 5 for y in range(h)], 6, zlib.Z_FIXED), write_png(rgb, "rgb", [1] * h, 0, cuts=[10, 20, 300]),
             write_png(rgba, "rgba", [2] * h, 6, zlib.Z_RLE, cuts=list(range(1, 200))), pil_png(smooth_noise(rng, h, w)),
             pil_png(np.zeros((h, w, 3), np.uint8)), write_png(gray, "gray8", [0] * h, 6, zlib.Z_HUFFMAN_ONLY), pil_png(rgb, compress_level=1)]
    assert len(files) == 13 and Image.open(io.BytesIO(files[1])).mode == "RGBA"
    return files


@pytest.mark.gpu
def test_one_call_many_files():
    """13 files of one size (RGB, RGBA, gray8; different writers and chunkings) in one call equal the same files decoded alone; a padded image
    stride; guard bands around the pixels, the status words and the workspace (checked inside Decode)."""
    rng = np.random.default_rng(70)
    h, w = 33, 47
    files = thirteen_files(rng, h, w)
    together = check_files(files, RGB8, h, w, pad=37)
    for i in (0, 1, 2, 8, 12):
        alone = check_files([files[i]], RGB8, h, w)
        assert np.array_equal(alone.images[0], together.images[i])
    maps = [rng.integers(0, 65536, size=(h, w)).astype(np.uint16) for _ in range(5)]
    check_files([pil_png(m) if k % 2 else write_png(m, "gray16", [k % 5] * h, 6, cuts=[5, 6]) for k, m in enumerate(maps)], GRAY16, h, w, pad=6, want=maps)


def _dynamic_block_with_oversubscribed_lengths() -> bytes:
    """BFINAL, BTYPE = 10, HLIT = HDIST = 0, HCLEN = 15: nineteen code-length code lengths of 1 (only two codes of one bit exist)"""
    acc, n = 0, 0
    for v, k in [(1, 1), (2, 2), (0, 5), (0, 5), (15, 4)] + [(1, 3)] * 19:
        acc |= v << n
        n += k
    body = acc.to_bytes((n + 7) // 8, "little") + b"\0" * 8
    return b"\x78\x01" + body + struct.pack(">I", 1)


@pytest.mark.gpu
def test_malformed_files_beside_good_ones():
    """Every malformed file ends with its documented status; the good files of the same call decode exactly; the guard bands hold; the next
    decode on the same workspace is exact."""
    rng = np.random.default_rng(80)
    h, w = 14, 14
    img = image_of(rng, h, w, "rgb")
    ft = [y % 5 for y in range(h)]
    good = write_png(img, "rgb", ft, 6)
    filtered = apply_filters(raw_rows(img, "rgb"), 3, ft)
    z = deflate(filtered, 6)
    S = _lib
    bad = {}
    flipped = bytearray(good)
    flipped[8 + 25 + 8 + 20] ^= 0x10  # inside the IDAT payload, CRC left alone
    bad["flipped payload byte"] = (bytes(flipped), {S.PNGDEC_BAD_CRC})
    structural = {S.PNGDEC_BAD_ADLER, S.PNGDEC_BAD_BLOCK_TYPE, S.PNGDEC_BAD_STORED_LEN, S.PNGDEC_BAD_CODE, S.PNGDEC_BAD_SYMBOL, S.PNGDEC_BAD_DISTANCE,
                  S.PNGDEC_STREAM_SHORT, S.PNGDEC_STREAM_LONG, S.PNGDEC_INPUT_EXHAUSTED}
    zc = bytearray(z)
    zc[len(z) // 2] ^= 0x04
    bad["corrupted stream, CRCs right"] = (png_file(h, w, "rgb", bytes(zc)), structural)
    za = bytearray(z)
    za[-1] ^= 1
    bad["wrong Adler-32"] = (png_file(h, w, "rgb", bytes(za)), {S.PNGDEC_BAD_ADLER})
    bad["stream cut short"] = (png_file(h, w, "rgb", z[:len(z) * 2 // 3]), {S.PNGDEC_INPUT_EXHAUSTED, S.PNGDEC_STREAM_SHORT} | structural)
    bad["Adler cut off"] = (png_file(h, w, "rgb", z[:-2]), {S.PNGDEC_INPUT_EXHAUSTED})
    bad["one row short"] = (png_file(h, w, "rgb", deflate(filtered[:-(1 + 3 * w)])), {S.PNGDEC_STREAM_SHORT})
    bad["one row too long"] = (png_file(h, w, "rgb", deflate(filtered + filtered[:1 + 3 * w])), {S.PNGDEC_STREAM_LONG})
    f5 = bytearray(filtered)
    f5[3 * (1 + 3 * w)] = 5
    bad["filter byte 5"] = (png_file(h, w, "rgb", deflate(bytes(f5))), {S.PNGDEC_BAD_FILTER})
    fb = FixedBlock()
    fb.lit(0)
    fb.lit(7)
    fb.match(3, 5)  # two bytes exist
    for _ in range(30):
        fb.lit(1)
    bad["distance before the start"] = (png_file(h, w, "rgb", fb.finish(payload=b"")), {S.PNGDEC_BAD_DISTANCE})
    bad["over-subscribed lengths"] = (png_file(h, w, "rgb", _dynamic_block_with_oversubscribed_lengths()), {S.PNGDEC_BAD_CODE})
    bad["reserved block type"] = (png_file(h, w, "rgb", b"\x78\x01\x07" + b"\0" * 8), {S.PNGDEC_BAD_BLOCK_TYPE})
    bad["stored LEN/NLEN"] = (png_file(h, w, "rgb", b"\x78\x01\x01\x05\x00\xfa\xfe" + b"\0" * 9), {S.PNGDEC_BAD_STORED_LEN})
    bad["zlib header"] = (png_file(h, w, "rgb", b"\x79\x01" + z[2:]), {S.PNGDEC_BAD_ZLIB_HEADER})
    bad["another size"] = (write_png(image_of(rng, 7, 1, "rgb"), "rgb"), {S.PNGDEC_HEADER_MISMATCH})
    bad["another format"] = (write_png(image_of(rng, h, w, "gray16"), "gray16"), {S.PNGDEC_HEADER_MISMATCH})
    ihdr_bad = bytearray(good)
    ihdr_bad[30] ^= 0xFF  # IHDR's CRC
    bad["IHDR CRC"] = (bytes(ihdr_bad), {S.PNGDEC_BAD_CRC})
    names = list(bad)
    files, kinds = [], []
    for k, name in enumerate(names):  # a good file between any two bad ones
        files += [good if k % 2 else pil_png(img), bad[name][0]]
        kinds += [None, name]
    files.append(good)
    kinds.append(None)
    d = Decode(files, RGB8, h, w, pad=5)
    for i, name in enumerate(kinds):
        if name is None:
            assert d.st[i] == 0 and np.array_equal(d.images[i], img), (i, int(d.st[i]))
        else:
            assert int(d.st[i]) in bad[name][1] and d.st[i] != 0, (name, int(d.st[i]))
            assert (d.images[i] == 0xA5).all(), name  # a rejected file has written no pixel: the sentinel is still there
    # a span table that points outside its file (what the probe never hands out) is refused by the kernel itself
    def lying(f):
        rc, info, spans = probe(f)
        spans = spans.copy()
        spans[0, 1] = len(f)
        return rc, info, spans
    calls = {"n": 0}

    def second_lies(f):
        calls["n"] += 1
        return lying(f) if calls["n"] == 2 else probe(f)

    d2 = Decode([good, good, good], RGB8, h, w, work=d.work, spans_of=second_lies)
    assert d2.st.tolist()[0] == 0 and d2.st[1] == S.PNGDEC_BAD_FRAMING and d2.st[2] == 0
    # the same workspace, an ordinary decode
    d3 = Decode([good, pil_png(img)], RGB8, h, w, work=d.work)
    assert d3.st.tolist() == [0, 0] and all(np.array_equal(im, img) for im in d3.images)


# ------------------------------------------------------------------------------------------------------- decode.ImageDecoder
@pytest.mark.gpu
def test_png_decoder_class_groups_falls_back_and_raises(tmp_path):
    from PIL import Image

    from crossscore_amd.decode import ImageDecoder, read_image_u8, read_metric_map_u16

    rng = np.random.default_rng(90)
    paths, kinds = [], []

    def put(name, data, gray16=False):
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
        kinds.append(gray16)
        return p

    put("a_rgb_20x30.png", pil_png(image_of(rng, 20, 30, "rgb")))
    put("b_map_20x30.png", pil_png(image_of(rng, 20, 30, "gray16")), True)
    put("c_rgba_20x30.png", pil_png(image_of(rng, 20, 30, "rgba")))
    put("d_rgb_7x5.png", pil_png(image_of(rng, 7, 5, "rgb")))
    put("e_gray_20x30.png", write_png(image_of(rng, 20, 30, "gray8"), "gray8", [4] * 20))
    put("f_map_9x9.png", pil_png(image_of(rng, 9, 9, "gray16")), True)
    buf = io.BytesIO()
    Image.fromarray(image_of(rng, 20, 30, "rgb")).save(buf, format="JPEG")
    put("g_photo.jpg", buf.getvalue())
    put("h_interlaced.png", interlaced_png(image_of(rng, 6, 5, "rgb")))
    put("i_rgb_20x30.png", pil_png(image_of(rng, 20, 30, "rgb"), optimize=True))
    dec = ImageDecoder("cuda")
    handle = dec.decode(paths, kinds)
    handle.wait()
    handle.check()
    assert sorted(os.path.basename(p) for p in handle.host_paths) == ["g_photo.jpg", "h_interlaced.png"]
    assert dec.stats() == {"png_decoded_gpu": 7, "png_decoded_host": 2}
    for p, g, t in zip(paths, kinds, handle.tensors):
        want = read_metric_map_u16(p) if g else read_image_u8(p)
        assert t.is_cuda and t.is_contiguous() and t.dtype == (torch.int16 if g else torch.uint8) and tuple(t.shape) == want.shape, p
        got = t.cpu().numpy()
        assert np.array_equal(got.view(np.uint16) if g else got, want), p
    # files of one (size, kind) are slices of one tensor, in request order
    a, c, e, i = (handle.tensors[k] for k in (0, 2, 4, 8))
    assert c.data_ptr() == a.data_ptr() + 20 * 30 * 3 and e.data_ptr() == c.data_ptr() + 20 * 30 * 3 and i.data_ptr() == e.data_ptr() + 20 * 30 * 3
    # a file whose stream is damaged raises, naming its path
    good = open(paths[0], "rb").read()
    damaged = bytearray(good)
    damaged[60] ^= 0x40
    bad_path = put("z_damaged.png", bytes(damaged))
    handle = dec.decode([paths[0], bad_path, paths[8]])
    with pytest.raises(ValueError, match="z_damaged.png"):
        handle.check()
    # a 16-bit map asked for as an image is the host reader's error, as without the decoder
    with pytest.raises(ValueError):
        dec.decode([paths[1]], False)


@pytest.mark.gpu
def test_a_request_without_any_device_group(tmp_path):
    """No path at all, and a request whose every file goes to PIL: the group loop runs zero times and the handle is complete all the same."""
    from PIL import Image

    from crossscore_amd.decode import ImageDecoder, read_image_u8

    dec = ImageDecoder("cuda")
    handle = dec.decode([])
    assert handle.tensors == [] and handle.paths == [] and handle.host_paths == []
    handle.wait()
    handle.check()
    rng = np.random.default_rng(93)
    buf = io.BytesIO()
    Image.fromarray(image_of(rng, 8, 8, "rgb")).save(buf, format="JPEG")
    paths = [str(tmp_path / "interlaced_5x7.png"), str(tmp_path / "photo_8x8.jpg")]
    for p, data in zip(paths, (interlaced_png(image_of(rng, 5, 7, "rgb")), buf.getvalue())):
        with open(p, "wb") as f:
            f.write(data)
    handle = dec.decode(paths)
    handle.wait()
    handle.check()
    assert handle.host_paths == paths
    assert dec.stats() == {"png_decoded_gpu": 0, "png_decoded_host": 2}
    assert dec.jpeg_stats() == {"jpeg_decoded_gpu": 0, "jpeg_decoded_host": 0}
    assert dec.progressive_stats() == {"jpeg_progressive_gpu": 0, "jpeg_progressive_host": 0}
    for p, t in zip(paths, handle.tensors):
        want = read_image_u8(p)
        assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == want.shape, p
        assert np.array_equal(t.cpu().numpy(), want), p


@pytest.mark.gpu
def test_png_decoder_does_not_wait_for_the_stream(tmp_path):
    """decode() returns while its stream is still busy with work queued before it (pinned, non-blocking uploads; status words behind the event)."""
    from crossscore_amd.decode import ImageDecoder, read_image_u8

    if not hasattr(torch.cuda, "_sleep"):
        pytest.skip("torch.cuda._sleep is not available")
    rng = np.random.default_rng(91)
    paths = []
    for k in range(4):
        p = str(tmp_path / f"q{k}.png")
        open(p, "wb").write(pil_png(image_of(rng, 20, 30, "rgb")))
        paths.append(p)
    dec = ImageDecoder("cuda")
    dec.decode(paths).check()  # kernels, pinned blocks and allocator pools exist from here on
    torch.cuda.synchronize()
    with torch.cuda.stream(dec.stream):
        torch.cuda._sleep(200_000_000)  # ~0.1 s of device time ahead of the decode on its stream
    handle = dec.decode(paths)
    assert not handle.event.query()  # the host is back while the decoder's stream is still busy
    handle.wait()
    handle.check()
    for p, t in zip(paths, handle.tensors):
        assert np.array_equal(t.cpu().numpy(), read_image_u8(p))


@pytest.mark.gpu
def test_input_stage_takes_device_images_without_a_copy():
    from crossscore_amd.data import InputStage

    rng = np.random.default_rng(92)
    img = smooth_noise(rng, 60, 84)
    stage = InputStage(torch.device("cuda"), resize_short_side=56)
    d_img = torch.from_numpy(img).cuda()
    a, b = torch.empty((3, 56, 78), device="cuda"), torch.empty((3, 56, 78), device="cuda")
    stage(img, a)
    stage(d_img, b)
    assert torch.equal(a, b)
    desc = stage.describe(d_img)
    assert desc.data.data_ptr() == d_img.data_ptr() and (desc.h, desc.w) == (60, 84)
    with pytest.raises(ValueError):
        stage.describe(d_img.to(torch.int16))
