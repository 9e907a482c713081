"""Host side of crossscore_amd/decode.py: the upload block's layout against numbers worked out by hand from the parts' sizes, probe_file's
routing of in-memory files, and the keys of the decoder's three counters.  No GPU."""
import collections
import io
import os
import struct
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
from crossscore_amd import _lib  # noqa: E402
from crossscore_amd import decode  # noqa: E402

FILES = (b"\x11", bytes(range(0x20, 0x28)), bytes(range(0x40, 0x4D)))  # 1, 8 and 13 bytes
SPANS = (np.array([[1, 2]], np.uint32), np.array([[3, 4], [5, 6]], np.uint32), np.array([[7, 8]], np.uint32))  # 1, 2 and 1 spans
SENTINEL = 0xA5


# ------------------------------------------------------------------------------------------------------------ the block
def test_layout_of_a_png_group():
    # files 22 -> 24 | offsets 3 * 8 = 24 | lengths 3 * 4 = 12 -> 16 | span_off 4 * 4 = 16 | spans 4 * 8 = 32
    at, size = decode.block_layout([1, 8, 13], [1, 2, 1])
    assert at == {"files": 0, "offsets": 24, "lengths": 48, "span_off": 64, "spans": 80}
    assert size == 112


def test_layout_of_a_jpeg_group():
    at, size = decode.block_layout([1, 8, 13])
    assert at == {"files": 0, "offsets": 24, "lengths": 48}
    assert size == 64


def _filled(files, spans):
    at, size = decode.block_layout([len(f) for f in files], None if spans is None else [len(s) for s in spans])
    bv = np.full((size,), SENTINEL, np.uint8)
    decode.fill_block(bv, at, files, spans)
    return at, bv


@pytest.mark.parametrize("with_spans", [True, False])
def test_filled_block(with_spans):
    at, bv = _filled(FILES, SPANS if with_spans else None)
    written = np.zeros(bv.shape, bool)

    def part(a, nbytes, dtype):
        written[a:a + nbytes] = True
        return bv[a:a + nbytes].view(dtype)

    for f, o in zip(FILES, (0, 1, 9)):
        assert part(o, len(f), np.uint8).tobytes() == f
    assert part(at["offsets"], 24, np.uint64).tolist() == [0, 1, 9]
    assert part(at["lengths"], 12, np.uint32).tolist() == [1, 8, 13]
    if with_spans:
        assert part(at["span_off"], 16, np.uint32).tolist() == [0, 1, 3, 4]
        assert part(at["spans"], 32, np.uint32).reshape(4, 2).tolist() == [[1, 2], [3, 4], [5, 6], [7, 8]]
    # the padding (2 bytes behind the files, 4 behind the lengths) is not written
    assert int((~written).sum()) == 6 and (bv[~written] == SENTINEL).all()


def test_single_file_group():
    at, size = decode.block_layout([5], [3])
    assert at == {"files": 0, "offsets": 8, "lengths": 16, "span_off": 24, "spans": 32} and size == 56
    assert decode.block_layout([5]) == ({"files": 0, "offsets": 8, "lengths": 16}, 24)
    at, bv = _filled([b"abcde"], [np.array([[9, 8], [7, 6], [5, 4]], np.uint32)])
    assert bv[:5].tobytes() == b"abcde" and (bv[5:8] == SENTINEL).all()
    assert bv[8:16].view(np.uint64).tolist() == [0] and bv[16:20].view(np.uint32).tolist() == [5] and (bv[20:24] == SENTINEL).all()
    assert bv[24:32].view(np.uint32).tolist() == [0, 3] and bv[32:56].view(np.uint32).tolist() == [9, 8, 7, 6, 5, 4]


def test_group_whose_total_is_a_multiple_of_8():
    # files 16, no padding | offsets 16 | lengths 8 | span_off 12 -> 16 | spans 2 * 8
    at, size = decode.block_layout([3, 13], [1, 1])
    assert at == {"files": 0, "offsets": 16, "lengths": 32, "span_off": 40, "spans": 56} and size == 72
    files = [b"xyz", bytes(range(13))]
    at, bv = _filled(files, [np.array([[1, 1]], np.uint32), np.array([[2, 2]], np.uint32)])
    assert bv[:16].tobytes() == files[0] + files[1]
    assert bv[16:32].view(np.uint64).tolist() == [0, 3] and bv[32:40].view(np.uint32).tolist() == [3, 13]
    assert bv[40:52].view(np.uint32).tolist() == [0, 1, 2] and (bv[52:56] == SENTINEL).all()
    assert bv[56:72].view(np.uint32).tolist() == [1, 1, 2, 2]


# ------------------------------------------------------------------------------------------------------------ probe_file
def _pil_bytes(arr, fmt, **kw) -> bytes:
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format=fmt, **kw)
    return buf.getvalue()


def _rgb():
    return np.random.default_rng(5).integers(0, 256, size=(8, 8, 3)).astype(np.uint8)


def _interlaced_png() -> bytes:
    """An 8 x 8 Adam7 RGB file of zeros (PIL writes none): only its framing and IHDR matter to the probe."""
    def chunk(typ, payload):
        return struct.pack(">I", len(payload)) + typ + payload + struct.pack(">I", zlib.crc32(typ + payload))

    rows = [b"\0" + bytes(3 * w) for w, h in ((1, 1), (1, 1), (2, 1), (2, 2), (4, 2), (4, 4), (8, 4)) for _ in range(h)]
    return (decode.PNG_SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 8, 8, 8, 2, 0, 0, 1)) + chunk(b"IDAT", zlib.compress(b"".join(rows)))
            + chunk(b"IEND", b""))


def test_probe_file_takes_an_rgb_png():
    data = _pil_bytes(_rgb(), "PNG")
    p = decode.probe_file(data, png=True)
    assert p.fmt == "png" and p.data is data and not p.progressive
    assert (p.info.height, p.info.width, p.info.kind) == (8, 8, _lib.PNG_RGB8)
    assert p.spans.dtype == np.uint32 and p.spans.shape == (p.info.num_idat, 2)


def test_probe_file_leaves_a_png_alone_with_png_off():
    p = decode.probe_file(_pil_bytes(_rgb(), "PNG"), png=False)
    assert p.fmt is None and p.info is None and p.spans is None and not p.progressive


def test_probe_file_reads_the_kind_of_a_16_bit_map():
    m = np.random.default_rng(6).integers(0, 65536, size=(8, 8)).astype(np.uint16)
    p = decode.probe_file(_pil_bytes(m, "PNG"), png=True)
    assert p.fmt == "png" and p.info.kind == _lib.PNG_GRAY16


def test_probe_file_refuses_an_interlaced_png():
    from PIL import Image

    data = _interlaced_png()
    assert Image.open(io.BytesIO(data)).size == (8, 8) and Image.open(io.BytesIO(data)).info.get("interlace") == 1
    p = decode.probe_file(data, png=True)
    assert p.fmt == "png" and p.info is None and p.spans is None


def test_probe_file_takes_a_baseline_jpeg():
    p = decode.probe_file(_pil_bytes(_rgb(), "JPEG"), jpeg=True)
    assert p.fmt == "jpeg" and not p.progressive and p.spans is None
    assert (p.info.height, p.info.width) == (8, 8)


@pytest.mark.parametrize("png", [True, False])
def test_probe_file_without_jpeg_sees_no_jpeg(png):
    p = decode.probe_file(_pil_bytes(_rgb(), "JPEG"), png=png, jpeg=False)
    assert p.fmt is None and p.info is None and p.spans is None and not p.progressive  # a file that is no PNG: PIL's


def test_probe_file_with_progressive_off_refuses_a_progressive_jpeg():
    data = _pil_bytes(_rgb(), "JPEG", progressive=True)
    assert decode.is_progressive_jpeg(data)
    p = decode.probe_file(data, jpeg=True, progressive=False)
    assert p.fmt == "jpeg" and p.info is None and not p.progressive


def test_probe_file_with_progressive_on_flags_and_takes_it():
    p = decode.probe_file(_pil_bytes(_rgb(), "JPEG", progressive=True), jpeg=True, progressive=True)
    assert p.fmt == "jpeg" and p.progressive and (p.info.height, p.info.width) == (8, 8)
    q = decode.probe_file(_pil_bytes(_rgb(), "JPEG"), jpeg=True, progressive=True)  # a baseline file beside it: taken, not flagged
    assert q.fmt == "jpeg" and not q.progressive and q.info is not None


# ------------------------------------------------------------------------------------------------------------ the counters
def test_stats_keys_start_at_zero():
    dec = decode.ImageDecoder.__new__(decode.ImageDecoder)  # (the constructor opens a stream; the counters need no device)
    dec.counts = collections.Counter()
    assert dec.stats() == {"png_decoded_gpu": 0, "png_decoded_host": 0}
    assert dec.jpeg_stats() == {"jpeg_decoded_gpu": 0, "jpeg_decoded_host": 0}
    assert dec.progressive_stats() == {"jpeg_progressive_gpu": 0, "jpeg_progressive_host": 0}
    assert not dec.counts  # reading adds no key
