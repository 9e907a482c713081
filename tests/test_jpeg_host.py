"""Host side of the device JPEG decoder: tests/jpeg_oracle.py -- the decoder's arithmetic in numpy int64 -- equals PIL
bit for bit over a grid of PIL-written baseline files; cs_jpeg_probe reads the right fields, says what is not taken and never runs past the
bytes it was given; this_main.jpeg_decoder is validated.  No GPU."""
import ctypes as C
import io
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
import jpeg_oracle  # noqa: E402
from crossscore_amd import _lib  # noqa: E402
from crossscore_amd.config import load_config  # noqa: E402
from jpeg_files import SAMPLING_CODE, SAMPLINGS, adobe_spliced, as_440, content, grid_files, jpeg_bytes, pil_array, probe  # noqa: E402

NEW_SYMBOLS = ("cs_jpeg_probe", "cs_jpeg_decode_workspace_bytes", "cs_op_jpeg_decode")


def test_new_symbols_declared_listed_and_exported():
    hdr = open(os.path.join(REPO, "include", "crossscore_hip.h")).read()
    declared = set(re.findall(r"\b(cs_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "cs_jpeg_info" in hdr and "CS_JPGDEC_BAD_RESTART" in hdr
    assert "jpegdec.hip" in __import__("crossscore_amd.build", fromlist=["SOURCES"]).SOURCES
    codes = dict(re.findall(r"CS_JPGDEC_([A-Z_]+) = (\d+)", hdr))
    for name, value in codes.items():
        assert getattr(_lib, "JPGDEC_" + name) == int(value), name
    assert len(codes) == 8


def test_oracle_equals_pil_over_the_grid():
    n = 0
    for name, data in grid_files():
        want = pil_array(data)
        got = jpeg_oracle.decode(data)
        assert got.shape == want.shape and got.dtype == np.uint8 and np.array_equal(got, want), name
        n += 1
    assert n > 500


def test_narrow_subsampled_files_do_not_match():
    """libjpeg replaces the triangle filter by replication when the chroma width is <= 2: the reason for the W >= 5 rule."""
    for h, w in ((2, 3), (5, 4)):
        for s in (1, 2):
            data = jpeg_bytes(content("noise", h, w), s, quality=90)
            assert not np.array_equal(jpeg_oracle.decode(data), pil_array(data)), (h, w, s)
    for s in (1, 2):
        data = jpeg_bytes(content("noise", 5, 5), s, quality=90)
        assert np.array_equal(jpeg_oracle.decode(data), pil_array(data)), s


def test_probe_reads_the_fields_of_each_accepted_kind():
    img = content("mix", 17, 23)
    for s in SAMPLINGS:
        for extra, ri in ((dict(), 0), (dict(restart_marker_blocks=3), 3), (dict(restart_marker_rows=1), -1)):
            data = jpeg_bytes(img, s, quality=90, **extra)
            rc, info = probe(data)
            assert rc == _lib.CS_OK, _lib.last_error()
            hdr = jpeg_oracle.parse(data)
            assert (info.height, info.width, info.components, info.sampling) == (17, 23, 1 if s == "gray" else 3, SAMPLING_CODE[s])
            assert info.entropy_offset == hdr["entropy"] and info.restart_interval == hdr["ri"]
            assert ri < 0 or info.restart_interval == ri
            assert data[info.entropy_offset - 3:info.entropy_offset] == b"\x00\x3f\x00"  # Ss, Se, Ah / Al: the end of SOS
    data = jpeg_bytes(img, 2, quality=90, optimize=True, comment=b"x" * 300, dpi=(72, 72))  # COM and a longer APP0 are skipped
    assert probe(data)[0] == _lib.CS_OK


def test_probe_says_what_is_not_taken():
    from PIL import Image

    img = content("mix", 17, 23)

    def save(im, **kw):
        buf = io.BytesIO()
        im.save(buf, format="JPEG", **kw)
        return buf.getvalue()

    good = jpeg_bytes(img, 2)
    cases = {"progressive": save(Image.fromarray(img), progressive=True), "cmyk": save(Image.fromarray(img).convert("CMYK")),
             "4:4:0": as_440(jpeg_bytes(img, 1)), "adobe app14": adobe_spliced(good), "subsampled, 4 wide": jpeg_bytes(img[:, :4], 2),
             "4:2:2, 3 wide": jpeg_bytes(img[:, :3], 1)}
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG")
    cases["png"] = buf.getvalue()
    assert pil_array(cases["adobe app14"]).shape == (17, 23, 3)  # PIL still opens the spliced file
    for name, data in cases.items():
        rc, info = probe(data)
        assert rc == _lib.CS_ERR_UNSUPPORTED and info.sampling == -1, (name, rc, _lib.last_error())
        assert b"jpeg_probe" in _lib.load().cs_last_error() and len(_lib.last_error()) > 20
    assert probe(jpeg_bytes(img[:, :4], 0))[0] == _lib.CS_OK and probe(jpeg_bytes(img[:, :5], 2))[0] == _lib.CS_OK


def test_probe_refuses_every_truncated_header():
    """Each prefix of the header is CS_ERR_BAD_ARG; the bytes behind the prefix are not there at all (a copy of exactly n bytes)."""
    lib = _lib.load()
    img = content("mix", 17, 23)
    for data in (jpeg_bytes(img, 2, quality=90, restart_marker_blocks=3), jpeg_bytes(img, "gray", optimize=True)):
        off = probe(data)[1].entropy_offset
        for n in range(off + 1):
            buf = (C.c_uint8 * max(n, 1)).from_buffer_copy(data[:n] if n else b"\0")
            info = _lib.CsJpegInfo()
            assert lib.cs_jpeg_probe(buf, n, C.byref(info)) == _lib.CS_ERR_BAD_ARG, (n, _lib.last_error())
            assert info.sampling == -1
        info = _lib.CsJpegInfo()
        assert lib.cs_jpeg_probe(data, off + 1, C.byref(info)) == _lib.CS_OK
    # a segment length that points past the end
    d = bytearray(jpeg_bytes(img, 2))
    d[4:6] = b"\xff\xff"
    assert probe(bytes(d))[0] == _lib.CS_ERR_BAD_ARG


def test_workspace_and_arguments_are_checked_on_the_host():
    lib = _lib.load()
    f = lib.cs_jpeg_decode_workspace_bytes
    assert f(2, 17, 23, 1000) > f(1, 17, 23, 1000) >= 3 * 32 * 32 * 3  # coefficients (int16) and samples of three planes padded to 16 x 16
    assert f(1, 4096, 4096, 1) > 0
    for args in ((0, 8, 8, 100), (70000, 8, 8, 100), (1, 0, 8, 100), (1, 8, 0, 100), (1, 4097, 8, 100), (1, 8, 4097, 100), (1, 8, 8, 0)):
        assert f(*args) == 0, args
    dummy = (C.c_uint8 * 64)()
    p = C.cast(dummy, C.c_void_p)

    def call(i=1, h=16, w=16, stride=768, total=100, files=p, pixels=p, status=p, work=p):
        return lib.cs_op_jpeg_decode(files, p, p, total, i, h, w, pixels, stride, status, work, None)

    for kw, word in ((dict(w=0), b"sizes"), (dict(i=0), b"sizes"), (dict(i=70000), b"sizes"), (dict(stride=767), b"stride"), (dict(total=0), b"file bytes"),
                     (dict(files=None), b"null"), (dict(pixels=None), b"null"), (dict(status=None), b"null"), (dict(work=None), b"null")):
        assert call(**kw) == _lib.CS_ERR_BAD_ARG, kw
        assert word in lib.cs_last_error(), (kw, lib.cs_last_error())
    assert call(h=4097, stride=4097 * 48) == _lib.CS_ERR_UNSUPPORTED and b"4096" in lib.cs_last_error()
    odd = C.c_void_p(C.addressof(dummy) + 16 + 1)
    assert call(work=odd) == _lib.CS_ERR_BAD_ARG and b"aligned" in lib.cs_last_error()


def test_jpeg_decoder_key_is_validated():
    from crossscore_amd.decode import jpeg_decoder_choice, png_decoder_choice

    for name in ("default_predict", "default_test"):
        assert jpeg_decoder_choice(load_config(name)) == "host"
        assert jpeg_decoder_choice(load_config(name, ["this_main.jpeg_decoder=gpu"])) == "gpu"
        assert png_decoder_choice(load_config(name, ["this_main.jpeg_decoder=gpu"])) == "host"
        with pytest.raises(ValueError, match="jpeg_decoder"):
            jpeg_decoder_choice(load_config(name, ["this_main.jpeg_decoder=pil"]))
        cfg = load_config(name)
        del cfg.this_main["jpeg_decoder"]  # a config file written before the key existed
        assert jpeg_decoder_choice(cfg) == "host"
