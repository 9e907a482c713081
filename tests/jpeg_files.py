"""JPEG files for the decoder and driver tests: image contents, PIL-written baseline and progressive grids, re-coded scan scripts PIL never
writes (tests/jpeg_progressive_oracle.py), header patches, and the two probes.  The decoders' arithmetic in numpy: tests/jpeg_oracle.py."""
import ctypes as C
import io

import numpy as np

import jpeg_oracle
import jpeg_progressive_oracle as prog
from crossscore_amd import _lib

SAMPLINGS = (0, 1, 2, "gray")  # PIL's subsampling 0 (4:4:4), 1 (4:2:2), 2 (4:2:0); a one-component file
SAMPLING_CODE = {"gray": _lib.JPEG_GRAY, 0: _lib.JPEG_444, 1: _lib.JPEG_422, 2: _lib.JPEG_420}
SIZES = [(8, 8), (16, 16), (17, 23), (9, 31), (33, 50), (1, 1)]  # (H, W); 1 x 1 for 4:4:4 and gray only (subsampled files need W >= 5)
CONTENTS = ("smooth", "noise", "mix")
QUALITY = [dict(quality=30), dict(quality=90), dict(quality=100), dict(quality=90, optimize=True)]
RESTARTS = [dict(), dict(restart_marker_blocks=1), dict(restart_marker_blocks=3), dict(restart_marker_rows=1)]


def content(kind: str, h: int, w: int, seed: int = 0) -> np.ndarray:
    """(h, w, 3) uint8: smooth waves, uniform noise, or waves under Gaussian noise"""
    rng = np.random.default_rng(seed * 1000 + h * 37 + w)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    waves = np.stack([128 + 100 * np.sin(y / 7 + c) * np.cos(x / 9 - c) for c in range(3)], axis=-1)
    if kind == "smooth":
        a = waves
    elif kind == "noise":
        a = rng.integers(0, 256, size=(h, w, 3))
    else:
        a = waves + rng.normal(0, 20, size=(h, w, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


def jpeg_bytes(img: np.ndarray, sampling=2, **kw) -> bytes:
    """img (h, w, 3) written by PIL: sampling 0 / 1 / 2 as PIL's subsampling, "gray" as a one-component file of channel 0"""
    from PIL import Image

    buf = io.BytesIO()
    if sampling == "gray":
        Image.fromarray(img[:, :, 0]).save(buf, format="JPEG", **kw)
    else:
        Image.fromarray(img).save(buf, format="JPEG", subsampling=sampling, **kw)
    return buf.getvalue()


def pil_array(data: bytes) -> np.ndarray:
    from PIL import Image

    return np.array(Image.open(io.BytesIO(data)))


def grid_files(sizes=SIZES, samplings=SAMPLINGS, contents=CONTENTS, quality=QUALITY, restarts=RESTARTS):
    """(name, bytes) over the grid: every quality form without restart markers, every restart form at quality 90, and quality 30 / 100 with
    optimised tables under restart_marker_blocks=3"""
    forms = [dict(q) for q in quality] + [dict(quality=90, **r) for r in restarts if r]
    if any(r for r in restarts):
        forms += [dict(quality=30, optimize=True, restart_marker_blocks=3), dict(quality=100, optimize=True, restart_marker_rows=1)]
    for h, w in sizes:
        for s in samplings:
            if s in (1, 2) and w < 5:
                continue
            for kind in contents:
                img = content(kind, h, w)
                for form in forms:
                    yield f"{h}x{w} {s} {kind} {form}", jpeg_bytes(img, s, **form)


def probe(data: bytes, n=None):
    lib = _lib.load()
    info = _lib.CsJpegInfo()
    rc = lib.cs_jpeg_probe(data, len(data) if n is None else n, C.byref(info))
    return rc, info


def adobe_spliced(data: bytes) -> bytes:
    """a 12-byte Adobe APP14 segment (transform 1) behind SOI"""
    return data[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01" + data[2:]


def as_440(data_422: bytes) -> bytes:
    """The header of a 4:4:0 frame: luma 1 x 2 in the SOF of a file PIL wrote as 4:2:2 (this PIL's writer takes 0 / 1 / 2 only, so the file is
    made here; the probe reads headers)."""
    d = bytearray(data_422)
    k = d.find(b"\xff\xc0")
    assert d[k + 11] == 0x21
    d[k + 11] = 0x12
    return bytes(d)


# ---- progressive files ------------------------------------------------------------------------------------------------------------------
# (H, W, samplings): 5 x 5 is the smallest subsampled file, 1 x 1 gray the smallest of all
GRID_SIZES = [(8, 8, SAMPLINGS), (9, 11, SAMPLINGS), (17, 23, SAMPLINGS), (33, 47, SAMPLINGS), (5, 5, (2,)), (1, 1, ("gray",))]
GRID_FORMS = [dict(quality=30), dict(quality=75, optimize=True), dict(quality=95), dict(quality=100),
              dict(quality=75, restart_marker_blocks=1), dict(quality=95, restart_marker_blocks=3), dict(quality=30, optimize=True, restart_marker_blocks=3)]

# the scan script of libjpeg's jpeg_simple_progression for three components: what PIL writes
PIL_SCRIPT = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1),
              ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
# scripts PIL never writes, each legal and complete, none above 32 scans
SCRIPTS = {
    "spectral selection only": [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 5, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0), ((0,), 6, 63, 0, 0)],
    "non-interleaved DC": [((0,), 0, 0, 0, 1), ((1,), 0, 0, 0, 0), ((2,), 0, 0, 0, 0), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0),
                           ((2,), 1, 63, 0, 0)],
    "chain 3 2 1 0": ([((0, 1, 2), 0, 0, 0, 3), ((0, 1, 2), 0, 0, 3, 2), ((0, 1, 2), 0, 0, 2, 1), ((0, 1, 2), 0, 0, 1, 0)] +
                      [((c,), 1, 63, 0, 3) for c in range(3)] + [((c,), 1, 63, a + 1, a) for a in (2, 1, 0) for c in range(3)]),
    "single-coefficient bands": ([((0, 1, 2), 0, 0, 0, 0)] + [((0,), k, k, 0, 0) for k in range(1, 25)] +
                                 [((0,), 25, 63, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)]),
    "chroma AC before luma AC": [((0, 1, 2), 0, 0, 0, 0), ((1,), 1, 63, 0, 1), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 1, 0), ((2,), 1, 63, 1, 0),
                                 ((0,), 1, 63, 0, 1), ((0,), 1, 63, 1, 0)],
}


def progressive_grid(sizes=GRID_SIZES, forms=GRID_FORMS):
    """(name, progressive file, its baseline twin: the same image and settings) over sampling x quality x optimize x restart x sizes"""
    for h, w, samplings in sizes:
        for s in samplings:
            img = content("mix", h, w, seed=h)
            for form in forms:
                yield f"{h}x{w} {s} {form}", jpeg_bytes(img, s, progressive=True, **form), jpeg_bytes(img, s, **form)


def recoded(script, sampling=2, h=33, w=47, restart=0, quality=90, seed=3):
    """(file under `script`, its baseline twin); the PIL condition is asserted here: PIL opens the file and returns the twin's pixels exactly"""
    twin = jpeg_bytes(content("mix", h, w, seed=seed), sampling, quality=quality)
    hdr = jpeg_oracle.parse(twin)
    data = prog.write_progressive(jpeg_oracle.coefficients(twin, hdr), hdr, script, restart=restart)
    assert np.array_equal(pil_array(data), pil_array(twin)), "the re-coder's file is not what PIL makes of the twin"
    return data, twin


def probe_ex(data: bytes, flags=_lib.JPEG_PROGRESSIVE, n=None):
    lib = _lib.load()
    info, scans = _lib.CsJpegInfo(), _lib.CsJpegScanInfo()
    rc = lib.cs_jpeg_probe_ex(data, len(data) if n is None else n, flags, C.byref(info), C.byref(scans))
    return rc, info, scans


def patch_sos(data: bytes, scan: int, **kw) -> bytes:
    """scan `scan` (from 0) with Ss / Se / Ah / Al replaced"""
    sc = prog.parse(data)["scans"][scan]
    at = sc["start"] - 3
    ss, se, ahal = data[at], data[at + 1], data[at + 2]
    ss, se = kw.get("ss", ss), kw.get("se", se)
    ah, al = kw.get("ah", ahal >> 4), kw.get("al", ahal & 15)
    return data[:at] + bytes([ss, se, ah << 4 | al]) + data[at + 3:]
