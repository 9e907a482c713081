"""Host side of the progressive JPEG decoder: cs_jpeg_probe_ex is cs_jpeg_probe with flags = 0 and, with
CS_JPEG_PROGRESSIVE, takes complete progressive files, says why it refuses the others and never runs past the bytes it was given;
tests/jpeg_progressive_oracle.py -- the entropy decoder csrc/jpegprog.hip restates, and a re-coder for scan scripts PIL never writes -- equals
PIL bit for bit.  No GPU."""
import ctypes as C
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
import jpeg_progressive_oracle as prog  # noqa: E402
from crossscore_amd import _lib  # noqa: E402
from crossscore_amd.config import load_config  # noqa: E402
from jpeg_files import (GRID_FORMS, PIL_SCRIPT, SAMPLING_CODE, SCRIPTS, adobe_spliced, content, jpeg_bytes, patch_sos, pil_array, probe, probe_ex,  # noqa: E402
                        progressive_grid, recoded)

NEW_SYMBOLS = ("cs_jpeg_probe_ex", "cs_jpeg_decode_workspace_bytes_ex", "cs_op_jpeg_decode_ex", "cs_debug_jpeg_scan_levels")


def fields(info):
    return tuple(getattr(info, name) for name, _ in info._fields_)


def drop_scan(data: bytes, scan: int) -> bytes:
    scans = prog.parse(data)["scans"]
    return data[:scans[scan]["sos"]] + data[scans[scan]["end"]:]


def test_new_symbols_declared_listed_and_exported():
    hdr = open(os.path.join(REPO, "include", "crossscore_hip.h")).read()
    declared = set(re.findall(r"\b(cs_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"CS_JPEG_PROGRESSIVE\s+1\b", hdr) and re.search(r"CS_JPGDEC_BAD_SCAN\s+8\b", hdr) and "cs_jpeg_scan_info" in hdr
    assert _lib.JPEG_PROGRESSIVE == 1 and _lib.JPGDEC_BAD_SCAN == 8
    assert "jpegprog.hip" in __import__("crossscore_amd.build", fromlist=["SOURCES"]).SOURCES


def test_flags_zero_is_the_plain_probe():
    img = content("mix", 17, 23)
    good = jpeg_bytes(img, 2, quality=90, restart_marker_blocks=3)
    cases = [good, jpeg_bytes(img, "gray", optimize=True), jpeg_bytes(img, 1, progressive=True), adobe_spliced(good), jpeg_bytes(img[:, :4], 2), b"\x89PNG\r\n\x1a\n" + good,
             good[:40], good[:2], good[:3], good[:probe(good)[1].entropy_offset], b"\xff"]
    for data in cases:
        rc0, info0 = probe(data)
        text0 = _lib.last_error() if rc0 else ""
        rc1, info1, scans = probe_ex(data, 0)
        text1 = _lib.last_error() if rc1 else ""
        assert (rc0, fields(info0), text0) == (rc1, fields(info1), text1), data[:16]
        if rc1 == _lib.CS_OK:
            assert (scans.process, scans.scans, scans.entropy_offset) == (0, 1, info1.entropy_offset)
    assert probe_ex(good, 2)[0] == _lib.CS_ERR_BAD_ARG  # an unknown flag
    rc, info, scans = probe_ex(good)  # a baseline file under the flag: taken as before
    assert rc == _lib.CS_OK and fields(info) == fields(probe(good)[1]) and (scans.process, scans.scans) == (0, 1)


def test_pil_progressive_files_are_taken_with_the_right_fields():
    n = 0
    for name, data, twin in progressive_grid():
        rc, info, scans = probe_ex(data)
        assert rc == _lib.CS_OK, (name, _lib.last_error())
        base = probe(twin)[1]
        gray = info.components == 1
        assert (info.height, info.width, info.components, info.sampling, info.restart_interval) == \
            (base.height, base.width, base.components, base.sampling, base.restart_interval), name
        assert info.sampling == SAMPLING_CODE["gray" if gray else int(name.split(" ")[1])], name
        h = prog.parse(data)
        assert (scans.process, scans.scans) == (1, 6 if gray else 10) and len(h["scans"]) == scans.scans, name
        assert scans.entropy_offset == info.entropy_offset == h["scans"][0]["start"], name
        assert probe(data)[0] == _lib.CS_ERR_UNSUPPORTED, name  # the plain probe still refuses it
        n += 1
    assert n == (4 * 4 + 2) * len(GRID_FORMS)
    h = prog.parse(jpeg_bytes(content("mix", 17, 23), 2, progressive=True))
    assert [(tuple(c for c, _, _ in s["comps"]), s["ss"], s["se"], s["ah"], s["al"]) for s in h["scans"]] == PIL_SCRIPT


def test_what_the_extended_probe_refuses_and_why():
    good, _ = recoded(PIL_SCRIPT)
    assert probe_ex(good)[0] == _lib.CS_OK
    dqt = good[good.find(b"\xff\xdb"):good.find(b"\xff\xdb") + 69]
    second = prog.parse(good)["scans"][1]["sos"]
    many, _ = recoded([((0, 1, 2), 0, 0, 0, 0)] + [((0,), k, k, 0, 0) for k in range(1, 29)] + [((0,), 29, 63, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 62, 0, 0),
                                                                                                ((2,), 63, 63, 0, 0)])
    assert len(prog.parse(many)["scans"]) == 33
    narrow = jpeg_bytes(content("mix", 17, 23)[:, :4], 2, progressive=True)
    cases = {
        "refinement before first coding": (patch_sos(good, 1, ah=3), "never coded"),
        "wrong Ah": (patch_sos(good, 5, ah=3, al=2), "is not where it stands"),
        "Ah that is not Al + 1": (patch_sos(good, 5, ah=3, al=1), "Ah = Al \\+ 1"),
        "AC before DC": (drop_scan(recoded(SCRIPTS["non-interleaved DC"])[0], 1), "before its first DC scan"),
        "an interleaved AC scan": (patch_sos(good, 0, ss=1, se=5), "one component"),
        "Ss > Se": (patch_sos(good, 1, ss=6, se=5), "Ss <= Se"),
        "Al = 14": (patch_sos(good, 1, al=14), "13 at most"),
        "33 scans": (many, "more than 32 scans"),
        "DQT after the first SOS": (good[:second] + dqt + good[second:], "DQT segment .* behind the first scan"),
        "DRI after the first SOS": (good[:second] + b"\xff\xdd\x00\x04\x00\x00" + good[second:], "DRI segment .* behind the first scan"),
        "a missing EOI": (good[:-2], "no EOI"),
        "an incomplete progression": (drop_scan(good, 9), "incomplete progression"),
        "first-coded twice": (patch_sos(good, 4, ss=5), "for the first time again"),
        "subsampled, 4 wide": (narrow, "replication upsampler"),
    }
    assert pil_array(cases["an incomplete progression"][0]).shape == (33, 47, 3)  # PIL opens it: that is block smoothing's ground
    for name, (data, why) in cases.items():
        rc, info, _ = probe_ex(data)
        assert rc == _lib.CS_ERR_UNSUPPORTED and info.sampling == -1, (name, rc, _lib.last_error())
        assert re.search(why, _lib.last_error()) and _lib.last_error().startswith("jpeg_probe"), (name, _lib.last_error())


def test_every_prefix_is_refused():
    """Each prefix up to the first scan's data is CS_ERR_BAD_ARG, each later one is refused; the bytes behind the prefix are not there at all (a
    copy of exactly n bytes)."""
    lib = _lib.load()
    img = content("mix", 17, 23)
    for data in (jpeg_bytes(img, 2, quality=90, progressive=True, restart_marker_blocks=3), jpeg_bytes(img, "gray", progressive=True)):
        rc, info, scans = probe_ex(data)
        assert rc == _lib.CS_OK
        for n in range(len(data)):
            buf = (C.c_uint8 * max(n, 1)).from_buffer_copy(data[:n] if n else b"\0")
            got = _lib.CsJpegInfo()
            rc = lib.cs_jpeg_probe_ex(buf, n, _lib.JPEG_PROGRESSIVE, C.byref(got), None)
            if n <= scans.entropy_offset:
                assert rc == _lib.CS_ERR_BAD_ARG, (n, _lib.last_error())
            else:
                assert rc in (_lib.CS_ERR_BAD_ARG, _lib.CS_ERR_UNSUPPORTED), n
            assert got.sampling == -1


def test_oracle_equals_the_baseline_twin_and_pil():
    for name, data, twin in progressive_grid():
        h = prog.parse(data)
        _, _, own = prog._geometry(h)
        stats = {}
        for c, (got, want) in enumerate(zip(prog.coefficients(data, h, stats), jpeg_oracle.coefficients(twin))):
            rows, cols = own[c]
            assert np.array_equal(got[:rows, :cols], want[:rows, :cols]), (name, c)  # the real blocks: non-interleaved scans leave the padding out
            assert np.array_equal(got[..., 0], want[..., 0]), (name, c)  # the interleaved DC scans code every block of the MCUs
        want = pil_array(data)
        got = prog.decode(data)
        assert got.shape == want.shape and got.dtype == np.uint8 and np.array_equal(got, want), name
        assert np.array_equal(want, pil_array(twin)), name  # a complete progressive file gets no block smoothing


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_recoder_scripts_satisfy_the_pil_condition(name):
    for sampling, restart in ((2, 0), (0, 1), (1, 5)):
        data, twin = recoded(SCRIPTS[name], sampling, restart=restart)  # asserts PIL's pixels
        assert np.array_equal(prog.decode(data), pil_array(twin)), (name, sampling, restart)
        rc, _, scans = probe_ex(data)
        assert rc == _lib.CS_OK and scans.scans == len(SCRIPTS[name]), (name, _lib.last_error())


def test_jpeg_progressive_key_is_validated():
    from crossscore_amd.decode import jpeg_progressive_choice

    for name in ("default_predict", "default_test"):
        assert jpeg_progressive_choice(load_config(name)) == "host"
        assert jpeg_progressive_choice(load_config(name, ["this_main.jpeg_decoder=gpu", "this_main.jpeg_progressive=gpu"])) == "gpu"
        assert jpeg_progressive_choice(load_config(name, ["this_main.jpeg_decoder=gpu"])) == "host"
        with pytest.raises(ValueError, match="jpeg_decoder=gpu"):
            jpeg_progressive_choice(load_config(name, ["this_main.jpeg_progressive=gpu"]))
        with pytest.raises(ValueError, match="jpeg_progressive"):
            jpeg_progressive_choice(load_config(name, ["this_main.jpeg_decoder=gpu", "this_main.jpeg_progressive=pil"]))
        cfg = load_config(name)
        del cfg.this_main["jpeg_progressive"]  # a config file written before the key existed
        assert jpeg_progressive_choice(cfg) == "host"


def test_workspace_grows_with_the_flag_only():
    lib = _lib.load()
    f, g = lib.cs_jpeg_decode_workspace_bytes, lib.cs_jpeg_decode_workspace_bytes_ex
    for args in ((1, 17, 23, 1000), (5, 540, 720, 10 ** 6), (1, 4096, 4096, 1)):
        assert g(*args, 0) == f(*args)
        i, h, w, _ = args
        assert g(*args, _lib.JPEG_PROGRESSIVE) >= f(*args) + i * 32 * 4 * (-(-h // 8)) * (-(-w // 8))  # a restart table per scan
    assert g(1, 17, 23, 1000, 2) == 0 and g(0, 17, 23, 1000, 1) == 0 and g(1, 4097, 8, 100, 1) == 0
    dummy = (C.c_uint8 * 64)()
    p = C.cast(dummy, C.c_void_p)
    assert lib.cs_op_jpeg_decode_ex(p, p, p, 100, 1, 16, 16, p, 768, p, p, 2, None) == _lib.CS_ERR_BAD_ARG and b"flags" in lib.cs_last_error()
    assert lib.cs_op_jpeg_decode_ex(p, p, p, 100, 1, 16, 16, p, 767, p, p, 1, None) == _lib.CS_ERR_BAD_ARG and b"stride" in lib.cs_last_error()
