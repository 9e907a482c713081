"""The progressive JPEG decoder on the device (csrc/jpegprog.hip, cs_op_jpeg_decode_ex with CS_JPEG_PROGRESSIVE,
decode.ImageDecoder(jpeg=True, progressive=True)): every decoded image equals, bit for bit, what read_image_u8 makes of PIL's array for the same
bytes and what the baseline twin gives in the same call.  No tolerances.  Malformed files end with their documented status beside good files
that still decode; pixels, status words and workspace sit inside guard bands."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
import jpeg_oracle  # noqa: E402
import jpeg_progressive_oracle as prog  # noqa: E402
from crossscore_amd import _lib  # noqa: E402
from guard import guarded  # noqa: E402
from jpeg_files import PIL_SCRIPT, SCRIPTS, content, jpeg_bytes, patch_sos, pil_array, probe_ex, progressive_grid, recoded  # noqa: E402

P = _lib.JPEG_PROGRESSIVE


def expected(data: bytes) -> np.ndarray:
    from crossscore_amd.decode import read_image_u8

    return read_image_u8(io.BytesIO(data))


class Decode:
    """cs_op_jpeg_decode_ex on files of one size, inside guard bands: pixels (padded image stride), status and workspace."""

    def __init__(self, files, h, w, flags=P, pad=0, work=None):
        lib = _lib.load()
        n = len(files)
        lengths = np.array([len(f) for f in files], dtype=np.uint32)
        offsets = np.zeros(n, dtype=np.uint64)
        offsets[1:] = np.cumsum(lengths.astype(np.uint64))[:-1]
        total = int(lengths.sum())
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
        self.keep = [dev(np.frombuffer(b"".join(files), np.uint8)), dev(offsets), dev(lengths)]
        self.stride = h * w * 3 + pad
        self.pix = guarded((n, h * w * 3), torch.uint8, ld=self.stride, guard_rows=1)
        self.status = guarded((n,), torch.int32, guard_rows=0)
        ws = lib.cs_jpeg_decode_workspace_bytes_ex(n, h, w, total, flags)
        assert ws > 0
        self.work = work if work is not None else guarded((ws,), torch.uint8, guard_rows=0)
        assert self.work.shape[0] >= ws
        _lib.check(lib.cs_op_jpeg_decode_ex(*(C.c_void_p(t.data_ptr()) for t in self.keep), total, n, h, w, C.c_void_p(self.pix.view.data_ptr()), self.stride,
                                            C.c_void_p(self.status.view.data_ptr()), C.c_void_p(self.work.view.data_ptr()), flags,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        self.pix.check("pixels")
        self.status.check("status")
        self.work.check("workspace")
        self.st = self.status.view.cpu().numpy()
        raw = self.pix.view.cpu().numpy()
        self.images = [raw[i].reshape(h, w, 3) for i in range(n)]


def check_files(files, h, w, names=None, **kw):
    """every file decodes with status 0 to the host reader's array"""
    d = Decode(files, h, w, **kw)
    for i, f in enumerate(files):
        name = names[i] if names else i
        assert d.st[i] == 0, (name, int(d.st[i]))
        assert np.array_equal(d.images[i], expected(f)), name
    return d


@pytest.fixture
def levels_switch():
    yield _lib.load().cs_debug_jpeg_scan_levels
    _lib.load().cs_debug_jpeg_scan_levels(1)


@pytest.mark.gpu
def test_the_grid_equals_pil_and_the_baseline_twin():
    """One call per size: progressive files and their baseline twins alternate, every sampling in the same call."""
    groups = {}
    for name, data, twin in progressive_grid():
        h, w = (int(v) for v in name.split(" ")[0].split("x"))
        groups.setdefault((h, w), []).append((name, data, twin))
    n = 0
    for (h, w), members in groups.items():
        files = [f for _, data, twin in members for f in (data, twin)]
        names = [f"{name} {kind}" for name, _, _ in members for kind in ("progressive", "twin")]
        d = check_files(files, h, w, names, pad=(h + w) % 7)
        for k, (name, _, _) in enumerate(members):
            assert np.array_equal(d.images[2 * k], d.images[2 * k + 1]), name
        n += len(members)
    assert n == 18 * 7


@pytest.mark.gpu
def test_mixed_call_and_the_same_call_without_the_flag():
    h, w = 33, 47
    base = [jpeg_bytes(content("mix", h, w, seed=i), s, quality=90, **extra) for i, (s, extra) in enumerate(((2, {}), ("gray", {}), (0, dict(restart_marker_blocks=2))))]
    progs = [jpeg_bytes(content("noise", h, w, seed=i), s, quality=q, progressive=True) for i, (s, q) in enumerate(((2, 90), (1, 100), ("gray", 50)))]
    files = [progs[0], base[0], base[1], progs[1], progs[2], base[2]]
    mixed = check_files(files, h, w, pad=3)
    plain = Decode(files, h, w, flags=0, pad=3)
    assert plain.st.tolist() == [2, 0, 0, 2, 2, 0]  # CS_JPGDEC_HEADER_MISMATCH for SOF2, as cs_op_jpeg_decode says
    for i in (1, 2, 5):
        assert np.array_equal(plain.images[i], mixed.images[i])
    for i in (0, 3, 4):
        assert (plain.images[i] == 0xA5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_hand_scripts_decode(name):
    h, w = 33, 47
    files = [recoded(SCRIPTS[name], s, h, w, restart=r)[0] for s, r in ((2, 0), (0, 1), (1, 5))]
    assert all(probe_ex(f)[0] == _lib.CS_OK for f in files)
    check_files(files, h, w, pad=1)


@pytest.mark.gpu
def test_a_long_end_of_band_run_and_one_block_restart_intervals():
    img = np.full((264, 264, 3), 97, dtype=np.uint8)
    img[258:263, 257:262] = np.arange(75, dtype=np.uint8).reshape(5, 5, 3) * 3  # one detail, in the last block
    flat = jpeg_bytes(img, "gray", quality=90, progressive=True)
    stats = {}
    assert np.array_equal(prog.decode(flat), pil_array(flat))
    prog.quantised(flat, stats=stats)
    assert stats["max_eobrun"] >= 1024, stats
    check_files([flat, jpeg_bytes(img, "gray", quality=90)], 264, 264)
    h, w = 33, 47  # restart interval of one block in non-interleaved scans: 5 x 6 luma blocks, 3 x 3 chroma blocks, each its own interval
    check_files([recoded(PIL_SCRIPT, s, h, w, restart=1)[0] for s in (2, 1, 0)] + [recoded(SCRIPTS["non-interleaved DC"], 2, h, w, restart=1)[0]], h, w)


@pytest.mark.gpu
def test_levels_on_and_off_give_the_same_bytes(levels_switch):
    h, w = 33, 47
    files = [jpeg_bytes(content("mix", h, w, seed=1), 2, quality=95, progressive=True), jpeg_bytes(content("mix", h, w, seed=2), 0, quality=75, progressive=True, restart_marker_blocks=1),
             jpeg_bytes(content("noise", h, w, seed=3), "gray", progressive=True, restart_marker_blocks=3), recoded(SCRIPTS["chain 3 2 1 0"], 2, h, w, restart=2)[0],
             recoded(SCRIPTS["single-coefficient bands"], 1, h, w)[0]]
    runs = {}
    for on in (1, 0, 1):
        levels_switch(on)
        runs[on] = check_files(files, h, w, pad=2)
    for a, b in zip(runs[0].images, runs[1].images):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_a_file_decodes_the_same_alone_and_at_every_position_of_a_batch():
    h, w = 33, 50
    files = [jpeg_bytes(content("mix", h, w, seed=0), 2, quality=90, progressive=True), jpeg_bytes(content("noise", h, w, seed=1), 0, quality=100),
             jpeg_bytes(content("smooth", h, w, seed=2), 1, quality=30, progressive=True, restart_marker_blocks=1),
             jpeg_bytes(content("mix", h, w, seed=3), "gray", quality=90, progressive=True), recoded(SCRIPTS["chroma AC before luma AC"], 2, h, w, restart=3)[0]]
    alone = [check_files([f], h, w).images[0] for f in files]
    for shift in range(5):
        order = [(i + shift) % 5 for i in range(5)]
        d = check_files([files[i] for i in order], h, w, pad=shift)
        for pos, i in enumerate(order):
            assert np.array_equal(d.images[pos], alone[i]), (shift, pos)


def _replace(data: bytes, at: int, new: bytes, old_len=None) -> bytes:
    return data[:at] + new + data[at + (len(new) if old_len is None else old_len):]


@pytest.mark.gpu
def test_malformed_files_beside_good_ones():
    """Each malformed file sits between two good ones: it reports its documented status and its image keeps the sentinel; the neighbours decode
    exactly; the guard bands hold (checked inside Decode)."""
    S = _lib
    h, w = 33, 47
    first = jpeg_bytes(content("mix", h, w, seed=1), 2, quality=90, progressive=True, restart_marker_blocks=1)
    last = jpeg_bytes(content("noise", h, w, seed=2), 0, quality=95)
    plain = jpeg_bytes(content("mix", h, w, seed=4), 2, quality=90, progressive=True)
    scans, rscans = prog.parse(plain)["scans"], prog.parse(first)["scans"]
    assert len(scans) == 10 and len(rscans) == 10
    bad = {}
    for k, sc in enumerate(scans):  # the file ends half way through scan k: the data is short, or the walk finds no EOI
        bad[f"truncated inside scan {k + 1}"] = (plain[:(sc["start"] + sc["end"]) // 2], {S.JPGDEC_INPUT_EXHAUSTED, S.JPGDEC_BAD_FRAMING})
        cut = plain[:(sc["start"] + sc["end"]) // 2] + plain[sc["end"]:]  # scan k is short, the rest of the file follows
        bad[f"scan {k + 1} cut short"] = (cut, {S.JPGDEC_INPUT_EXHAUSTED, S.JPGDEC_BAD_CODE, S.JPGDEC_BAD_SYMBOL})
    # a corrupted code in an AC refinement scan: our fixed AC table has 176 codes of eight bits, so the byte FE is no code
    hand = recoded(PIL_SCRIPT, 2, h, w)[0]
    hs = prog.parse(hand)["scans"][5]
    assert (hs["ss"], hs["ah"]) == (1, 2)
    bad["no code in an AC refinement scan"] = (_replace(hand, hs["start"], b"\xfe\xfe\xfe\xfe"), {S.JPGDEC_BAD_CODE})
    assert probe_ex(plain)[0] == S.CS_OK
    for name, patched in (("Ah patched after probing", patch_sos(plain, 5, ah=3, al=2)), ("band patched after probing", patch_sos(plain, 4, ss=5)),
                          ("interleaved AC patched after probing", patch_sos(plain, 0, ss=1, se=5)), ("last scan dropped", plain[:scans[9]["sos"]] + plain[scans[9]["end"]:])):
        bad[name] = (patched, {S.JPGDEC_BAD_SCAN})
    marks = jpeg_oracle.restart_markers(first, rscans[4]["start"], rscans[4]["end"])
    assert len(marks) == 5 * 6 - 1
    bad["misnumbered RST in scan 5"] = (_replace(first, marks[2][0], b"\xff\xd5"), {S.JPGDEC_BAD_RESTART})
    bad["RST deleted in scan 5"] = (_replace(first, marks[4][0], b"", 2), {S.JPGDEC_BAD_RESTART})
    sof = plain.find(b"\xff\xc2")
    bad["SOF of another size"] = (_replace(plain, sof + 5, bytes([0, h + 1])), {S.JPGDEC_HEADER_MISMATCH})
    bad["a file of another size"] = (jpeg_bytes(content("mix", 17, 23), 2, progressive=True), {S.JPGDEC_HEADER_MISMATCH})
    anything = set(range(9))
    rng = np.random.default_rng(11)
    for k in (1, 5, 9):  # random bytes in the place of a first AC scan, an AC refinement scan and the last scan
        sc = scans[k]
        noise = rng.integers(0, 255, size=sc["end"] - sc["start"], dtype=np.uint8).tobytes()
        bad[f"random bytes in scan {k + 1}"] = (plain[:sc["start"]] + noise + plain[sc["end"]:], anything)
    work = None
    for name, (data, allowed) in bad.items():
        d = Decode([first, data, last], h, w, pad=11, work=work)
        work = d.work  # one workspace for every call: nothing a malformed file left there reaches the next decode
        assert d.st[0] == 0 and d.st[2] == 0, (name, d.st.tolist())
        assert np.array_equal(d.images[0], expected(first)) and np.array_equal(d.images[2], expected(last)), name
        assert int(d.st[1]) in allowed, (name, int(d.st[1]))
        if allowed is not anything:
            assert d.st[1] != 0, name
        if d.st[1] != 0:
            assert (d.images[1] == 0xA5).all(), name  # a rejected file has written no pixel
    d = check_files([plain, last, first], h, w, work=work)  # the same workspace, an ordinary decode
    assert d.st.tolist() == [0, 0, 0]


@pytest.mark.gpu
def test_decoder_class_takes_progressive_files(tmp_path):
    from PIL import Image

    from crossscore_amd.decode import ImageDecoder, read_image_u8

    paths = []

    def put(name, data):
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)

    def png(img):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="PNG")
        return buf.getvalue()

    put("a_rgb_20x30.png", png(content("mix", 20, 30, seed=1)))
    put("b_photo_20x30.jpg", jpeg_bytes(content("mix", 20, 30, seed=2), 2, quality=90))
    put("c_photo_20x30.JPG", jpeg_bytes(content("noise", 20, 30, seed=3), 0, quality=95, restart_marker_blocks=2))
    put("d_progressive.jpg", jpeg_bytes(content("mix", 20, 30, seed=6), 2, progressive=True))
    put("e_named_png_is_jpeg.png", jpeg_bytes(content("smooth", 20, 30, seed=4), 1))
    put("f_gray_9x11.jpeg", jpeg_bytes(content("mix", 9, 11, seed=5), "gray"))
    put("g_rgb_9x11.png", png(content("noise", 9, 11, seed=7)))

    def check(handle):
        handle.wait()
        handle.check()
        for p, t in zip(paths, handle.tensors):
            want = read_image_u8(p)
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.uint8 and tuple(t.shape) == want.shape, p
            assert np.array_equal(t.cpu().numpy(), want), p
        return sorted(os.path.basename(p) for p in handle.host_paths)

    dec = ImageDecoder("cuda", jpeg=True, progressive=True)
    assert check(dec.decode(paths)) == []
    assert dec.stats() == {"png_decoded_gpu": 2, "png_decoded_host": 0}
    assert dec.jpeg_stats() == {"jpeg_decoded_gpu": 5, "jpeg_decoded_host": 0}
    assert dec.progressive_stats() == {"jpeg_progressive_gpu": 1, "jpeg_progressive_host": 0}
    # an incomplete progressive file is PIL's (block smoothing), and counted so
    whole = open(paths[3], "rb").read()
    last = prog.parse(whole)["scans"][-1]
    put("h_incomplete.jpg", whole[:last["sos"]] + whole[last["end"]:])
    assert check(dec.decode(paths)) == ["h_incomplete.jpg"]
    assert dec.progressive_stats() == {"jpeg_progressive_gpu": 2, "jpeg_progressive_host": 1}
    paths.pop()
    old = ImageDecoder("cuda", jpeg=True)  # as before
    assert check(old.decode(paths)) == ["d_progressive.jpg"]
    assert old.jpeg_stats() == {"jpeg_decoded_gpu": 4, "jpeg_decoded_host": 1} and old.progressive_stats() == {"jpeg_progressive_gpu": 0, "jpeg_progressive_host": 0}
    with pytest.raises(ValueError, match="jpeg=True"):
        ImageDecoder("cuda", progressive=True)
