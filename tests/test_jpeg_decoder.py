"""The device JPEG decoder (csrc/jpegdec.hip, cs_op_jpeg_decode, decode.ImageDecoder(jpeg=True)): every decoded image equals, bit for bit, what
read_image_u8 makes of PIL's array for the same bytes.  No tolerances.  Malformed files end with their documented status beside good files that
still decode; pixels, status words and workspace sit inside guard bands."""
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
from crossscore_amd import _lib  # noqa: E402
from guard import guarded  # noqa: E402
from jpeg_files import SAMPLINGS, content, grid_files, jpeg_bytes, probe  # noqa: E402


def expected(data: bytes) -> np.ndarray:
    from crossscore_amd.decode import read_image_u8

    return read_image_u8(io.BytesIO(data))


class Decode:
    """cs_op_jpeg_decode on files of one size, inside guard bands: pixels (padded image stride), status and workspace."""

    def __init__(self, files, h, w, pad=0, work=None):
        lib = _lib.load()
        n = len(files)
        lengths = np.array([len(f) for f in files], dtype=np.uint32)
        offsets = np.zeros(n, dtype=np.uint64)
        offsets[1:] = np.cumsum(lengths.astype(np.uint64))[:-1]
        total = int(lengths.sum())
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
        self.keep = [dev(np.frombuffer(b"".join(files), np.uint8)), dev(offsets), dev(lengths)]
        self.stride = h * w * 3 + pad
        self.pix = guarded((n, h * w * 3), torch.uint8, ld=self.stride, guard_rows=1)  # one image of sentinel before and behind
        self.status = guarded((n,), torch.int32, guard_rows=0)
        ws = lib.cs_jpeg_decode_workspace_bytes(n, h, w, total)
        assert ws > 0
        self.work = work if work is not None else guarded((ws,), torch.uint8, guard_rows=0)
        assert self.work.shape[0] >= ws
        _lib.check(lib.cs_op_jpeg_decode(*(C.c_void_p(t.data_ptr()) for t in self.keep), total, n, h, w, C.c_void_p(self.pix.view.data_ptr()), self.stride,
                                         C.c_void_p(self.status.view.data_ptr()), C.c_void_p(self.work.view.data_ptr()),
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


def by_size(named_files):
    groups = {}
    for name, data in named_files:
        h, w = (int(v) for v in name.split(" ")[0].split("x"))
        groups.setdefault((h, w), []).append((name, data))
    return groups


@pytest.mark.gpu
def test_the_grid_equals_pil():
    """The host test's grid (sampling x quality / optimised tables x restart forms x sizes x content): one call per size, so every call mixes
    4:4:4, 4:2:2, 4:2:0 and gray files."""
    n = 0
    for (h, w), members in by_size(grid_files()).items():
        check_files([d for _, d in members], h, w, [m for m, _ in members], pad=(h + w) % 7)
        n += len(members)
    assert n > 500


@pytest.mark.gpu
def test_sizes_where_the_stages_can_go_wrong():
    """5 x 5 (smallest subsampled); 15 x 17 and 16 x 33 (partial MCUs on both edges, odd chroma width); 17 x 23; 64 x 72 and 56 x 72 with one MCU
    per restart interval (more intervals than waves: 72 / 40 / 20 and 63 / 35 / 20 of them, 63 and 35 no multiples of four); 40 x 72 with one MCU
    row per interval; 130 x 70, whose 4:2:0 chroma crosses several block-row seams of the vertical filter."""
    cases = [((5, 5), {}), ((15, 17), {}), ((16, 33), {}), ((17, 23), {}), ((17, 23), dict(restart_marker_blocks=1)), ((64, 72), dict(restart_marker_blocks=1)),
             ((56, 72), dict(restart_marker_blocks=1)), ((40, 72), dict(restart_marker_rows=1)), ((130, 70), {}), ((130, 70), dict(restart_marker_blocks=2))]
    for (h, w), extra in cases:
        files, names = [], []
        for s in SAMPLINGS:
            for kind, q in (("mix", 90), ("noise", 100), ("smooth", 50)):
                files.append(jpeg_bytes(content(kind, h, w, seed=3), s, quality=q, **extra))
                names.append(f"{h}x{w} {s} {kind} q{q} {extra}")
        check_files(files, h, w, names, pad=5)
    hdr = jpeg_oracle.parse(jpeg_bytes(content("mix", 56, 72), 0, restart_marker_blocks=1))
    assert hdr["ri"] == 1  # 63 intervals


@pytest.mark.gpu
def test_a_file_decodes_the_same_alone_and_at_every_position_of_a_batch():
    h, w = 33, 50
    files = [jpeg_bytes(content(k, h, w, seed=i), s, quality=q, **extra)
             for i, (k, s, q, extra) in enumerate((("mix", 2, 90, {}), ("noise", 0, 100, {}), ("smooth", 1, 30, dict(restart_marker_blocks=1)),
                                                    ("mix", "gray", 90, {}), ("noise", 2, 75, dict(restart_marker_rows=1))))]
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
    h, w = 33, 50
    first = jpeg_bytes(content("mix", h, w, seed=1), 2, quality=90, restart_marker_blocks=1)  # 3 x 4 MCUs: 11 markers
    last = jpeg_bytes(content("noise", h, w, seed=2), 0, quality=95)
    plain = jpeg_bytes(content("mix", h, w, seed=4), 2, quality=90)
    gray = jpeg_bytes(content("mix", h, w, seed=5), "gray", quality=90)
    hp, hf = jpeg_oracle.parse(plain), jpeg_oracle.parse(first)
    marks = jpeg_oracle.restart_markers(first, hf["entropy"], jpeg_oracle.scan_end(first, hf["entropy"]))
    assert len(marks) == 11 and [n for _, n in marks] == [k & 7 for k in range(11)]
    bad = {}
    e = hp["entropy"]
    bad["scan truncated mid-MCU"] = (plain[:e + (len(plain) - e) // 2], {S.JPGDEC_INPUT_EXHAUSTED})
    bad["scan truncated mid-MCU, restart intervals"] = (first[:marks[5][0] - 3], {S.JPGDEC_INPUT_EXHAUSTED, S.JPGDEC_BAD_RESTART})
    bad["restart marker with the wrong number"] = (_replace(first, marks[2][0], b"\xff\xd5"), {S.JPGDEC_BAD_RESTART})
    bad["restart marker deleted"] = (_replace(first, marks[4][0], b"", 2), {S.JPGDEC_BAD_RESTART})
    bad["surplus restart marker"] = (_replace(first, marks[6][0], b"\xff\xd6\xff\xd7", 2), {S.JPGDEC_BAD_RESTART})
    dht = next(pos for m, pos, _ in hp["segments"] if m == 0xC4)
    bad["over-subscribed DHT"] = (_replace(plain, dht + 5, b"\x03"), {S.JPGDEC_BAD_TABLE})  # three codes of one bit
    bad["DHT counts past the segment"] = (_replace(plain, dht + 5 + 15, b"\xc8"), {S.JPGDEC_BAD_TABLE})  # 200 codes of 16 bits
    hg = jpeg_oracle.parse(gray)
    assert sorted(hg["dc"]) == [0] and sorted(hg["ac"]) == [0]
    bad["scan selects an undefined table"] = (_replace(gray, hg["entropy"] - 4, b"\x11"), {S.JPGDEC_BAD_TABLE})
    sof = next(pos for m, pos, _ in hp["segments"] if m == 0xC0)
    bad["SOF of another size"] = (_replace(plain, sof + 5, bytes([0, h + 1])), {S.JPGDEC_HEADER_MISMATCH})
    bad["a file of another size"] = (jpeg_bytes(content("mix", 17, 23), 2), {S.JPGDEC_HEADER_MISMATCH})
    bad["segment length past the file"] = (_replace(plain, 4, b"\xff\xff"), {S.JPGDEC_BAD_FRAMING})
    bad["no SOI"] = (b"\x89PNG" + plain[4:], {S.JPGDEC_BAD_FRAMING})
    bad["ends before SOS"] = (plain[:e - 20], {S.JPGDEC_BAD_FRAMING})
    anything = set(range(8))
    rng = np.random.default_rng(7)
    n_scan = len(plain) - e - 2
    bad["entropy bytes FF FF"] = (plain[:e + 40] + b"\xff" * (n_scan - 40) + plain[-2:], anything)
    bad["entropy bytes FF 00"] = (plain[:e + 40] + b"\xff\x00" * ((n_scan - 40) // 2) + plain[-2:], anything)
    bad["entropy bytes FF D0"] = (first[:hf["entropy"] + 10] + b"\xff\xd0" * 40 + first[-2:], anything)
    for k in range(3):
        bad[f"entropy bytes random {k}"] = (plain[:e] + rng.integers(0, 256, size=n_scan, dtype=np.uint8).tobytes() + plain[-2:], anything)
        r = rng.integers(0, 255, size=len(first) - hf["entropy"] - 2, dtype=np.uint8).tobytes()  # no FF: the markers below stay the only ones
        body = bytearray(r)
        for pos, n in marks:
            body[pos - hf["entropy"]:pos - hf["entropy"] + 2] = bytes([0xFF, 0xD0 + n])
        bad[f"random bytes between the restart markers {k}"] = (first[:hf["entropy"]] + bytes(body) + first[-2:], anything)
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
    d = check_files([gray, plain, first], h, w, work=work)  # the same workspace, an ordinary decode
    assert d.st.tolist() == [0, 0, 0]


@pytest.mark.gpu
def test_png_decoder_class_takes_jpeg_files(tmp_path):
    from PIL import Image

    from crossscore_amd.decode import ImageDecoder, read_image_u8

    paths = []

    def put(name, data):
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
        return p

    def png(img):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="PNG")
        return buf.getvalue()

    buf = io.BytesIO()
    Image.fromarray(content("mix", 20, 30, seed=6)).save(buf, format="JPEG", progressive=True)
    put("a_rgb_20x30.png", png(content("mix", 20, 30, seed=1)))
    put("b_photo_20x30.jpg", jpeg_bytes(content("mix", 20, 30, seed=2), 2, quality=90))
    put("c_photo_20x30.JPG", jpeg_bytes(content("noise", 20, 30, seed=3), 0, quality=95, restart_marker_blocks=2))
    put("d_progressive.jpg", buf.getvalue())
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

    dec = ImageDecoder("cuda", jpeg=True)
    handle = dec.decode(paths)
    assert check(handle) == ["d_progressive.jpg"]
    assert dec.stats() == {"png_decoded_gpu": 2, "png_decoded_host": 0}
    assert dec.jpeg_stats() == {"jpeg_decoded_gpu": 4, "jpeg_decoded_host": 1}
    b, c, e = (handle.tensors[k] for k in (1, 2, 4))  # the JPEG files of one size are slices of one tensor, in request order
    assert c.data_ptr() == b.data_ptr() + 20 * 30 * 3 and e.data_ptr() == c.data_ptr() + 20 * 30 * 3
    # the default-constructed decoder is what it was: every JPEG goes through PIL and counts as a host file
    dec0 = ImageDecoder("cuda")
    assert check(dec0.decode(paths)) == ["b_photo_20x30.jpg", "c_photo_20x30.JPG", "d_progressive.jpg", "e_named_png_is_jpeg.png", "f_gray_9x11.jpeg"]
    assert dec0.stats() == {"png_decoded_gpu": 2, "png_decoded_host": 5} and dec0.jpeg_stats() == {"jpeg_decoded_gpu": 0, "jpeg_decoded_host": 0}
    # png=False: the PNG files take the host path inside the decoder
    dec1 = ImageDecoder("cuda", png=False, jpeg=True)
    assert check(dec1.decode(paths)) == ["a_rgb_20x30.png", "d_progressive.jpg", "g_rgb_9x11.png"]
    assert dec1.stats() == {"png_decoded_gpu": 0, "png_decoded_host": 2} and dec1.jpeg_stats() == {"jpeg_decoded_gpu": 4, "jpeg_decoded_host": 1}
    # a damaged scan raises, naming the path and the status; a JPEG asked for as a 16-bit map is the host reader's error, as before
    good = open(paths[1], "rb").read()
    e0 = probe(good)[1].entropy_offset
    bad_path = put("z_damaged.jpg", good[:e0 + (len(good) - e0) // 2])
    handle = dec.decode([paths[1], bad_path, paths[2]])
    with pytest.raises(ValueError, match=r"z_damaged\.jpg.*JPEG.*status 6"):
        handle.check()
    with pytest.raises(ValueError):
        dec.decode([paths[1]], True)
