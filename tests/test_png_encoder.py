"""Device PNG encoder (cs_op_png_encode, cs_op_denorm_to_rgb8, writers.PngEncoder): host-side contract on the CPU, files on the GPU.

PIL alone is not a sufficient validator (it decodes files whose Adler-32 or last chunk CRC are wrong), so the files go through the chunk
parser of tests/png_files.py (signature, every chunk's length / type / CRC, chunk order) and through zlib.decompress over the concatenated
IDAT payloads (which verifies Adler-32), before PIL's pixels are compared."""
import ctypes as C
import io
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
from crossscore_amd import _lib  # noqa: E402
from crossscore_amd.config import load_config  # noqa: E402
from png_files import GRAY16, RGB8, check_png, contents, encode_raw, filtered_size, parse_chunks, row_bytes  # noqa: E402

NEW_SYMBOLS = ("cs_png_bound", "cs_png_workspace_bytes", "cs_op_png_encode", "cs_op_denorm_to_rgb8")


def test_validator_rejects_what_pil_accepts():
    """The parser and zlib catch a wrong chunk CRC and a wrong Adler-32 (guards the guard)."""
    from PIL import Image

    buf = io.BytesIO()
    img = np.arange(12 * 9 * 3, dtype=np.uint8).reshape(12, 9, 3)
    Image.fromarray(img).save(buf, format="PNG")
    good = buf.getvalue()
    check_png(good, img, RGB8)
    bad = bytearray(good)
    bad[-13] ^= 1  # last byte of the IDAT chunk's CRC
    with pytest.raises(AssertionError):
        parse_chunks(bytes(bad))
    chunks = parse_chunks(good)
    idat = bytearray(b"".join(p for t, p in chunks if t == b"IDAT"))
    idat[-1] ^= 1  # Adler-32
    with pytest.raises(zlib.error):
        zlib.decompress(bytes(idat))


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_new_symbols_declared_listed_and_exported():
    hdr = open(os.path.join(REPO, "include", "crossscore_hip.h")).read()
    declared = set(re.findall(r"\b(cs_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "CS_PNG_GRAY16" in hdr and "CS_PNG_RGB8" in hdr
    assert "png.hip" in __import__("crossscore_amd.build", fromlist=["SOURCES"]).SOURCES


SIZES_BOUND = [(1, 1), (14, 14), (75, 91), (518, 518), (518, 686), (1036, 1036)]


@pytest.mark.parametrize("kind", [GRAY16, RGB8])
@pytest.mark.parametrize("h,w", SIZES_BOUND)
def test_bound_and_workspace_are_host_arithmetic(kind, h, w):
    lib = _lib.load()
    f = filtered_size(kind, h, w)
    b = lib.cs_png_bound(kind, h, w)
    assert f <= b <= 1.005 * f + 256, (f, b)
    ws = lib.cs_png_workspace_bytes(kind, 8, h, w)
    assert ws >= b and ws == 8 * lib.cs_png_workspace_bytes(kind, 1, h, w)


def test_bound_of_unknown_kind_or_size_is_zero():
    lib = _lib.load()
    assert lib.cs_png_bound(2, 4, 4) == 0 and lib.cs_png_bound(RGB8, 0, 4) == 0 and lib.cs_png_bound(RGB8, 4, -1) == 0
    assert lib.cs_png_bound(RGB8, 4096, 4096) > 0 and lib.cs_png_bound(RGB8, 4097, 16) == 0
    assert lib.cs_png_workspace_bytes(RGB8, 0, 4, 4) == 0


def test_png_encode_rejects_bad_arguments_on_the_host():
    """Unknown kind, W = 0, a slot below the bound: CS_ERR_BAD_ARG with a message, before any device call (this runs without a GPU)."""
    lib = _lib.load()
    dummy = (C.c_uint8 * 64)()
    p = C.cast(dummy, C.c_void_p)
    bound = lib.cs_png_bound(RGB8, 16, 16)

    def call(kind, i, h, w, stride, slot):
        return lib.cs_op_png_encode(p, kind, i, h, w, stride, p, slot, p, p, None)

    for args, word in (((7, 1, 16, 16, 768, bound), b"kind"), ((RGB8, 1, 16, 0, 768, bound), b"sizes"), ((RGB8, 0, 16, 16, 768, bound), b"sizes"),
                       ((RGB8, 1, 16, 16, 768, bound - 1), b"bound"), ((RGB8, 1, 16, 16, 767, bound), b"stride"),
                       ((GRAY16, 1, 16, 16, 513, lib.cs_png_bound(GRAY16, 16, 16)), b"stride")):
        assert call(*args) == _lib.CS_ERR_BAD_ARG, args
        assert word in lib.cs_last_error(), (args, lib.cs_last_error())
    assert call(RGB8, 1, 4097, 16, 4097 * 48, 1 << 30) == _lib.CS_ERR_UNSUPPORTED and b"4096" in lib.cs_last_error()
    assert lib.cs_op_png_encode(None, RGB8, 1, 16, 16, 768, p, bound, p, p, None) == _lib.CS_ERR_BAD_ARG
    assert lib.cs_op_denorm_to_rgb8(None, 1, 4, 4, None, None, None, None) == _lib.CS_ERR_BAD_ARG


def test_png_encoder_key_is_validated():
    from crossscore_amd.writers import png_encoder_choice

    for name in ("default_predict", "default_test"):
        assert png_encoder_choice(load_config(name)) == "host"
        assert png_encoder_choice(load_config(name, ["this_main.png_encoder=gpu"])) == "gpu"
        with pytest.raises(ValueError):
            png_encoder_choice(load_config(name, ["this_main.png_encoder=zip"]))
    cfg = load_config("default_predict")
    del cfg.this_main["png_encoder"]  # a config file written before the key existed
    assert png_encoder_choice(cfg) == "host"


# ----------------------------------------------------------------------------------------------------------------- GPU


SIZES = [(1, 1), (1, 7), (14, 14), (75, 91), (518, 518), (518, 686), (1036, 1036)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [GRAY16, RGB8])
@pytest.mark.parametrize("h,w", SIZES)
def test_files_are_valid_and_pixel_exact(kind, h, w):
    imgs = contents(kind, h, w)
    dev_imgs = torch.from_numpy(imgs.view(np.int16) if kind == GRAY16 else imgs).cuda()
    files, ln, bound = encode_raw(dev_imgs, kind)
    raw = h * row_bytes(kind, w)
    print(f"kind {kind} {h}x{w}: bound {bound}, raw {raw}, lengths const/ramp/noise/map {ln.tolist()}")
    for i, name in enumerate(("constant", "ramp", "noise", "score map")):
        assert ln[i] <= bound, (name, ln[i], bound)  # (the noise image takes the stored fallback: its fixed-Huffman form is ~1.06 x raw)
        check_png(files[i], imgs[i], kind)
    if (h, w) == (518, 686) and kind == RGB8:
        assert ln[0] < raw / 10, (ln[0], raw)  # long matches are really emitted


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [GRAY16, RGB8])
def test_slot_larger_than_the_bound_and_untouched_tail(kind):
    h, w = 75, 91
    imgs = contents(kind, h, w)
    dev_imgs = torch.from_numpy(imgs.view(np.int16) if kind == GRAY16 else imgs).cuda()
    lib = _lib.load()
    slot = lib.cs_png_bound(kind, h, w) + 37  # odd slot size: files start at any byte alignment
    files, ln, _ = encode_raw(dev_imgs, kind, slot=slot)
    for i in range(4):
        check_png(files[i], imgs[i], kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,h,w", [(GRAY16, 75, 91), (RGB8, 518, 518)])
def test_bytes_do_not_depend_on_the_batch(kind, h, w):
    """Image k of a batch of 8 = the same image alone = the same image at another position among other images."""
    parts = [contents(kind, h, w), contents(kind, h, w)[::-1].copy()]
    parts[1][0] = np.roll(parts[1][0], 5, axis=1)  # eight different images
    parts[1][3] = np.roll(parts[1][3], 3, axis=0)
    imgs = np.concatenate(parts)
    as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if kind == GRAY16 else np.ascontiguousarray(a)).cuda()  # noqa: E731
    batch, _, _ = encode_raw(as_dev(imgs), kind)
    assert len(batch) == 8
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    shuffled, _, _ = encode_raw(as_dev(imgs[perm]), kind)
    for k in range(8):
        alone, _, _ = encode_raw(as_dev(imgs[k:k + 1]), kind)
        assert alone[0] == batch[k], k
        assert shuffled[perm.index(k)] == batch[k], k


def _processed_images():
    """Tensors from the real input stage: one image without a resize, one with, one all-zero placeholder -> [(3, h, w) fp32 device]."""
    from crossscore_amd.data import InputStage

    rng = np.random.Generator(np.random.PCG64(21))
    dev = torch.device("cuda")
    outs = []
    for (h, w), short in (((70, 84), -1), ((150, 201), 56), ((61, 93), 70)):
        img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        img[0, :6] = [[0, 0, 0], [255, 255, 255], [0, 255, 0], [255, 0, 255], [1, 1, 1], [254, 254, 254]]
        st = InputStage(dev, resize_short_side=short)
        _, crop = st.geometry(h, w)
        o = torch.empty((3, crop[2], crop[3]), dtype=torch.float32, device=dev)
        st(img, o)
        outs.append(o)
    st = InputStage(dev, resize_short_side=-1)
    outs.append(st.zero_image_value[:, None, None].expand(3, 33, 47).contiguous())  # the placeholder of a missing reference: black after Normalize
    outs.append(torch.zeros((3, 20, 31), dtype=torch.float32, device=dev))          # an all-zero tensor
    return outs


@pytest.mark.gpu
def test_denorm_equals_the_host_form_bit_for_bit():
    from crossscore_amd.data import IMAGENET_MEAN_STD
    from crossscore_amd.writers import BatchWriter, denorm_to_rgb8

    ms = torch.tensor(list(IMAGENET_MEAN_STD), dtype=torch.float32)
    host = BatchWriter.__new__(BatchWriter)
    host.img_mean_std = ms
    for t in _processed_images():
        want = host._de_norm_u8(t)
        got = denorm_to_rgb8(t[None], ms).cpu().numpy()[0]
        assert got.shape == want.shape and np.array_equal(got, want), np.abs(got.astype(int) - want.astype(int)).max()
    same = _processed_images()[0]
    got = denorm_to_rgb8(torch.stack([same, same, same]), ms).cpu().numpy()
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], host._de_norm_u8(same))


@pytest.mark.gpu
def test_png_encoder_class_sync_and_async():
    from crossscore_amd.writers import PngEncoder

    enc = PngEncoder()
    for kind, (h, w) in ((GRAY16, (75, 91)), (RGB8, (14, 14))):
        imgs = contents(kind, h, w)
        dev = torch.from_numpy(imgs.view(np.int16) if kind == GRAY16 else imgs).cuda()
        files = enc.encode(dev)
        raw, _, _ = encode_raw(dev, kind)
        assert files == raw
        for i in range(4):
            check_png(files[i], imgs[i], kind)
        handle = enc.encode_async(dev)
        assert len(handle) == 4 and handle.bytes(2) == raw[2] and handle.result() == raw
    with pytest.raises(ValueError):
        enc.encode(torch.zeros((2, 4, 4), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        enc.encode(torch.zeros((2, 4, 4, 3), dtype=torch.uint8))


@pytest.mark.gpu
def test_async_encode_does_not_wait_for_the_stream():
    """encode_async queues behind work already on the stream and returns while the stream is still busy."""
    from crossscore_amd.writers import PngEncoder

    enc = PngEncoder()
    imgs = contents(RGB8, 75, 91)
    dev = torch.from_numpy(imgs).cuda()
    want = enc.encode(dev)  # kernels, pinned blocks and allocator pools exist from here on
    # device time ahead of the encode on the current stream, from the project's own op: 16 encodes of 8 noise images of 1036 x 1036
    # (1 573 segment workgroups each, with one workgroup per compute unit at a time), into buffers allocated beforehand
    lib = _lib.load()
    h, w, n = 1036, 1036, 8
    big = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
    slot = lib.cs_png_bound(RGB8, h, w)
    out = torch.empty((n, slot), dtype=torch.uint8, device="cuda")
    lengths = torch.empty((n,), dtype=torch.int32, device="cuda")
    work = torch.empty((lib.cs_png_workspace_bytes(RGB8, n, h, w),), dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for _ in range(16):
        _lib.check(lib.cs_op_png_encode(C.c_void_p(big.data_ptr()), RGB8, n, h, w, h * w * 3, C.c_void_p(out.data_ptr()), slot,
                                        C.c_void_p(lengths.data_ptr()), C.c_void_p(work.data_ptr()), st))
    handle = enc.encode_async(dev)
    assert not torch.cuda.current_stream().query()  # the host is back while the stream is still busy
    assert handle.result() == want
