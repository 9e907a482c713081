"""PNG files for the encoder, decoder and driver tests: a validator stricter than PIL, the pieces of a hand-written file, test images, and the raw
call of the device encoder.

PIL alone is not a sufficient validator (it decodes files whose Adler-32 or last chunk CRC are wrong), so the files go through the chunk
parser here (signature, every chunk's length / type / CRC, chunk order) and through zlib.decompress over the concatenated IDAT payloads (which
verifies Adler-32), before PIL's pixels are compared."""
import ctypes as C
import io
import struct
import zlib

import numpy as np

from crossscore_amd import _lib

GRAY16, RGB8 = _lib.PNG_GRAY16, _lib.PNG_RGB8
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def row_bytes(kind, w):
    return w * (2 if kind == GRAY16 else 3)


def filtered_size(kind, h, w):
    return h * (1 + row_bytes(kind, w))


# ----------------------------------------------------------------------------------------------------------- the validator
def parse_chunks(data: bytes):
    """[(type, payload)] of a PNG file; asserts the signature, every chunk's CRC, the order IHDR, IDAT..., IEND and that nothing follows."""
    assert data[:8] == SIGNATURE, data[:8]
    pos, chunks = 8, []
    while pos < len(data):
        assert pos + 12 <= len(data), "truncated chunk"
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        typ = data[pos + 4:pos + 8]
        assert pos + 12 + n <= len(data), (typ, n, "chunk runs past the end of the file")
        payload = data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(typ + payload), (typ, len(chunks), hex(crc), hex(zlib.crc32(typ + payload)))
        chunks.append((typ, payload))
        pos += 12 + n
        if typ == b"IEND":
            break
    assert pos == len(data), "bytes after IEND"
    types = [t for t, _ in chunks]
    assert types[0] == b"IHDR" and types[-1] == b"IEND" and len(types) >= 3 and all(t == b"IDAT" for t in types[1:-1]), types
    assert len(chunks[0][1]) == 13 and len(chunks[-1][1]) == 0
    return chunks


def unfilter(stream: bytes, h: int, rb: int, bpp: int) -> np.ndarray:
    """PNG filter types 0-4 undone: (h, rb) uint8 raw row bytes."""
    a = np.frombuffer(stream, np.uint8).reshape(h, 1 + rb)
    assert a[:, 0].max() <= 4, "illegal filter type"
    out = np.zeros((h, rb), np.uint8)
    for y in range(h):
        ft, line = int(a[y, 0]), a[y, 1:]
        prev = out[y - 1] if y else np.zeros(rb, np.uint8)
        if ft == 0:
            out[y] = line
        elif ft == 1:  # Sub: a running sum per byte lane of the pixel
            for c in range(min(bpp, rb)):
                out[y, c::bpp] = np.cumsum(line[c::bpp].astype(np.uint64)).astype(np.uint8)
        elif ft == 2:
            out[y] = line + prev
        else:
            cur = np.zeros(rb, np.int64)
            for x in range(rb):
                left = cur[x - bpp] if x >= bpp else 0
                up = int(prev[x])
                ul = int(prev[x - bpp]) if x >= bpp else 0
                if ft == 3:
                    pred = (left + up) // 2
                else:
                    p = left + up - ul
                    pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
                    pred = left if pa <= pb and pa <= pc else (up if pb <= pc else ul)
                cur[x] = (int(line[x]) + pred) & 255
            out[y] = cur
    return out


def check_png(data: bytes, img: np.ndarray, kind: int):
    """Every condition of a valid, pixel-exact file."""
    from PIL import Image

    h, w = img.shape[:2]
    rb, bpp = row_bytes(kind, w), 2 if kind == GRAY16 else 3
    chunks = parse_chunks(data)
    ihdr = struct.unpack(">IIBBBBB", chunks[0][1])
    assert ihdr == (w, h, 16 if kind == GRAY16 else 8, 0 if kind == GRAY16 else 2, 0, 0, 0), ihdr
    stream = zlib.decompress(b"".join(p for t, p in chunks if t == b"IDAT"))  # raises on a wrong Adler-32
    assert len(stream) == h * (1 + rb)
    raw = unfilter(stream, h, rb, bpp)
    want = img.astype(">u2").view(np.uint8).reshape(h, rb) if kind == GRAY16 else img.reshape(h, rb)
    assert np.array_equal(raw, want)
    pil = Image.open(io.BytesIO(data))
    assert pil.mode == ("I;16" if kind == GRAY16 else "RGB"), pil.mode
    assert np.array_equal(np.array(pil), img)


# ------------------------------------------------------------------------------------------------------------ writing files
def chunk(typ: bytes, payload: bytes, crc=None) -> bytes:
    return struct.pack(">I", len(payload)) + typ + payload + struct.pack(">I", zlib.crc32(typ + payload) if crc is None else crc)


def ihdr(h, w, ct, depth, interlace=0) -> bytes:
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ct, 0, 0, interlace))


def pil_png(img, **kw) -> bytes:
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG", **kw)
    return buf.getvalue()


def interlaced_png(img: np.ndarray) -> bytes:
    """An Adam7 file written by hand (PIL reads them and writes none): filter type 0 on every pass row."""
    h, w = img.shape[:2]
    rows = []
    for y0, x0, dy, dx in ((0, 0, 8, 8), (0, 4, 8, 8), (4, 0, 8, 4), (0, 2, 4, 4), (2, 0, 4, 2), (0, 1, 2, 2), (1, 0, 2, 1)):
        sub = img[y0::dy, x0::dx]
        if sub.shape[0] and sub.shape[1]:
            rows += [b"\0" + sub[y].tobytes() for y in range(sub.shape[0])]
    return SIGNATURE + ihdr(h, w, 2, 8, interlace=1) + chunk(b"IDAT", zlib.compress(b"".join(rows))) + chunk(b"IEND", b"")


def image_of(rng, h, w, form):
    if form == "gray16":
        return rng.integers(0, 65536, size=(h, w)).astype(np.uint16)
    c = {"gray8": (), "rgb": (3,), "rgba": (4,)}[form]
    base = rng.integers(0, 256, size=(h, w) + c).astype(np.int64)
    ramp = (np.arange(h)[:, None] * 5 + np.arange(w)[None, :] * 3).reshape((h, w) + (1,) * len(c))
    return ((base // 8 + ramp) % 256).astype(np.uint8)  # locally smooth: every filter type and real matches


# ------------------------------------------------------------------------------------------------------------ the device encoder
def encode_raw(pixels, kind: int, slot=None):
    """cs_op_png_encode itself on a device tensor of I images: (files, lengths, bound)."""
    import torch

    lib = _lib.load()
    I, H, W = (int(v) for v in pixels.shape[:3])
    bound = lib.cs_png_bound(kind, H, W)
    slot = bound if slot is None else slot
    out = torch.zeros((I, slot), dtype=torch.uint8, device="cuda")
    lengths = torch.zeros((I,), dtype=torch.int32, device="cuda")
    work = torch.empty((lib.cs_png_workspace_bytes(kind, I, H, W),), dtype=torch.uint8, device="cuda")
    _lib.check(lib.cs_op_png_encode(C.c_void_p(pixels.data_ptr()), kind, I, H, W, H * row_bytes(kind, W), C.c_void_p(out.data_ptr()), slot,
                                    C.c_void_p(lengths.data_ptr()), C.c_void_p(work.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    ln = lengths.cpu().numpy()
    o = out.cpu().numpy()
    return [o[i, :ln[i]].tobytes() for i in range(I)], ln, bound


def score_map(h, w, seed):
    """A score map as the model leaves it: smooth structure at the patch scale plus pixel noise, values over [0, 1] and slightly beyond."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    s = 0.55 + 0.3 * np.sin(xx / 23.0 + 0.3) * np.cos(yy / 17.0) + 0.15 * np.sin((xx + yy) / 7.0)
    s += rng.normal(0, 0.01, size=s.shape)
    return (np.round(s * 64) / 64).astype(np.float32) if seed % 2 else s.astype(np.float32)


def contents(kind, h, w):
    """constant, horizontal ramp, uniform noise, a score map converted by cs_op_score_to_gray16 / cs_op_score_to_rgb -> (4, ...) array."""
    import torch

    from crossscore_amd.writers import ScoreMapEncoder

    rng = np.random.Generator(np.random.PCG64(h * 4099 + w))
    dev = torch.device("cuda")
    score = torch.from_numpy(score_map(h, w, h + w)).to(dev)[None]
    if kind == GRAY16:
        const = np.full((h, w), 0xA1B2, np.uint16)
        ramp = np.broadcast_to((np.arange(w, dtype=np.uint32) * 257 % 65536).astype(np.uint16), (h, w))
        noise = rng.integers(0, 65536, size=(h, w), dtype=np.uint16)
        real = ScoreMapEncoder("ssim", 0, 1, "gray", dev).device_image(score).cpu().numpy().view(np.uint16)[0]
    else:
        const = np.broadcast_to(np.array([200, 17, 96], np.uint8), (h, w, 3))
        ramp = np.broadcast_to(np.stack([np.arange(w) % 256, (np.arange(w) // 2) % 256, 255 - np.arange(w) % 256], 1).astype(np.uint8), (h, w, 3))
        noise = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        real = ScoreMapEncoder("ssim", 0, 1, "rgb", dev).device_image(score).cpu().numpy()[0]
    return np.stack([const, ramp, noise, real])
