"""Baseline JPEG decoder in numpy int64, from file bytes: the arithmetic csrc/jpegdec.hip restates -- canonical Huffman
decode with restart intervals, dequantisation, the jpeg_idct_islow integer IDCT (CONST_BITS 13, PASS1_BITS 2), the "fancy" triangle chroma
upsampling of 4:2:2 / 4:2:0 and the 16-bit fixed-point YCbCr -> RGB conversion.  tests/test_jpeg_host.py pins it to PIL's pixels, bit for bit;
the GPU tests compare the device decoder with PIL directly and use parse() to cut files apart."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class JpegError(ValueError):
    pass


def parse(data: bytes) -> dict:
    """Marker walk up to SOS: {"width", "height", "comps": [(id, h, v, tq)], "scan": [(comp index, td, ta)], "qt": {id: (64,) zig-zag order},
    "dc" / "ac": {id: (counts[16], symbols)}, "ri", "entropy": offset of the entropy-coded data, "segments": [(marker, offset of FF, end)]}"""
    if data[:2] != b"\xff\xd8":
        raise JpegError("no SOI")
    out = {"qt": {}, "dc": {}, "ac": {}, "ri": 0, "segments": [], "comps": None, "sof": None}
    pos = 2
    while True:
        if pos + 4 > len(data) or data[pos] != 0xFF:
            raise JpegError(f"bad framing at {pos}")
        m = data[pos + 1]
        n = (data[pos + 2] << 8) | data[pos + 3]
        end = pos + 2 + n
        if n < 2 or end > len(data):
            raise JpegError(f"segment at {pos} runs past the file")
        seg = data[pos + 4:end]
        out["segments"].append((m, pos, end))
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            out["sof"] = m
            out["height"], out["width"] = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            out["precision"] = seg[0]
            out["comps"] = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])]
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                tc, th = seg[p] >> 4, seg[p] & 15
                counts = list(seg[p + 1:p + 17])
                ns = sum(counts)
                out["ac" if tc else "dc"][th] = (counts, list(seg[p + 17:p + 17 + ns]))
                p += 17 + ns
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                if seg[p] >> 4:
                    raise JpegError("16-bit quantisation table")
                out["qt"][seg[p] & 15] = np.array(list(seg[p + 1:p + 65]), dtype=np.int64)
                p += 65
        elif m == 0xDD:
            out["ri"] = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            ns = seg[0]
            ids = [c[0] for c in out["comps"]]
            out["scan"] = [(ids.index(seg[1 + 2 * i]), seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(ns)]
            out["entropy"] = end
            return out
        pos = end


def scan_end(data: bytes, start: int) -> int:
    """offset of the first marker behind `start` that is neither a stuffed FF 00 nor RSTn (EOI in a well-formed file), or len(data)"""
    i = start
    while i + 1 < len(data):
        if data[i] == 0xFF and data[i + 1] != 0 and not 0xD0 <= data[i + 1] <= 0xD7 and data[i + 1] != 0xFF:
            return i
        i += 1
    return len(data)


def restart_markers(data: bytes, start: int, end: int):
    """[(offset, n)] of every RSTn in data[start:end)"""
    return [(i, data[i + 1] - 0xD0) for i in range(start, end - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]


class _Bits:
    def __init__(self, raw: bytes):
        raw = raw.replace(b"\xff\x00", b"\xff")
        self.total = 8 * len(raw)
        self.v = int.from_bytes(raw + b"\0\0\0\0", "big")
        self.shift = self.total + 32
        self.pos = 0

    def peek16(self):
        return (self.v >> (self.shift - self.pos - 16)) & 0xFFFF

    def take(self, n):
        if n == 0:
            return 0
        r = (self.v >> (self.shift - self.pos - n)) & ((1 << n) - 1)
        self.pos += n
        if self.pos > self.total:
            raise JpegError("entropy data exhausted")
        return r


class _Huff:
    def __init__(self, counts, symbols):
        self.first, self.start, self.counts, self.symbols = [0] * 17, [0] * 17, [0] + list(counts), symbols
        code = off = 0
        for l in range(1, 17):
            self.first[l], self.start[l] = code, off
            code = (code + self.counts[l]) << 1
            off += self.counts[l]

    def decode(self, b: _Bits):
        w = b.peek16()
        for l in range(1, 17):
            c = w >> (16 - l)
            if c - self.first[l] < self.counts[l] and c >= self.first[l]:
                b.take(l)
                return self.symbols[self.start[l] + c - self.first[l]]
        raise JpegError("no such code")


def coefficients(data: bytes, hdr=None):
    """Dequantised coefficients in natural order: per component of the scan an int64 array (block rows, block columns, 64), padded to whole MCUs."""
    h = hdr or parse(data)
    comps = h["comps"]
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mx, my = -(-h["width"] // (8 * hmax)), -(-h["height"] // (8 * vmax))
    planes = [np.zeros((my * c[2], mx * c[1], 64), dtype=np.int64) for c in comps]
    dc = {k: _Huff(*v) for k, v in h["dc"].items()}
    ac = {k: _Huff(*v) for k, v in h["ac"].items()}
    start, end = h["entropy"], scan_end(data, h["entropy"])
    marks = restart_markers(data, start, end)
    ri, total = h["ri"], mx * my
    nint = -(-total // ri) if ri else 1
    if len(marks) != nint - 1 or any(n != (k & 7) for k, (_, n) in enumerate(marks)):
        raise JpegError("restart markers")
    bounds = [start] + [p + 2 for p, _ in marks]
    ends = [p for p, _ in marks] + [end]
    for k in range(nint):
        b = _Bits(data[bounds[k]:ends[k]])
        pred = [0] * len(comps)
        for mcu in range(k * ri if ri else 0, min(total, (k + 1) * ri) if ri else total):
            my0, mx0 = divmod(mcu, mx)
            for ci, td, ta in h["scan"]:
                _, ch, cv, tq = comps[ci]
                q = h["qt"][tq]
                for by in range(cv):
                    for bx in range(ch):
                        blk = planes[ci][my0 * cv + by, mx0 * ch + bx]
                        s = dc[td].decode(b)
                        if s > 11:
                            raise JpegError("DC category")
                        v = b.take(s)
                        pred[ci] += v if s == 0 or v >> (s - 1) else v - (1 << s) + 1
                        blk[0] = pred[ci] * q[0]
                        kk = 1
                        while kk < 64:
                            rs = ac[ta].decode(b)
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                kk += 16
                                continue
                            kk += r
                            if kk > 63 or s > 10:
                                raise JpegError("AC symbol")
                            v = b.take(s)
                            blk[ZIGZAG[kk]] = (v if v >> (s - 1) else v - (1 << s) + 1) * q[kk]
                            kk += 1
    return planes


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_1d(c, shift):
    """jpeg_idct_islow's butterfly along the last axis (8 entries) of an int64 array"""
    c0, c1, c2, c3, c4, c5, c6, c7 = (c[..., i] for i in range(8))
    z1 = (c2 + c6) * 4433
    t2 = z1 - c6 * 15137
    t3 = z1 + c2 * 6270
    t0 = (c0 + c4) << 13
    t1 = (c0 - c4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = c7, c5, c3, c1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3], axis=-1)
    return _descale(out, shift)


def idct(blocks: np.ndarray) -> np.ndarray:
    """(..., 64) dequantised coefficients -> (..., 8, 8) samples 0..255: pass 1 over columns (DESCALE 11), pass 2 over rows (DESCALE 18), + 128"""
    b = blocks.reshape(blocks.shape[:-1] + (8, 8))
    ws = np.swapaxes(_idct_1d(np.swapaxes(b, -1, -2), 11), -1, -2)
    return np.clip(_idct_1d(ws, 18) + 128, 0, 255)


def sample_plane(blocks: np.ndarray) -> np.ndarray:
    by, bx = blocks.shape[:2]
    return idct(blocks).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def upsample_h2v1(p: np.ndarray) -> np.ndarray:
    """fancy 4:2:2 upsampling of the real chroma samples p (rows, n) -> (rows, 2 n)"""
    n = p.shape[1]
    left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    out = np.empty((p.shape[0], 2 * n), dtype=np.int64)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def upsample_h2v2(p: np.ndarray) -> np.ndarray:
    """fancy 4:2:0 upsampling of the real chroma samples p (m, n) -> (2 m, 2 n)"""
    m, n = p.shape
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    down = np.concatenate([p[1:], p[-1:]], axis=0)
    out = np.empty((2 * m, 2 * n), dtype=np.int64)
    for v, other in ((0, up), (1, down)):
        s = 3 * p + other
        left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        even, odd = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
        out[v::2, 0::2], out[v::2, 1::2] = even, odd
    return out


def ycc_to_rgb(y, cb, cr) -> np.ndarray:
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(data: bytes) -> np.ndarray:
    """np.array(PIL.Image.open(file)) for a baseline file: (H, W) uint8 for one component, (H, W, 3) uint8 RGB for three"""
    h = parse(data)
    if h["sof"] != 0xC0 or h["precision"] != 8:
        raise JpegError("not baseline")
    H, W = h["height"], h["width"]
    planes = [sample_plane(c) for c in coefficients(data, h)]
    if len(planes) == 1:
        return planes[0][:H, :W].astype(np.uint8)
    hs, vs = h["comps"][0][1], h["comps"][0][2]
    if any(c[1:3] != (1, 1) for c in h["comps"][1:]) or (hs, vs) not in ((1, 1), (2, 1), (2, 2)):
        raise JpegError("sampling")
    ch, cw = -(-H // vs), -(-W // hs)
    chroma = [p[:ch, :cw] for p in planes[1:]]
    if (hs, vs) == (2, 1):
        chroma = [upsample_h2v1(p) for p in chroma]
    elif (hs, vs) == (2, 2):
        chroma = [upsample_h2v2(p) for p in chroma]
    return ycc_to_rgb(planes[0][:H, :W], chroma[0][:H, :W], chroma[1][:H, :W])
