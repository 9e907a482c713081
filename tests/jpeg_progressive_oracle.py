"""Progressive JPEG in plain Python / numpy, beside tests/jpeg_oracle.py (whose parsing, Huffman decode, IDCT and pixel stages it reuses): the
entropy decoder csrc/jpegprog.hip restates -- multi-scan, spectral selection, successive approximation, end-of-band
runs, restart intervals per scan -- and a re-coder that writes the coefficients of a baseline file under any legal scan script, so that the
tests have progressive files PIL's own writer never makes.  tests/test_jpeg_progressive_host.py pins both to PIL, bit for bit."""
import numpy as np

import jpeg_oracle
from jpeg_oracle import ZIGZAG, JpegError, _Bits, _Huff


def parse(data: bytes) -> dict:
    """The walk over the whole file: jpeg_oracle.parse()'s frame fields ("width", "height", "comps", "qt", "ri", "sof", "precision") and
    "scans": [{"comps": [(component index, td, ta)], "ss", "se", "ah", "al", "dc" / "ac": the tables in force {id: (counts, symbols)},
    "start", "end": the scan's entropy-coded bytes}], "eoi": offset of EOI or None."""
    if data[:2] != b"\xff\xd8":
        raise JpegError("no SOI")
    out = {"qt": {}, "ri": 0, "comps": None, "sof": None, "scans": [], "eoi": None}
    dc, ac = {}, {}
    pos = 2
    while True:
        if pos + 2 <= len(data) and data[pos:pos + 2] == b"\xff\xd9":
            out["eoi"] = pos
            return out
        if pos + 4 > len(data) or data[pos] != 0xFF:
            raise JpegError(f"bad framing at {pos}")
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        n = (data[pos + 2] << 8) | data[pos + 3]
        end = pos + 2 + n
        if n < 2 or end > len(data):
            raise JpegError(f"segment at {pos} runs past the file")
        seg = data[pos + 4:end]
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            out["sof"], out["precision"] = m, seg[0]
            out["height"], out["width"] = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            out["comps"] = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])]
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                counts = list(seg[p + 1:p + 17])
                (ac if seg[p] >> 4 else dc)[seg[p] & 15] = (counts, list(seg[p + 17:p + 17 + sum(counts)]))
                p += 17 + sum(counts)
        elif m == 0xDB:
            for p in range(0, len(seg), 65):
                out["qt"][seg[p] & 15] = np.array(list(seg[p + 1:p + 65]), dtype=np.int64)
        elif m == 0xDD:
            out["ri"] = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            ns = seg[0]
            ids = [c[0] for c in out["comps"]]
            stop = jpeg_oracle.scan_end(data, end)
            out["scans"].append({"comps": [(ids.index(seg[1 + 2 * i]), seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(ns)],
                                 "ss": seg[1 + 2 * ns], "se": seg[2 + 2 * ns], "ah": seg[3 + 2 * ns] >> 4, "al": seg[3 + 2 * ns] & 15,
                                 "dc": dict(dc), "ac": dict(ac), "start": end, "end": stop, "sos": pos})
            end = stop
        pos = end


def _geometry(h):
    comps = h["comps"]
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mx, my = -(-h["width"] // (8 * hmax)), -(-h["height"] // (8 * vmax))
    own = [(-(-(-(-h["height"] * c[2] // vmax)) // 8), -(-(-(-h["width"] * c[1] // hmax)) // 8)) for c in comps]  # (rows, columns) of real blocks
    return mx, my, own


def _units(h, scan_comps):
    """The scan's units in coding order: per unit the list of (position in the scan, component, block row, block column)."""
    mx, my, own = _geometry(h)
    if len(scan_comps) == 1:
        ci = scan_comps[0]
        return [[(0, ci, by, bx)] for by in range(own[ci][0]) for bx in range(own[ci][1])]
    units = []
    for m in range(mx * my):
        my0, mx0 = divmod(m, mx)
        units.append([(i, ci, my0 * h["comps"][ci][2] + by, mx0 * h["comps"][ci][1] + bx)
                      for i, ci in enumerate(scan_comps) for by in range(h["comps"][ci][2]) for bx in range(h["comps"][ci][1])])
    return units


def quantised(data: bytes, hdr=None, stats=None):
    """Quantised coefficients of a progressive file in zig-zag order: per component an int64 array (block rows, block columns, 64), padded to
    whole MCUs (blocks no scan visits stay zero).  stats, a dict, receives "max_eobrun": the longest end-of-band run of the streams."""
    h = hdr or parse(data)
    mx, my, _ = _geometry(h)
    planes = [np.zeros((my * c[2], mx * c[1], 64), dtype=np.int64) for c in h["comps"]]
    longest = 0
    for sc in h["scans"]:
        ss, se, ah, al = sc["ss"], sc["se"], sc["ah"], sc["al"]
        units = _units(h, [c for c, _, _ in sc["comps"]])
        ri = min(h["ri"], len(units)) if h["ri"] else len(units)
        nint = -(-len(units) // ri)
        marks = jpeg_oracle.restart_markers(data, sc["start"], sc["end"])
        if len(marks) != nint - 1 or any(n != (k & 7) for k, (_, n) in enumerate(marks)):
            raise JpegError("restart markers")
        bounds = [sc["start"]] + [p + 2 for p, _ in marks]
        ends = [p for p, _ in marks] + [sc["end"]]
        dct = {k: _Huff(*v) for k, v in sc["dc"].items()}
        act = {k: _Huff(*v) for k, v in sc["ac"].items()}
        p1 = 1 << al
        for k in range(nint):
            b = _Bits(data[bounds[k]:ends[k]])
            pred = [0] * len(sc["comps"])
            eobrun = 0
            for unit in units[k * ri:(k + 1) * ri]:
                for i, ci, by, bx in unit:
                    blk = planes[ci][by, bx]
                    _, td, ta = sc["comps"][i]
                    if ss == 0:
                        if ah == 0:
                            s = dct[td].decode(b)
                            if s > 11:
                                raise JpegError("DC category")
                            v = b.take(s)
                            pred[i] += v if s == 0 or v >> (s - 1) else v - (1 << s) + 1
                            blk[0] = pred[i] * p1
                        elif b.take(1):
                            blk[0] |= p1
                        continue
                    kk = ss
                    if ah == 0:
                        if eobrun:
                            eobrun -= 1
                            continue
                        while kk <= se:
                            rs = act[ta].decode(b)
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r == 15:
                                    kk += 16
                                    continue
                                eobrun = (1 << r) + (b.take(r) if r else 0)
                                longest = max(longest, eobrun)
                                eobrun -= 1
                                break
                            kk += r
                            if kk > se or s > 10:
                                raise JpegError("AC symbol")
                            v = b.take(s)
                            blk[kk] = (v if v >> (s - 1) else v - (1 << s) + 1) * p1
                            kk += 1
                        continue
                    if eobrun == 0:  # T.81 G.1.2.3
                        while kk <= se:
                            rs = act[ta].decode(b)
                            r, s = rs >> 4, rs & 15
                            new = 0
                            if s:
                                if s != 1:
                                    raise JpegError("AC refinement size")
                                new = p1 if b.take(1) else -p1
                            elif r != 15:
                                eobrun = (1 << r) + (b.take(r) if r else 0)
                                longest = max(longest, eobrun)
                                break
                            while kk <= se:
                                if blk[kk] != 0:
                                    if b.take(1) and not blk[kk] & p1:
                                        blk[kk] += p1 if blk[kk] >= 0 else -p1
                                else:
                                    r -= 1
                                    if r < 0:
                                        break
                                kk += 1
                            if new:
                                if kk > se:
                                    raise JpegError("AC refinement run")
                                blk[kk] = new
                            kk += 1
                    if eobrun > 0:
                        while kk <= se:
                            if blk[kk] != 0 and b.take(1) and not blk[kk] & p1:
                                blk[kk] += p1 if blk[kk] >= 0 else -p1
                            kk += 1
                        eobrun -= 1
    if stats is not None:
        stats["max_eobrun"] = longest
    return planes


def coefficients(data: bytes, hdr=None, stats=None):
    """jpeg_oracle.coefficients() for a progressive file: dequantised, natural order."""
    h = hdr or parse(data)
    out = []
    for c, q in zip(h["comps"], quantised(data, h, stats)):
        nat = np.zeros_like(q)
        nat[..., ZIGZAG] = q * h["qt"][c[3]]
        out.append(nat)
    return out


def decode(data: bytes) -> np.ndarray:
    """np.array(PIL.Image.open(file)) for a complete progressive file"""
    h = parse(data)
    if h["sof"] != 0xC2 or h["precision"] != 8:
        raise JpegError("not progressive")
    H, W = h["height"], h["width"]
    planes = [jpeg_oracle.sample_plane(c) for c in coefficients(data, h)]
    if len(planes) == 1:
        return planes[0][:H, :W].astype(np.uint8)
    hs, vs = h["comps"][0][1], h["comps"][0][2]
    ch, cw = -(-H // vs), -(-W // hs)
    chroma = [p[:ch, :cw] for p in planes[1:]]
    if (hs, vs) == (2, 1):
        chroma = [jpeg_oracle.upsample_h2v1(p) for p in chroma]
    elif (hs, vs) == (2, 2):
        chroma = [jpeg_oracle.upsample_h2v2(p) for p in chroma]
    return jpeg_oracle.ycc_to_rgb(planes[0][:H, :W], chroma[0][:H, :W], chroma[1][:H, :W])


# ---- the re-coder
DC_TABLE = ([0, 0, 0, 12] + [0] * 12, list(range(12)))  # categories 0 .. 11, four bits each
AC_SYMBOLS = sorted((r << 4) | s for r in range(16) for s in range(11))  # run / size, ZRL and EOB0 .. EOB14: 176 codes of eight bits
AC_TABLE = ([0] * 7 + [len(AC_SYMBOLS)] + [0] * 8, AC_SYMBOLS)


class _Writer:
    def __init__(self):
        self.out = bytearray()
        self.acc = self.n = 0

    def bits(self, v, n):
        self.acc = (self.acc << n) | (v & ((1 << n) - 1))
        self.n += n
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 255
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.bits((1 << (8 - self.n)) - 1, 8 - self.n)

    def dc(self, s):
        self.bits(s, 4)

    def ac(self, sym):
        self.bits(AC_SYMBOLS.index(sym), 8)


def _dht(tc, th, table):
    body = bytes([tc << 4 | th]) + bytes(table[0]) + bytes(table[1])
    return b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body


def write_progressive(coefficients, header, script, restart=0) -> bytes:
    """A progressive file of the dequantised natural-order `coefficients` (jpeg_oracle.coefficients() of a baseline file) and that file's
    parsed `header`, coded under `script`: [(component indices, Ss, Se, Ah, Al)].  restart: units per restart interval, 0 for none.  The
    Huffman tables are fixed ones, defined anew before every scan that uses them.  Nothing checks that the script is legal or complete."""
    comps = header["comps"]
    quant = []
    for c, nat in zip(comps, coefficients):
        q = nat[..., ZIGZAG] // header["qt"][c[3]]
        assert np.array_equal(q * header["qt"][c[3]], nat[..., ZIGZAG])
        quant.append(q)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in sorted(set(c[3] for c in comps)):
        out += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(int(v) for v in header["qt"][t])
    out += b"\xff\xc2" + (8 + 3 * len(comps)).to_bytes(2, "big") + b"\x08" + header["height"].to_bytes(2, "big") + header["width"].to_bytes(2, "big")
    out += bytes([len(comps)]) + b"".join(bytes([c[0], c[1] << 4 | c[2], c[3]]) for c in comps)
    if restart:
        out += b"\xff\xdd\x00\x04" + restart.to_bytes(2, "big")
    for scan_comps, ss, se, ah, al in script:
        if ss == 0 and ah == 0:
            out += _dht(0, 0, DC_TABLE)
        elif ss > 0:
            out += _dht(1, 0, AC_TABLE)
        out += b"\xff\xda" + (6 + 2 * len(scan_comps)).to_bytes(2, "big") + bytes([len(scan_comps)])
        out += b"".join(bytes([comps[ci][0], 0]) for ci in scan_comps) + bytes([ss, se, ah << 4 | al])
        units = _units(header, list(scan_comps))
        ri = min(restart, len(units)) if restart else len(units)
        for k in range(-(-len(units) // ri)):
            if k:
                out += bytes([0xFF, 0xD0 + ((k - 1) & 7)])
            w = _Writer()
            pred = [0] * len(scan_comps)
            state = {"eobrun": 0, "be": []}

            def emit_eobrun():
                if state["eobrun"]:
                    n = state["eobrun"].bit_length() - 1
                    w.ac(n << 4)
                    w.bits(state["eobrun"], n)
                    state["eobrun"] = 0
                    for bit in state["be"]:
                        w.bits(bit, 1)
                    state["be"] = []

            for unit in units[k * ri:(k + 1) * ri]:
                for i, ci, by, bx in unit:
                    blk = [int(v) for v in quant[ci][by, bx]]
                    if ss == 0:
                        if ah:
                            w.bits((blk[0] >> al) & 1, 1)
                            continue
                        v = blk[0] >> al
                        diff, pred[i] = v - pred[i], v
                        s = abs(diff).bit_length()
                        w.dc(s)
                        w.bits(diff if diff >= 0 else diff - 1, s)
                        continue
                    r = 0
                    if ah == 0:
                        for kk in range(ss, se + 1):
                            a = abs(blk[kk]) >> al
                            if a == 0:
                                r += 1
                                continue
                            emit_eobrun()
                            while r > 15:
                                w.ac(0xF0)
                                r -= 16
                            s = a.bit_length()
                            w.ac(r << 4 | s)
                            w.bits(a if blk[kk] > 0 else ~a, s)
                            r = 0
                        if r:
                            state["eobrun"] += 1
                            if state["eobrun"] == 0x7FFF:
                                emit_eobrun()
                        continue
                    absv = {kk: abs(blk[kk]) >> al for kk in range(ss, se + 1)}
                    last_new = max([kk for kk, a in absv.items() if a == 1], default=-1)
                    br = []
                    for kk in range(ss, se + 1):
                        a = absv[kk]
                        if a == 0:
                            r += 1
                            continue
                        while r > 15 and kk <= last_new:
                            emit_eobrun()
                            w.ac(0xF0)
                            r -= 16
                            for bit in br:
                                w.bits(bit, 1)
                            br = []
                        if a > 1:
                            br.append(a & 1)
                            continue
                        emit_eobrun()
                        w.ac(r << 4 | 1)
                        w.bits(0 if blk[kk] < 0 else 1, 1)
                        for bit in br:
                            w.bits(bit, 1)
                        br = []
                        r = 0
                    if r or br:
                        state["eobrun"] += 1
                        state["be"] += br
                        if state["eobrun"] == 0x7FFF or len(state["be"]) > 937:
                            emit_eobrun()
            emit_eobrun()
            w.flush()
            out += w.out
    return bytes(out + b"\xff\xd9")
