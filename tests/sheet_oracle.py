"""Plain numpy statement of the preview sheet (include/crossscore_hip.h, cs_op_sheet_compose): the six panel kinds and the painting order in int64,
the area resampling as the direct double sum.  The glyphs and every formula are written out here, not imported from crossscore_amd, so the tests
compare two statements of the definition.  Also the separable form of the resampling, which the tests show equal to the double sum."""
import numpy as np

FILL, IMAGE, BLEND, RAMP, FRAME, TEXT = range(6)
CHARS = "0123456789.- "
# thirteen 5 x 7 glyphs in the order of CHARS; '#' is a set bit
GLYPHS = [
    [".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."],
    ["..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."],
    [".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####"],
    ["#####", "...#.", "..#..", "...#.", "....#", "#...#", ".###."],
    ["...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#."],
    ["#####", "#....", "####.", "....#", "....#", "#...#", ".###."],
    ["..##.", ".#...", "#....", "####.", "#...#", "#...#", ".###."],
    ["#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#..."],
    [".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###."],
    [".###.", "#...#", "#...#", ".####", "....#", "...#.", ".##.."],
    [".....", ".....", ".....", ".....", ".....", ".##..", ".##.."],
    [".....", ".....", ".....", "#####", ".....", ".....", "....."],
    [".....", ".....", ".....", ".....", ".....", ".....", "....."],
]


class P:
    """one panel: kind, the rectangle, and what the kind reads (src / src2: (h, w, 3) uint8 arrays; RAMP: src a (256, 3) table)"""

    def __init__(self, kind, y, x, h, w, src=None, src2=None, rgb=(0, 0, 0), param=0, text=""):
        self.kind, self.y, self.x, self.h, self.w = kind, y, x, h, w
        self.src, self.src2, self.rgb, self.param, self.text = src, src2, rgb, param, text


def weights(s, d):
    """(s, d) int64: w[i][j] = max(0, min((i + 1) d, (j + 1) s) - max(i d, j s)), the overlap of source cell i with destination cell j"""
    i = np.arange(s, dtype=np.int64)[:, None]
    j = np.arange(d, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((i + 1) * d, (j + 1) * s) - np.maximum(i * d, j * s))


def resample(img, dh, dw):
    """(sh, sw, 3) -> (dh, dw, 3): per channel S = sum_iy sum_ix wy wx v, out = (S + (sh sw) // 2) // (sh sw); the double sum, pixel by pixel
    over the source cells with a weight"""
    v = np.asarray(img).astype(np.int64)
    sh, sw = v.shape[:2]
    wy, wx = weights(sh, dh), weights(sw, dw)
    out = np.zeros((dh, dw, 3), dtype=np.int64)
    for r in range(dh):
        iy = np.nonzero(wy[:, r])[0]
        for c in range(dw):
            ix = np.nonzero(wx[:, c])[0]
            w2 = wy[iy, r][:, None] * wx[ix, c][None, :]
            out[r, c] = (w2[:, :, None] * v[iy[0]:iy[-1] + 1, ix[0]:ix[-1] + 1]).sum(axis=(0, 1))
    area = sh * sw
    assert out.max(initial=0) < 2 ** 32
    return ((out + area // 2) // area).astype(np.uint8)


def resample_separable(img, dh, dw):
    """the same with the horizontal sums of every source row formed first, then the vertical sums (two integer matrix products)"""
    v = np.asarray(img).astype(np.int64)
    sh, sw = v.shape[:2]
    wy, wx = weights(sh, dh), weights(sw, dw)
    hs = np.einsum("yxc,xj->yjc", v, wx)
    out = np.einsum("yjc,yr->rjc", hs, wy)
    area = sh * sw
    return ((out + area // 2) // area).astype(np.uint8)


def blend(a, b):
    return ((np.asarray(a).astype(np.int64) + np.asarray(b).astype(np.int64) + 1) >> 1).astype(np.uint8)


def text_mask(text, scale):
    """(7 scale, (6 n - 1) scale) bool: character i in the cell at column 6 scale i"""
    n = len(text)
    m = np.zeros((7 * scale, (6 * n - 1) * scale), dtype=bool)
    for i, ch in enumerate(text):
        g = GLYPHS[CHARS.index(ch)]
        for gy in range(7):
            for gx in range(5):
                if g[gy][gx] == "#":
                    m[gy * scale:(gy + 1) * scale, (6 * i + gx) * scale:(6 * i + gx + 1) * scale] = True
    return m


def compose(panels, canvas_h, canvas_w, canvas=None):
    """the canvas (canvas_h, canvas_w, 3) uint8: zeros (or `canvas`, painted further in place), then the panels in order"""
    if canvas is None:
        canvas = np.zeros((canvas_h, canvas_w, 3), dtype=np.uint8)
    assert canvas.shape == (canvas_h, canvas_w, 3) and canvas.dtype == np.uint8
    for p in panels:
        assert 0 <= p.y and 0 <= p.x and p.h > 0 and p.w > 0 and p.y + p.h <= canvas_h and p.x + p.w <= canvas_w
        view = canvas[p.y:p.y + p.h, p.x:p.x + p.w]
        if p.kind == FILL:
            view[:] = p.rgb
        elif p.kind == IMAGE:
            view[:] = resample(p.src, p.h, p.w)
        elif p.kind == BLEND:
            assert p.src.shape == p.src2.shape
            view[:] = resample(blend(p.src, p.src2), p.h, p.w)
        elif p.kind == RAMP:
            table = np.asarray(p.src).reshape(256, 3)
            for r in range(p.h):
                view[r] = table[255 - (r * 256) // p.h]
        elif p.kind == FRAME:
            r = np.arange(p.h)[:, None]
            c = np.arange(p.w)[None, :]
            view[(r < p.param) | (r >= p.h - p.param) | (c < p.param) | (c >= p.w - p.param)] = p.rgb
        elif p.kind == TEXT:
            assert (p.h, p.w) == (7 * p.param, (6 * len(p.text) - 1) * p.param)
            view[text_mask(p.text, p.param)] = p.rgb
        else:
            raise ValueError(p.kind)
    return canvas
