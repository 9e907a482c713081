"""cs_op_sheet_compose against the numpy statement of tests/sheet_oracle.py.  The canvas holds bytes, so every comparison
is byte equality; it sits inside the guard bands of tests/guard.py, so a store outside it is seen too."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import sheet_oracle as oracle  # noqa: E402
from guard import guarded, poisoned_in  # noqa: E402
from sheet_oracle import BLEND, FILL, FRAME, IMAGE, RAMP, TEXT, P  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PAIRS = [((1, 1), (1, 1)), ((1, 1), (3, 5)), ((7, 5), (7, 5)), ((14, 14), (7, 7)), ((37, 53), (10, 17)), ((5, 9), (11, 4)), ((130, 70), (33, 65)),
         ((266, 266), (129, 64)), ((518, 518), (103, 103))]
OFFSETS = (0, 1, 63, 64, 65)


def _lib_():
    from crossscore_amd import _lib

    return _lib, _lib.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bound(panels):
    """oracle panels (numpy sources) -> vis panels (device sources; one upload per array)"""
    from crossscore_amd import vis

    up = {}

    def dev(a):
        if a is None or isinstance(a, torch.Tensor):
            return a
        if id(a) not in up:
            up[id(a)] = _dev(a)
        return up[id(a)]

    return [vis.Panel(p.kind, f"p{i}", p.y, p.x, p.h, p.w, src=dev(p.src), src2=dev(p.src2), rgb=tuple(p.rgb), param=p.param, text=p.text)
            for i, p in enumerate(panels)]


def run(panels, canvas_h, canvas_w, bound=None):
    """the op on a guarded canvas -> its bytes on the host (the guard bands checked)"""
    from crossscore_amd import vis

    g = guarded((canvas_h, canvas_w, 3), torch.uint8)
    vis.compose(bound if bound is not None else _bound(panels), canvas_h, canvas_w, out=g.view)
    g.check("canvas")
    return g.view.cpu().numpy()


def _host(p):
    """an oracle panel whose sources may be device tensors -> numpy sources"""
    f = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else a  # noqa: E731
    return P(p.kind, p.y, p.x, p.h, p.w, f(p.src), f(p.src2), p.rgb, p.param, p.text)


def check(panels, canvas_h, canvas_w):
    got = run(panels, canvas_h, canvas_w)
    want = oracle.compose([_host(p) for p in panels], canvas_h, canvas_w)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    return got


def _contents(sh, sw, seed):
    rng = np.random.default_rng(seed)
    two = np.where(rng.integers(0, 2, (sh, sw, 1)) > 0, np.uint8(255), np.uint8(0)).repeat(3, axis=2)
    two[..., 1] = 255 - two[..., 1]
    return [rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8), np.ascontiguousarray(two), np.full((sh, sw, 3), 255, np.uint8)]


@pytest.mark.parametrize("src,dst", PAIRS, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in PAIRS])
def test_resampling(src, dst):
    (sh, sw), (dh, dw) = src, dst
    panels = [P(IMAGE, 1, 2 + k * (dw + 1), dh, dw, src=img) for k, img in enumerate(_contents(sh, sw, sh * 7 + dw))]
    got = check(panels, dh + 2, 3 * (dw + 1) + 3)
    assert (got[1:1 + dh, 2 + 2 * (dw + 1):2 + 2 * (dw + 1) + dw] == 255).all()  # the all-255 image stays all 255


def test_a_source_with_padded_rows_whose_padding_is_ff():
    sh, sw, dh, dw = 37, 53, 10, 17
    img = np.random.default_rng(2).integers(0, 200, (sh, sw, 3), dtype=np.uint8)
    flat = poisoned_in(_dev(img.reshape(sh, sw * 3)), ld=sw * 3 + 5)  # (sh, 3 sw) rows 3 sw + 5 bytes apart, 255 in between and around
    src = flat.as_strided((sh, sw, 3), (sw * 3 + 5, 3, 1), flat.storage_offset())
    assert src.stride(0) == sw * 3 + 5 and np.array_equal(src.cpu().numpy(), img)
    got = check([P(IMAGE, 0, 0, dh, dw, src=src), P(BLEND, 0, dw, dh, dw, src=src, src2=_dev(img)), P(IMAGE, dh, 0, sh, sw, src=src)], dh + sh, sw)
    assert got.max() < 200  # no padding byte reached the canvas
    assert np.array_equal(got[dh:, :sw], img)


@pytest.fixture(scope="module")
def edge_reference():
    img = np.random.default_rng(3).integers(0, 256, (20, 30, 3), dtype=np.uint8)
    return img, oracle.resample(img, 63, 66)


@pytest.mark.parametrize("oy", OFFSETS)
def test_panel_edges_against_tile_edges(oy, edge_reference):
    """a 63 x 66 image panel, a frame, a text and a ramp at every offset pair on a canvas three tiles a side whose rows are 4 k + 1 bytes long"""
    img, resized = edge_reference
    ch, cw = 160, 171
    dimg = _dev(img)
    table = np.random.default_rng(4).integers(0, 256, (256, 3), dtype=np.uint8)
    dtable = _dev(table)
    for ox in OFFSETS:
        rest = [P(FRAME, oy, ox, 63, 66, rgb=(255, 0, 255), param=2), P(TEXT, oy + 3, ox + 3, 14, 46, rgb=(1, 2, 3), param=2, text="-1.5"),
                P(RAMP, oy, ox + 66, 64, 5, src=dtable), P(FILL, oy + 63, ox, 1, 71, rgb=(9, 8, 7))]
        got = run([P(IMAGE, oy, ox, 63, 66, src=dimg)] + rest, ch, cw)
        want = np.zeros((ch, cw, 3), dtype=np.uint8)
        want[oy:oy + 63, ox:ox + 66] = resized
        oracle.compose([_host(p) for p in rest], ch, cw, canvas=want)
        assert np.array_equal(got, want), (oy, ox)


def test_overlapping_panels_in_both_orders_and_uncovered_pixels():
    a, b = _contents(9, 12, 5)[:2]
    pa, pb, pf = P(IMAGE, 2, 3, 18, 24, src=a), P(IMAGE, 10, 15, 9, 12, src=b), P(FILL, 5, 1, 40, 8, rgb=(7, 0, 200))
    first = check([pa, pb, pf], 70, 80)
    second = check([pf, pb, pa], 70, 80)
    assert not np.array_equal(first, second)
    covered = np.zeros((70, 80), dtype=bool)
    for p in (pa, pb, pf):
        covered[p.y:p.y + p.h, p.x:p.x + p.w] = True
    assert (first[~covered] == 0).all() and (second[~covered] == 0).all()
    assert (check([], 5, 7) == 0).all()  # no panel at all: a black canvas


def test_blend_with_both_byte_extremes():
    rng = np.random.default_rng(6)
    a = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    a[0, :4, 0], b[0, :4, 0] = [0, 0, 255, 255], [0, 255, 255, 254]
    a[1], b[1] = 255, 255
    a[2], b[2] = 0, 0
    got = check([P(BLEND, 0, 0, 9, 11, src=a, src2=b), P(BLEND, 9, 0, 4, 5, src=a, src2=b), P(BLEND, 0, 11, 13, 20, src=b, src2=a)], 13, 31)
    assert got[0, :4, 0].tolist() == [0, 128, 255, 255] and (got[1, :11] == 255).all() and (got[2, :11] == 0).all()


def test_ramp_heights():
    table = np.random.default_rng(7).integers(0, 256, (256, 3), dtype=np.uint8)
    got = check([P(RAMP, 0, 3 * k, h, 3, src=table) for k, h in enumerate((1, 255, 256, 300))], 300, 12)
    assert np.array_equal(got[0, 0], table[255]) and np.array_equal(got[:256, 6], table[::-1]) and np.array_equal(got[299, 9], table[0])


def test_frames_thin_and_thicker_than_half():
    base = P(FILL, 0, 0, 40, 90, rgb=(10, 20, 30))
    got = check([base, P(FRAME, 2, 3, 20, 30, rgb=(255, 0, 255), param=1), P(FRAME, 5, 40, 9, 30, rgb=(0, 255, 0), param=5),
                 P(FRAME, 30, 3, 1, 1, rgb=(1, 1, 1), param=1)], 40, 90)
    assert tuple(got[3, 4]) == (10, 20, 30) and tuple(got[2, 3]) == (255, 0, 255)  # the inside is untouched
    assert (got[5:14, 40:70] == (0, 255, 0)).all()                                  # thicker than half: the whole rectangle


@pytest.mark.parametrize("scale", [1, 3])
def test_text_with_every_character(scale):
    text = oracle.CHARS
    h, w = 7 * scale, (6 * len(text) - 1) * scale
    got = check([P(FILL, 0, 0, h + 2, w + 2, rgb=(40, 40, 40)), P(TEXT, 1, 1, h, w, rgb=(250, 251, 252), param=scale, text=text),
                 P(TEXT, h + 3, 0, 7, 95, rgb=(5, 6, 7), param=1, text="0123456789.- 012")], h + 11, max(w + 2, 95))
    assert (got[1:1 + h, 1:1 + w] == (250, 251, 252)).all(axis=2).sum() == scale * scale * sum(r.count("#") for g in oracle.GLYPHS for r in g)


def _sheet(H, W, n_ref, has_gt, window, seed):
    from crossscore_amd import vis

    rng = np.random.default_rng(seed)
    images = {k: rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for k in ["query", "gt", "diff"] + [f"ref{k}" for k in range(n_ref)]}
    images["score"] = rng.integers(0, 256, (H - 2, W - 1, 3), dtype=np.uint8)  # (a map smaller than the query, as with a partial patch)
    images["query_on_map"] = images["query"][:H - 2, :W - 1]
    images["turbo"] = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    canvas_h, canvas_w, panels = vis.sheet_layout(H, W, n_ref, has_gt, window is not None)
    bound = vis.bind(panels, images, {"score_mean": 0.4567, "gt_mean": -0.25, "l1": None}, (H - 2, W - 1), window)
    return canvas_h, canvas_w, [P(p.kind, p.y, p.x, p.h, p.w, p.src, p.src2, p.rgb, p.param, p.text) for p in bound]


def test_a_full_sheet():
    canvas_h, canvas_w, panels = _sheet(28, 42, 6, True, (9, 20, 14), 8)
    assert {p.kind for p in panels} == {FILL, IMAGE, BLEND, RAMP, FRAME, TEXT}
    check(panels, canvas_h, canvas_w)


def test_two_calls_and_two_canvases_give_equal_bytes():
    canvas_h, canvas_w, panels = _sheet(56, 70, 5, False, (0, 0, 56), 9)
    bound = _bound(panels)
    runs = [run(None, canvas_h, canvas_w, bound=bound) for _ in range(3)]
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
    assert np.array_equal(runs[0], oracle.compose(panels, canvas_h, canvas_w))


@pytest.mark.parametrize("lead", [1, 2, 3])
def test_a_canvas_at_any_byte_address(lead):
    """the canvas `lead` bytes behind a 16-byte boundary, rows of 4 k + 3 bytes: every low-bit combination of a row's first address"""
    from crossscore_amd import vis

    ch, cw = 70, 69
    img = _contents(30, 31, 10)[0]
    panels = [P(FILL, 0, 0, ch, cw, rgb=(3, 4, 5)), P(IMAGE, 1, 1, 66, 67, src=img)]
    g = guarded((lead + ch * cw * 3,), torch.uint8)
    canvas = g.view[lead:].view(ch, cw, 3)
    assert canvas.data_ptr() % 4 == lead
    vis.compose(_bound(panels), ch, cw, out=canvas)
    g.check("canvas")
    assert (g.view[:lead].cpu().numpy() == 0xA5).all()
    assert np.array_equal(canvas.cpu().numpy(), oracle.compose(panels, ch, cw))


def _struct(kind, y, x, h, w, src=None, shape=(0, 0, 0), src2=None, shape2=(0, 0, 0), param=0, text=b""):
    _lib, _ = _lib_()
    s = _lib.CsSheetPanel(kind=kind, dst_y=y, dst_x=x, dst_h=h, dst_w=w, param=param, text=text)
    s.src, (s.src_h, s.src_w, s.src_row_bytes) = (src.data_ptr() if src is not None else None), shape
    s.src2, (s.src2_h, s.src2_w, s.src2_row_bytes) = (src2.data_ptr() if src2 is not None else None), shape2
    return s


def test_every_error_returns_its_status_and_leaves_the_canvas_untouched():
    _lib, lib = _lib_()
    BAD, UNSUP = _lib.CS_ERR_BAD_ARG, _lib.CS_ERR_UNSUPPORTED
    ch, cw = 40, 50
    g = guarded((ch, cw, 3), torch.uint8)
    img = _dev(np.zeros((8, 9, 3), np.uint8))
    other = _dev(np.zeros((8, 10, 3), np.uint8))
    table = _dev(np.zeros((256, 3), np.uint8))
    ok_img = dict(src=img, shape=(8, 9, 27))
    good = _struct(FILL, 0, 0, 4, 4)
    cases = [
        ("outside right", BAD, [_struct(FILL, 0, 47, 4, 4)]), ("outside below", BAD, [_struct(FILL, 37, 0, 4, 4)]),
        ("negative corner", BAD, [_struct(FILL, -1, 0, 4, 4)]), ("negative column", BAD, [_struct(FILL, 0, -1, 4, 4)]),
        ("empty height", BAD, [_struct(FILL, 0, 0, 0, 4)]), ("empty width", BAD, [_struct(FILL, 0, 0, 4, 0)]),
        ("unknown kind", BAD, [_struct(6, 0, 0, 4, 4)]), ("negative kind", BAD, [_struct(-1, 0, 0, 4, 4)]),
        ("image without source", BAD, [_struct(IMAGE, 0, 0, 4, 4, shape=(8, 9, 27))]),
        ("image with short rows", BAD, [_struct(IMAGE, 0, 0, 4, 4, src=img, shape=(8, 9, 26))]),
        ("image with an empty source", BAD, [_struct(IMAGE, 0, 0, 4, 4, src=img, shape=(0, 9, 27))]),
        ("blend without second", BAD, [_struct(BLEND, 0, 0, 4, 4, **ok_img, shape2=(8, 9, 27))]),
        ("blend of unequal widths", BAD, [_struct(BLEND, 0, 0, 4, 4, **ok_img, src2=other, shape2=(8, 10, 30))]),
        ("blend of unequal heights", BAD, [_struct(BLEND, 0, 0, 4, 4, **ok_img, src2=other, shape2=(7, 9, 30))]),
        ("ramp without table", BAD, [_struct(RAMP, 0, 0, 4, 4)]),
        ("frame without thickness", BAD, [_struct(FRAME, 0, 0, 4, 4, param=0)]),
        ("text of the wrong width", BAD, [_struct(TEXT, 0, 0, 7, 18, param=1, text=b"1.5")]),
        ("text of the wrong height", BAD, [_struct(TEXT, 0, 0, 8, 17, param=1, text=b"1.5")]),
        ("text at the wrong scale", BAD, [_struct(TEXT, 0, 0, 7, 17, param=2, text=b"1.5")]),
        ("text without scale", BAD, [_struct(TEXT, 0, 0, 7, 17, param=0, text=b"1.5")]),
        ("text with an unknown character", BAD, [_struct(TEXT, 0, 0, 7, 17, param=1, text=b"1,5")]),
        ("empty text", BAD, [_struct(TEXT, 0, 0, 7, 5, param=1, text=b"")]),
        ("a bad panel behind good ones", BAD, [good, good, _struct(FILL, 0, 47, 4, 4)]),
        ("49 panels", UNSUP, [good] * 49),
        ("a source above 4096", UNSUP, [_struct(IMAGE, 0, 0, 4, 4, src=img, shape=(4097, 9, 27))]),
        ("a rectangle above 4096", UNSUP, [_struct(FILL, 0, 0, 4097, 4)]),
    ]
    for what, status, panels in cases:
        arr = (_lib.CsSheetPanel * len(panels))(*panels)
        rc = lib.cs_op_sheet_compose(arr, len(panels), C.c_void_p(g.view.data_ptr()), ch, cw, None)
        assert rc == status, (what, rc, _lib.last_error())
        assert _lib.last_error().startswith("sheet_compose"), what
    one = (_lib.CsSheetPanel * 1)(good)
    for what, status, args in [("no canvas", BAD, (one, 1, None, ch, cw)), ("no panels", BAD, (None, 1, C.c_void_p(g.view.data_ptr()), ch, cw)),
                               ("a negative count", BAD, (one, -1, C.c_void_p(g.view.data_ptr()), ch, cw)),
                               ("an empty canvas", BAD, (one, 1, C.c_void_p(g.view.data_ptr()), 0, cw)),
                               ("a canvas above 4096", UNSUP, (one, 1, C.c_void_p(g.view.data_ptr()), 4097, cw))]:
        assert lib.cs_op_sheet_compose(*args, None) == status, what
    torch.cuda.synchronize()
    assert bool((g.ibase == g.sentinel).all())  # nothing was launched: view and guard bands hold the poison
    with pytest.raises(ValueError, match="sheet_compose"):
        _lib.check(lib.cs_op_sheet_compose((_lib.CsSheetPanel * 1)(_struct(FILL, 0, 47, 4, 4)), 1, C.c_void_p(g.view.data_ptr()), ch, cw, None))
    # the limits themselves are taken: 48 panels, and the largest text
    arr = (_lib.CsSheetPanel * 48)(*([good] * 47 + [_struct(TEXT, 10, 0, 7, 47, param=1, text=b"12345678")]))
    assert lib.cs_op_sheet_compose(arr, 48, C.c_void_p(g.view.data_ptr()), ch, cw, None) == 0
    g.check("canvas")
