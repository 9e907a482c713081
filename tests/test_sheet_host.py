"""Host side of the preview sheet (crossscore_amd/vis.py), without a GPU: properties of the numpy statement
(tests/sheet_oracle.py), the layout, the numbers' text and the options."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import sheet_oracle as oracle  # noqa: E402

from crossscore_amd import vis  # noqa: E402
from crossscore_amd.config import load_config  # noqa: E402

PAIRS = [((1, 1), (1, 1)), ((1, 1), (3, 5)), ((7, 5), (7, 5)), ((14, 14), (7, 7)), ((37, 53), (10, 17)), ((5, 9), (11, 4)), ((33, 20), (9, 31))]


def test_equal_sizes_copy():
    img = np.random.default_rng(0).integers(0, 256, (7, 5, 3), dtype=np.uint8)
    assert np.array_equal(oracle.resample(img, 7, 5), img)


def test_a_factor_two_is_the_rounded_mean_of_four_and_a_half_rounds_up():
    img = np.random.default_rng(1).integers(0, 256, (14, 14, 3), dtype=np.uint8)
    img[0:2, 0:2, 0] = [[1, 2], [3, 4]]      # sum 10: 2.5 -> 3
    img[0:2, 0:2, 1] = [[0, 0], [1, 1]]      # sum 2: 0.5 -> 1
    img[0:2, 0:2, 2] = [[255, 255], [255, 254]]  # sum 1019: 254.75 -> 255
    want = (img.astype(np.int64).reshape(7, 2, 7, 2, 3).sum(axis=(1, 3)) + 2) // 4
    got = oracle.resample(img, 7, 7)
    assert np.array_equal(got, want)
    assert tuple(got[0, 0]) == (3, 1, 255)


@pytest.mark.parametrize("src,dst", PAIRS)
def test_a_constant_image_stays_constant_and_separable_equals_the_double_sum(src, dst):
    for v in (0, 1, 127, 255):
        assert np.array_equal(oracle.resample(np.full(src + (3,), v, np.uint8), *dst), np.full(dst + (3,), v, np.uint8))
    img = np.random.default_rng(src[0] * 100 + dst[1]).integers(0, 256, src + (3,), dtype=np.uint8)
    assert np.array_equal(oracle.resample(img, *dst), oracle.resample_separable(img, *dst))
    w = oracle.weights(src[1], dst[1])
    assert (w.sum(axis=0) == src[1]).all() and (w.sum(axis=1) == dst[1]).all()  # every destination cell weighs sw, every source cell dw


def test_product_and_oracle_hold_the_same_characters_and_constants():
    assert vis.CHARS == oracle.CHARS and len(oracle.GLYPHS) == 13
    assert (vis.FILL, vis.IMAGE, vis.BLEND, vis.RAMP, vis.FRAME, vis.TEXT) == (oracle.FILL, oracle.IMAGE, oracle.BLEND, oracle.RAMP, oracle.FRAME,
                                                                                 oracle.TEXT)
    font = open(os.path.join(REPO, "crossscore_amd", "csrc", "sheet_font.h")).read()
    rows = [int(v, 16) for line in font.split("\n") if line.lstrip().startswith("{0x") for v in line[line.index("{") + 1:line.index("}")].split(",")]
    assert rows == [int(r.replace("#", "1").replace(".", "0"), 2) for g in oracle.GLYPHS for r in g]  # the header's rows are the oracle's glyphs
    m = oracle.text_mask("1 ", 2)
    assert m.shape == (14, 22) and m[:, 10:].sum() == 0 and m.sum() == 4 * sum(r.count("#") for r in oracle.GLYPHS[1])


def _rects_inside(canvas_h, canvas_w, panels):
    for p in panels:
        assert p.h > 0 and p.w > 0 and 0 <= p.y and 0 <= p.x and p.y + p.h <= canvas_h and p.x + p.w <= canvas_w, p


def _overlap(a, b):
    return a.y < b.y + b.h and b.y < a.y + a.h and a.x < b.x + b.w and b.x < a.x + a.w


@pytest.mark.parametrize("size", [(28, 42), (56, 70), (518, 518), (1, 1), (37, 3)])
@pytest.mark.parametrize("n_ref", [0, 1, 5, 6])
@pytest.mark.parametrize("has_gt", [False, True])
@pytest.mark.parametrize("has_window", [False, True])
def test_layout(size, n_ref, has_gt, has_window):
    H, W = size
    canvas_h, canvas_w, panels = vis.sheet_layout(H, W, n_ref, has_gt, has_window)
    assert (canvas_h, canvas_w, panels) == vis.sheet_layout(H, W, n_ref, has_gt, has_window)  # deterministic
    _rects_inside(canvas_h, canvas_w, panels)
    images = [p for p in panels if p.kind in (vis.IMAGE, vis.BLEND, vis.RAMP, vis.TEXT)]
    for i, a in enumerate(images):
        for b in images[i + 1:]:
            assert not _overlap(a, b), (a, b)
    roles = [p.role for p in panels]
    want = ["background", "query", "colour_bar", "score", "score_mean", "overlay"] + (["gt", "gt_mean", "diff", "l1"] if has_gt else [])
    want += [f"ref{k}" for k in range(n_ref)] + (["window_score", "window_overlay"] if has_window else [])
    assert roles == want
    by = {p.role: p for p in panels}
    assert (by["background"].kind, by["background"].h, by["background"].w, by["background"].rgb) == (vis.FILL, canvas_h, canvas_w, vis.BACKGROUND)
    assert (by["query"].kind, by["query"].h, by["query"].w, by["query"].src) == (vis.IMAGE, H, W, "query")
    assert (by["colour_bar"].kind, by["colour_bar"].h, by["colour_bar"].src) == (vis.RAMP, H, "turbo")
    hh, hw = max(1, H // 2), max(1, W // 2)
    assert (by["overlay"].kind, by["overlay"].src, by["overlay"].src2, by["overlay"].h, by["overlay"].w) == (vis.BLEND, "query_on_map", "score", hh, hw)
    for role in ["score"] + (["gt", "diff"] if has_gt else []) + [f"ref{k}" for k in range(n_ref)]:
        assert (by[role].kind, by[role].src, by[role].h, by[role].w) == (vis.IMAGE, role, hh, hw)
    for role in ["score_mean"] + (["gt_mean", "l1"] if has_gt else []):
        assert (by[role].kind, by[role].h, by[role].w, by[role].param) == (vis.TEXT, 7 * vis.TEXT_SCALE, (6 * vis.TEXT_CHARS - 1) * vis.TEXT_SCALE, vis.TEXT_SCALE)
    # five thumbnails to a row, row-major
    for k in range(n_ref):
        assert by[f"ref{k}"].y == by["ref0"].y + (k // 5) * (hh + vis.GAP) and by[f"ref{k}"].x == by["ref0"].x + (k % 5) * (hw + vis.GAP)
    if has_window:  # a frame lies on the panel it outlines, in magenta, and is painted behind it in the order
        for role in ("score", "overlay"):
            f, p = by[f"window_{role}"], by[role]
            assert (f.kind, f.y, f.x, f.h, f.w, f.rgb) == (vis.FRAME, p.y, p.x, p.h, p.w, (255, 0, 255)) and roles.index(f.role) > roles.index(role)


def test_layout_limits():
    vis.sheet_layout(518, 518, 5, True, True)
    with pytest.raises(ValueError, match="4096"):
        vis.sheet_layout(4090, 100, 0, False, False)
    with pytest.raises(ValueError, match="4096"):
        vis.sheet_layout(100, 4000, 0, False, False)
    with pytest.raises(ValueError, match="4096"):
        vis.sheet_layout(1000, 1000, 40, False, False)  # eight rows of thumbnails
    with pytest.raises(ValueError, match="48"):
        vis.sheet_layout(28, 42, 43, False, False)
    assert len(vis.sheet_layout(28, 42, 42, False, False)[2]) == 48


def test_window_rect_and_bind():
    canvas_h, canvas_w, panels = vis.sheet_layout(56, 70, 2, False, True)
    score = next(p for p in panels if p.role == "score")
    assert vis.window_rect(score, 56, 70, 0, 0, 56) == (score.y, score.x, 28, 28)
    assert vis.window_rect(score, 56, 70, 41, 55, 14) == (score.y + 20, score.x + 27, 7, 7)
    assert vis.window_rect(score, 56, 70, 55, 69, 1) == (score.y + 27, score.x + 34, 1, 1)  # never empty, never outside the panel
    images = {k: k.upper() for k in ("query", "query_on_map", "score", "turbo", "ref0", "ref1")}
    bound = vis.bind(panels, images, {"score_mean": 0.5}, (56, 70), (41, 55, 14))
    assert [p.role for p in bound] == [p.role for p in panels]
    by = {p.role: p for p in bound}
    assert by["overlay"].src == "QUERY_ON_MAP" and by["overlay"].src2 == "SCORE" and by["ref1"].src == "REF1" and by["score_mean"].text == " 0.500"
    assert (by["window_overlay"].h, by["window_overlay"].w) == (7, 7)
    assert [p.role for p in vis.bind(panels, images, {}, (56, 70), None)] == [p.role for p in panels if not p.role.startswith("window_")]
    _rects_inside(canvas_h, canvas_w, bound)


def test_number_text():
    assert vis.number_text(0.5) == " 0.500" and vis.number_text(-0.1234) == "-0.123" and vis.number_text(1.0) == " 1.000"
    assert vis.number_text(None) == "     -" and vis.number_text(float("nan")) == "     -" and vis.number_text(-12.3456) == "-12.34"
    assert all(c in vis.CHARS for v in (0.0, -1.0, 123456.0, float("inf")) for c in vis.number_text(v))


def _cfg(name, *over):
    return load_config(name, list(over))


@pytest.mark.parametrize("name,phase", [("default_predict", "predict"), ("default_test", "test")])
def test_options(name, phase):
    assert _cfg(name).this_main.vis_sheet is False  # the YAML's default
    assert vis.sheet_options(_cfg(name), phase) == (False, 0)
    assert vis.sheet_options(_cfg(name, "this_main.vis_sheet=True"), phase) == (True, 1)
    for n in (0, 2):
        assert vis.sheet_options(_cfg(name, "this_main.vis_sheet=True", f"logger.{phase}.write.config.vis_img_every_n_steps={n}"), phase) == (True, n)
    cfg = _cfg(name)
    del cfg.this_main["vis_sheet"]
    assert vis.sheet_options(cfg, phase) == (False, 0)
    with pytest.raises(ValueError, match="vis_sheet"):
        vis.sheet_options(_cfg(name, "this_main.vis_sheet=sometimes"), phase)
    for bad in ("-1", "1.5", "often"):
        with pytest.raises(ValueError, match="vis_img_every_n_steps"):
            vis.sheet_options(_cfg(name, "this_main.vis_sheet=True", f"logger.{phase}.write.config.vis_img_every_n_steps={bad}"), phase)
    with pytest.raises(ValueError, match="fused_input_stage=True"):
        vis.sheet_options(_cfg(name, "this_main.vis_sheet=True", "this_main.fused_input_stage=True"), phase)
    assert vis.sheet_options(_cfg(name, "this_main.fused_input_stage=True"), phase) == (False, 0)  # without the key nothing is refused here


def test_cadence():
    assert [i for i in range(5) if vis.sheet_due(i, 1)] == [0, 1, 2, 3, 4]
    assert [i for i in range(5) if vis.sheet_due(i, 2)] == [0, 2, 4]
    assert [i for i in range(5) if vis.sheet_due(i, 0)] == []
