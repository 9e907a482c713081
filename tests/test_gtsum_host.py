"""Host side of the ground-truth score summary (crossscore_amd/summarise_gt.py, crossscore_amd/summary.py), without a GPU: the four integer
sums of a frame are formed here with numpy int64 and handed to rows_from_sums.  The CSV must equal, string for string, what the reference's
SummaryWriterGroundTruth wrote for the same tree (tests/golden/s0_gt_summary.json, made by tests/golden/make_golden_summary.py), and the reader
what the reference's SummaryReader returned."""
import csv
import math
import os
import re
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from gt_summary_golden import GOLDEN, TOKEN, golden_rows, read_rows  # noqa: E402
from nvs_tree import make_tree  # noqa: E402

from crossscore_amd import summarise_gt as sg  # noqa: E402
from crossscore_amd import summary as sm  # noqa: E402


def numpy_sums(ssim_u16, mae_u16):
    cs, cm = ssim_u16.astype(np.int64), mae_u16.astype(np.int64)
    return int(cs.sum()), int(np.clip(cs, 32767, 65534).sum()), int(cm.sum()), int((cm * cm).sum())


def sums_of_files(frames):
    from crossscore_amd.decode import read_metric_map_u16

    sums, sizes = [], []
    for fr in frames:
        a, b = read_metric_map_u16(fr.first), read_metric_map_u16(fr.second)
        sums.append(numpy_sums(a, b))
        sizes.append(a.shape)
    return sums, sizes


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("gtsum"))
    path = make_tree(os.path.join(root, "gaussian", "mfr"), seed=GOLDEN["seed"])
    dir_in = os.path.join(path, "res_540")
    frames = sg.list_frames(dir_in, "files")
    sums, sizes = sums_of_files(frames)
    return {"root": root, "dir_in": dir_in, "frames": frames, "rows": sg.rows_from_sums(frames, sums, sizes)}


def test_csv_equals_the_references_string_for_string(tree, tmp_path, capsys):
    path = sg.write_csv(tree["dir_in"], tmp_path, tree["rows"])
    assert path == str(tmp_path / "mfr" / "gaussian.csv")
    assert f"Write to csv {path} (NORMAL)" in capsys.readouterr().out
    columns, rows = read_rows(path)
    assert columns == GOLDEN["columns"] == sg.COLUMNS
    want = golden_rows("rows", tree["root"])
    assert len(rows) == len(want) == 17
    assert rows == want
    assert not any(r[0] == "scene_b" for r in rows)  # no metric_map directory: absent


def test_frames_are_listed_in_the_string_order_of_the_directories(tree):
    dirs = []
    for fr in tree["frames"]:
        d = os.path.relpath(os.path.dirname(os.path.dirname(fr.ssim_path)), tree["dir_in"])
        if d not in dirs:
            dirs.append(d)
    assert dirs == sorted(dirs)
    a_test = [d for d in dirs if d.startswith("scene_a/test/")]
    assert a_test == ["scene_a/test/ours_1000/metric_map", "scene_a/test/ours_30000/metric_map", "scene_a/test/ours_7000/metric_map"]
    for fr in tree["frames"]:
        assert fr.first == fr.ssim_path and fr.second == fr.ssim_path.replace("/metric_map/ssim/", "/metric_map/mae/")


def test_compute_source_lists_the_same_frames_from_renders_and_gt(tree):
    files = [f for f in tree["frames"]]
    comp = sg.list_frames(tree["dir_in"], "compute")
    # scene_b has renders/ and gt/ but no maps: compute lists it, files cannot
    assert [f.ssim_path for f in comp if "/scene_b/" not in f.ssim_path] == [f.ssim_path for f in files]
    assert sum("/scene_b/" in f.ssim_path for f in comp) == 2
    for f in comp:
        assert f.first == f.ssim_path.replace("/metric_map/ssim/", "/renders/") and f.second == f.ssim_path.replace("/metric_map/ssim/", "/gt/")
    with pytest.raises(ValueError):
        sg.list_frames(tree["dir_in"], "maps")


def test_skip_overwrite_and_fast_debug(tree, tmp_path, capsys):
    rows = tree["rows"]
    path = sg.write_csv(tree["dir_in"], tmp_path, rows)
    first = open(path).read()
    capsys.readouterr()
    called = []

    def never():
        called.append(1)
        return rows[:1]

    assert sg.write_csv(tree["dir_in"], tmp_path, never, force=False) is None  # SKIP: the rows are not even formed
    assert f"Write to csv {path} (SKIP)" in capsys.readouterr().out
    assert not called and open(path).read() == first
    assert sg.write_csv(tree["dir_in"], tmp_path, never, force=True) == path
    assert f"Write to csv {path} (OVERWRITE)" in capsys.readouterr().out
    assert called and len(read_rows(path)[1]) == 1
    # --fast_debug N > 0: the reference breaks behind batch N of 16 rows; N <= 0 keeps everything
    many = [rows[i % len(rows)] for i in range(40)]
    for n, want in ((1, 32), (2, 40), (0, 40), (-1, 40)):
        sg.write_csv(tree["dir_in"], tmp_path, many, force=True, fast_debug=n)
        assert len(read_rows(path)[1]) == want, n
    assert read_rows(path)[1][:17] == read_rows(path)[1][17:34]


@pytest.mark.parametrize("code", [0, 32766, 32767, 32768, 65534, 65535])
def test_clip_on_single_codes_is_the_references_fp32_expression(code):
    """metric_map_read (utils/io/images.py:38-43) then .clip(0, 1).mean() (score_summariser.py:40) on a one-pixel map."""
    m = np.array([[code]], dtype=np.uint16)
    ref = (m.astype(np.float32) / 32767 - 1)
    want_n11, want_01 = float(ref.mean()), float(ref.clip(0, 1).mean())
    got = sg.values_from_sums(numpy_sums(m, m), 1)
    assert abs(got[0] - want_n11) <= 2.0 ** -23 * max(1.0, abs(want_n11))  # one fp32 rounding of the reference
    assert abs(got[1] - want_01) <= 2.0 ** -23
    assert got[1] == {0: 0.0, 32766: 0.0, 32767: 0.0, 32768: 1 / 32767, 65534: 1.0, 65535: 1.0}[code]
    assert 0.0 <= got[1] <= 1.0


def test_zero_mse_prints_inf(tmp_path):
    z = np.zeros((3, 5), dtype=np.uint16)
    frames = [sg.Frame("/d/gaussian/mfr/res_540/s/test/ours_1/metric_map/ssim/frame_00000.png", "", "")]
    rows = sg.rows_from_sums(frames, [numpy_sums(np.full((3, 5), 65534, np.uint16), z)], [z.shape])
    assert rows[0][:3] == ["s", "d/gaussian/mfr/res_540/s/test/ours_1", "00000.png"]
    assert rows[0][3:7] == [1.0, 1.0, 0.0, 0.0] and rows[0][7] == math.inf
    path = sg.write_csv("/d/gaussian/mfr/res_540", tmp_path, rows)
    assert read_rows(path)[1][0][3:] == ["1.0000", "1.0000", "0.0000", "0.0000", "inf"]


def test_values_are_the_stated_rational_functions_in_fp64():
    s, n = (123456789, 234567890, 98765432, 2 ** 53 + 12345), 5000
    got = sg.values_from_sums(s, n)
    mse = s[3] / (65535 ** 2 * n)
    assert got == (s[0] / (32767 * n) - 1, (s[1] - 32767 * n) / (32767 * n), s[2] / (65535 * n), mse, -10 * math.log10(mse))


def test_mismatching_ssim_and_mae_listings_raise(tree, tmp_path):
    src = os.path.join(tree["dir_in"], "scene_a", "test", "ours_1000")
    dst = tmp_path / "res_540" / "scene_a" / "test" / "ours_1000"
    shutil.copytree(src, dst)
    assert len(sg.list_frames(tmp_path / "res_540", "files")) == 2
    os.remove(dst / "metric_map" / "mae" / "frame_00001.png")
    with pytest.raises(ValueError, match="same file names"):
        sg.list_frames(tmp_path / "res_540", "files")


# ------------------------------------------------------------------------------------------------------------------ summary.py
@pytest.fixture()
def summaries(tree, tmp_path):
    gt_dir, pred_dir = tmp_path / "gt", tmp_path / "pred"
    sg.write_csv(tree["dir_in"], gt_dir, tree["rows"])
    os.makedirs(pred_dir / GOLDEN["dataset"])
    with open(pred_dir / GOLDEN["dataset"] / f"{GOLDEN['method']}.csv", "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(GOLDEN["pred_columns"])
        w.writerows(golden_rows("pred_rows", tree["root"]))
    return str(gt_dir), str(pred_dir)


def _same_records(got, want, root):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for k, v in w.items():
            if isinstance(v, str):
                assert g[k] == v.replace(TOKEN, root.lstrip("/")), k
            else:
                assert g[k] == pytest.approx(v, abs=1e-9), k  # a "%.4f" field parsed by two float parsers


@pytest.mark.parametrize("name", list(GOLDEN["read_summary"]))
def test_read_summary_filters_and_order_are_the_references(tree, summaries, name):
    case = GOLDEN["read_summary"][name]
    args = (case["method_list"], case["scene_list"], case["split_list"], case["iter_list"])
    for which, d in zip(("gt", "pred"), summaries):
        got = sm.read_summary(d, GOLDEN["dataset"], *args)
        _same_records(got, case[which], tree["root"])
        assert got == sorted(got, key=lambda r: (r["scene_name"], r["rendered_dir"], r["image_name"], r["method_name"]))
    assert len(case["gt"]) == (17 if name == "all" else 4)


def test_read_summary_rejects_an_unknown_method_and_keeps_exact_iterations(summaries):
    gt_dir, _ = summaries
    with pytest.raises(ValueError, match="nerf is not available"):
        sm.read_summary(gt_dir, GOLDEN["dataset"], ["nerf"], [""], [""], [])
    rows = sm.read_summary(gt_dir, GOLDEN["dataset"], [""], ["scene_a"], ["train"], [7000])
    assert len(rows) == 3 and all(r["rendered_dir"].endswith("/scene_a/train/ours_7000") and r["method_name"] == "gaussian" for r in rows)
    assert sm.read_summary(gt_dir, GOLDEN["dataset"], [""], ["scene_none"], [""], []) == []


def test_check_rows_raises_the_references_three_errors(summaries):
    gt = sm.read_summary(summaries[0], GOLDEN["dataset"], [""], [""], [""], [])
    pred = sm.read_summary(summaries[1], GOLDEN["dataset"], [""], [""], [""], [])

    def verdict(a, b):
        try:
            sm.check_summary_gt_prediction_rows(a, b)
            return None
        except ValueError as e:
            return str(e)

    other_dir = [dict(r) for r in pred]
    other_dir[0]["rendered_dir"] = pred[1]["rendered_dir"] + "_x"
    other_name = [dict(r) for r in pred]
    other_name[0]["image_name"] = "99999.png"
    got = {"match": verdict(gt, pred), "length": verdict(gt, pred[:-1]), "rendered_dir": verdict(gt, other_dir),
           "image_name": verdict(gt, other_name)}
    assert got == GOLDEN["check"]
    with pytest.raises(ValueError):
        sm.correlate(gt, pred[:-1], "gt_ssim_0_1", "pred_ssim_0_1")


def test_correlate_is_corrcoef(summaries, capsys):
    gt = sm.read_summary(summaries[0], GOLDEN["dataset"], [""], [""], [""], [])
    pred = sm.read_summary(summaries[1], GOLDEN["dataset"], [""], [""], [""], [])
    res = sm.correlate(gt, pred, "gt_ssim_0_1", "pred_ssim_0_1")
    g = np.array([r["gt_ssim_0_1"] for r in gt])
    p = np.array([r["pred_ssim_0_1"] for r in pred])
    assert abs(res["all"] - np.corrcoef(g, p)[0, 1]) <= 1e-12
    assert set(res["scenes"]) == {"scene_a", "scene_c"}
    sel = np.array([r["scene_name"] == "scene_a" for r in gt])
    assert abs(res["scenes"]["scene_a"] - np.corrcoef(g[sel], p[sel])[0, 1]) <= 1e-12
    assert abs(res["scenes"]["scene_c"] - np.corrcoef(g[~sel], p[~sel])[0, 1]) <= 1e-12
    rng = np.random.default_rng(3)
    x = rng.normal(size=1000)
    y = 0.3 * x + rng.normal(size=1000)
    assert abs(sm.pearson(x, y) - np.corrcoef(x, y)[0, 1]) <= 1e-12
    assert math.isnan(sm.pearson([1.0], [2.0])) and math.isnan(sm.pearson([1.0, 1.0], [2.0, 3.0]))
    # the command prints the same numbers and infers the one pred_* column
    assert sm.main(["--gt", summaries[0], "--pred", summaries[1], "--dataset", GOLDEN["dataset"]]) == 0
    out = capsys.readouterr().out
    assert "gt_ssim_0_1 against pred_ssim_0_1" in out and f"correlation all: {res['all']:.6f}" in out


def test_the_new_ops_are_declared_bound_and_built():
    from crossscore_amd import _lib, build

    assert "gtsum.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "gtsum.hip"))
    hdr = open(os.path.join(REPO, "include", "crossscore_hip.h")).read()
    lib = _lib.load()
    for name in ("cs_op_metric_map_sums_u16", "cs_op_gt_metric_sums_u8"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and name in _lib.SYMBOLS and hasattr(lib, name), name
    # bad arguments are rejected on the host, before anything touches a device
    assert lib.cs_op_metric_map_sums_u16(None, None, 1, 4, 4, 4, 16, None, None) == _lib.CS_ERR_BAD_ARG
    assert lib.cs_op_gt_metric_sums_u8(None, None, 1, 4, 4, 48, None, None) == _lib.CS_ERR_BAD_ARG
