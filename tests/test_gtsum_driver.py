"""`python -m crossscore_amd.summarise_gt` end to end on the tree of tests/nvs_tree.py: files mode against the reference's CSV
(tests/golden/s0_gt_summary.json) with both PNG decoders, compute mode on a tree without metric_map/ against files mode on the same tree once
crossscore_amd.metric_maps has filled it, and the join of the ground-truth CSV with the predicted CSV of an evaluate run (summary.correlate)."""
import json
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from gt_summary_golden import GOLDEN, golden_rows, read_rows  # noqa: E402
from nvs_tree import make_tree  # noqa: E402
from scenes import run_evaluate  # noqa: E402

torch = pytest.importorskip("torch")


@pytest.fixture(autouse=True)
def _in_tmp(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """(root, dataset path): the summary names its file after the two directories above res_540"""
    root = str(tmp_path_factory.mktemp("gtsum"))
    return root, make_tree(os.path.join(root, "gaussian", "mfr"), seed=GOLDEN["seed"])


@pytest.mark.gpu
@pytest.mark.parametrize("decoder", ["host", "gpu"])
def test_files_mode_writes_the_references_csv(tree, tmp_path, decoder, capsys):
    from crossscore_amd import summarise_gt as sg

    root, path = tree
    assert sg.main(["--dir_in", os.path.join(path, "res_540"), "--dir_out", str(tmp_path / "out"), "-n", "2", "--png_decoder", decoder]) == 0
    csv_path = tmp_path / "out" / "mfr" / "gaussian.csv"
    assert f"Write to csv {csv_path} (NORMAL)" in capsys.readouterr().out
    columns, rows = read_rows(csv_path)
    assert columns == GOLDEN["columns"] and rows == golden_rows("rows", root)
    # -f False leaves the file alone, --fast_debug is the reference's (one batch of 16 is never cut short by N = 0 or below)
    before = open(csv_path).read()
    assert sg.main(["--dir_in", os.path.join(path, "res_540"), "--dir_out", str(tmp_path / "out"), "-f", "False", "--source", "compute"]) == 0
    assert "(SKIP)" in capsys.readouterr().out and open(csv_path).read() == before


@pytest.mark.gpu
def test_compute_mode_equals_files_mode_on_the_generated_maps(tree, tmp_path):
    from crossscore_amd import summarise_gt as sg
    from crossscore_amd.config import load_config
    from crossscore_amd.metric_maps import generate

    _, path = tree
    bare = tmp_path / "gaussian" / "mfr"
    shutil.copytree(os.path.join(path, "res_540", "scene_a"), bare / "res_540" / "scene_a", ignore=shutil.ignore_patterns("metric_map"))
    shutil.copy(os.path.join(path, "res_540", "split.json"), bare / "res_540" / "split.json")
    dir_in = str(bare / "res_540")
    assert sg.list_frames(dir_in, "files") == []
    comp = sg.summarise(dir_in, tmp_path / "compute", num_workers=2, source="compute")
    assert comp["frames"] == 15 and not os.path.exists(bare / "res_540" / "scene_a" / "test" / "ours_1000" / "metric_map")
    gpu = sg.summarise(dir_in, tmp_path / "compute_gpu", num_workers=2, source="compute", png_decoder="gpu")
    res = generate(load_config("default_test", [f"data.dataset.path={bare}", "data.dataset.num_gaussians_iters=-1"]))
    assert len(res["written"]) == 30
    files = sg.summarise(dir_in, tmp_path / "files", num_workers=2, source="files")
    want = open(files["csv"], "rb").read()
    assert files["frames"] == 15 and want.count(b"\n") == 16
    assert open(comp["csv"], "rb").read() == want and open(gpu["csv"], "rb").read() == want


@pytest.mark.gpu
def test_sizes_that_differ_raise(tree, tmp_path):
    from PIL import Image

    from crossscore_amd import summarise_gt as sg

    _, path = tree
    d = tmp_path / "gaussian" / "mfr" / "res_540" / "scene_b"
    shutil.copytree(os.path.join(path, "res_540", "scene_b"), d)
    Image.fromarray(np.zeros((60, 80, 3), np.uint8)).save(d / "test" / "ours_1000" / "gt" / "frame_00000.png")
    with pytest.raises(ValueError, match=r"renders/frame_00000\.png is 60x84 and .*gt/frame_00000\.png is 60x80"):
        sg.summarise(str(tmp_path / "gaussian" / "mfr" / "res_540"), tmp_path / "o", num_workers=2, source="compute")


@pytest.mark.gpu
def test_ground_truth_and_predicted_summaries_join(tree, tmp_path, capsys):
    """The row keys of the two programs agree: evaluate's predicted CSV and summarise_gt's CSV of the same tree line up frame by frame."""
    from crossscore_amd import summarise_gt as sg
    from crossscore_amd import summary as sm

    _, path = tree
    res, _, _, _ = run_evaluate(path, tmp_path, "eval", [])
    pred_dir = os.path.join(res["out_dir"], "score_summary")
    assert os.path.exists(os.path.join(pred_dir, "mfr", "gaussian.csv"))
    sg.summarise(os.path.join(path, "res_540"), tmp_path / "gt", num_workers=2)
    # the test split evaluated scene_a (iterations 1000 and 7000) and scene_b, which has no maps to summarise
    filters = ([""], ["scene_a"], [""], [1000, 7000])
    gt = sm.read_summary(tmp_path / "gt", "mfr", *filters)
    pred = sm.read_summary(pred_dir, "mfr", *filters)
    assert len(gt) == len(pred) == 10
    out = sm.correlate(gt, pred, "gt_ssim_0_1", sm.infer_pred_column(pred))
    assert set(out["scenes"]) == {"scene_a"} and np.isfinite(out["all"]) and out["all"] == out["scenes"]["scene_a"]
    capsys.readouterr()
    assert sm.main(["--gt", str(tmp_path / "gt"), "--pred", pred_dir, "--dataset", "mfr", "--scenes", "scene_a", "--iters", "1000", "7000"]) == 0
    assert f"correlation all: {out['all']:.6f}" in capsys.readouterr().out
    assert json.dumps(out["all"])  # a plain float
