"""this_main.score_pool through the drivers: predict on the small synthetic scene of tests/scenes.py, evaluate on the tree of
tests/nvs_tree.py.  The CSV is compared string for string with the numpy statement (tests/score_pool_oracle.py) of the 16-bit score-map PNGs the same
run wrote, and of the ground-truth tensors evaluate hands to its tests; a run without the key writes what it wrote before."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import score_pool_oracle as oracle  # noqa: E402
from crossscore_amd import pooling  # noqa: E402
from crossscore_amd import summary as sm  # noqa: E402
from crossscore_amd.config import load_config  # noqa: E402
from nets import SMALL, state_dict_for  # noqa: E402
from nvs_tree import make_tree  # noqa: E402
from scenes import make_scene_with_copies, run_evaluate, tree_bytes  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NO_IMGS = ["logger.predict.write.flag.image_query=False", "logger.predict.write.flag.image_reference=False"]
SIGNED = True  # model.predict.metric.type=ssim: the gray16 writer stores [-1, 1]


def _predict(out, qd, rd, sd, *over):
    from crossscore_amd.predict import predict

    cfg = load_config("default_predict", [f"data.dataset.query_dir={qd}", f"data.dataset.reference_dir={rd}", f"model.backbone.from_pretrained={SMALL}",
                                          "this_main.resize_short_side=56", "data.neighbour_config.cross=2", "data.loader.validation.batch_size=2",
                                          f"logger.predict.out_dir={out}", "logger.predict.write.config.score_map_colour_mode=gray",
                                          "logger.predict.write.flag.item_path_json=True", *NO_IMGS, *over])
    assert pooling.signed_range_of(cfg.model.predict.metric.type) is SIGNED
    return predict(cfg, state_dict=sd, now="T")


def _pool_files(out_dir):
    root = os.path.join(out_dir, "score_pool")
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    root = tmp_path_factory.mktemp("score_pool")
    qd, rd = make_scene_with_copies(str(root / "data"))
    return root, qd, rd, state_dict_for(SMALL, 6)


@pytest.mark.parametrize("encoder", ["host", "gpu"])
def test_predict_csv_is_the_pool_of_the_written_pngs(scene, encoder):
    from PIL import Image

    root, qd, rd, sd = scene
    window = 14 if encoder == "host" else 56  # (56: the default, the whole height of the 56-pixel maps)
    over = ["this_main.score_pool=True", f"this_main.png_encoder={encoder}"] + (["this_main.score_pool_window=14"] if window == 14 else [])
    res = _predict(str(root / f"on_{encoder}"), qd, rd, sd, *over)
    assert res["score_pool"] is True
    assert _pool_files(res["out_dir"]) == ["mfr/gaussian.csv"]
    path = os.path.join(res["out_dir"], "score_pool", "mfr", "gaussian.csv")
    assert path in res["files"]
    names = pooling.value_names(pooling.PERMILLE, window)
    header, rows = oracle.read_rows(path)
    assert header == ["scene_name", "rendered_dir", "image_name"] + [f"pred_{k}" for k in names]
    _, summary_rows = oracle.read_rows(os.path.join(res["out_dir"], "score_summary", "mfr", "gaussian.csv"))
    assert [r[:3] for r in rows] == [r[:3] for r in summary_rows] and len(rows) == 6  # the score summary's images in its order
    for i, r in enumerate(rows):
        png = os.path.join(res["out_dir"], "batch", "score_map_ref_cross", f"r0_B{i // 2:04}_b{i % 2:03}_s00001_test_ours_1000_renders_frame_{i:05}.png")
        codes = np.array(Image.open(png))
        assert codes.dtype == np.uint16 and r[2] == f"{i:05}.png"
        assert r[3:] == oracle.fields(codes, pooling.PERMILLE, window, SIGNED), (i, encoder)
    # the 16-bit mean is the score summary's mean up to the truncation of the codes: one code at the most, plus the summary's four digits
    for r, s in zip(rows, summary_rows):
        assert abs(float(r[3]) - float(s[3])) <= 1.0 / 32767 + 1e-4


def test_the_key_changes_no_other_file_and_depth_changes_nothing(scene):
    root, qd, rd, sd = scene
    off = _predict(str(root / "off"), qd, rd, sd, "this_main.batches_in_flight=3")
    on3 = _predict(str(root / "on3"), qd, rd, sd, "this_main.batches_in_flight=3", "this_main.score_pool=True")
    on1 = _predict(str(root / "on1"), qd, rd, sd, "this_main.batches_in_flight=1", "this_main.score_pool=True")
    assert off["score_pool"] is False and not os.path.exists(os.path.join(off["out_dir"], "score_pool"))
    a, b, c = tree_bytes(off["out_dir"]), tree_bytes(on3["out_dir"]), tree_bytes(on1["out_dir"])
    pool = os.path.join("score_pool", "mfr", "gaussian.csv")
    assert sorted(b) == sorted(list(a) + [pool]) and sorted(c) == sorted(b)
    for rel in a:
        assert a[rel] == b[rel] == c[rel], rel
    assert b[pool] == c[pool]


def test_a_window_larger_than_the_map_is_refused_with_both_named(scene):
    root, qd, rd, sd = scene
    with pytest.raises(ValueError, match=r"score_pool_window=57.*56x"):
        _predict(str(root / "bad_window"), qd, rd, sd, "this_main.score_pool=True", "this_main.score_pool_window=57")
    with pytest.raises(ValueError, match="score_pool_window needs"):
        _predict(str(root / "bad_alone"), qd, rd, sd, "this_main.score_pool_window=14")


def _key(path):
    parts = path.split("/")
    return os.path.join(*parts[:-2]), parts[-1].replace("frame_", "")


@pytest.mark.parametrize("mode", ["files", "compute"])
def test_evaluate_pools_prediction_and_ground_truth(tmp_path_factory, tmp_path, monkeypatch, mode, capsys):
    monkeypatch.chdir(tmp_path)  # the log/<now>/test_empty_ckpt/version_<n> directories land here
    tree = make_tree(tmp_path_factory.mktemp("score_pool_nvs") / "nvs" / "tree")
    window = 14
    res, cap, _, _ = run_evaluate(tree, tmp_path, "out", ["this_main.score_pool=True", f"this_main.score_pool_window={window}",
                                                          f"this_main.gt_metric_maps={mode}"])
    assert res["score_pool"] is True
    files = _pool_files(res["out_dir"])
    root = os.path.join(res["out_dir"], "score_summary")
    assert files == sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs) and len(files) == 1
    names = pooling.value_names(pooling.PERMILLE, window)
    columns = [f"pred_{k}" for k in names] + [f"gt_{k}" for k in names]
    header, rows = oracle.read_rows(os.path.join(res["out_dir"], "score_pool", files[0]))
    assert header == ["scene_name", "rendered_dir", "image_name"] + columns and len(rows) == 12
    _, summary_rows = oracle.read_rows(os.path.join(root, files[0]))
    assert [r[:3] for r in rows] == [r[:3] for r in summary_rows]
    by_key = {(r[1], r[2]): r for r in rows}
    seen = nan_rows = 0
    for c in cap:
        for b, qp in enumerate(c["item_paths"]["query/img"]):
            r = by_key[_key(qp)]
            assert r[3:3 + len(names)] == oracle.fields(oracle.gray16(c["score"][b], SIGNED), pooling.PERMILLE, window, SIGNED), qp
            placeholder = mode == "files" and "scene_b" in qp  # scene_b has no metric_map directory
            want = ["nan"] * len(names) if placeholder else oracle.fields(oracle.gray16(c["gt"][b], SIGNED), pooling.PERMILLE, window, SIGNED)
            assert r[3 + len(names):] == want, qp
            seen += 1
            nan_rows += placeholder
    assert seen == 12 and (nan_rows >= 1 if mode == "files" else nan_rows == 0)
    # the correlation of the run summary = summary.pearson over the file's own columns, placeholder rows left out
    keep = [r for r in rows if r[-1] != "nan"]
    corr = res["score_pool_correlation"]
    assert sorted(corr) == sorted(names)
    for k in names:
        want = sm.pearson([float(r[3 + columns.index(f"pred_{k}")]) for r in keep], [float(r[3 + columns.index(f"gt_{k}")]) for r in keep])
        assert corr[k] == want or (np.isnan(corr[k]) and np.isnan(want)), k
    # crossscore_amd.summary reads <run>/score_pool like a score summary (here on both sides: the file holds the gt_ columns too)
    pool_dir = os.path.join(res["out_dir"], "score_pool")
    dataset = files[0].split(os.sep)[0]
    assert sm.main(["--gt", pool_dir, "--pred", pool_dir, "--dataset", dataset, "--gt_column", "gt_low050", "--pred_column", "pred_low050"]) == 0
    out = capsys.readouterr().out
    assert "12 frames, gt_low050 against pred_low050" in out
    if mode == "compute":
        assert f"correlation all: {corr['low050']:.6f}" in out
