"""this_main.vis_sheet through the drivers: predict on the small synthetic scene of tests/scenes.py, evaluate on the tree
of tests/nvs_tree.py.  Every vis/ file is compared byte for byte with the numpy statement's (tests/sheet_oracle.py) composition of the PNG files
the same run wrote for item 0 under batch/, with the numbers of its CSVs; a run without the key writes what it wrote before."""
import glob
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import sheet_oracle as oracle  # noqa: E402
from crossscore_amd import vis  # noqa: E402
from crossscore_amd.config import load_config  # noqa: E402
from crossscore_amd.writers import colormap_table  # noqa: E402
from nets import SMALL, state_dict_for  # noqa: E402
from nvs_tree import make_tree  # noqa: E402
from scenes import make_scene_with_copies, read_csv_dicts, run_evaluate, tree_bytes  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ON = "this_main.vis_sheet=True"


def _predict(out, qd, rd, sd, *over):
    from crossscore_amd.predict import predict

    cfg = load_config("default_predict", [f"data.dataset.query_dir={qd}", f"data.dataset.reference_dir={rd}", f"model.backbone.from_pretrained={SMALL}",
                                          "this_main.resize_short_side=56", "data.neighbour_config.cross=2", "data.loader.validation.batch_size=2",
                                          f"logger.predict.out_dir={out}", *over])
    assert cfg.logger.predict.write.config.score_map_colour_mode == "rgb" and cfg.logger.predict.write.flag.image_reference  # the defaults
    return predict(cfg, state_dict=sd, now="T")


def _png(path):
    from PIL import Image

    return np.array(Image.open(path))


def _one(pattern):
    hits = sorted(glob.glob(pattern))
    assert len(hits) == 1, (pattern, hits)
    return hits[0]


def _sheets(out_dir):
    d = os.path.join(out_dir, "vis")
    return sorted(os.listdir(d)) if os.path.isdir(d) else []


def _number(v):
    """a number as the sheet prints it: "%.3f", right-aligned in six characters"""
    return ("%.3f" % v)[:6].rjust(6)


def _want_sheet(out_dir, batch_idx, numbers, has_gt=False, window=None, extra=None):
    """the oracle's composition of what the run wrote for item 0 of the batch"""
    b = os.path.join(out_dir, "batch")
    stem = f"r0_B{batch_idx:04}_b000_"
    images = {"query": _png(_one(os.path.join(b, "image_query", stem + "*.png"))), "turbo": colormap_table("turbo"),
              "score": _png(_one(os.path.join(b, "score_map_ref_cross", stem + "*.png")))}
    refs = sorted(glob.glob(os.path.join(b, "image_reference", stem + "*", "cross", "ref*.png")))
    images.update({f"ref{k}": _png(p) for k, p in enumerate(refs)})
    images.update(extra or {})
    H, W = images["query"].shape[:2]
    map_h, map_w = images["score"].shape[:2]  # the query's whole patches
    assert map_h <= H and map_w <= W
    images["query_on_map"] = images["query"][:map_h, :map_w]
    canvas_h, canvas_w, panels = vis.sheet_layout(H, W, len(refs), has_gt, window is not None)
    bound = vis.bind(panels, images, {}, (map_h, map_w), window)
    ps = [oracle.P(p.kind, p.y, p.x, p.h, p.w, p.src, p.src2, p.rgb, p.param, numbers[p.role] if p.kind == oracle.TEXT else "") for p in bound]
    return oracle.compose(ps, canvas_h, canvas_w)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    root = tmp_path_factory.mktemp("sheet")
    qd, rd = make_scene_with_copies(str(root / "data"))
    return root, qd, rd, state_dict_for(SMALL, 6)


@pytest.fixture(scope="module")
def runs(scene):
    """the runs the predict tests share: the key on with each encoder (three batches in flight), on one at a time, and off"""
    root, qd, rd, sd = scene
    return {name: _predict(str(root / name), qd, rd, sd, *over) for name, over in (
        ("host", [ON]), ("gpu", [ON, "this_main.png_encoder=gpu"]), ("one", [ON, "this_main.batches_in_flight=1"]), ("off", []))}


def test_predict_sheets_are_the_composition_of_the_written_pngs(runs):
    res = runs["host"]
    assert res["vis_sheet"] is True and res["vis_sheets"] == 3 and res["input_stage"].startswith("two-launch")
    assert _sheets(res["out_dir"]) == [f"r0_B{i:04}_b0.png" for i in range(3)]
    rows = read_csv_dicts(os.path.join(res["out_dir"], "score_summary", "mfr", "gaussian.csv"))
    column = [k for k in rows[0] if k.startswith("pred_")][0]
    for i in range(3):
        path = os.path.join(res["out_dir"], "vis", f"r0_B{i:04}_b0.png")
        assert path in res["files"]
        row = rows[2 * i]  # item 0 of batch i is frame 2 i; the file is sorted by frame
        assert row["image_name"] == f"{2 * i:05}.png"
        want = _want_sheet(res["out_dir"], i, {"score_mean": _number(float(row[column]))})
        got = _png(path)
        assert got.shape == want.shape and np.array_equal(got, want), i
    assert len({open(os.path.join(res["out_dir"], "vis", f), "rb").read() for f in _sheets(res["out_dir"])}) == 3  # three different sheets


def test_both_encoders_and_every_depth_give_the_same_sheets(runs):
    host, gpu, one = runs["host"], runs["gpu"], runs["one"]
    assert gpu["png_encoder"] == "gpu" and _sheets(gpu["out_dir"]) == _sheets(host["out_dir"]) == _sheets(one["out_dir"])
    for f in _sheets(host["out_dir"]):
        assert np.array_equal(_png(os.path.join(host["out_dir"], "vis", f)), _png(os.path.join(gpu["out_dir"], "vis", f))), f
    a, b = tree_bytes(host["out_dir"]), tree_bytes(one["out_dir"])
    assert sorted(a) == sorted(b)
    for rel in a:
        assert a[rel] == b[rel], rel  # one batch in flight or three: equal files


def test_the_key_changes_no_other_file(runs):
    on, off = runs["host"], runs["off"]
    assert off["vis_sheet"] is False and off["vis_sheets"] == 0 and not os.path.exists(os.path.join(off["out_dir"], "vis"))
    a, b = tree_bytes(off["out_dir"]), tree_bytes(on["out_dir"])
    assert sorted(b) == sorted(list(a) + [os.path.join("vis", f) for f in _sheets(on["out_dir"])])
    for rel in a:
        assert a[rel] == b[rel], rel


def test_cadence(scene, runs):
    root, qd, rd, sd = scene
    two = _predict(str(root / "two"), qd, rd, sd, ON, "logger.predict.write.config.vis_img_every_n_steps=2")
    none = _predict(str(root / "none"), qd, rd, sd, ON, "logger.predict.write.config.vis_img_every_n_steps=0")
    assert _sheets(two["out_dir"]) == ["r0_B0000_b0.png", "r0_B0002_b0.png"] and two["vis_sheets"] == 2
    assert _sheets(none["out_dir"]) == [] and none["vis_sheets"] == 0 and none["vis_sheet"] is True
    every = tree_bytes(runs["host"]["out_dir"])
    for f in _sheets(two["out_dir"]):
        assert tree_bytes(two["out_dir"])[os.path.join("vis", f)] == every[os.path.join("vis", f)]


def test_sheets_do_not_need_the_batch_writer_and_refuse_the_one_pass_stage(scene):
    root, qd, rd, sd = scene
    res = _predict(str(root / "nobatch"), qd, rd, sd, ON, "logger.predict.write.flag.batch=False")
    assert _sheets(res["out_dir"]) == [f"r0_B{i:04}_b0.png" for i in range(3)] and not os.path.exists(os.path.join(res["out_dir"], "batch"))
    with pytest.raises(ValueError, match="fused_input_stage=True"):
        _predict(str(root / "fused"), qd, rd, sd, ON, "this_main.fused_input_stage=True")


def test_the_worst_window_is_framed_where_the_pool_csv_says(scene):
    root, qd, rd, sd = scene
    res = _predict(str(root / "pool"), qd, rd, sd, ON, "this_main.score_pool=True", "this_main.score_pool_window=14")
    rows = read_csv_dicts(os.path.join(res["out_dir"], "score_summary", "mfr", "gaussian.csv"))
    pool = read_csv_dicts(os.path.join(res["out_dir"], "score_pool", "mfr", "gaussian.csv"))
    column = [k for k in rows[0] if k.startswith("pred_")][0]
    for i in range(3):
        window = (int(pool[2 * i]["pred_window_y"]), int(pool[2 * i]["pred_window_x"]), 14)
        want = _want_sheet(res["out_dir"], i, {"score_mean": _number(float(rows[2 * i][column]))}, window=window)
        got = _png(os.path.join(res["out_dir"], "vis", f"r0_B{i:04}_b0.png"))
        assert np.array_equal(got, want), i
        H, W = _png(_one(os.path.join(res["out_dir"], "batch", "score_map_ref_cross", f"r0_B{i:04}_b000_*.png"))).shape[:2]
        query = _png(_one(os.path.join(res["out_dir"], "batch", "image_query", f"r0_B{i:04}_b000_*.png")))
        score = next(p for p in vis.sheet_layout(query.shape[0], query.shape[1], 2, False, True)[2] if p.role == "score")
        y, x = score.y + window[0] * score.h // H, score.x + window[1] * score.w // W  # the corner, scaled into the panel by floor
        assert tuple(got[y, x]) == (255, 0, 255) and tuple(got[y + 1, x + 1]) != (255, 0, 255)  # magenta, one pixel thick


def test_evaluate_sheets_show_the_ground_truth_and_the_difference(tmp_path_factory, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    tree = make_tree(tmp_path_factory.mktemp("sheet_nvs") / "nvs" / "tree")
    res, cap, _, _ = run_evaluate(tree, tmp_path, "out", [ON, "logger.test.write.flag.score_map_gt=True", "logger.test.write.flag.image_query=True",
                                                          "logger.test.write.flag.image_reference=True",
                                                          "logger.test.write.config.score_map_colour_mode=rgb"])
    assert res["vis_sheet"] is True and res["vis_sheets"] == len(cap) == 3
    assert _sheets(res["out_dir"]) == [f"r0_B{i:04}_b0.png" for i in range(3)]
    table = colormap_table("turbo")
    summary = {}
    for path in glob.glob(os.path.join(res["out_dir"], "score_summary", "*", "*.csv")):
        for r in read_csv_dicts(path):
            summary[(r["rendered_dir"], r["image_name"])] = float([v for k, v in r.items() if k.startswith("pred_")][0])
    for c in cap:
        i = c["batch_idx"]
        parts = c["item_paths"]["query/img"][0].split("/")
        mean = summary[(os.path.join(*parts[:-2]), parts[-1].replace("frame_", ""))]
        score, gt, n = c["score"][0], c["gt"][0], c["score"][0].size
        y = np.abs(score - gt).astype(np.float32) * np.float32(256)  # cs_op_score_to_rgb on [0, 1]
        diff = table[np.where(y >= 256, 255, np.where(y >= 0, np.minimum(y, 255).astype(np.int64), 0))]
        gt_png = _png(_one(os.path.join(res["out_dir"], "batch", "score_map_gt", f"r0_B{i:04}_b000_*.png")))
        numbers = {"score_mean": _number(mean), "gt_mean": _number(float(c["stats"][0][2]) / n), "l1": _number(float(c["stats"][0][0]) / n)}
        want = _want_sheet(res["out_dir"], i, numbers, has_gt=True, extra={"gt": gt_png, "diff": diff})
        got = _png(os.path.join(res["out_dir"], "vis", f"r0_B{i:04}_b0.png"))
        assert got.shape == want.shape and np.array_equal(got, want), i
