"""this_main.reference_use / reference_use_images through the drivers: predict on the small synthetic scene of
tests/test_select_driver.py, evaluate on the test split of tests/nvs_tree.py.  reference_use.csv does not depend on how the tokens are made, its rows
are the fp64 means of the module's outputs, its reference columns are reference_selection.csv's, the image files exist under both PNG encoders with
equal pixels, and a run without the keys writes what it wrote before."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from crossscore_amd import scoring  # noqa: E402
from crossscore_amd.config import load_config  # noqa: E402
from nvs_tree import make_tree  # noqa: E402
from nets import SMALL, state_dict_for  # noqa: E402
from scenes import make_scene_with_copies, tree_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

NO_IMGS = ["logger.predict.write.flag.image_query=False", "logger.predict.write.flag.image_reference=False"]
EMPTY = "empty_image"


def _predict(out, qd, rd, sd, *over):
    from crossscore_amd.predict import predict

    cfg = load_config("default_predict", [f"data.dataset.query_dir={qd}", f"data.dataset.reference_dir={rd}", f"model.backbone.from_pretrained={SMALL}",
                                          "this_main.resize_short_side=56", "data.neighbour_config.cross=2", "data.loader.validation.batch_size=2",
                                          f"logger.predict.out_dir={out}", "logger.predict.write.config.score_map_colour_mode=gray",
                                          "logger.predict.write.flag.item_path_json=True", *NO_IMGS, *over])
    return predict(cfg, state_dict=sd, now="T")


def _csv(out_dir, name="reference_use.csv"):
    with open(os.path.join(out_dir, name)) as f:
        return list(csv.reader(f))


class _Recorder:
    """scoring.reference_use_row with its arguments kept: the module's outputs of every query, as the driver read them"""

    def __init__(self, monkeypatch):
        self.calls = []
        inner = scoring.reference_use_row

        def wrapped(share, peak_prob, entropy):
            self.calls.append((share.clone(), peak_prob.clone(), entropy.clone()))
            return inner(share, peak_prob, entropy)

        monkeypatch.setattr(scoring, "reference_use_row", wrapped)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    root = tmp_path_factory.mktemp("ref_use")
    qd, rd = make_scene_with_copies(str(root / "data"))
    return root, qd, rd, state_dict_for(SMALL, 6)


@pytest.mark.parametrize("strategy", ["similar", "random"])
def test_the_csv_holds_the_means_of_the_modules_outputs_however_the_tokens_are_made(scene, strategy, monkeypatch):
    root, qd, rd, sd = scene
    rec = _Recorder(monkeypatch)
    common = [f"data.neighbour_config.strategy={strategy}", "this_main.reference_use=True"]
    base = _predict(str(root / f"{strategy}_base"), qd, rd, sd, *common, "this_main.fused_input_stage=False", "this_main.batches_in_flight=3")
    assert base["reference_use"] is True and os.path.join(base["out_dir"], "reference_use.csv") in base["files"]
    rows = _csv(base["out_dir"])
    assert rows[0] == ["query", "reference_0", "reference_1", "share_0", "share_1", "peak_0", "peak_1", "focus"]
    assert [r[0] for r in rows[1:]] == [f"frame_{i:05}.png" for i in range(6)] and len(rec.calls) == 6
    names = set(os.listdir(rd))
    for r, (share, peak, ent) in zip(rows[1:], rec.calls):
        assert r[1] in names and r[2] in names
        N, h, w = share.shape
        assert (N, h, w) == (2, 4, 5) and tuple(ent.shape) == (4, 5)
        want = (["%.4f" % v for v in share.numpy().astype(np.float64).reshape(N, -1).mean(axis=1)] +
                ["%.4f" % v for v in peak.numpy().astype(np.float64).reshape(N, -1).mean(axis=1)] +
                ["%.4f" % (1.0 - ent.numpy().astype(np.float64).mean() / np.log2(N * h * w))])
        assert r[3:] == want, (r, want)
        assert abs(float(r[3]) + float(r[4]) - 1.0) <= 1e-3 and 0.0 <= float(r[7]) <= 1.0
        assert all(float(r[5 + k]) <= float(r[3 + k]) + 1e-4 for k in range(N))
    if strategy == "similar":  # the references are the ones reference_selection.csv lists
        assert [r[:3] for r in rows] == [r[:3] for r in _csv(base["out_dir"], "reference_selection.csv")]
    want = open(os.path.join(base["out_dir"], "reference_use.csv"), "rb").read()
    variants = [("auto", 1, True), ("auto", 3, True)] + ([(False, 1, False), ("auto", 3, False)] if strategy == "random" else [])
    for fused, depth, cached in variants:
        res = _predict(str(root / f"{strategy}_{fused}_{depth}_{cached}"), qd, rd, sd, *common, f"this_main.fused_input_stage={fused}",
                       f"this_main.batches_in_flight={depth}", f"this_main.cache_reference_tokens={cached}")
        assert res["input_stage"].startswith("one-pass" if fused == "auto" else "two-launch")
        assert open(os.path.join(res["out_dir"], "reference_use.csv"), "rb").read() == want, (fused, depth, cached)
    # without the keys: no such file, and every other file as with them
    off = _predict(str(root / f"{strategy}_off"), qd, rd, sd, f"data.neighbour_config.strategy={strategy}", "this_main.fused_input_stage=False",
                   "this_main.batches_in_flight=3")
    assert off["reference_use"] is False
    a, b = tree_bytes(off["out_dir"]), tree_bytes(base["out_dir"])
    assert sorted(a) == sorted(k for k in b if k != "reference_use.csv") and "reference_use.csv" in b
    for rel in a:
        assert a[rel] == b[rel], rel


def test_image_files_exist_and_both_encoders_give_the_same_pixels(scene, monkeypatch):
    from PIL import Image

    from crossscore_amd.writers import colormap_table, focus_map

    root, qd, rd, sd = scene
    rec = _Recorder(monkeypatch)
    over = ["data.neighbour_config.strategy=similar", "this_main.reference_use=True", "this_main.reference_use_images=True"]
    host = _predict(str(root / "img_host"), qd, rd, sd, *over, "this_main.png_encoder=host")
    n_host = len(rec.calls)
    gpu = _predict(str(root / "img_gpu"), qd, rd, sd, *over, "this_main.png_encoder=gpu")
    sel = _csv(host["out_dir"])[1:]
    table = colormap_table("turbo")

    def index(x):  # cs_op_score_to_rgb on [0, 1]
        y = x.astype(np.float32) * np.float32(256)
        return np.where(y >= 256, 255, np.where(y >= 0, np.minimum(y, 255).astype(np.int64), 0))

    for i, row in enumerate(sel):
        stem = f"r0_B{i // 2:04}_b{i % 2:03}_s00001_test_ours_1000_renders_frame_{i:05}"
        rel = os.path.join("batch", "reference_use", stem, "cross")
        share, _, ent = rec.calls[i]
        want = {"focus.png": table[index(focus_map(ent[None], 2)[0].numpy())]}
        for k, name in enumerate(row[1:3]):
            want[f"ref{k:02}_s00001_test_ours_1000_gt_{os.path.splitext(name)[0]}.png"] = table[index(share[k].numpy())]
        assert sorted(os.listdir(os.path.join(host["out_dir"], rel))) == sorted(want)
        for name, pixels in want.items():
            assert os.path.join(host["out_dir"], rel, name) in host["files"]
            a = np.array(Image.open(os.path.join(host["out_dir"], rel, name)))
            b = np.array(Image.open(os.path.join(gpu["out_dir"], rel, name)))
            assert a.shape == (4, 5, 3) and np.array_equal(a, b), (rel, name)
            assert np.array_equal(a, pixels), (rel, name)
    assert n_host == 6 and len(rec.calls) == 12
    for (s0, p0, e0), (s1, p1, e1) in zip(rec.calls[:6], rec.calls[6:]):
        assert torch.equal(s0, s1) and torch.equal(p0, p1) and torch.equal(e0, e1)
    assert gpu["png_files"]["png_gpu_files"] >= 18 and host["png_files"]["png_gpu_files"] == 0


def test_options_are_checked_before_the_run(scene):
    root, qd, rd, sd = scene
    with pytest.raises(ValueError, match="reference_use_images"):
        _predict(str(root / "bad0"), qd, rd, sd, "this_main.reference_use_images=True")
    with pytest.raises(ValueError, match="reference_use_images"):
        _predict(str(root / "bad1"), qd, rd, sd, "this_main.reference_use=True", "this_main.reference_use_images=True", "logger.predict.write.flag.batch=False")


def test_evaluate_names_padded_places_as_the_selection_does(tmp_path_factory):
    from crossscore_amd.evaluate import evaluate

    tree = make_tree(tmp_path_factory.mktemp("ref_use_nvs") / "nvs" / "tree")
    sd = state_dict_for(SMALL, 6)
    outs = []
    cwd = os.getcwd()
    for name, fused, depth in (("a", False, 3), ("b", "auto", 1)):
        work = str(tmp_path_factory.mktemp(f"ref_use_eval_{name}"))
        os.chdir(work)
        try:
            cfg = load_config("default_test", [f"data.dataset.path={tree}", f"model.backbone.from_pretrained={SMALL}", "this_main.resize_short_side=56",
                                               "data.dataset.num_gaussians_iters=2", "data.loader.validation.batch_size=4",
                                               "data.loader.validation.num_workers=2", "data.neighbour_config.cross=2",
                                               "data.neighbour_config.strategy=similar", "logger.test.out_dir=out",
                                               "logger.test.write.flag.image_query=False", "logger.test.write.flag.image_reference=False",
                                               "this_main.reference_use=True", f"this_main.fused_input_stage={fused}", f"this_main.batches_in_flight={depth}"])
            with torch.no_grad():
                res = evaluate(cfg, state_dict=sd, now="NOW")
        finally:
            os.chdir(cwd)
        assert res["reference_use"] is True
        outs.append(os.path.join(work, "out"))
    use, sel = _csv(outs[0]), _csv(outs[0], "reference_selection.csv")
    assert len(use) == 13 and [r[:3] for r in use] == [r[:3] for r in sel]
    padded = [r for r in use[1:] if EMPTY in r[1:3]]
    assert padded and all(r[0].count("/") == 4 for r in use[1:])
    for r in use[1:]:
        assert abs(float(r[3]) + float(r[4]) - 1.0) <= 1e-3
    assert open(os.path.join(outs[0], "reference_use.csv"), "rb").read() == open(os.path.join(outs[1], "reference_use.csv"), "rb").read()
