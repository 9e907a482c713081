"""evaluate with data.neighbour_config.strategy=similar on the test split of tests/nvs_tree.py, cross = 2: the candidate
lists hold 3 (a real choice), 2 (= N) and 1 file (padding with "empty_image").  Every query chooses inside its own list, the scores are
forward_cached on what it chose, and the run does not depend on how the tokens are made or where the ground truth comes from."""
import csv
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from crossscore_amd.config import load_config  # noqa: E402
from nets import SMALL, state_dict_for  # noqa: E402
from nvs_tree import make_tree  # noqa: E402
from scenes import tree_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

EMPTY = "empty_image"


def _config(tree, *over):
    return load_config("default_test", [f"data.dataset.path={tree}", f"model.backbone.from_pretrained={SMALL}", "this_main.resize_short_side=56",
                                        "data.dataset.num_gaussians_iters=2", "data.loader.validation.batch_size=4",
                                        "data.loader.validation.num_workers=2", "data.neighbour_config.cross=2",
                                        "data.neighbour_config.strategy=similar", "logger.test.out_dir=out",
                                        "logger.test.write.flag.item_path_json=True", "logger.test.write.flag.image_query=False",
                                        "logger.test.write.flag.image_reference=False", *over])


def _run(tree, root, name, sd, *over):
    """one evaluate run in a directory of its own (log/<now>/test_empty_ckpt/version_0 lands in the working directory) -> (result, capture)"""
    from crossscore_amd.evaluate import evaluate

    cwd = os.getcwd()
    work = os.path.join(str(root), name)
    os.makedirs(work)
    os.chdir(work)
    try:
        cfg = _config(tree, *over)
        cap = []
        with torch.no_grad():
            res = evaluate(cfg, state_dict=sd, now="NOW", capture=cap)
        return dict(res, work=work), cap
    finally:
        os.chdir(cwd)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """the tree with metric_map/ written by the project's own generator (so that files and compute read the same ground truth), and the base run"""
    from crossscore_amd.metric_maps import generate

    tree = make_tree(tmp_path_factory.mktemp("grouped") / "nvs" / "tree")
    for root, dirs, _ in os.walk(tree):
        if "metric_map" in dirs:
            shutil.rmtree(os.path.join(root, "metric_map"))
            dirs.remove("metric_map")
    generate(load_config("default_test", [f"data.dataset.path={tree}"]))
    root = tmp_path_factory.mktemp("grouped_runs")
    sd = state_dict_for(SMALL, 6)
    base, cap = _run(tree, root, "base", sd, "this_main.fused_input_stage=False", "this_main.png_decoder=host", "this_main.batches_in_flight=3",
                     "this_main.gt_metric_maps=files")
    return tree, root, sd, base, cap


def _selection(res):
    with open(os.path.join(res["work"], "out", "reference_selection.csv")) as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["query", "reference_0", "reference_1", "similarity_0", "similarity_1"]
    return rows[1:]


def test_every_query_chooses_inside_its_own_candidate_list(scene):
    from crossscore_amd.nvs import NvsItems

    tree, _, _, base, cap = scene
    assert base["reference_strategy"] == "similar" and base["input_stage"].startswith("two-launch")
    items = NvsItems(tree, None, "test", {"strategy": "similar", "cross": 2, "deterministic": True}, "ssim", 2, candidates=True)
    group_of = {items[i]["query/img"]: items.groups[items[i]["reference/cross/group"]] for i in range(len(items))}
    sel = _selection(base)
    assert len(sel) == 12 and len(group_of) == 12
    name = lambda p: "/".join(p.split(os.sep)[-5:])  # noqa: E731
    by_query = {name(q): g for q, g in group_of.items()}
    sizes = []
    for row in sel:
        group = [name(p) for p in by_query[row[0]]]
        sizes.append(len(group))
        picks = [r for r in row[1:3] if r != EMPTY]
        assert all(r in group for r in picks) and len(set(picks)) == len(picks), row
        assert len(picks) == min(2, len(group)), row
        for r, s in zip(row[1:3], row[3:5]):
            assert (s == "") == (r == EMPTY) and (r == EMPTY or -1.0001 <= float(s) <= 1.0001), row
        if len(picks) == 2:
            assert float(row[3]) >= float(row[4]), row
    assert sorted(set(sizes)) == [1, 2, 3]
    # the item-path JSON names what was chosen, "empty_image" in the padded places
    listed = {}
    for B in range(3):
        paths = json.load(open(os.path.join(base["work"], "out", "batch", "item_path_json", f"r0_B{B:04}.json")))
        for b, q in enumerate(paths["query/img"]):
            listed[name(q)] = [r if r == EMPTY else name(r) for r in paths["reference/cross/imgs"][b]]
    assert listed == {row[0]: row[1:3] for row in sel}
    # metrics.csv is finite
    m = list(csv.DictReader(open(os.path.join(base["work"], base["version_dir"], "metrics.csv"))))[0]
    assert all(np.isfinite(float(m[k])) for k in ("test/loss", "test/loss_cross", "test/corr_cross", "test/psnr_cross"))


def test_the_scores_are_forward_cached_on_the_chosen_files(scene):
    from crossscore_amd.data import InputStage
    from crossscore_amd.decode import read_image_u8
    from crossscore_amd.model import CrossScoreNet

    tree, _, sd, base, cap = scene
    dev = torch.device("cuda", 0)
    net = CrossScoreNet(_config(tree))  # the run's own model section; trainer.precision 16-mixed: IEEE half operands
    net.load_state_dict(sd, strict=True)
    net.operand_dtype = "fp16"
    net = net.to(dev)
    stage = InputStage(dev, resize_short_side=56, integer_patches=True)
    assert len(cap) == 3
    for c in cap:
        qs = c["item_paths"]["query/img"]
        B = len(qs)
        q = torch.empty((B, 3, 56, 70), device=dev)
        r = torch.empty((B, 2, 3, 56, 70), device=dev)
        for b, qp in enumerate(qs):
            stage(read_image_u8(qp), q[b])
            for n in range(2):
                rp = c["item_paths"]["reference/cross/imgs"][n][b]
                if rp == EMPTY:
                    r[b, n] = stage.zero_image_value[:, None, None]
                else:
                    stage(read_image_u8(rp), r[b, n])
        tokens = net.encode_references(r.reshape(B * 2, 3, 56, 70))
        want = net.forward_cached(q, tokens.reshape(B, 2, *tokens.shape[1:]))["score_map_ref_cross"]
        torch.cuda.synchronize()
        assert np.array_equal(want.cpu().numpy(), c["score"]), c["batch_idx"]


@pytest.mark.parametrize("fused,decoder,depth,gt", [("auto", "host", 3, "files"), (False, "gpu", 3, "compute"), (False, "host", 1, "files"),
                                                    ("auto", "gpu", 1, "compute")])
def test_the_run_does_not_depend_on_how_it_is_fed(scene, fused, decoder, depth, gt):
    """one-pass and two-launch input stage, device and host decoder, one and three batches in flight, ground truth from files and computed: the
    same bytes in every file, the CSVs included"""
    tree, root, sd, base, _ = scene
    res, _ = _run(tree, root, f"v_{fused}_{decoder}_{depth}_{gt}", sd, f"this_main.fused_input_stage={fused}", f"this_main.png_decoder={decoder}",
                  f"this_main.batches_in_flight={depth}", f"this_main.gt_metric_maps={gt}")
    assert res["input_stage"].startswith("one-pass" if fused == "auto" else "two-launch") and res["gt_metric_maps"] == gt
    if decoder == "gpu":
        assert res["png_decoded"]["png_decoded_gpu"] > 0 and res["png_decoded"]["png_decoded_host"] == 0
    a, b = tree_bytes(base["work"]), tree_bytes(res["work"])
    assert sorted(a) == sorted(b) and len(a) > 8
    assert os.path.join("out", "reference_selection.csv") in a and any(k.endswith("metrics.csv") for k in a) and os.path.join("out", "test_batches.csv") in a
    for rel in a:
        if gt == "compute" and rel.startswith(os.path.join("out", "batch", "item_path_json")):
            # the one field that names an INPUT of the ground truth: the metric-map file with files, "empty_image" with compute (nvs.NvsItems,
            # compute_gt); every other field, the chosen references among them, is the same
            ja, jb = json.loads(a[rel]), json.loads(b[rel])
            assert all(p != EMPTY for p in ja.pop("query/score_map")) and all(p == EMPTY for p in jb.pop("query/score_map"))
            assert ja == jb, rel
            continue
        assert a[rel] == b[rel], rel


def test_a_second_processed_size_names_the_remedy(scene, tmp_path):
    """one bank has one patch grid: scene_c's 540 x 720 images beside scene_a's 60 x 84 without a resize"""
    tree, _, sd, _, _ = scene
    with open(os.path.join(tree, "res_540", "split.json")) as f:
        splits = json.load(f)
    mixed = str(tmp_path / "nvs" / "tree")
    shutil.copytree(tree, mixed)
    with open(os.path.join(mixed, "res_540", "split.json"), "w") as f:
        json.dump(dict(splits, test=["scene_b", "scene_c"]), f)
    with pytest.raises(ValueError, match="crop_mode=dataset_default"):
        _run(mixed, tmp_path, "mixed", sd, "this_main.resize_short_side=-1", "data.loader.validation.batch_size=2",
             "data.loader.validation.shuffle=False", "this_main.fused_input_stage=False")
