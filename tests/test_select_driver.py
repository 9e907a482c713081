"""predict with data.neighbour_config.strategy=similar: a synthetic scene of 6 queries and 7 references, three of the
references byte copies of queries under other names.  A copy is bit-identical to its query, so it is that query's first reference whatever
the weights are; everything else is compared between runs."""
import csv
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from crossscore_amd import data as csdata  # noqa: E402
from nets import SMALL, TINY, state_dict_for  # noqa: E402
from scenes import COPIES, make_scene_with_copies, run_predict_similar, tree_bytes  # noqa: E402

pytestmark = pytest.mark.gpu


def _selection(out_dir):
    with open(os.path.join(out_dir, "reference_selection.csv")) as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["query", "reference_0", "reference_1", "similarity_0", "similarity_1"]
    return rows[1:]


def test_a_copied_query_takes_its_copy_first(tmp_path):
    qd, rd = make_scene_with_copies(str(tmp_path / "data"))
    sd = state_dict_for(TINY, 6)
    res = run_predict_similar(str(tmp_path / "out"), qd, rd, TINY, sd, "model.need_attn_weights=True", "logger.predict.write.flag.attn_weights=True")
    out = res["out_dir"]
    assert res["reference_strategy"] == "similar" and len(res["rows"]) == 6
    assert os.path.join(out, "reference_selection.csv") in res["files"]
    sel = _selection(out)
    assert [r[0] for r in sel] == [f"frame_{i:05}.png" for i in range(6)]
    for i, name in COPIES.items():
        assert sel[i][1] == name and abs(float(sel[i][3]) - 1.0) < 1e-4, sel[i]
    names = set(os.listdir(rd))
    for r in sel:
        assert r[1] in names and r[2] in names and r[1] != r[2] and float(r[3]) >= float(r[4])
    # the item-path JSON, the reference images and the attention images name what was chosen
    for B in range(3):
        paths = json.load(open(os.path.join(out, "batch", "item_path_json", f"r0_B{B:04}.json")))
        for b in range(2):
            i = 2 * B + b
            assert paths["query/img"][b].endswith(f"frame_{i:05}.png")
            assert [os.path.basename(p) for p in paths["reference/cross/imgs"][b]] == sel[i][1:3]
            stem = f"r0_B{B:04}_b{b:03}_s00001_test_ours_1000_renders_frame_{i:05}"
            refs = sorted(os.listdir(os.path.join(out, "batch", "image_reference", stem, "cross")))
            assert len(refs) == 2 and all(os.path.splitext(n)[0] in refs[k] for k, n in enumerate(sel[i][1:3]))
            att = sorted(os.listdir(os.path.join(out, "batch", "attn_weights", stem, "cross")))
            assert len(att) == 2 and all(os.path.splitext(n)[0] in att[k] for k, n in enumerate(sel[i][1:3]))
    # a copied query's reference image 0 is its own processed image
    from PIL import Image
    stem = "r0_B0000_b001_s00001_test_ours_1000_renders_frame_00001"
    ref0 = sorted(os.listdir(os.path.join(out, "batch", "image_reference", stem, "cross")))[0]
    assert np.array_equal(np.array(Image.open(os.path.join(out, "batch", "image_reference", stem, "cross", ref0))),
                          np.array(Image.open(os.path.join(out, "batch", "image_query", stem + ".png"))))


def test_a_query_never_lists_itself_when_the_directories_coincide(tmp_path):
    qd, _ = make_scene_with_copies(str(tmp_path / "data"))
    sd = state_dict_for(TINY, 6)
    res = run_predict_similar(str(tmp_path / "out"), qd, qd, TINY, sd)
    sel = _selection(res["out_dir"])
    assert len(sel) == 6
    for r in sel:
        assert r[0] not in r[1:3], r
    # without the exclusion every query is its own best match
    free = run_predict_similar(str(tmp_path / "out_free"), qd, qd, TINY, sd, "this_main.similar_exclude_self=False")
    for r in _selection(free["out_dir"]):
        assert r[1] == r[0] and abs(float(r[3]) - 1.0) < 1e-4, r


@pytest.fixture(scope="module")
def small_scene(tmp_path_factory):
    root = tmp_path_factory.mktemp("select_small")
    qd, rd = make_scene_with_copies(str(root / "data"))
    sd = state_dict_for(SMALL, 6)
    no_imgs = ["logger.predict.write.flag.image_query=False", "logger.predict.write.flag.image_reference=False"]
    base = run_predict_similar(str(root / "base"), qd, rd, SMALL, sd, *no_imgs, "this_main.fused_input_stage=False", "this_main.png_decoder=host", "this_main.batches_in_flight=3")
    return root, qd, rd, sd, no_imgs, base


@pytest.mark.parametrize("fused,decoder,depth", [("auto", "host", 3), (False, "gpu", 3), (False, "host", 1), ("auto", "gpu", 1)])
def test_the_run_does_not_depend_on_how_the_tokens_are_made(small_scene, fused, decoder, depth):
    """one-pass and two-launch input stage, device and host PNG decoder, one and three batches in flight: the same bytes in every file"""
    root, qd, rd, sd, no_imgs, base = small_scene
    assert base["input_stage"].startswith("two-launch")
    res = run_predict_similar(str(root / f"v_{fused}_{decoder}_{depth}"), qd, rd, SMALL, sd, *no_imgs, f"this_main.fused_input_stage={fused}",
                              f"this_main.png_decoder={decoder}", f"this_main.batches_in_flight={depth}")
    assert res["input_stage"].startswith("one-pass" if fused == "auto" else "two-launch")
    if decoder == "gpu":
        assert res["png_decoded"]["png_decoded_gpu"] == 6 + 7 and res["png_decoded"]["png_decoded_host"] == 0
    a, b = tree_bytes(base["out_dir"]), tree_bytes(res["out_dir"])
    assert sorted(a) == sorted(b) and len(a) > 8
    for rel in a:
        assert a[rel] == b[rel], rel


def test_the_scores_are_forward_cached_on_the_listed_references(small_scene, monkeypatch):
    """a second run with the reference's own strategy, its sampler replaced by the lists the first run chose: the cached path (forward_cached on
    those references) writes the same score CSV and the same score maps"""
    root, qd, rd, sd, no_imgs, base = small_scene
    sel = _selection(base["out_dir"])
    lists = [[os.path.join(rd, n) for n in r[1:3]] for r in sel]
    calls = iter(lists)
    monkeypatch.setattr(csdata, "sample_references", lambda ref_list, n_sample, deterministic, rng=None: list(next(calls)))
    res = run_predict_similar(str(root / "listed"), qd, rd, SMALL, sd, *no_imgs, "data.neighbour_config.strategy=random", "this_main.fused_input_stage=False")
    assert res["reference_strategy"] == "random" and not os.path.exists(os.path.join(res["out_dir"], "reference_selection.csv"))
    a, b = tree_bytes(base["out_dir"]), tree_bytes(res["out_dir"])
    shared = [rel for rel in a if rel.startswith(("score_summary", os.path.join("batch", "score_map_ref_cross"), os.path.join("batch", "item_path_json")))]
    assert len(shared) >= 1 + 6 + 3
    for rel in shared:
        assert a[rel] == b[rel], rel
    assert base["rows"] == res["rows"]
