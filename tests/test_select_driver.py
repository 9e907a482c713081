"""predict with data.neighbour_config.strategy=similar: a synthetic scene of 6 queries and 7 references, three of the
references byte copies of queries under other names.  A copy is bit-identical to its query, so it is that query's first reference whatever
the weights are; everything else is compared between runs."""
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
from crossscore_amd import data as csdata  # noqa: E402
from crossscore_amd import synth  # noqa: E402
from crossscore_amd.config import load_config, model_config  # noqa: E402

pytestmark = pytest.mark.gpu

TINY = "synthetic/dinov2-tiny"
SMALL = "synthetic/dinov2-small-2l"  # the ViT-S width: what the one-pass input stage takes
COPIES = {1: "copy_b.png", 3: "copy_a.png", 4: "zz_copy.png"}  # query index -> its copy's name in reference_dir (before, between and behind the others)


def _make_scene(root, n_query=6, n_other=4, h=70, w=90, seed=7):
    from PIL import Image

    rng = np.random.Generator(np.random.PCG64(seed))
    base = os.path.join(root, "gaussian", "mfr", "res_540", "s00001", "test", "ours_1000")
    qd, rd = os.path.join(base, "renders"), os.path.join(base, "gt")
    os.makedirs(qd)
    os.makedirs(rd)
    yy, xx = np.mgrid[0:h, 0:w]
    for d, n, off in ((qd, n_query, 0), (rd, n_other, 100)):
        for i in range(n):
            img = np.stack([(xx * 3 + i * 17 + off) % 256, (yy * 2 + i * 29) % 256, (xx + yy + i * 11) % 256], axis=2).astype(np.uint8)
            img = (img.astype(np.int32) + rng.integers(-20, 21, size=img.shape)).clip(0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(d, f"frame_{i:05}.png"))
    for i, name in COPIES.items():
        shutil.copyfile(os.path.join(qd, f"frame_{i:05}.png"), os.path.join(rd, name))
    return qd, rd


def _weights(backbone):
    from crossscore_amd.model import CrossScoreNet

    arch = CrossScoreNet(model_config(**{"backbone.from_pretrained": backbone})).arch
    return {k: torch.from_numpy(v) for k, v in synth.make_state_dict(arch, 6).items()}


def _run(out, qd, rd, backbone, sd, *over):
    from crossscore_amd.predict import predict

    cfg = load_config("default_predict", [f"data.dataset.query_dir={qd}", f"data.dataset.reference_dir={rd}", f"model.backbone.from_pretrained={backbone}",
                                          "this_main.resize_short_side=56", "data.neighbour_config.cross=2", "data.neighbour_config.strategy=similar",
                                          "data.loader.validation.batch_size=2", f"logger.predict.out_dir={out}",
                                          "logger.predict.write.config.score_map_colour_mode=gray", "logger.predict.write.flag.item_path_json=True", *over])
    return predict(cfg, state_dict=sd, now="T")


def _selection(out_dir):
    with open(os.path.join(out_dir, "reference_selection.csv")) as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["query", "reference_0", "reference_1", "similarity_0", "similarity_1"]
    return rows[1:]


def _tree(out_dir):
    files = {}
    for d, _, fs in os.walk(out_dir):
        for f in fs:
            p = os.path.join(d, f)
            files[os.path.relpath(p, out_dir)] = open(p, "rb").read()
    return files


def test_a_copied_query_takes_its_copy_first(tmp_path):
    qd, rd = _make_scene(str(tmp_path / "data"))
    sd = _weights(TINY)
    res = _run(str(tmp_path / "out"), qd, rd, TINY, sd, "model.need_attn_weights=True", "logger.predict.write.flag.attn_weights=True")
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
    qd, _ = _make_scene(str(tmp_path / "data"))
    sd = _weights(TINY)
    res = _run(str(tmp_path / "out"), qd, qd, TINY, sd)
    sel = _selection(res["out_dir"])
    assert len(sel) == 6
    for r in sel:
        assert r[0] not in r[1:3], r
    # without the exclusion every query is its own best match
    free = _run(str(tmp_path / "out_free"), qd, qd, TINY, sd, "this_main.similar_exclude_self=False")
    for r in _selection(free["out_dir"]):
        assert r[1] == r[0] and abs(float(r[3]) - 1.0) < 1e-4, r


@pytest.fixture(scope="module")
def small_scene(tmp_path_factory):
    root = tmp_path_factory.mktemp("select_small")
    qd, rd = _make_scene(str(root / "data"))
    sd = _weights(SMALL)
    no_imgs = ["logger.predict.write.flag.image_query=False", "logger.predict.write.flag.image_reference=False"]
    base = _run(str(root / "base"), qd, rd, SMALL, sd, *no_imgs, "this_main.fused_input_stage=False", "this_main.png_decoder=host", "this_main.batches_in_flight=3")
    return root, qd, rd, sd, no_imgs, base


@pytest.mark.parametrize("fused,decoder,depth", [("auto", "host", 3), (False, "gpu", 3), (False, "host", 1), ("auto", "gpu", 1)])
def test_the_run_does_not_depend_on_how_the_tokens_are_made(small_scene, fused, decoder, depth):
    """one-pass and two-launch input stage, device and host PNG decoder, one and three batches in flight: the same bytes in every file"""
    root, qd, rd, sd, no_imgs, base = small_scene
    assert base["input_stage"].startswith("two-launch")
    res = _run(str(root / f"v_{fused}_{decoder}_{depth}"), qd, rd, SMALL, sd, *no_imgs, f"this_main.fused_input_stage={fused}",
               f"this_main.png_decoder={decoder}", f"this_main.batches_in_flight={depth}")
    assert res["input_stage"].startswith("one-pass" if fused == "auto" else "two-launch")
    if decoder == "gpu":
        assert res["png_decoded"]["png_decoded_gpu"] == 6 + 7 and res["png_decoded"]["png_decoded_host"] == 0
    a, b = _tree(base["out_dir"]), _tree(res["out_dir"])
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
    res = _run(str(root / "listed"), qd, rd, SMALL, sd, *no_imgs, "data.neighbour_config.strategy=random", "this_main.fused_input_stage=False")
    assert res["reference_strategy"] == "random" and not os.path.exists(os.path.join(res["out_dir"], "reference_selection.csv"))
    a, b = _tree(base["out_dir"]), _tree(res["out_dir"])
    shared = [rel for rel in a if rel.startswith(("score_summary", os.path.join("batch", "score_map_ref_cross"), os.path.join("batch", "item_path_json")))]
    assert len(shared) >= 1 + 6 + 3
    for rel in shared:
        assert a[rel] == b[rel], rel
    assert base["rows"] == res["rows"]
