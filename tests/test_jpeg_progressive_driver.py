"""this_main.jpeg_progressive through the drivers: with this_main.jpeg_decoder=gpu, predict and evaluate compute the same thing, bit for bit,
whether the progressive JPEG inputs are decoded by PIL (host) or on the device (gpu) -- the same output files byte for byte, the same CSV rows,
the same ground-truth tensors -- and no JPEG is left to the host in the gpu run.  summarise_gt --jpeg_progressive writes the same CSV."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from nvs_tree import make_tree  # noqa: E402
from jpeg_files import content, jpeg_bytes  # noqa: E402
from nets import SMALL, TINY, state_dict_for  # noqa: E402
from scenes import make_scene, tree_bytes  # noqa: E402

torch = pytest.importorskip("torch")
GPU = ["this_main.jpeg_decoder=gpu", "this_main.jpeg_progressive=gpu"]
NONE = {"jpeg_progressive_gpu": 0, "jpeg_progressive_host": 0}


@pytest.fixture(autouse=True)
def _in_tmp(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)  # evaluate's log/<now>/... directories land here


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """5 PNG queries and 4 JPEG references of 70 x 90 (-> 56 x 72), half of them progressive: 4:2:0 baseline, 4:4:4 progressive with restart
    markers, 4:2:2 baseline under a .png name, 4:2:0 progressive"""
    qd, rd = make_scene(str(tmp_path_factory.mktemp("scene")), n_query=5, n_ref=4, h=70, w=90)
    for f in os.listdir(rd):
        os.remove(os.path.join(rd, f))
    refs = {"ref_0.jpg": jpeg_bytes(content("mix", 70, 90, seed=11), 2, quality=90),
            "ref_1.JPG": jpeg_bytes(content("mix", 70, 90, seed=12), 0, quality=95, progressive=True, restart_marker_blocks=4),
            "ref_2.png": jpeg_bytes(content("smooth", 70, 90, seed=13), 1, quality=80), "ref_3.jpg": jpeg_bytes(content("mix", 70, 90, seed=14), 2, progressive=True)}
    for name, data in refs.items():
        with open(os.path.join(rd, name), "wb") as f:
            f.write(data)
    return qd, rd


def _common(qd, rd, back, cache=True, fused="auto"):
    return [f"data.dataset.query_dir={qd}", f"data.dataset.reference_dir={rd}", f"model.backbone.from_pretrained={back}", "this_main.resize_short_side=56",
            "data.neighbour_config.cross=3", "data.neighbour_config.deterministic=False", "data.loader.validation.batch_size=2",
            f"this_main.cache_reference_tokens={cache}", f"this_main.fused_input_stage={fused}"]


@pytest.mark.gpu
@pytest.mark.parametrize("cache,fused", [(True, "auto"), (False, "auto"), (True, False)])
def test_predict_is_the_same_with_progressive_files_on_the_device(tmp_path, scene, cache, fused):
    from crossscore_amd.config import load_config
    from crossscore_amd.predict import predict

    qd, rd = scene
    sd = state_dict_for(SMALL, 5)
    common = _common(qd, rd, SMALL, cache, fused)
    runs = {}
    for name, extra in (("host", []), ("jpeg", ["this_main.jpeg_decoder=gpu"]), ("gpu", GPU)):
        with torch.no_grad():
            runs[name] = predict(load_config("default_predict", common + extra + [f"logger.predict.out_dir={tmp_path}/out_{name}"]), state_dict=sd, now="T")
    host = tree_bytes(runs["host"]["out_dir"])
    assert len(host) > 5 and any(k.endswith(".png") for k in host) and any(k.endswith(".csv") for k in host)
    for name in ("jpeg", "gpu"):
        got = tree_bytes(runs[name]["out_dir"])
        assert sorted(got) == sorted(host), name
        for rel in host:
            assert got[rel] == host[rel], (name, rel)  # score-map PNGs, processed images, CSVs: byte for byte
        assert runs[name]["rows"] == runs["host"]["rows"], name
    st, pr = runs["gpu"]["jpeg_decoded"], runs["gpu"]["jpeg_progressive_decoded"]
    assert runs["gpu"]["jpeg_progressive"] == "gpu" and st["jpeg_decoded_host"] == 0 and st["jpeg_decoded_gpu"] >= 4, st
    assert pr["jpeg_progressive_host"] == 0 and pr["jpeg_progressive_gpu"] >= 2, pr
    if cache:  # every reference goes through the decoder once
        assert st["jpeg_decoded_gpu"] == 4 and pr["jpeg_progressive_gpu"] == 2
    # without the new key the counters are what they were: the progressive references are the host's
    st = runs["jpeg"]["jpeg_decoded"]
    assert runs["jpeg"]["jpeg_progressive"] == "host" and runs["jpeg"]["jpeg_progressive_decoded"] == NONE
    assert st["jpeg_decoded_gpu"] >= 2 and st["jpeg_decoded_host"] >= 2, st
    assert runs["host"]["jpeg_progressive"] == "host" and runs["host"]["jpeg_progressive_decoded"] == NONE
    assert runs["host"]["jpeg_decoded"] == {"jpeg_decoded_gpu": 0, "jpeg_decoded_host": 0}


@pytest.mark.gpu
def test_the_new_key_alone_raises(tmp_path, scene):
    from crossscore_amd.config import load_config
    from crossscore_amd.predict import predict

    qd, rd = scene
    sd = state_dict_for(TINY, 5)
    for extra in (["this_main.jpeg_progressive=gpu"], ["this_main.jpeg_decoder=gpu", "this_main.jpeg_progressive=pil"]):
        with pytest.raises(ValueError, match="jpeg_progressive"):
            predict(load_config("default_predict", _common(qd, rd, TINY) + extra + [f"logger.predict.out_dir={tmp_path}/x"]), state_dict=sd, now="T")


def _jpeg_gt(tree):
    """every gt/ file of the tree as JPEG bytes (under its .png name), every other one progressive"""
    from PIL import Image

    n = 0
    for d, dirs, fs in os.walk(tree):
        # the file system's directory order must not decide which file gets which options: PIL cannot write the two 720 x 540 noise frames as a
        # progressive file at 4:4:4, or at 4:2:2 with restart markers (its whole-file buffer of width x height bytes is too small: "Suspension not
        # allowed here").  In sorted order they get 4:2:2 progressive and 4:2:0 baseline with restart markers
        dirs.sort()
        if os.path.basename(d) != "gt":
            continue
        for f in sorted(fs):
            p = os.path.join(d, f)
            img = np.array(Image.open(p))
            with open(p, "wb") as out:
                # restart_marker_blocks, not _rows: with rows libjpeg writes a DRI before every scan of a progressive file, which the probe leaves to PIL
                out.write(jpeg_bytes(img, (2, 0, 1)[n % 3], quality=90, progressive=bool(n % 2), **(dict(restart_marker_blocks=3) if n % 4 > 1 else {})))
            n += 1
    return n


@pytest.mark.gpu
def test_evaluate_is_the_same_with_progressive_files_on_the_device(tmp_path, tmp_path_factory):
    from crossscore_amd.config import load_config
    from crossscore_amd.evaluate import evaluate

    tree = make_tree(tmp_path_factory.mktemp("nvs"))
    assert _jpeg_gt(tree) > 4
    sd = state_dict_for(TINY, 7)
    common = [f"data.dataset.path={tree}", f"model.backbone.from_pretrained={TINY}", "this_main.resize_short_side=56",
              "data.dataset.num_gaussians_iters=2", "data.loader.validation.batch_size=4", "data.loader.validation.num_workers=2",
              "data.neighbour_config.deterministic=True", "logger.test.write.flag.score_map_gt=True", "this_main.gt_metric_maps=compute"]
    runs, caps = {}, {}
    for name, extra in (("host", []), ("gpu", GPU)):
        np.random.seed(0)
        caps[name] = []
        with torch.no_grad():
            runs[name] = evaluate(load_config("default_test", common + extra + [f"logger.test.out_dir={tmp_path}/out_{name}"]),
                                  state_dict=sd, now=f"NOW_{name}", capture=caps[name])
    host, got = tree_bytes(runs["host"]["out_dir"]), tree_bytes(runs["gpu"]["out_dir"])
    assert "test_batches.csv" in host and sorted(got) == sorted(host)
    for rel in host:
        assert got[rel] == host[rel], rel
    assert open(os.path.join(runs["gpu"]["version_dir"], "metrics.csv"), "rb").read() == open(os.path.join(runs["host"]["version_dir"], "metrics.csv"), "rb").read()
    assert repr(runs["gpu"]["metrics"]) == repr(runs["host"]["metrics"])
    assert len(caps["gpu"]) == len(caps["host"]) > 0
    for a, b in zip(caps["host"], caps["gpu"]):
        assert a["item_paths"] == b["item_paths"]
        assert np.array_equal(a["gt"], b["gt"], equal_nan=True) and np.array_equal(a["score"], b["score"]) and np.array_equal(a["stats"], b["stats"], equal_nan=True)
    assert runs["gpu"]["jpeg_decoded"]["jpeg_decoded_host"] == 0 and runs["gpu"]["jpeg_decoded"]["jpeg_decoded_gpu"] > 4
    assert runs["gpu"]["jpeg_progressive_decoded"]["jpeg_progressive_gpu"] >= 2 and runs["gpu"]["jpeg_progressive_decoded"]["jpeg_progressive_host"] == 0
    assert runs["host"]["jpeg_progressive_decoded"] == NONE


@pytest.mark.gpu
def test_summarise_gt_writes_the_same_csv(tmp_path, tmp_path_factory):
    from crossscore_amd import summarise_gt as sg

    root = str(tmp_path_factory.mktemp("gtsum"))
    path = make_tree(os.path.join(root, "gaussian", "mfr"))
    assert _jpeg_gt(path) > 4
    dir_in = os.path.join(path, "res_540")
    assert sg.main(["--dir_in", dir_in, "--dir_out", str(tmp_path / "host"), "-n", "2", "--source", "compute"]) == 0
    assert sg.main(["--dir_in", dir_in, "--dir_out", str(tmp_path / "gpu"), "-n", "2", "--source", "compute", "--jpeg_decoder", "gpu", "--jpeg_progressive", "gpu"]) == 0
    want = open(tmp_path / "host" / "mfr" / "gaussian.csv", "rb").read()
    assert want.count(b"\n") > 4 and open(tmp_path / "gpu" / "mfr" / "gaussian.csv", "rb").read() == want
    with pytest.raises(ValueError, match="jpeg_decoder=gpu"):
        sg.summarise(dir_in, tmp_path / "x", num_workers=2, source="compute", jpeg_progressive="gpu")
