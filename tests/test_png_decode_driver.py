"""this_main.png_decoder through the drivers: predict and evaluate compute the same thing, bit for bit, whether the PNG inputs are decoded by PIL
on the loader's threads (host) or on the device (gpu: decode.ImageDecoder behind a window of upcoming files) -- the same files byte for byte, the same
CSV rows, the same ground-truth tensors."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from nets import SMALL, TINY, state_dict_for  # noqa: E402
from nvs_tree import make_tree  # noqa: E402
from png_files import image_of, interlaced_png, pil_png  # noqa: E402
from scenes import make_scene, tree_bytes  # noqa: E402

torch = pytest.importorskip("torch")


@pytest.fixture(autouse=True)
def _in_tmp(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)  # evaluate's log/<now>/... directories land here


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """5 queries, 4 references of 70 x 90 (-> 56 x 72: the one-launch patch embedding takes even widths); query 1 is an RGBA file (alpha dropped on the device), query 2 an interlaced one (the host fallback inside
    a gpu run)."""
    qd, rd = make_scene(str(tmp_path_factory.mktemp("scene")), n_query=5, n_ref=4, h=70, w=90)
    rng = np.random.default_rng(3)
    with open(os.path.join(qd, "frame_00001.png"), "wb") as f:
        f.write(pil_png(image_of(rng, 70, 90, "rgba")))
    with open(os.path.join(qd, "frame_00002.png"), "wb") as f:
        f.write(interlaced_png(image_of(rng, 70, 90, "rgb")))
    return qd, rd


@pytest.mark.gpu
@pytest.mark.parametrize("cache", [True, False])
@pytest.mark.parametrize("one_pass", [True, False])
def test_predict_is_the_same_with_either_decoder(tmp_path, scene, cache, one_pass):
    from crossscore_amd.config import load_config
    from crossscore_amd.predict import predict

    qd, rd = scene
    sd = state_dict_for(SMALL, 5)
    common = [f"data.dataset.query_dir={qd}", f"data.dataset.reference_dir={rd}", f"model.backbone.from_pretrained={SMALL}",
              "this_main.resize_short_side=56", "data.neighbour_config.cross=3", "data.neighbour_config.deterministic=False",
              "data.loader.validation.batch_size=2", f"this_main.cache_reference_tokens={cache}", f"this_main.fused_input_stage={one_pass}"]
    if one_pass:  # the one-pass input stage writes no processed image
        common += ["logger.predict.write.flag.image_query=False", "logger.predict.write.flag.image_reference=False"]
    runs = {}
    # a window smaller than one batch (2 queries + their references), the default, and one larger than the whole run
    for name, extra in (("host", ["this_main.png_decoder=host"]), ("plain", []), ("gpu1", ["this_main.png_decoder=gpu", "this_main.png_decode_window=1"]),
                        ("gpu", ["this_main.png_decoder=gpu"]), ("gpu1000", ["this_main.png_decoder=gpu", "this_main.png_decode_window=1000"])):
        with torch.no_grad():
            runs[name] = predict(load_config("default_predict", common + extra + [f"logger.predict.out_dir={tmp_path}/out_{name}"]), state_dict=sd, now="T")
    host = tree_bytes(runs["host"]["out_dir"])
    assert len(host) > 5 and any(k.endswith(".png") for k in host) and any(k.endswith(".csv") for k in host)
    for name in ("plain", "gpu1", "gpu", "gpu1000"):
        got = tree_bytes(runs[name]["out_dir"])
        assert sorted(got) == sorted(host), name
        for rel in host:
            assert got[rel] == host[rel], (name, rel)  # score-map PNGs, processed images, CSVs: byte for byte
        assert runs[name]["rows"] == runs["host"]["rows"], name
        assert runs[name]["input_stage"] == runs["host"]["input_stage"]
    assert runs["host"]["input_stage"].startswith("one-pass" if one_pass else "two-launch")
    assert runs["host"]["png_decoder"] == runs["plain"]["png_decoder"] == "host" and runs["gpu"]["png_decoder"] == "gpu"
    assert runs["host"]["png_decoded"] == {"png_decoded_gpu": 0, "png_decoded_host": 0}
    for name in ("gpu1", "gpu", "gpu1000"):
        st = runs[name]["png_decoded"]
        assert st["png_decoded_host"] == 1 and st["png_decoded_gpu"] >= 4 + 3, (name, st)  # the interlaced query; the other queries and references
    if cache:  # every file goes through the decoder once
        assert runs["gpu1000"]["png_decoded"]["png_decoded_gpu"] <= 4 + 4


@pytest.mark.gpu
def test_predict_rejects_an_unknown_decoder_and_a_damaged_file(tmp_path, scene):
    from crossscore_amd.config import load_config
    from crossscore_amd.predict import predict

    qd, rd = scene
    sd = state_dict_for(TINY, 5)
    common = [f"data.dataset.query_dir={qd}", f"data.dataset.reference_dir={rd}", f"model.backbone.from_pretrained={TINY}",
              "this_main.resize_short_side=56", "data.neighbour_config.cross=3", "data.loader.validation.batch_size=2"]
    with pytest.raises(ValueError, match="png_decoder"):
        predict(load_config("default_predict", common + ["this_main.png_decoder=pil", f"logger.predict.out_dir={tmp_path}/x"]), state_dict=sd, now="T")
    with pytest.raises(ValueError, match="png_decode_window"):
        predict(load_config("default_predict", common + ["this_main.png_decoder=gpu", "this_main.png_decode_window=0", f"logger.predict.out_dir={tmp_path}/y"]),
                state_dict=sd, now="T")
    # a query whose IDAT payload is damaged: the run stops with the file's name
    bad_q = tmp_path / "queries"
    bad_q.mkdir()
    for f in sorted(os.listdir(qd)):
        data = bytearray(open(os.path.join(qd, f), "rb").read())
        if f == "frame_00003.png":
            data[70] ^= 0x20
        (bad_q / f).write_bytes(bytes(data))
    with pytest.raises(ValueError, match="frame_00003.png"), torch.no_grad():
        predict(load_config("default_predict", common + [f"data.dataset.query_dir={bad_q}", "this_main.png_decoder=gpu", f"logger.predict.out_dir={tmp_path}/z"]),
                state_dict=sd, now="T")


@pytest.mark.gpu
@pytest.mark.parametrize("gt_metric_maps", ["files", "compute"])
def test_evaluate_is_the_same_with_either_decoder(tmp_path, tmp_path_factory, gt_metric_maps):
    """files: the 16-bit metric maps are decoded on the device; compute: the captured images are."""
    from crossscore_amd.config import load_config
    from crossscore_amd.evaluate import evaluate

    tree = make_tree(tmp_path_factory.mktemp("nvs"))
    sd = state_dict_for(TINY, 7)
    common = [f"data.dataset.path={tree}", f"model.backbone.from_pretrained={TINY}", "this_main.resize_short_side=56",
              "data.dataset.num_gaussians_iters=2", "data.loader.validation.batch_size=4", "data.loader.validation.num_workers=2",
              "data.neighbour_config.deterministic=True", "logger.test.write.flag.score_map_gt=True", f"this_main.gt_metric_maps={gt_metric_maps}"]
    runs, caps = {}, {}
    for name, extra in (("host", ["this_main.png_decoder=host"]), ("gpu", ["this_main.png_decoder=gpu"]),
                        ("gpu3", ["this_main.png_decoder=gpu", "this_main.png_decode_window=3"])):
        np.random.seed(0)
        caps[name] = []
        with torch.no_grad():
            runs[name] = evaluate(load_config("default_test", common + extra + [f"logger.test.out_dir={tmp_path}/out_{name}"]), state_dict=sd, now=f"NOW_{name}",
                                  capture=caps[name])
    host = tree_bytes(runs["host"]["out_dir"])
    assert "test_batches.csv" in host and any(k.endswith(".png") for k in host)
    metrics = open(os.path.join(runs["host"]["version_dir"], "metrics.csv"), "rb").read()
    for name in ("gpu", "gpu3"):
        got = tree_bytes(runs[name]["out_dir"])
        assert sorted(got) == sorted(host)
        for rel in host:
            assert got[rel] == host[rel], (name, rel)
        assert open(os.path.join(runs[name]["version_dir"], "metrics.csv"), "rb").read() == metrics
        assert repr(runs[name]["metrics"]) == repr(runs["host"]["metrics"])
        assert len(caps[name]) == len(caps["host"]) > 0
        for a, b in zip(caps["host"], caps[name]):
            assert a["item_paths"] == b["item_paths"]
            assert np.array_equal(a["gt"], b["gt"], equal_nan=True) and np.array_equal(a["score"], b["score"]) and np.array_equal(a["stats"], b["stats"], equal_nan=True)
        assert runs[name]["png_decoder"] == "gpu" and runs[name]["png_decoded"]["png_decoded_gpu"] > 12 and runs[name]["png_decoded"]["png_decoded_host"] == 0
    assert runs["host"]["png_decoder"] == "host" and runs["host"]["gt_metric_maps"] == gt_metric_maps
