"""this_main.jpeg_decoder through the drivers: predict and evaluate compute the same thing, bit for bit, whether the baseline JPEG inputs are decoded
by PIL on the loader's threads (host) or on the device (gpu: decode.ImageDecoder(jpeg=True) behind the window of upcoming files) -- the same output
files byte for byte, the same CSV rows, the same ground-truth tensors."""
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from nvs_tree import make_tree  # noqa: E402
from jpeg_files import content, jpeg_bytes, probe  # noqa: E402
from nets import SMALL, TINY, state_dict_for  # noqa: E402
from scenes import make_scene, tree_bytes  # noqa: E402

torch = pytest.importorskip("torch")


@pytest.fixture(autouse=True)
def _in_tmp(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)  # evaluate's log/<now>/... directories land here


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """5 PNG queries and 4 JPEG references of 70 x 90 (-> 56 x 72): 4:2:0, 4:4:4 with restart markers, 4:2:2 under a .png name, one progressive
    (the host fallback inside a gpu run)."""
    from PIL import Image

    qd, rd = make_scene(str(tmp_path_factory.mktemp("scene")), n_query=5, n_ref=4, h=70, w=90)
    for f in os.listdir(rd):
        os.remove(os.path.join(rd, f))
    buf = io.BytesIO()
    Image.fromarray(content("mix", 70, 90, seed=14)).save(buf, format="JPEG", progressive=True)
    refs = {"ref_0.jpg": jpeg_bytes(content("mix", 70, 90, seed=11), 2, quality=90), "ref_1.JPG": jpeg_bytes(content("mix", 70, 90, seed=12), 0, quality=95, restart_marker_blocks=4),
            "ref_2.png": jpeg_bytes(content("smooth", 70, 90, seed=13), 1, quality=80), "ref_3.jpg": buf.getvalue()}
    for name, data in refs.items():
        with open(os.path.join(rd, name), "wb") as f:
            f.write(data)
    return qd, rd


def _common(qd, rd, back, cache=True):
    return [f"data.dataset.query_dir={qd}", f"data.dataset.reference_dir={rd}", f"model.backbone.from_pretrained={back}", "this_main.resize_short_side=56",
            "data.neighbour_config.cross=3", "data.neighbour_config.deterministic=False", "data.loader.validation.batch_size=2",
            f"this_main.cache_reference_tokens={cache}"]


@pytest.mark.gpu
@pytest.mark.parametrize("cache", [True, False])
def test_predict_is_the_same_with_either_jpeg_decoder(tmp_path, scene, cache):
    from crossscore_amd.config import load_config
    from crossscore_amd.predict import predict

    qd, rd = scene
    sd = state_dict_for(SMALL, 5)
    common = _common(qd, rd, SMALL, cache)
    runs = {}
    for name, extra in (("host", ["this_main.jpeg_decoder=host"]), ("absent", None), ("gpu", ["this_main.jpeg_decoder=gpu"]),
                        ("both", ["this_main.jpeg_decoder=gpu", "this_main.png_decoder=gpu"]),
                        ("gpu1", ["this_main.jpeg_decoder=gpu", "this_main.png_decode_window=1"])):
        cfg = load_config("default_predict", common + (extra or []) + [f"logger.predict.out_dir={tmp_path}/out_{name}"])
        if extra is None:
            del cfg.this_main["jpeg_decoder"]  # a config file written before the key existed
        with torch.no_grad():
            runs[name] = predict(cfg, state_dict=sd, now="T")
    host = tree_bytes(runs["host"]["out_dir"])
    assert len(host) > 5 and any(k.endswith(".png") for k in host) and any(k.endswith(".csv") for k in host)
    for name in ("absent", "gpu", "both", "gpu1"):
        got = tree_bytes(runs[name]["out_dir"])
        assert sorted(got) == sorted(host), name
        for rel in host:
            assert got[rel] == host[rel], (name, rel)  # score-map PNGs, processed images, CSVs: byte for byte
        assert runs[name]["rows"] == runs["host"]["rows"], name
    for name in ("host", "absent"):
        assert runs[name]["jpeg_decoder"] == "host" and runs[name]["jpeg_decoded"] == {"jpeg_decoded_gpu": 0, "jpeg_decoded_host": 0}
        assert runs[name]["png_decoded"] == {"png_decoded_gpu": 0, "png_decoded_host": 0}
    for name in ("gpu", "both", "gpu1"):
        st = runs[name]["jpeg_decoded"]
        assert runs[name]["jpeg_decoder"] == "gpu" and st["jpeg_decoded_gpu"] > 0 and st["jpeg_decoded_host"] >= 1, (name, st)  # the progressive file
        if cache:  # every reference goes through the decoder once
            assert st["jpeg_decoded_gpu"] <= 3 and st["jpeg_decoded_host"] == 1, (name, st)
    assert runs["gpu"]["png_decoder"] == "host" and runs["gpu"]["png_decoded"] == {"png_decoded_gpu": 0, "png_decoded_host": 0}
    assert runs["both"]["png_decoder"] == "gpu" and runs["both"]["png_decoded"] == {"png_decoded_gpu": 5, "png_decoded_host": 0}


@pytest.mark.gpu
def test_predict_rejects_an_unknown_value_and_a_corrupt_jpeg(tmp_path, scene):
    from crossscore_amd.config import load_config
    from crossscore_amd.predict import predict

    qd, rd = scene
    sd = state_dict_for(TINY, 5)
    common = _common(qd, rd, TINY)
    with pytest.raises(ValueError, match="jpeg_decoder"):
        predict(load_config("default_predict", common + ["this_main.jpeg_decoder=pil", f"logger.predict.out_dir={tmp_path}/x"]), state_dict=sd, now="T")
    bad_r = tmp_path / "references"
    bad_r.mkdir()
    for f in sorted(os.listdir(rd)):
        data = open(os.path.join(rd, f), "rb").read()
        if f == "ref_0.jpg":  # the scan ends half way: the probe takes the file, the device says input exhausted
            e = probe(data)[1].entropy_offset
            data = data[:e + (len(data) - e) // 2]
        (bad_r / f).write_bytes(data)
    with pytest.raises(ValueError, match=r"ref_0\.jpg"), torch.no_grad():
        predict(load_config("default_predict", common + [f"data.dataset.reference_dir={bad_r}", "this_main.jpeg_decoder=gpu", f"logger.predict.out_dir={tmp_path}/z"]),
                state_dict=sd, now="T")


@pytest.mark.gpu
def test_evaluate_is_the_same_with_either_jpeg_decoder(tmp_path, tmp_path_factory):
    """this_main.gt_metric_maps=compute reads the captured images: every gt/ file of the tree holds JPEG bytes here (under its .png name: the
    decoder sniffs the content, as PIL does)."""
    from PIL import Image

    from crossscore_amd.config import load_config
    from crossscore_amd.evaluate import evaluate

    tree = make_tree(tmp_path_factory.mktemp("nvs"))
    n = 0
    for d, _, fs in os.walk(tree):
        if os.path.basename(d) != "gt":
            continue
        for f in sorted(fs):
            p = os.path.join(d, f)
            img = np.array(Image.open(p))
            with open(p, "wb") as out:
                out.write(jpeg_bytes(img, (2, 0, 1)[n % 3], quality=90, **(dict(restart_marker_rows=1) if n % 2 else {})))
            n += 1
    assert n > 4
    sd = state_dict_for(TINY, 7)
    common = [f"data.dataset.path={tree}", f"model.backbone.from_pretrained={TINY}", "this_main.resize_short_side=56",
              "data.dataset.num_gaussians_iters=2", "data.loader.validation.batch_size=4", "data.loader.validation.num_workers=2",
              "data.neighbour_config.deterministic=True", "logger.test.write.flag.score_map_gt=True", "this_main.gt_metric_maps=compute"]
    runs, caps = {}, {}
    for name in ("host", "gpu"):
        np.random.seed(0)
        caps[name] = []
        with torch.no_grad():
            runs[name] = evaluate(load_config("default_test", common + [f"this_main.jpeg_decoder={name}", f"logger.test.out_dir={tmp_path}/out_{name}"]),
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
    assert runs["host"]["jpeg_decoder"] == "host" and runs["host"]["jpeg_decoded"] == {"jpeg_decoded_gpu": 0, "jpeg_decoded_host": 0}
    assert runs["gpu"]["jpeg_decoder"] == "gpu" and runs["gpu"]["jpeg_decoded"]["jpeg_decoded_gpu"] > 4 and runs["gpu"]["jpeg_decoded"]["jpeg_decoded_host"] == 0
    assert runs["gpu"]["png_decoder"] == "host"
