"""this_main.png_encoder through the drivers: predict and evaluate write the same tree of files with the host (PIL) and the gpu
(cs_op_png_encode) encoder -- the same relative paths, every PNG valid and decoding to identical pixels, the CSVs identical byte for byte;
the host run's files are byte-identical to a run that does not name the key."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from nvs_tree import make_tree  # noqa: E402
from png_files import parse_chunks  # noqa: E402
from scenes import make_scene  # noqa: E402
from nets import TINY  # noqa: E402

torch = pytest.importorskip("torch")

GPU_DIRS = ("score_map_", "image_query", "image_reference")  # outputs the gpu encoder takes; attention images and JSON stay on the host


@pytest.fixture(autouse=True)
def _in_tmp(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)  # evaluate's log/<now>/... directories land here


def _rel_files(res):
    out = res["out_dir"]
    rel = sorted(os.path.relpath(f, out) for f in res["files"] if os.path.abspath(f).startswith(os.path.abspath(out) + os.sep))
    on_disk = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    assert set(rel) <= set(on_disk)
    return on_disk


def _is_gpu_png(rel):
    parts = rel.split(os.sep)
    return rel.endswith(".png") and parts[0] == "batch" and parts[1].startswith(GPU_DIRS)


def _compare_runs(host, gpu, plain):
    """host / gpu / plain: result dicts of the three runs (plain = the key not given)."""
    from PIL import Image

    fh, fg, fp = _rel_files(host), _rel_files(gpu), _rel_files(plain)
    assert fh == fg == fp and len(fh) > 5
    n_gpu = 0
    for rel in fh:
        a, b, c = (open(os.path.join(r["out_dir"], rel), "rb").read() for r in (host, gpu, plain))
        assert a == c, rel  # the default path writes exactly the files it wrote before the key existed
        if rel.endswith(".png"):
            parse_chunks(b)
            ia, ib = Image.open(os.path.join(host["out_dir"], rel)), Image.open(os.path.join(gpu["out_dir"], rel))
            assert ia.mode == ib.mode and ia.size == ib.size, rel
            assert np.array_equal(np.array(ia), np.array(ib)), rel
            if _is_gpu_png(rel):
                n_gpu += 1
                assert a != b, rel  # really another encoder
            else:
                assert a == b, rel
        else:
            assert a == b, rel  # CSVs, JSON: byte for byte
    assert n_gpu > 0
    assert host["png_encoder"] == plain["png_encoder"] == "host" and gpu["png_encoder"] == "gpu"
    assert gpu["png_files"]["png_gpu_files"] == n_gpu
    assert host["png_files"]["png_gpu_files"] == 0 and plain["png_files"]["png_gpu_files"] == 0
    n_png = sum(rel.endswith(".png") for rel in fh)
    assert host["png_files"]["png_host_files"] == n_png and gpu["png_files"]["png_host_files"] == n_png - n_gpu
    return n_gpu


@pytest.mark.gpu
@pytest.mark.parametrize("colour_mode", ["rgb", "gray"])
def test_predict_writes_the_same_tree_with_either_encoder(tmp_path, colour_mode):
    """The reference's default write flags (score maps, processed query and reference images), plus attention images and the item-path
    JSON, which keep the host path."""
    from crossscore_amd import synth
    from crossscore_amd.config import load_config, model_config
    from crossscore_amd.model import CrossScoreNet
    from crossscore_amd.predict import predict

    qd, rd = make_scene(str(tmp_path / "data"), n_query=5, n_ref=4)
    arch = CrossScoreNet(model_config(**{"backbone.from_pretrained": TINY})).arch
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(arch, 5).items()}
    common = [f"data.dataset.query_dir={qd}", f"data.dataset.reference_dir={rd}", f"model.backbone.from_pretrained={TINY}",
              "this_main.resize_short_side=56", "data.neighbour_config.cross=3", "data.neighbour_config.deterministic=True",
              "data.loader.validation.batch_size=2", f"logger.predict.write.config.score_map_colour_mode={colour_mode}",
              "logger.predict.write.flag.item_path_json=True", "model.need_attn_weights=True", "logger.predict.write.flag.attn_weights=True"]
    runs = {}
    for name, extra in (("host", ["this_main.png_encoder=host"]), ("gpu", ["this_main.png_encoder=gpu"]), ("plain", [])):
        np.random.seed(0)
        with torch.no_grad():
            runs[name] = predict(load_config("default_predict", common + extra + [f"logger.predict.out_dir={tmp_path}/out_{name}"]), state_dict=sd, now="T")
    n_gpu = _compare_runs(runs["host"], runs["gpu"], runs["plain"])
    assert n_gpu == 5 + 5 + 5 * 3  # score maps, query images, reference images
    assert [r for r in runs["host"]["rows"]] == [r for r in runs["gpu"]["rows"]]
    with pytest.raises(ValueError):
        predict(load_config("default_predict", common + ["this_main.png_encoder=zip", f"logger.predict.out_dir={tmp_path}/out_x"]), state_dict=sd, now="T")


@pytest.mark.gpu
@pytest.mark.parametrize("colour_mode", ["rgb", "gray"])
def test_evaluate_writes_the_same_tree_with_either_encoder(tmp_path, tmp_path_factory, colour_mode):
    """The test phase with score_map_gt on: prediction and ground-truth maps, processed images."""
    from crossscore_amd import synth
    from crossscore_amd.config import load_config, model_config
    from crossscore_amd.evaluate import evaluate
    from crossscore_amd.model import CrossScoreNet

    tree = make_tree(tmp_path_factory.mktemp("nvs"))
    arch = CrossScoreNet(model_config(**{"backbone.from_pretrained": TINY})).arch
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(arch, 7).items()}
    common = [f"data.dataset.path={tree}", f"model.backbone.from_pretrained={TINY}", "this_main.resize_short_side=56",
              "data.dataset.num_gaussians_iters=2", "data.loader.validation.batch_size=4", "data.loader.validation.num_workers=2",
              "data.neighbour_config.deterministic=True", "logger.test.write.flag.score_map_gt=True",
              f"logger.test.write.config.score_map_colour_mode={colour_mode}"]
    runs = {}
    for name, extra in (("host", ["this_main.png_encoder=host"]), ("gpu", ["this_main.png_encoder=gpu"]), ("plain", [])):
        np.random.seed(0)
        with torch.no_grad():
            runs[name] = evaluate(load_config("default_test", common + extra + [f"logger.test.out_dir={tmp_path}/out_{name}"]), state_dict=sd, now=f"NOW_{name}")
    n_gpu = _compare_runs(runs["host"], runs["gpu"], runs["plain"])
    gt = [f for f in _rel_files(runs["gpu"]) if f.startswith(os.path.join("batch", "score_map_gt"))]
    assert len(gt) == 12 and n_gpu >= 24  # 12 items: prediction + GT maps, plus whatever processed images the default flags write
    assert repr(runs["host"]["metrics"]) == repr(runs["gpu"]["metrics"]) == repr(runs["plain"]["metrics"])
