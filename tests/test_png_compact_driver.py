"""this_main.png_compression through the drivers: predict, evaluate and metric_maps write the same tree of files with png_encoder=gpu in the
fast and the compact form -- the same relative paths, every PNG valid and decoding to identical pixels, CSVs identical byte for byte, the compact
tree smaller -- and the key changes nothing with png_encoder=host."""
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
from scenes import make_scene, tree_bytes  # noqa: E402
from nets import TINY  # noqa: E402

torch = pytest.importorskip("torch")


@pytest.fixture(autouse=True)
def _in_tmp(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)  # evaluate's log/<now>/... directories land here


def _compare_trees(fast, compact, host=None, host_compact=None):
    """{relative path: bytes} of each run -> (PNG bytes of fast, of compact)."""
    import io

    from PIL import Image

    assert sorted(fast) == sorted(compact) and len(fast) >= 2
    differ = 0
    for rel in sorted(fast):
        a, b = fast[rel], compact[rel]
        if rel.endswith(".png"):
            parse_chunks(a)
            parse_chunks(b)
            ia, ib = Image.open(io.BytesIO(a)), Image.open(io.BytesIO(b))
            assert ia.mode == ib.mode and ia.size == ib.size and np.array_equal(np.array(ia), np.array(ib)), rel
            differ += a != b
        else:
            assert a == b, rel  # CSVs, JSON: byte for byte
    assert differ > 0
    if host is not None:
        assert sorted(host) == sorted(fast)
        assert host == host_compact  # the key is ignored with png_encoder=host: every file byte for byte
    png = lambda t: sum(len(v) for k, v in t.items() if k.endswith(".png"))  # noqa: E731
    print(f"PNG bytes: fast {png(fast)}, compact {png(compact)}" + (f", host {png(host)}" if host is not None else ""))
    assert sum(map(len, compact.values())) < sum(map(len, fast.values()))
    return png(fast), png(compact)


@pytest.mark.gpu
def test_predict_fast_and_compact(tmp_path):
    from crossscore_amd import synth
    from crossscore_amd.config import load_config, model_config
    from crossscore_amd.model import CrossScoreNet
    from crossscore_amd.predict import predict

    qd, rd = make_scene(str(tmp_path / "data"), n_query=5, n_ref=4)
    arch = CrossScoreNet(model_config(**{"backbone.from_pretrained": TINY})).arch
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(arch, 5).items()}
    common = [f"data.dataset.query_dir={qd}", f"data.dataset.reference_dir={rd}", f"model.backbone.from_pretrained={TINY}",
              "this_main.resize_short_side=56", "data.neighbour_config.cross=3", "data.neighbour_config.deterministic=True",
              "data.loader.validation.batch_size=2", "logger.predict.write.config.score_map_colour_mode=rgb"]
    runs = {}
    for name, extra in (("fast", ["this_main.png_encoder=gpu", "this_main.png_compression=fast"]),
                        ("compact", ["this_main.png_encoder=gpu", "this_main.png_compression=compact"]),
                        ("host", ["this_main.png_encoder=host"]), ("host_compact", ["this_main.png_encoder=host", "this_main.png_compression=compact"])):
        np.random.seed(0)
        with torch.no_grad():
            runs[name] = predict(load_config("default_predict", common + extra + [f"logger.predict.out_dir={tmp_path}/out_{name}"]), state_dict=sd, now="T")
    trees = {k: tree_bytes(r["out_dir"]) for k, r in runs.items()}
    _compare_trees(trees["fast"], trees["compact"], trees["host"], trees["host_compact"])
    assert runs["fast"]["rows"] == runs["compact"]["rows"] == runs["host"]["rows"]
    assert runs["fast"]["png_compression"] == "fast" and runs["compact"]["png_compression"] == "compact" and runs["host"]["png_compression"] == "fast"
    assert runs["host_compact"]["png_compression"] == "compact" and runs["host_compact"]["png_encoder"] == "host"
    assert runs["compact"]["png_files"] == runs["fast"]["png_files"] and runs["compact"]["png_files"]["png_gpu_files"] == 5 + 5 + 5 * 3
    assert runs["host_compact"]["png_files"]["png_gpu_files"] == 0
    with pytest.raises(ValueError, match="fast | compact"):
        predict(load_config("default_predict", common + ["this_main.png_compression=best", f"logger.predict.out_dir={tmp_path}/out_x"]), state_dict=sd, now="T")


@pytest.mark.gpu
def test_evaluate_fast_and_compact(tmp_path, tmp_path_factory):
    from crossscore_amd import synth
    from crossscore_amd.config import load_config, model_config
    from crossscore_amd.evaluate import evaluate
    from crossscore_amd.model import CrossScoreNet

    tree = make_tree(tmp_path_factory.mktemp("nvs"), scenes=["scene_a", "scene_b"])
    arch = CrossScoreNet(model_config(**{"backbone.from_pretrained": TINY})).arch
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(arch, 7).items()}
    common = [f"data.dataset.path={tree}", f"model.backbone.from_pretrained={TINY}", "this_main.resize_short_side=56",
              "data.dataset.num_gaussians_iters=2", "data.loader.validation.batch_size=4", "data.loader.validation.num_workers=2",
              "data.neighbour_config.deterministic=True", "logger.test.write.flag.score_map_gt=True", "logger.test.write.config.score_map_colour_mode=gray"]
    runs = {}
    for name, extra in (("fast", ["this_main.png_encoder=gpu"]), ("compact", ["this_main.png_encoder=gpu", "this_main.png_compression=compact"]),
                        ("host", []), ("host_compact", ["this_main.png_compression=compact"])):
        np.random.seed(0)
        with torch.no_grad():
            runs[name] = evaluate(load_config("default_test", common + extra + [f"logger.test.out_dir={tmp_path}/out_{name}"]), state_dict=sd, now=f"NOW_{name}")
    trees = {k: tree_bytes(r["out_dir"]) for k, r in runs.items()}
    _compare_trees(trees["fast"], trees["compact"], trees["host"], trees["host_compact"])
    assert repr(runs["fast"]["metrics"]) == repr(runs["compact"]["metrics"]) == repr(runs["host"]["metrics"])
    assert [runs[k]["png_compression"] for k in ("fast", "compact", "host", "host_compact")] == ["fast", "compact", "fast", "compact"]
    assert runs["compact"]["png_files"] == runs["fast"]["png_files"] and runs["compact"]["png_files"]["png_gpu_files"] >= 24


@pytest.mark.gpu
def test_metric_maps_fast_and_compact(tmp_path):
    from crossscore_amd.config import load_config
    from crossscore_amd.metric_maps import generate

    res, trees = {}, {}
    for name, extra in (("fast", []), ("compact", ["this_main.png_compression=compact"])):
        root = make_tree(tmp_path / name, scenes=["scene_b"])  # the smallest scene: 60 x 84, no metric_map directory yet
        before = set(tree_bytes(root))
        res[name] = generate(load_config("default_test", [f"data.dataset.path={root}", "data.dataset.num_gaussians_iters=-1"] + extra))
        trees[name] = {k: v for k, v in tree_bytes(root).items() if k not in before}
        assert len(trees[name]) == len(res[name]["written"]) == res[name]["png_gpu_files"] >= 2 and all(k.endswith(".png") for k in trees[name])
    assert res["fast"]["png_compression"] == "fast" and res["compact"]["png_compression"] == "compact"
    _compare_trees(trees["fast"], trees["compact"])
    with pytest.raises(ValueError, match="fast | compact"):
        generate(load_config("default_test", [f"data.dataset.path={tmp_path}/fast", "this_main.png_compression=best"]))
