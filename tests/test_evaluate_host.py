"""Test phase (crossscore_amd/evaluate.py, nvs.py), host side: the NvsDataset walker against the reference's golden, configs, output naming,
and the metric arithmetic against numpy fp64.  No GPU."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from crossscore_amd import evaluate as ev  # noqa: E402
from crossscore_amd.config import load_config  # noqa: E402
from crossscore_amd.nvs import NvsItems, get_paths, random_order  # noqa: E402
from nvs_tree import make_tree  # noqa: E402

GOLD = json.load(open(os.path.join(HERE, "golden", "n0_nvs_items.json")))
CROSS = {"strategy": "random", "cross": 5, "deterministic": True}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp("nvs"))


def _rel(item, root):
    r = lambda p: p if p == "empty_image" else os.path.relpath(p, root)  # noqa: E731
    return {k: (r(v) if isinstance(v, str) else [r(x) for x in v]) for k, v in item.items()}


@pytest.mark.parametrize("det,seed,key", [(True, 0, "deterministic"), (False, 1, "random_seed1")])
def test_walker_matches_reference_items(tree, det, seed, key):
    items = NvsItems(tree, None, "test", dict(CROSS, deterministic=det), "ssim", 2)
    np.random.seed(seed)
    got = [_rel(items[i], tree) for i in range(len(items))]
    assert got == GOLD[key]


def test_walker_mae_maps_and_dataset_list(tree):
    items = NvsItems(tree, None, "test", CROSS, "mae", 2)
    assert [os.path.relpath(items[i]["query/score_map"], tree) if items[i]["query/score_map"] != "empty_image" else "empty_image"
            for i in range(9)] == GOLD["mae_score_maps"]
    # mse reads the MAE maps; a list of two paths is the two datasets concatenated in order
    assert items._index == NvsItems(tree, "res_540", "test", CROSS, "mse", 2)._index
    two = NvsItems([tree, tree], None, "test", CROSS, "ssim", 2)
    assert len(two) == 2 * len(items) and two._index[len(items):] == NvsItems(tree, None, "test", CROSS, "ssim", 2)._index
    # every iteration without the cut: scene_a has three
    assert len(NvsItems(tree, None, "test", CROSS, "ssim", -1)) == len(items) + 3 + 2


def test_walker_errors(tree, tmp_path):
    with pytest.raises(ValueError, match="data_split"):
        NvsItems(tree, None, "validation", CROSS, "ssim", 2)
    with pytest.raises(ValueError, match="metric type"):
        NvsItems(tree, None, "test", CROSS, "psnr", 2)
    # one metric map fewer than renders: count mismatch
    bad = make_tree(tmp_path / "bad", scenes=["scene_a"])
    os.remove(os.path.join(bad, "res_540", "scene_a", "test", "ours_1000", "metric_map", "ssim", "frame_00001.png"))
    with pytest.raises(ValueError, match="mismatch"):
        NvsItems(bad, None, "test", CROSS, "ssim", 2)
    # the reference's placeholder count is the split's iterations so far: a missing metric directory over two iterations mismatches
    with pytest.raises(ValueError, match="mismatch"):
        get_paths([Path(bad, "res_540", "scene_a")], 2, "metric_map/none")


def test_gt_stage_rejects_a_map_of_another_size():
    import torch

    from crossscore_amd.data import InputStage

    stage = InputStage(torch.device("cpu"), resize_short_side=-1)
    with pytest.raises(ValueError, match="differ in size"):
        stage.metric_map(np.zeros((10, 12), np.uint16), (10, 14), 0, torch.empty((10, 14)))
    with pytest.raises(ValueError, match="uint16"):
        stage.metric_map(np.zeros((10, 14), np.float32), (10, 14), 0, torch.empty((10, 14)))


def test_read_metric_map_accepts_i16_and_i32(tmp_path, monkeypatch):
    from PIL import Image

    from crossscore_amd.decode import read_metric_map_u16

    m = (np.arange(12 * 7, dtype=np.uint32) * 781 % 65536).astype(np.uint16).reshape(12, 7)
    Image.fromarray(m).save(tmp_path / "a.png")
    got = read_metric_map_u16(str(tmp_path / "a.png"))
    assert got.dtype == np.uint16 and np.array_equal(got, m)
    # PIL versions that open 16-bit PNGs in mode "I" hand out int32 arrays
    monkeypatch.setattr(Image, "open", lambda p: Image.fromarray(m.astype(np.int32)))
    got = read_metric_map_u16(str(tmp_path / "a.png"))
    assert got.dtype == np.uint16 and np.array_equal(got, m)


def test_default_test_config():
    cfg = load_config("default_test")
    assert cfg.this_main.crop_mode == "integer_patches" and cfg.this_main.data_split == "test"
    assert cfg.data.loader.validation.batch_size == 24 and cfg.data.loader.validation.shuffle is True
    assert cfg.data.dataset.resolution is None and cfg.data.dataset.num_gaussians_iters == -1
    assert isinstance(cfg.data.dataset.path, list)
    assert cfg.logger.test.write.flag.item_path_json is True and cfg.logger.test.write.flag.score_map_gt is False
    assert cfg.logger.test.write.config.score_map_colour_mode == "gray"
    assert cfg.model.loss.fn == "l1" and cfg.trainer.limit_test_batches == 1.0
    assert cfg.this_main.cache_reference_tokens is True and cfg.this_main.fused_input_stage == "auto"
    assert "hydra" not in cfg
    cfg = load_config("default_test", ["data.dataset.path=/t", "model.predict.metric.type=mae", "this_main.crop_mode=null",
                                       "trainer.limit_test_batches=3"])
    assert cfg.data.dataset.path == "/t" and cfg.model.predict.metric.type == "mae" and cfg.this_main.crop_mode is None
    assert cfg.trainer.limit_test_batches == 3


def test_out_dir_and_version_naming(tmp_path):
    cfg = load_config("default_test", [f"trainer.ckpt_path_to_load={tmp_path}/run/ckpts/x.ckpt"])
    v, o = ev.resolve_dirs(cfg)
    assert v == str(tmp_path / "run" / "test" / "version_0") and o == v + "_"  # alias "": a trailing "_"
    os.makedirs(o)
    v1, _ = ev.resolve_dirs(cfg)
    assert v1.endswith("version_1")  # "version_0_" counts as version 0, as Lightning's CSVLogger reads it
    cfg.alias = "abc"
    assert ev.resolve_dirs(cfg)[1] == v1 + "_abc"
    cfg.logger.test.out_dir = str(tmp_path / "mine")
    assert ev.resolve_dirs(cfg)[1] == str(tmp_path / "mine")
    cfg = load_config("default_test")
    v, o = ev.resolve_dirs(cfg, now="NOW")
    assert v == os.path.join("log", "NOW", "test_empty_ckpt", "version_0") and o == v + "_"


def test_limit_batches():
    assert ev.limit_batches(10, 1.0) == 10 and ev.limit_batches(10, 0.25) == 2 and ev.limit_batches(10, 3) == 3 and ev.limit_batches(2, 5) == 2
    with pytest.raises(ValueError):
        ev.limit_batches(10, 0.01)
    with pytest.raises(ValueError):
        ev.limit_batches(10, -1)


def _sums(s, g):
    s, g = s.astype(np.float64), g.astype(np.float64)
    return np.stack([np.abs(s - g).sum((1, 2)), s.sum((1, 2)), g.sum((1, 2)), (s * s).sum((1, 2)), (g * g).sum((1, 2)),
                     (s * g).sum((1, 2))], 1)


def test_batch_metrics_against_numpy():
    rng = np.random.default_rng(3)
    s = rng.random((3, 20, 28), dtype=np.float32)
    g = (0.6 * s + 0.4 * rng.random((3, 20, 28), dtype=np.float32)).astype(np.float32)
    m = ev.batch_metrics(_sums(s, g), 20 * 28)
    d = np.abs(s.astype(np.float64) - g)
    assert m["loss"] == pytest.approx(d.mean(), rel=1e-12)
    assert m["corr"] == pytest.approx(np.corrcoef(s.ravel().astype(np.float64), g.ravel().astype(np.float64))[0, 1], rel=1e-9)
    assert m["psnr"] == pytest.approx(-10 * np.log10(d.mean() ** 2), rel=1e-12)
    g[1, 3, 4] = np.nan  # a NaN GT map: the batch's values are NaN
    assert all(np.isnan(v) for v in ev.batch_metrics(_sums(s, g), 20 * 28).values())


def test_epoch_values_are_batch_size_weighted_means():
    rows = [dict(batch_size=4, loss=0.1, corr=0.5, psnr=20.0), dict(batch_size=2, loss=0.4, corr=-0.1, psnr=8.0)]
    m = ev.epoch_metrics(ev.weighted_sums(rows))
    assert m["test/loss"] == pytest.approx((4 * 0.1 + 2 * 0.4) / 6, rel=1e-15) and m["test/loss"] == m["test/loss_cross"]
    assert m["test/corr_cross"] == pytest.approx((4 * 0.5 - 2 * 0.1) / 6, rel=1e-15)
    assert m["test/psnr_cross"] == pytest.approx((80 + 16) / 6, rel=1e-15)
    rows.append(dict(batch_size=1, loss=float("nan"), corr=float("nan"), psnr=float("nan")))
    assert all(np.isnan(v) for v in ev.epoch_metrics(ev.weighted_sums(rows)).values())


def test_metrics_csv_columns(tmp_path):
    p = ev.write_metrics_csv(str(tmp_path / "version_0"), {"test/loss": 0.25, "test/loss_cross": 0.25, "test/corr_cross": 0.5,
                                                           "test/psnr_cross": 12.0})
    import csv

    rows = list(csv.DictReader(open(p)))
    assert len(rows) == 1 and set(rows[0]) == {"test/loss", "test/loss_cross", "test/corr_cross", "test/psnr_cross", "epoch", "step"}
    assert float(rows[0]["test/corr_cross"]) == 0.5 and rows[0]["epoch"] == "0"


def test_random_order_is_seeded():
    assert random_order(10, 1) == random_order(10, 1) and sorted(random_order(10, 1)) == list(range(10))
    assert random_order(10, 1) != random_order(10, 2)


def test_gloo_world2_sum_over_ranks(tmp_path):
    """world_size-2 gloo run of the epoch reduction: (sum bs * v, sum bs) summed over the ranks gives the global weighted mean."""
    script = tmp_path / "worker.py"
    script.write_text(
        "from crossscore_amd.parallel import init_from_env, sum_over_ranks, gather_objects\n"
        "from crossscore_amd.evaluate import weighted_sums, epoch_metrics\n"
        "rank, local, world = init_from_env('gloo')\n"
        "rows = [dict(batch_size=3, loss=0.1, corr=0.2, psnr=10.0)] if rank == 0 else [dict(batch_size=1, loss=0.5, corr=0.6, psnr=2.0)]\n"
        "tot = sum_over_ranks(weighted_sums(rows))\n"
        "assert tot[3] == 4.0, tot\n"
        "m = epoch_metrics(tot)\n"
        "assert abs(m['test/loss'] - (0.3 + 0.5) / 4) < 1e-15, m\n"
        "assert gather_objects(rank) == [0, 1]\n"
        "if rank == 0: print('GLOO_SUM_OK', world)\n")
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29743",
           str(script)]
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0 and "GLOO_SUM_OK 2" in res.stdout, res.stdout[-2000:]
