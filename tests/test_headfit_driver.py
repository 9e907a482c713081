"""python -m crossscore_amd.fit_head on the tree of tests/nvs_tree.py: the CSV and its StepLR schedule, the checkpoint in
evaluate, ground truth from files against ground truth computed on the device, and the configurations the driver refuses."""
import os
import shutil
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from nets import TINY, state_dict_for  # noqa: E402
from nvs_tree import make_tree  # noqa: E402
from scenes import read_csv_dicts  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _in_tmp(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp("nvs"))


def _overrides(tree, out, extra=()):
    return [f"data.dataset.path={tree}", f"model.backbone.from_pretrained={TINY}", "this_main.resize_short_side=56", "data.dataset.num_gaussians_iters=2",
            "data.loader.train.batch_size=4", "data.loader.train.num_workers=2", "data.neighbour_config.deterministic=True",
            f"logger.train.out_dir={out}"] + list(extra)


def _fit(tree, out, extra=(), sd=None):
    from crossscore_amd.config import load_config
    from crossscore_amd.fit_head import fit_head

    return fit_head(load_config("default_fit_head", _overrides(tree, out, extra)), state_dict=sd if sd is not None else state_dict_for(TINY, 7))


def test_two_epochs_csv_schedule_and_checkpoint_in_evaluate(tree, tmp_path):
    from crossscore_amd.config import load_config
    from crossscore_amd.evaluate import evaluate

    res = _fit(tree, tmp_path / "fit", ["trainer.max_epochs=2", "trainer.lr_scheduler.step_size=1", "trainer.lr_scheduler.gamma=0.5"])
    rows = read_csv_dicts(res["csv"])
    # one row per step: the train split's items (scene_a's renders of two iterations) in batches of 4, twice; StepLR(1, 0.5) stepped per epoch
    from crossscore_amd.nvs import NvsItems
    per_epoch = -(-len(NvsItems.from_config(load_config("default_fit_head", _overrides(tree, tmp_path / "fit")))) // 4)
    assert per_epoch >= 2 and res["steps"] == 2 * per_epoch
    assert [(r["epoch"], r["step"]) for r in rows] == [(str(i // per_epoch), str(i + 1)) for i in range(2 * per_epoch)]
    assert [float(r["lr"]) for r in rows] == [5e-4] * per_epoch + [2.5e-4] * per_epoch
    assert all(len(r["loss"].split(".")[1]) == 6 for r in rows)
    assert os.path.basename(res["checkpoint"]) == "last.ckpt" and os.path.basename(os.path.dirname(res["checkpoint"])) == "checkpoints"

    def train_loss(name, extra, sd):
        cfg = load_config("default_test", [f"data.dataset.path={tree}", f"model.backbone.from_pretrained={TINY}", "this_main.resize_short_side=56",
                                           "data.dataset.num_gaussians_iters=2", "data.loader.validation.batch_size=4",
                                           "data.loader.validation.num_workers=2", "data.neighbour_config.deterministic=True",
                                           "this_main.data_split=train", "logger.test.write.flag.batch=False",
                                           f"logger.test.out_dir={tmp_path}/{name}"] + extra)
        with torch.no_grad():
            return evaluate(cfg, state_dict=sd, now="NOW")["metrics"]["test/loss_cross"]

    start = train_loss("eval_start", [], state_dict_for(TINY, 7))
    fitted = train_loss("eval_fit", [f"trainer.ckpt_path_to_load={res['checkpoint']}"], None)
    print(f"test/loss_cross on the training split: {start:.6f} with the starting weights, {fitted:.6f} after {res['steps']} steps; csv {[r['loss'] for r in rows]}")
    assert fitted < start


def test_computed_and_file_ground_truth_give_the_same_csv(tree, tmp_path):
    from crossscore_amd.config import load_config
    from crossscore_amd.metric_maps import generate

    bare = tmp_path / "gaussian" / "mfr"
    shutil.copytree(os.path.join(tree, "res_540", "scene_a"), bare / "res_540" / "scene_a", ignore=shutil.ignore_patterns("metric_map"))
    shutil.copy(os.path.join(tree, "res_540", "split.json"), bare / "res_540" / "split.json")
    with pytest.raises(ValueError):
        _fit(str(bare), tmp_path / "none")  # a bare tree in files mode: the walk finds no ground-truth maps
    comp = _fit(str(bare), tmp_path / "compute", ["this_main.gt_metric_maps=compute"])
    assert comp["gt_metric_maps"] == "compute" and comp["steps"] >= 2
    generate(load_config("default_test", [f"data.dataset.path={bare}", "data.dataset.num_gaussians_iters=-1", "this_main.data_split=train"]))
    files = _fit(str(bare), tmp_path / "files")
    assert files["gt_metric_maps"] == "files"
    assert open(comp["csv"], "rb").read() == open(files["csv"], "rb").read()


def test_token_cache_on_and_off_give_the_same_csv(tree, tmp_path):
    on = _fit(tree, tmp_path / "on")
    off = _fit(tree, tmp_path / "off", ["this_main.cache_reference_tokens=False"])
    assert on["cache_reference_tokens"] and not off["cache_reference_tokens"] and on["steps"] == off["steps"] >= 2
    assert open(on["csv"], "rb").read() == open(off["csv"], "rb").read()


def test_refused_configurations(tree, tmp_path):
    with pytest.raises(ValueError, match="one device"):
        _fit(tree, tmp_path / "a", ["trainer.devices=[0,1]"])
    with pytest.raises(ValueError, match="do_reference_cross"):
        _fit(tree, tmp_path / "b", ["model.do_reference_cross=False"])
    with pytest.raises(ValueError, match="patch"):
        _fit(tree, tmp_path / "c", ["model.patch_size=16"])
    with pytest.raises(ValueError, match="ground-truth"):
        # the test split holds scene_b, which has no metric maps: placeholders
        _fit(tree, tmp_path / "d", ["this_main.data_split=test"])
