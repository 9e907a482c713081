"""python -m crossscore_amd.fit_head with this_main.fit_scope=tail on the tree of tests/nvs_tree.py: the CSV, the checkpoint
(exactly the ten tail tensors move) and that checkpoint in evaluate; fit_scope=head and no key at all are the run of before, byte for byte."""
import os
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


def _cfg(tree, out, extra=()):
    from crossscore_amd.config import load_config

    return load_config("default_fit_head", [f"data.dataset.path={tree}", f"model.backbone.from_pretrained={TINY}", "this_main.resize_short_side=56",
                                            "data.dataset.num_gaussians_iters=2", "data.loader.train.batch_size=4", "data.loader.train.num_workers=2",
                                            "data.neighbour_config.deterministic=True", f"logger.train.out_dir={out}"] + list(extra))


def _fit(cfg):
    from crossscore_amd.fit_head import fit_head

    return fit_head(cfg, state_dict=state_dict_for(TINY, 7))


def test_tail_two_epochs_checkpoint_and_evaluate(tree, tmp_path):
    from crossscore_amd.config import load_config, model_config
    from crossscore_amd.evaluate import evaluate
    from crossscore_amd.model import CrossScoreNet, load_lightning_checkpoint

    res = _fit(_cfg(tree, tmp_path / "fit", ["this_main.fit_scope=tail", "trainer.max_epochs=2"]))
    assert res["fit_scope"] == "tail" and res["steps"] >= 4
    rows = read_csv_dicts(res["csv"])
    assert list(rows[0]) == ["epoch", "step", "lr", "loss"] and len(rows) == res["steps"]
    losses = [float(r["loss"]) for r in rows]
    per_epoch = res["steps"] // 2
    print(f"tail fit losses {losses}")
    # "falling losses": the batches of one epoch hold different items, so step-to-step the loss need not fall; the same items come back in the
    # second epoch (in another order when the loader shuffles), and its summed loss is below the first's
    assert sum(losses[per_epoch:]) < sum(losses[:per_epoch])
    start = state_dict_for(TINY, 7)
    net = CrossScoreNet(model_config(**{"backbone.from_pretrained": TINY}))
    sd = load_lightning_checkpoint(res["checkpoint"])
    net.load_state_dict(sd, strict=True)
    moved = {k for k in sd if not torch.equal(sd[k], start[k])}
    assert moved == set(net.TAIL_KEYS), moved ^ set(net.TAIL_KEYS)

    def train_loss(name, extra, state):
        cfg = load_config("default_test", [f"data.dataset.path={tree}", f"model.backbone.from_pretrained={TINY}", "this_main.resize_short_side=56",
                                           "data.dataset.num_gaussians_iters=2", "data.loader.validation.batch_size=4",
                                           "data.loader.validation.num_workers=2", "data.neighbour_config.deterministic=True",
                                           "this_main.data_split=train", "logger.test.write.flag.batch=False",
                                           f"logger.test.out_dir={tmp_path}/{name}"] + extra)
        with torch.no_grad():
            return evaluate(cfg, state_dict=state, now="NOW")["metrics"]["test/loss_cross"]

    before = train_loss("eval_start", [], start)
    fitted = train_loss("eval_fit", [f"trainer.ckpt_path_to_load={res['checkpoint']}"], None)
    print(f"test/loss_cross on the training split: {before:.6f} with the starting weights, {fitted:.6f} after {res['steps']} tail steps")
    # the bound test_headfit_driver uses for the head: evaluate's L1 with the fitted checkpoint is below the starting weights'.  It is not tied
    # to the CSV's last loss: that is one batch BEFORE its step, evaluate's is the whole split after the last step
    assert fitted < before


def test_head_scope_and_no_key_are_the_run_of_before(tree, tmp_path):
    head = _fit(_cfg(tree, tmp_path / "head", ["this_main.fit_scope=head"]))
    cfg = _cfg(tree, tmp_path / "nokey")
    del cfg["this_main"]["fit_scope"]
    nokey = _fit(cfg)
    assert head["fit_scope"] == nokey["fit_scope"] == "head" and head["steps"] == nokey["steps"] >= 2
    assert open(head["csv"], "rb").read() == open(nokey["csv"], "rb").read()
    a, b = (torch.load(r["checkpoint"], map_location="cpu", weights_only=False)["state_dict"] for r in (head, nokey))
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    start = state_dict_for(TINY, 7)
    from crossscore_amd.model import CrossScoreNet
    assert {k[len("model."):] for k in a if not torch.equal(a[k], start[k[len("model."):]])} == set(CrossScoreNet.HEAD_KEYS)
    with pytest.raises(ValueError, match="fit_scope"):
        _fit(_cfg(tree, tmp_path / "bad", ["this_main.fit_scope=decoder"]))
