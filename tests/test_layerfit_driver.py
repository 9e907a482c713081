"""python -m crossscore_amd.fit_head with this_main.fit_scope=layer on the tree of tests/nvs_tree.py: the CSV, the checkpoint
(exactly the twenty-two tensors of the whole-layer fit move, every other key keeps its bits), that checkpoint in evaluate, and the refusal of a
decoder without self-attention at set-up."""
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


def test_layer_two_epochs_checkpoint_and_evaluate(tree, tmp_path):
    from crossscore_amd.config import load_config, model_config
    from crossscore_amd.evaluate import evaluate
    from crossscore_amd.fit_head import fit_head
    from crossscore_amd.model import CrossScoreNet, load_lightning_checkpoint

    res = fit_head(_cfg(tree, tmp_path / "fit", ["this_main.fit_scope=layer", "trainer.max_epochs=2"]), state_dict=state_dict_for(TINY, 7))
    assert res["fit_scope"] == "layer" and res["steps"] >= 4
    rows = read_csv_dicts(res["csv"])
    assert list(rows[0]) == ["epoch", "step", "lr", "loss"] and len(rows) == res["steps"]  # one row per step
    losses = [float(r["loss"]) for r in rows]
    per_epoch = res["steps"] // 2
    print(f"layer fit losses {losses}")
    assert sum(losses[per_epoch:]) < sum(losses[:per_epoch])  # (the same items come back in the second epoch: test_tailfit_driver)
    start = state_dict_for(TINY, 7)
    net = CrossScoreNet(model_config(**{"backbone.from_pretrained": TINY}))
    sd = load_lightning_checkpoint(res["checkpoint"])
    net.load_state_dict(sd, strict=True)
    assert set(sd) == set(start)
    moved = {k for k in sd if not torch.equal(sd[k], start[k])}
    assert len(net.LAYER_KEYS) == 22 and moved == set(net.LAYER_KEYS), moved ^ set(net.LAYER_KEYS)

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
    print(f"test/loss_cross on the training split: {before:.6f} with the starting weights, {fitted:.6f} after {res['steps']} layer steps")
    assert fitted < before


def test_no_self_attention_is_refused_at_set_up(tree, tmp_path, monkeypatch):
    """model.decoder_do_self_attn=False leaves the layer scope nothing to fit: a ValueError before the net is built or any forward runs"""
    import crossscore_amd.fit_head as fh

    monkeypatch.setattr(fh, "build_net", lambda *a, **k: pytest.fail("the configuration is refused before the net is built"))
    with pytest.raises(ValueError, match="decoder_do_self_attn"):
        fh.fit_head(_cfg(tree, tmp_path / "bad", ["this_main.fit_scope=layer", "model.decoder_do_self_attn=False"]), state_dict=state_dict_for(TINY, 7))
