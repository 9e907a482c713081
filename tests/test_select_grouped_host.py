"""Reference selection by similarity in the test phase, host side: the candidate lists nvs.NvsItems hands to the device-side
choice are exactly the lists the reference's sampler draws from, nothing is drawn for them, the run's options take the strategy for evaluate,
and reference_selection.csv names files unambiguously across scenes.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from crossscore_amd import data as csdata  # noqa: E402
from crossscore_amd import model as csmodel  # noqa: E402
from crossscore_amd.config import load_config  # noqa: E402
from crossscore_amd.nvs import NvsItems  # noqa: E402
from nvs_tree import make_tree  # noqa: E402

SIMILAR = {"strategy": "similar", "cross": 2, "deterministic": True}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp("nvs"))


@pytest.mark.parametrize("split,iters,compute_gt", [("test", 2, False), ("test", -1, False), ("test", 2, True), ("train", 2, False), ("val", 1, True)])
def test_an_items_group_is_the_list_random_draws_from(tree, split, iters, compute_gt):
    rnd = NvsItems(tree, None, split, dict(SIMILAR, strategy="random"), "ssim", iters, compute_gt)
    np.random.seed(5)
    state = np.random.get_state()
    sim = NvsItems(tree, None, split, SIMILAR, "ssim", iters, compute_gt, candidates=True)
    got = [sim[i] for i in range(len(sim))]
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]  # no RNG is drawn
    assert len(sim) == len(rnd) and len(sim) > 0
    for i, it in enumerate(got):
        cross = list(rnd._index[i][2])
        assert it["reference/cross/imgs"] is None
        assert sim.groups[it["reference/cross/group"]] == cross, i
        assert it["query/img"] == rnd._index[i][0] and it["query/score_map"] == rnd._index[i][1]
        assert ("query/gt" in it) == compute_gt and (not compute_gt or it["query/gt"] == rnd._index[i][3])
        scene_split_iter = it["query/img"].split(os.sep)[-5:-2]  # the other split of the query's own scene and iteration, captured images
        other = {"train": "test", "test": "train"}[scene_split_iter[1]]
        assert all(p.split(os.sep)[-5:-1] == [scene_split_iter[0], other, scene_split_iter[2], "gt"] for p in cross)
    # each distinct list once, in index order
    firsts = list(dict.fromkeys(tuple(rnd._index[i][2]) for i in range(len(rnd))))
    assert [tuple(g) for g in sim.groups] == firsts
    assert [it["reference/cross/group"] for it in got] == [firsts.index(tuple(rnd._index[i][2])) for i in range(len(rnd))]
    if split == "test" and iters == 2:
        assert sorted(len(g) for g in sim.groups) == [1, 1, 2, 2, 3, 3]
    # what the loader plans for such items: the queries (and the driver's extras) only
    assert csdata.batch_files(got[:3]) == [(it["query/img"], False) for it in got[:3]]
    assert csdata.item_paths(got[:3])["reference/cross/imgs"] is None


def test_from_config_asks_for_candidates_with_similar_only(tree):
    over = [f"data.dataset.path={tree}", "data.dataset.num_gaussians_iters=2", "data.neighbour_config.cross=2"]
    sim = NvsItems.from_config(load_config("default_test", over + ["data.neighbour_config.strategy=similar"]))
    assert sim.candidates and len(sim.groups) == 6 and "reference/cross/group" in sim[0]
    rnd = NvsItems.from_config(load_config("default_test", over))
    assert not rnd.candidates and rnd.groups == [] and "reference/cross/group" not in rnd[0] and len(rnd[0]["reference/cross/imgs"]) == 2
    with pytest.raises(NotImplementedError, match="predict only"):  # the bare constructor draws on the host
        NvsItems(tree, None, "test", SIMILAR, "ssim", 2)
    with pytest.raises(NotImplementedError):
        NvsItems(tree, None, "test", dict(SIMILAR, strategy="nearest"), "ssim", 2, candidates=True)


def test_options_take_similar_for_the_test_phase(tree, monkeypatch):
    from crossscore_amd import scoring

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)  # options() only reads the configuration behind this check

    def cfg(*over):
        return load_config("default_test", [f"data.dataset.path={tree}", "data.neighbour_config.strategy=similar", *over])

    o = scoring.options(cfg(), "test")
    assert o.strategy == "similar" and o.phase == "test"
    with pytest.raises(ValueError, match="zero_reference"):
        scoring.options(cfg("data.dataset.zero_reference=True"), "test")
    with pytest.raises(ValueError, match="cache_reference_tokens"):
        scoring.options(cfg("this_main.cache_reference_tokens=False"), "test")
    with pytest.raises(ValueError, match="cross"):
        scoring.options(cfg("data.neighbour_config.cross=0"), "test")
    with pytest.raises(NotImplementedError):
        scoring.options(load_config("default_test", [f"data.dataset.path={tree}", "data.neighbour_config.strategy=nearest"]), "test")


def test_reference_selection_csv_names_files_by_five_path_parts(tmp_path):
    from crossscore_amd import scoring

    a = "/d/res_540/scene_a/test/ours_1000/renders/frame_00000.png"
    b = "/d/res_540/scene_b/test/ours_1000/renders/frame_00000.png"
    ga = ["/d/res_540/scene_a/train/ours_1000/gt/frame_00002.png", "/d/res_540/scene_a/train/ours_1000/gt/frame_00000.png"]
    gb = ["/d/res_540/scene_b/train/ours_1000/gt/frame_00000.png", "empty_image"]
    path = scoring.write_reference_selection(str(tmp_path), [(a, ga, [0.98765, -0.00004]), (b, gb, [0.5, float("nan")])], 5)
    assert open(path).read().splitlines() == [
        "query,reference_0,reference_1,similarity_0,similarity_1",
        "scene_a/test/ours_1000/renders/frame_00000.png,scene_a/train/ours_1000/gt/frame_00002.png,scene_a/train/ours_1000/gt/frame_00000.png,0.9877,-0.0000",
        "scene_b/test/ours_1000/renders/frame_00000.png,scene_b/train/ours_1000/gt/frame_00000.png,empty_image,0.5000,"]
    # predict's form is unchanged: base names
    path = scoring.write_reference_selection(str(tmp_path), [("/a/q/frame_1.png", ["/a/r/x.png", "/a/r/y.png"], [0.98765, -0.00004])])
    assert open(path).read().splitlines() == ["query,reference_0,reference_1,similarity_0,similarity_1", "frame_1.png,x.png,y.png,0.9877,-0.0000"]


def test_group_offsets_are_checked_on_the_host():
    assert csmodel._group_offsets([0, 1, 5], 6).tolist() == [0, 1, 5] and csmodel._group_offsets([0, 6], 6).dtype == np.int32
    for bad in ([1, 5], [0, 5, 5], [0, 5, 4], [0, 7], [0], []):
        with pytest.raises(ValueError, match="offsets"):
            csmodel._group_offsets(bad, 6)


def test_a_bank_larger_than_the_cache_limit_names_the_count_and_the_key():
    groups = [["/s/a/gt/0.png", "/s/a/gt/1.png"], ["/s/b/gt/0.png", "empty_image"], ["/s/c/gt/0.png", "/s/c/gt/1.png"]]
    with pytest.raises(ValueError, match=r"hold 5 files.*this_main\.reference_cache_max_images=5"):  # 5 files + the placeholder's row
        csdata.ReferenceBank(None, None, None, (56, 70), 2, max_images=5, groups=groups)
    with pytest.raises(ValueError, match="holds no file"):
        csdata.ReferenceBank(None, None, None, (56, 70), 2, groups=[["empty_image"]])
