"""Reference selection by similarity, host side: properties of the oracle the GPU tests compare with (tests/select_oracle.py),
and how the configuration reaches the item lists and the run's options.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import select_oracle as so  # noqa: E402
from crossscore_amd import data as csdata  # noqa: E402
from crossscore_amd.config import load_config  # noqa: E402


def _tokens(I, Np, C, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.normal(size=(I, Np, C)) * 0.7).astype(np.float16)


# ------------------------------------------------------------------------------------------------------------------- the oracle
def test_a_pattern_added_to_every_image_leaves_the_selection_unchanged():
    """Every image carries the same multi-view PE; its pooled value is a constant offset of the means, and centring on the bank removes it."""
    rng = np.random.Generator(np.random.PCG64(2))
    bank, query = so.widen(_tokens(12, 9, 64, 3)), so.widen(_tokens(4, 9, 64, 4))
    pattern = rng.normal(size=(9, 64)) * 3.0
    idx0, s0 = so.choose(query, bank, 5)
    idx1, s1 = so.choose(query + pattern, bank + pattern, 5)
    assert min(so.top_gaps(s0, 5)) > 1e-6
    assert np.array_equal(idx0, idx1) and np.abs(s0 - s1).max() < 1e-12


def test_a_later_duplicate_ties_and_loses():
    bank = so.widen(_tokens(8, 5, 64, 5))
    bank = np.concatenate([bank, bank[2:3]])  # row 8 is row 2 again
    idx, s = so.choose(bank[2:3] + 0.0, bank, 9)
    assert s[0, 2] == s[0, 8]
    assert idx[0, 0] == 2 and idx[0, 1] == 8  # the query is row 2 itself: both come first, the lower index before the higher
    top1, _ = so.choose(bank[2:3] + 0.0, bank, 1)
    assert top1[0, 0] == 2


def test_exclude_is_honoured():
    bank = so.widen(_tokens(6, 5, 64, 6))
    free, s = so.choose(bank[:3] + 0.0, bank, 5, None)
    assert list(free[:, 0]) == [0, 1, 2]
    ex = np.array([0, -1, 2], dtype=np.int32)
    idx, _ = so.choose(bank[:3] + 0.0, bank, 5, ex)
    assert 0 not in idx[0] and 2 not in idx[2] and idx[1, 0] == 1
    assert sorted(idx[0]) == [1, 2, 3, 4, 5] and -1 not in idx
    short = so.select(s, 6, ex)  # more asked for than there are candidates: the remaining places say so
    assert short[0, 5] == -1 and short[1, 5] >= 0


def test_restatement_bounds_come_with_a_floor():
    t = so.widen(_tokens(2, 1, 64, 7))
    assert np.array_equal(so.mean_seq32(t).astype(np.float64), so.mean(t))  # one row: exact
    assert so.tolerance(so.mean(t), so.mean_seq32(t)) == 1e-7 * np.abs(so.mean(t)).max()
    t = so.widen(_tokens(2, 700, 64, 8))
    assert so.tolerance(so.mean(t), so.mean_seq32(t)) > 1e-7 * np.abs(so.mean(t)).max()


# ------------------------------------------------------------------------------------------------------------------- configuration
def _dirs(tmp_path, n_query=3, n_ref=4):
    qd, rd = tmp_path / "q", tmp_path / "r"
    qd.mkdir()
    rd.mkdir()
    for i in range(n_query):
        (qd / f"frame_{i:05}.png").write_bytes(b"")
    for i in range(n_ref):
        (rd / f"frame_{i:05}.png").write_bytes(b"")
    return str(qd), str(rd)


def test_similar_items_draw_nothing_and_carry_no_references(tmp_path):
    qd, rd = _dirs(tmp_path)
    np.random.seed(11)
    state = np.random.get_state()
    items = csdata.SimpleReferenceItems(qd, rd, {"strategy": "similar", "cross": 2, "deterministic": False})
    got = [items[i] for i in range(len(items))]
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    assert len(got) == 3 and all(it["reference/cross/imgs"] is None for it in got)
    assert [os.path.basename(it["query/img"]) for it in got] == [f"frame_{i:05}.png" for i in range(3)]
    assert len(items.reference_paths) == 4
    # what the loader plans for such items: the queries only; the collated paths wait for the batch's reference_index
    assert csdata.batch_files(got) == [(it["query/img"], False) for it in got]
    assert csdata.plan_decodes([got[:2], got[2:]], False, False) == [[(it["query/img"], False) for it in got[:2]], [(got[2]["query/img"], False)]]
    assert csdata.item_paths(got)["reference/cross/imgs"] is None
    # random is untouched
    rnd = csdata.SimpleReferenceItems(qd, rd, {"strategy": "random", "cross": 2, "deterministic": True})
    assert rnd[0]["reference/cross/imgs"] == rnd.reference_paths[:2]


def test_other_strategies_still_raise(tmp_path):
    qd, rd = _dirs(tmp_path)
    with pytest.raises(NotImplementedError):
        csdata.SimpleReferenceItems(qd, rd, {"strategy": "nearest", "cross": 3, "deterministic": True})


def test_evaluate_items_refuse_similar(tmp_path):
    from crossscore_amd import nvs

    split = nvs.DATA_SPLITS[0] if isinstance(nvs.DATA_SPLITS, (list, tuple)) else sorted(nvs.DATA_SPLITS)[0]
    with pytest.raises(NotImplementedError, match="predict only"):
        nvs.NvsItems(str(tmp_path), "res_540", split, {"strategy": "similar", "cross": 2, "deterministic": True}, "ssim")
    with pytest.raises(NotImplementedError):
        nvs.NvsItems(str(tmp_path), "res_540", split, {"strategy": "nearest", "cross": 2, "deterministic": True}, "ssim")


def _cfg(tmp_path, *over):
    qd, rd = str(tmp_path / "q"), str(tmp_path / "r")
    return load_config("default_predict", [f"data.dataset.query_dir={qd}", f"data.dataset.reference_dir={rd}", *over])


def test_options_of_a_similar_run(tmp_path, monkeypatch):
    from crossscore_amd import scoring

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)  # options() only reads the configuration behind this check
    o = scoring.options(_cfg(tmp_path, "data.neighbour_config.strategy=similar"), "predict")
    assert o.strategy == "similar" and o.exclude_self is True
    assert scoring.options(_cfg(tmp_path), "predict").strategy == "random"
    assert scoring.options(_cfg(tmp_path, "data.neighbour_config.strategy=similar", "this_main.similar_exclude_self=False"), "predict").exclude_self is False
    with pytest.raises(ValueError, match="zero_reference"):
        scoring.options(_cfg(tmp_path, "data.neighbour_config.strategy=similar", "data.dataset.zero_reference=True"), "predict")
    with pytest.raises(ValueError, match="cache_reference_tokens"):
        scoring.options(_cfg(tmp_path, "data.neighbour_config.strategy=similar", "this_main.cache_reference_tokens=False"), "predict")
    with pytest.raises(NotImplementedError):
        scoring.options(_cfg(tmp_path, "data.neighbour_config.strategy=nearest"), "predict")


def test_reference_selection_csv(tmp_path):
    from crossscore_amd import scoring

    path = scoring.write_reference_selection(str(tmp_path), [("/a/q/frame_1.png", ["/a/r/x.png", "/a/r/y.png"], [0.98765, -0.00004]),
                                                              ("/a/q/frame_2.png", ["/a/r/y.png", "/a/r/z.png"], [1.0, 0.5])])
    assert open(path).read().splitlines() == ["query,reference_0,reference_1,similarity_0,similarity_1", "frame_1.png,x.png,y.png,0.9877,-0.0000",
                                              "frame_2.png,y.png,z.png,1.0000,0.5000"]
