"""Ground-truth metric maps formed from the images, host side: the fp64 restatement of the definition
(tests/gtmap_oracle.py) has the properties the definition promises, the MAE code formula is exact, the config key is validated, the
walker's compute mode pairs every query with the captured image of its own view, and the new source is declared and built.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import gtmap_oracle as orc  # noqa: E402
from nvs_tree import make_tree  # noqa: E402

torch = pytest.importorskip("torch")
CROSS = {"strategy": "random", "cross": 5, "deterministic": True}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp("nvs"), scenes=["scene_a", "scene_b"])


def test_identical_images_give_exactly_one():
    a, _ = orc.case_pair("smooth+noise", 40, 52)
    assert torch.equal(orc.ssim_map(a, a.copy()), torch.ones((40, 52), dtype=torch.float64))
    assert int(orc.codes(orc.ssim_map(a, a.copy())).min()) == 65534 == int(orc.codes(orc.ssim_map(a, a.copy())).max())


# fp64's own rounding in these property checks: a window sum rounds each of its 121 products and additions (22 in the separable form), so
# G*(x*x) and mu^2 each carry up to 121 * 2^-53 * mu^2, and their difference is weighed against C2 = 9e-4: the SSIM value moves by up to
# FP64_WORST = 4 * 121 * 2^-53 / C2 = 6e-11 at mu = 1 in the worst case, by about sqrt(121) / 121 of that (5e-12 * mu^2) typically.  The
# 1e-12 checks therefore use levels up to 130 / 255 (mu^2 <= 0.26: the bound then checks the property, not fp64's rounding), and the bright
# levels, where the same cancellation that costs fp32 27 codes shows in fp64 too (3.6e-12 measured at 250 against 249), are held to FP64_WORST.
FP64_WORST = 4 * 121 * 2.0 ** -53 / orc.C2


def test_two_constant_images_away_from_the_border():
    for c1, c2, bound in ((0, 255, 1e-12), (17, 130, 1e-12), (60, 61, 1e-12), (100, 90, 1e-12), (250, 249, FP64_WORST), (255, 254, FP64_WORST)):
        a = np.full((30, 34, 3), c1, np.uint8)
        b = np.full((30, 34, 3), c2, np.uint8)
        m = orc.ssim_map(a, b)
        x, y = c1 / 255, c2 / 255
        want = (2 * x * y + orc.C1) / (x * x + y * y + orc.C1)  # both variances and the covariance vanish: the C2 factors cancel
        err = float((m[5:-5, 5:-5] - want).abs().max())
        print(f"constant {c1} against {c2}: max |fp64 - closed form| {err:.3e} (bound {bound:.1e})")
        assert err <= bound
        assert float((m[0, 0] - want).abs()) > 1e-6  # the zero padding is part of the definition: the 5-pixel frame sees it


def test_separable_equals_direct_and_symmetry():
    for name in ("smooth+noise", "noise vs noise", "shift blend", "flat bright"):
        a, b = orc.case_pair(name, 37, 45)
        for aa, bb, bound in ((a // 2, b // 2, 1e-12), (a, b, 2 * FP64_WORST)):  # halved levels: mu^2 <= 0.25, see FP64_WORST
            direct = orc.ssim_map(aa, bb)
            err = float((orc.ssim_map(aa, bb, separable=True) - direct).abs().max())
            print(f"{name}: max |separable - direct| {err:.3e} (bound {bound:.1e})")
            assert err <= bound
            assert float((orc.ssim_map(bb, aa) - direct).abs().max()) <= 1e-12  # symmetry: the same roundings on swapped operands


def test_window_sums_to_one_and_small_images_are_legal():
    assert abs(float(orc.gauss().sum()) - 1.0) <= 1e-15
    a = np.array([[[10, 20, 30]]], np.uint8)
    m = orc.ssim_map(a, a)
    assert m.shape == (1, 1) and float(m[0, 0]) == 1.0


def test_mae_code_formula_is_exact_for_every_sum():
    s = np.arange(766, dtype=np.int64)
    want = np.trunc(65535.0 * s.astype(np.float64) / 765.0).astype(np.int64)
    assert np.array_equal((257 * s) // 3, want)
    a = np.zeros((1, 766, 3), np.uint8)
    b = np.zeros((1, 766, 3), np.uint8)
    for i in range(766):  # every sum 0..765 as a pixel pair
        b[0, i] = (min(i, 255), min(max(i - 255, 0), 255), max(i - 510, 0))
    assert np.array_equal(orc.mae_codes(a, b).numpy()[0], want) and np.array_equal(orc.mae_codes(b, a).numpy()[0], want)


def test_gt_metric_maps_key_is_validated():
    from crossscore_amd.config import load_config
    from crossscore_amd.evaluate import gt_map_kind, gt_metric_maps_choice

    assert gt_metric_maps_choice(load_config("default_test")) == "files"
    assert gt_metric_maps_choice(load_config("default_test", ["this_main.gt_metric_maps=compute"])) == "compute"
    with pytest.raises(ValueError, match="gt_metric_maps"):
        gt_metric_maps_choice(load_config("default_test", ["this_main.gt_metric_maps=render"]))
    cfg = load_config("default_test")
    del cfg.this_main["gt_metric_maps"]  # a config file written before the key existed
    assert gt_metric_maps_choice(cfg) == "files"
    assert [gt_map_kind(t) for t in ("ssim", "mae", "mse")] == [0, 1, 1]
    with pytest.raises(ValueError, match="metric type"):
        gt_map_kind("psnr")


def test_walker_compute_mode_pairs_each_query_with_its_own_view(tree):
    from crossscore_amd.nvs import NvsItems

    plain = NvsItems(tree, None, "test", CROSS, "ssim", 2)
    comp = NvsItems(tree, None, "test", CROSS, "ssim", 2, compute_gt=True)
    assert len(comp) == len(plain) == 12
    for i in range(len(comp)):
        np.random.seed(i)  # short reference lists are padded and permuted by numpy's global RNG
        p = plain[i]
        np.random.seed(i)
        c = comp[i]
        assert set(c) == {"query/img", "query/score_map", "reference/cross/imgs", "query/gt"}
        assert c["query/img"] == p["query/img"] and c["reference/cross/imgs"] == p["reference/cross/imgs"]
        # same split, iteration directory and file name: <iter>/renders/<name> <-> <iter>/gt/<name>
        rd, name = os.path.split(c["query/img"])
        assert c["query/gt"] == os.path.join(os.path.dirname(rd), "gt", name) and os.path.basename(rd) == "renders"
        assert os.path.exists(c["query/gt"])
        assert c["query/score_map"] == "empty_image"  # metric_map/ is not looked at
    # mse and mae pair the same way
    assert NvsItems(tree, None, "test", CROSS, "mse", 2, compute_gt=True)._index == NvsItems(tree, None, "test", CROSS, "mae", 2, compute_gt=True)._index


def test_walker_compute_mode_does_not_look_at_metric_map(tree, tmp_path):
    from crossscore_amd.nvs import NvsItems

    bad = make_tree(tmp_path / "bad", scenes=["scene_a", "scene_b"])
    os.remove(os.path.join(bad, "res_540", "scene_a", "test", "ours_1000", "metric_map", "ssim", "frame_00001.png"))
    with pytest.raises(ValueError, match="mismatch"):
        NvsItems(bad, None, "test", CROSS, "ssim", 2)
    assert len(NvsItems(bad, None, "test", CROSS, "ssim", 2, compute_gt=True)) == 12


def test_walker_without_compute_mode_yields_todays_dicts(tree):
    from crossscore_amd.nvs import NvsItems

    items = NvsItems(tree, None, "test", CROSS, "ssim", 2)
    for i in range(len(items)):
        it = items[i]
        assert list(it) == ["query/img", "query/score_map", "reference/cross/imgs"]
    assert all(len(e) == 3 for e in items._index)
    a = items[0]
    assert a["query/score_map"].replace("metric_map/ssim", "renders") == a["query/img"]


def test_generator_walks_every_iteration_directory(tree):
    from crossscore_amd.config import load_config
    from crossscore_amd.metric_maps import iteration_dirs, pairs_of

    dirs = iteration_dirs(load_config("default_test", [f"data.dataset.path={tree}"]))
    rel = [os.path.relpath(d, os.path.join(tree, "res_540")) for d in dirs]
    assert rel == ["scene_a/train/ours_1000", "scene_a/train/ours_7000", "scene_a/train/ours_30000", "scene_a/test/ours_1000",
                   "scene_a/test/ours_7000", "scene_a/test/ours_30000", "scene_b/train/ours_1000", "scene_b/test/ours_1000"]
    assert [n for n, _, _ in pairs_of(dirs[0])] == ["frame_00000.png", "frame_00001.png", "frame_00002.png"]
    two = iteration_dirs(load_config("default_test", [f"data.dataset.path={tree}", "data.dataset.num_gaussians_iters=2"]))
    assert len(two) == 6
    with pytest.raises(ValueError, match="data_split"):
        iteration_dirs(load_config("default_test", [f"data.dataset.path={tree}", "this_main.data_split=validation"]))


def test_the_new_source_is_declared_bound_and_built():
    from crossscore_amd import _lib, build

    assert "gtmap.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "gtmap.hip"))
    hdr = open(os.path.join(REPO, "include", "crossscore_hip.h")).read()
    assert re.search(r"\bint\s+cs_op_gt_metric_map_u8\s*\(", hdr)
    assert re.search(r"CS_GTMAP_SSIM\s*=\s*0\s*,\s*CS_GTMAP_MAE\s*=\s*1", hdr)
    assert (_lib.GTMAP_SSIM, _lib.GTMAP_MAE) == (0, 1) and "cs_op_gt_metric_map_u8" in _lib.SYMBOLS
    lib = _lib.load()  # bad arguments are rejected on the host, before anything touches a device
    assert lib.cs_op_gt_metric_map_u8(None, None, 1, 4, 4, 48, 0, None, 4, None) == _lib.CS_ERR_BAD_ARG
