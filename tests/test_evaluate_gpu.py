"""Test phase on the GPU: the GT input stage (cs_op_metric_map_u16) against the reference's goldens, the score-vs-GT sums
(cs_op_score_gt_stats) against numpy fp64, and crossscore_amd.evaluate end to end on the tree of tests/nvs_tree.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from nvs_tree import make_tree  # noqa: E402
from scenes import read_csv_dicts, run_evaluate  # noqa: E402

torch = pytest.importorskip("torch")
MAPS = os.path.join(HERE, "golden", "n0_nvs_maps.npz")
MODES = {"ssim_-1_1": 0, "ssim_0_1": 1, "mae": 2, "mse": 3}


@pytest.fixture(autouse=True)
def _in_tmp(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)  # the log/<now>/test_empty_ckpt/version_<n> directories land here


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp("nvs"))


def _stage(short, integer_patches):
    from crossscore_amd.data import InputStage

    return InputStage(torch.device("cuda", 0), resize_short_side=short, integer_patches=integer_patches)


def _map_path(tree, query_rel, mode):
    sub = "metric_map/ssim" if mode.startswith("ssim") else "metric_map/mae"
    return os.path.join(tree, query_rel.replace("renders", sub))


@pytest.mark.gpu
@pytest.mark.parametrize("case,short,patches", [("a_noresize", -1, True), ("a_s518", 518, True), ("a_s37", 37, False), ("c_s518", 518, True)])
@pytest.mark.parametrize("mode", list(MODES))
def test_metric_map_kernel_matches_reference(tree, case, short, patches, mode):
    from crossscore_amd.decode import read_metric_map_u16

    g = np.load(MAPS)
    key = f"{case}/{mode}"
    m = read_metric_map_u16(_map_path(tree, str(g[key + "/query"]), mode))
    stage = _stage(short, patches)
    shape = tuple(int(v) for v in g[key + "/shape"])
    out = torch.empty(shape, dtype=torch.float32, device="cuda")
    stage.metric_map(m, m.shape, MODES[mode], out)
    y = out.cpu().numpy()
    if short < 0:  # no resize: the reference's float map, bit for bit
        assert np.array_equal(y, g[key + "/out"])
    elif key + "/out" in g.files:
        assert np.abs(y - g[key + "/out"]).max() <= 2e-6
    else:
        assert np.abs(y[::74] - g[key + "/rows"]).max() <= 2e-6
        assert np.abs(y[:, ::83] - g[key + "/cols"]).max() <= 2e-6
        assert abs(y.mean(dtype=np.float64) - float(g[key + "/mean"])) <= 1e-6


@pytest.mark.gpu
def test_metric_map_placeholders_and_bad_arguments():
    from crossscore_amd import _lib

    stage = _stage(56, True)
    for mode, want in MODES.items():
        out = torch.full((56, 70), 7.0, device="cuda")
        stage.metric_map(None, (60, 84), want, out)
        y = out.cpu().numpy()
        assert (np.isnan(y).all() if mode in ("mae", "mse") else (y == 0).all()), mode
    lib = _lib.load()
    m = torch.zeros((60, 84), dtype=torch.int16, device="cuda")
    out = torch.empty((56, 70), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.cs_op_metric_map_u16(p(m), 1, 60, 84, 84, 4, 60, 84, 0, 0, 56, 70, p(out), None, st) == _lib.CS_ERR_BAD_ARG
    assert b"mode" in lib.cs_last_error()
    assert lib.cs_op_metric_map_u16(p(m), 1, 60, 84, 84, 0, 60, 84, 5, 0, 56, 70, p(out), None, st) == _lib.CS_ERR_BAD_ARG  # crop outside
    assert lib.cs_op_metric_map_u16(p(m), 1, 60, 84, 80, 0, 60, 84, 0, 0, 56, 70, p(out), None, st) == _lib.CS_ERR_BAD_ARG  # stride < width
    assert lib.cs_op_metric_map_u16(p(m), 1, 60, 84, 84, 0, 56, 78, 0, 0, 56, 70, p(out), None, st) == _lib.CS_ERR_BAD_ARG  # resize, no scratch
    assert b"scratch" in lib.cs_last_error()
    assert lib.cs_op_metric_map_u16(p(m), 0, 60, 84, 84, 0, 60, 84, 0, 0, 56, 70, p(out), None, st) == _lib.CS_ERR_BAD_ARG  # no map
    with pytest.raises(ValueError, match="differ in size"):
        stage.metric_map(np.zeros((60, 80), np.uint16), (60, 84), 0, out)


@pytest.mark.gpu
@pytest.mark.parametrize("short", [-1, 56])
def test_metric_maps_batched_equal_one_at_a_time(tree, short):
    """One launch pair over a batch (maps of two source sizes, placeholders between them) gives each map's bits of the one-map call."""
    from crossscore_amd.decode import read_metric_map_u16

    stage = _stage(short, True)
    base = os.path.join(tree, "res_540", "scene_a", "test")
    small = [read_metric_map_u16(os.path.join(base, it, "metric_map", "mae", f"frame_{i:05d}.png")) for it in ("ours_1000", "ours_7000")
             for i in range(2)]
    other = np.ascontiguousarray(small[0][:, 2:])  # 60 x 82: another source size, the same processed size with integer patches
    maps = [small[0], None, other, small[1], small[2], None, small[3]]
    hws = [m.shape if m is not None else (60, 84) for m in maps]
    oh, ow = stage.geometry(60, 84)[1][2:]
    if stage.geometry(60, 82)[1][2:] != (oh, ow):
        maps[2], hws[2] = small[2], small[2].shape
    out = torch.empty((len(maps), oh, ow), device="cuda")
    stage.metric_maps(maps, hws, 2, out)
    for b, (m, hw) in enumerate(zip(maps, hws)):
        one = torch.empty((oh, ow), device="cuda")
        stage.metric_map(m, hw, 2, one)
        assert np.array_equal(out[b].cpu().numpy(), one.cpu().numpy(), equal_nan=True), b


@pytest.mark.gpu
def test_metric_maps_do_not_wait_for_the_stream(tree):
    """The GT stage queues behind work already on the stream without waiting for it (pinned, non-blocking uploads)."""
    from crossscore_amd.decode import read_metric_map_u16

    if not hasattr(torch.cuda, "_sleep"):
        pytest.skip("torch.cuda._sleep is not available")
    m = read_metric_map_u16(os.path.join(tree, "res_540", "scene_a", "test", "ours_1000", "metric_map", "ssim", "frame_00000.png"))
    stage = _stage(56, True)
    out = torch.empty((4, 56, 70), device="cuda")
    stage.metric_maps([m] * 4, [m.shape] * 4, 1, out)  # tables, pinned blocks and kernels exist from here on
    torch.cuda.synchronize()
    torch.cuda._sleep(200_000_000)  # ~0.1 s of device time ahead of the stage on the current stream
    stage.metric_maps([m, None, m, m], [m.shape] * 4, 1, out)
    assert not torch.cuda.current_stream().query()  # the host is back while the stream is still busy
    torch.cuda.synchronize()
    ref = torch.empty((56, 70), device="cuda")
    stage.metric_map(m, m.shape, 1, ref)
    assert torch.equal(out[0], ref) and torch.equal(out[3], ref) and (out[1] == 0).all()


def _stats(score, gt):
    from crossscore_amd import _lib

    lib = _lib.load()
    B, H, W = score.shape
    out = torch.empty((B, 6), dtype=torch.float64, device="cuda")
    scratch = torch.empty((lib.cs_score_gt_workspace_bytes(B, H, W),), dtype=torch.uint8, device="cuda")
    _lib.check(lib.cs_op_score_gt_stats(C.c_void_p(score.data_ptr()), C.c_void_p(gt.data_ptr()), B, H, W, C.c_void_p(out.data_ptr()),
                                        C.c_void_p(scratch.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out.cpu().numpy()


def _np_sums(s, g):
    s, g = s.astype(np.float64), g.astype(np.float64)
    return np.stack([np.abs(s - g).sum((1, 2)), s.sum((1, 2)), g.sum((1, 2)), (s * s).sum((1, 2)), (g * g).sum((1, 2)),
                     (s * g).sum((1, 2))], 1)


@pytest.mark.gpu
def test_score_gt_stats_kernel():
    from crossscore_amd import _lib

    rng = np.random.default_rng(5)
    B, H, W = 5, 518, 518  # 66 slabs per image
    s = rng.random((B, H, W), dtype=np.float32)
    g = (0.7 * s + 0.3 * rng.random((B, H, W), dtype=np.float32) - 0.1).astype(np.float32)
    got = _stats(torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda())
    want = _np_sums(s, g)
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    # one image alone and at the first and last position of a batch: the same bits
    alone = _stats(torch.from_numpy(s[2:3]).cuda(), torch.from_numpy(g[2:3]).cuda())
    for pos in (0, B - 1):
        idx = [2] + [i for i in range(B) if i != 2]
        if pos:
            idx = idx[1:] + idx[:1]
        perm = _stats(torch.from_numpy(s[idx]).cuda(), torch.from_numpy(g[idx]).cuda())
        assert np.array_equal(perm[pos], alone[0])
    # a small map (one partial slab) and NaN propagation
    s2, g2 = s[:2, :7, :9].copy(), g[:2, :7, :9].copy()
    g2[1, 3, 3] = np.nan
    got = _stats(torch.from_numpy(s2).cuda(), torch.from_numpy(g2).cuda())
    assert np.allclose(got[0], _np_sums(s2, g2)[0], rtol=1e-12, atol=0)
    assert np.isnan(got[1, [0, 2, 4, 5]]).all() and np.isfinite(got[1, [1, 3]]).all()
    lib = _lib.load()
    x = torch.zeros((1, 4, 4), device="cuda")
    assert lib.cs_op_score_gt_stats(C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()), 0, 4, 4, C.c_void_p(x.data_ptr()),
                                    C.c_void_p(x.data_ptr()), None) == _lib.CS_ERR_BAD_ARG
    assert lib.cs_op_score_gt_stats(C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()), 1, 4, 4, C.c_void_p(x.data_ptr()), None,
                                    None) == _lib.CS_ERR_BAD_ARG


@pytest.mark.gpu
def test_evaluate_end_to_end(tree, tmp_path):
    from PIL import Image

    from crossscore_amd.data import InputStage
    from crossscore_amd.decode import read_image_u8
    from crossscore_amd.evaluate import batch_metrics
    from crossscore_amd.writers import ScoreMapEncoder
    from oracle import crossscore_oracle as orc

    res, cap, sd, arch = run_evaluate(tree, tmp_path, "out", ["logger.test.write.flag.score_map_gt=True"])
    assert res["version_dir"] == os.path.join("log", "NOW", "test_empty_ckpt", "version_0")
    assert len(cap) == 3 and sum(c["gt"].shape[0] for c in cap) == 12  # 12 items in batches of 4
    # per-batch metrics from the kernel's sums = an fp64 recomputation from the run's own score and GT maps
    for c, row in zip(sorted(cap, key=lambda c: c["batch_idx"]), res["batches"]):
        want = batch_metrics(_np_sums(c["score"], c["gt"]), c["gt"].shape[1] * c["gt"].shape[2])
        s, g = c["score"].astype(np.float64).ravel(), c["gt"].astype(np.float64).ravel()
        assert row["loss"] == pytest.approx(np.abs(s - g).mean(), rel=1e-9)
        assert row["corr"] == pytest.approx(np.corrcoef(s, g)[0, 1], rel=1e-9)
        assert row["psnr"] == pytest.approx(-10 * np.log10(np.abs(s - g).mean() ** 2), rel=1e-9)
        assert all(row[k] == pytest.approx(want[k], rel=1e-12) for k in ("loss", "corr", "psnr"))
    # metrics.csv = the batch-size-weighted mean of test_batches.csv
    m = read_csv_dicts(os.path.join(res["version_dir"], "metrics.csv"))[0]
    rows = read_csv_dicts(os.path.join(res["out_dir"], "test_batches.csv"))
    w = np.array([float(r["batch_size"]) for r in rows])
    for col, key in (("loss", "test/loss"), ("corr", "test/corr_cross"), ("psnr", "test/psnr_cross")):
        assert float(m[key]) == pytest.approx((w * np.array([float(r[col]) for r in rows])).sum() / w.sum(), rel=1e-12)
    assert m["test/loss"] == m["test/loss_cross"]
    # the score maps against the oracle pipeline (InputStage's processed images -> fp32 forward) at the forward's bound
    stage = InputStage(torch.device("cuda", 0), resize_short_side=56, integer_patches=True)
    W = orc.to_torch({k: v.numpy() for k, v in sd.items()})
    c = cap[0]
    q = torch.empty((4, 3, 56, 70), device="cuda")
    r = torch.empty((4, 5, 3, 56, 70), device="cuda")
    for b, qp in enumerate(c["item_paths"]["query/img"]):
        stage(read_image_u8(qp), q[b])
        for n, rp in enumerate(c["item_paths"]["reference/cross/imgs"]):
            if rp[b] == "empty_image":
                r[b, n] = stage.zero_image_value[:, None, None]
            else:
                stage(read_image_u8(rp[b]), r[b, n])
    ref = orc.forward(W, dict(enc_heads=arch.enc_heads, pos_interp_legacy=True), q.cpu(), r.cpu(), False, 0)["score_map_ref_cross"].numpy()
    assert np.abs(c["score"] - ref).mean() < 1e-3
    # the score_map_gt PNGs are the encoder's images of the stage's GT maps
    enc = ScoreMapEncoder("ssim", 0, 1, "gray", torch.device("cuda", 0))
    for c in cap:
        want = enc(torch.from_numpy(c["gt"]).cuda())
        for b, qp in enumerate(c["item_paths"]["query/img"]):
            from crossscore_amd.writers import name_stem
            f = os.path.join(res["out_dir"], "batch", "score_map_gt", f"r0_B{c['batch_idx']:04}_b{b:03}_{name_stem(qp)}.png")
            assert np.array_equal(np.array(Image.open(f)).astype(np.int64), want[b].astype(np.int64)), f
    assert os.path.isdir(os.path.join(res["out_dir"], "score_summary")) and os.path.isdir(os.path.join(res["out_dir"], "batch", "item_path_json"))


@pytest.mark.gpu
def test_evaluate_input_paths_give_identical_metrics(tree, tmp_path):
    """cached / uncached reference tokens x one-pass / two-launch input stage (ViT-S width: the one-pass form's): the same bits."""
    back = "synthetic/dinov2-small-2l"
    got = {}
    for cache in (True, False):
        for fused in (True, False):
            res, cap, _, _ = run_evaluate(tree, tmp_path, f"o_{cache}_{fused}", [f"this_main.cache_reference_tokens={cache}",
                                                                                 f"this_main.fused_input_stage={fused}"], back=back)
            assert res["input_stage"].startswith("one-pass" if fused else "two-launch")
            got[(cache, fused)] = (res["metrics"], [r for r in res["batches"]], [c["score"] for c in cap])
    base = got[(True, True)]
    for k, v in got.items():
        assert v[0] == base[0] and v[1] == base[1], k
        assert all(np.array_equal(a, b) for a, b in zip(v[2], base[2])), k


@pytest.mark.gpu
def test_evaluate_nan_gt_and_crop_errors(tree, tmp_path):
    # mae: scene_b has no metric maps -> NaN placeholders -> that batch's values and the epoch values are NaN (not filtered)
    res, cap, _, _ = run_evaluate(tree, tmp_path, "mae", ["model.predict.metric.type=mae", "data.loader.validation.shuffle=False"])
    assert np.isnan(res["batches"][-1]["loss"]) and np.isfinite(res["batches"][0]["loss"])
    assert all(np.isnan(v) for v in res["metrics"].values())
    # crop_mode null with sides that are not whole patches: ValueError, as the reference fails in the L1 broadcast
    with pytest.raises(ValueError, match="crop_mode null"):
        run_evaluate(tree, tmp_path, "nocrop", ["this_main.crop_mode=null"])
