"""Ground-truth metric maps formed on the GPU from the images (cs_op_gt_metric_map_u8).

Op level: every pixel of every case against the fp64 restatement of the definition (tests/gtmap_oracle.py).  The accuracy bar is the error of the
reference form itself -- the same definition as a direct 11 x 11 conv2d in fp32 torch -- recomputed here per case, never taken from the kernel:
    max |kernel - fp64| <= bar,  |mean(kernel) - mean(fp64)| <= bar,  bar = max(max |fp32 direct - fp64|, 1 / 32767)
    per pixel  |code_kernel - code_fp64| <= 1 + ceil(32767 * bar)
The kernel's only output is the stored 16-bit sample, so its value is what a reader of the file sees, code / 32767 - 1, and it is compared with
the fp64 map as stored, codes(fp64) / 32767 - 1 (the 1 / 32767 floor of the bar is one step of that grid: against the unquantised fp64 map
the truncation alone would use it up).  The comparison is made in code units, in integers.  Identical images must give 65534 everywhere.
The test prints, per size and case, the fp32 direct form's error beside the kernel's largest code difference, the number of differing pixels
and max |code / 32767 - 1 + 0.5 / 32767 - fp64| less the truncation's half step (run with -s); DESIGN.md section 6 is where they are recorded.

Driver level: `python -m crossscore_amd.metric_maps` fills a tree without metric_map/, and evaluate with this_main.gt_metric_maps=compute on the
bare tree gives the bits of files mode on the filled one."""
import ctypes as C
import math
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import gtmap_oracle as orc  # noqa: E402
from guard import guarded_out, poisoned_in  # noqa: E402
from nvs_tree import make_tree  # noqa: E402
from scenes import read_csv_dicts, run_evaluate  # noqa: E402

torch = pytest.importorskip("torch")
SSIM, MAE = 0, 1
SIZES = [(1, 1), (7, 9), (11, 11), (60, 84), (270, 363), (540, 720)]


@pytest.fixture(autouse=True)
def _in_tmp(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _op(renders, gts, kind, pad=0, guard=False):
    """codes (B, H, W) int64 on the host; pad: extra samples per output row; guard: guard bands around the output and poison around the inputs"""
    from crossscore_amd import _lib

    lib = _lib.load()
    a = torch.from_numpy(np.stack(renders)).cuda()
    b = torch.from_numpy(np.stack(gts)).cuda()
    B, H, W, _ = a.shape
    if guard:
        a, b = poisoned_in(a.reshape(B, H * W * 3)), poisoned_in(b.reshape(B, H * W * 3))
        out, check = guarded_out((B, H, W), torch.int16, ld=W + pad)
    else:
        out, check = torch.empty((B, H, W + pad), dtype=torch.int16, device="cuda")[:, :, :W], None
    _lib.check(lib.cs_op_gt_metric_map_u8(_p(a), _p(b), B, H, W, H * W * 3, kind, _p(out), W + pad,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    if check is not None:
        check("gt metric map")
    return out.cpu().to(torch.int64) & 0xFFFF


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", SIZES)
def test_ssim_codes_within_the_reference_forms_own_error(h, w):
    pairs = [orc.case_pair(name, h, w) for name in orc.CASES]
    got = _op([p[0] for p in pairs], [p[1] for p in pairs], SSIM, pad=5, guard=True)  # the six cases as one batch
    for i, name in enumerate(orc.CASES):
        a, b = pairs[i]
        ref = orc.ssim_map(a, b)
        f32 = orc.ssim_map(a, b, torch.float32).double()
        err32 = float((f32 - ref).abs().max())
        bar_codes = max(err32 * 32767, 1.0)  # the bar in steps of 1 / 32767
        want = orc.codes(ref)
        d = got[i] - want
        mid = ((got[i].double() + 0.5) / 32767 - 1 - ref).abs().max() - 0.5 / 32767  # the kernel's error with the truncation's half step taken out
        print(f"{h}x{w} {name}: fp32 direct max error {err32:.2e} ({int((orc.codes(f32) - want).abs().max())} codes); kernel: "
              f"{int(d.abs().max())} codes off at most, {int((d != 0).sum())} of {d.numel()} pixels differ, mean difference "
              f"{float(d.double().mean()):+.4f} codes, error beyond truncation {max(float(mid), 0.0):.2e}")
        assert int(d.abs().max()) <= bar_codes, name
        assert abs(float(d.double().mean())) <= bar_codes, name
        assert int(d.abs().max()) <= 1 + math.ceil(bar_codes), name
        if name == "identical":
            assert bool((got[i] == 65534).all())


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", SIZES)
def test_mae_codes_are_the_integer_formula(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    a = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(3)]
    b = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(3)]
    a += [np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8), a[0]]
    b += [np.full((h, w, 3), 255, np.uint8), np.zeros((h, w, 3), np.uint8), a[0]]
    got = _op(a, b, MAE, pad=3, guard=True)
    for i in range(len(a)):
        assert torch.equal(got[i], orc.mae_codes(a[i], b[i])), i
    assert bool((got[3] == 65535).all()) and bool((got[4] == 65535).all()) and bool((got[5] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [SSIM, MAE])
def test_unaligned_images_and_strides(kind):
    """Images that start at every byte alignment, a stride above the image's size, poison between the images: the codes of the aligned call."""
    from crossscore_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(11)
    for h, w in ((7, 9), (33, 70), (16, 65)):
        a = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
        b = np.clip(a.astype(np.int64) + rng.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)
        want = _op(list(a), list(b), kind)
        for off in (1, 2, 3):
            stride = h * w * 3 + 5
            bufs = []
            for src in (a, b):
                buf = torch.full((off + 3 * stride + 64,), 255, dtype=torch.uint8, device="cuda")
                for i in range(3):
                    buf[off + i * stride: off + i * stride + h * w * 3] = torch.from_numpy(src[i].reshape(-1)).cuda()
                bufs.append(buf)
            out = torch.empty((3, h, w), dtype=torch.int16, device="cuda")
            _lib.check(lib.cs_op_gt_metric_map_u8(C.c_void_p(bufs[0].data_ptr() + off), C.c_void_p(bufs[1].data_ptr() + off), 3, h, w, stride, kind,
                                                  _p(out), w, None))
            torch.cuda.synchronize()
            assert torch.equal(out.cpu().to(torch.int64) & 0xFFFF, want), (h, w, off)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [SSIM, MAE])
@pytest.mark.parametrize("h,w", [(60, 84), (270, 363)])
def test_a_map_has_the_same_bits_alone_and_anywhere_in_a_batch(kind, h, w):
    rng = np.random.default_rng(5)
    pair = orc.case_pair("smooth+noise", h, w)
    alone = _op([pair[0]], [pair[1]], kind)[0]
    others = [(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for _ in range(8)]
    for pos in (0, 3, 7):
        batch = list(others)
        batch[pos] = pair
        got = _op([p[0] for p in batch], [p[1] for p in batch], kind)
        assert torch.equal(got[pos], alone), pos


@pytest.mark.gpu
def test_bad_arguments_launch_nothing():
    from crossscore_amd import _lib

    lib = _lib.load()
    a = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    out, check = guarded_out((2, 8, 8), torch.int16)
    f = lib.cs_op_gt_metric_map_u8
    assert f(_p(a), _p(a), 2, 8, 8, 192, 2, _p(out), 8, None) == _lib.CS_ERR_BAD_ARG and b"kind" in lib.cs_last_error()
    assert f(_p(a), _p(a), 0, 8, 8, 192, 0, _p(out), 8, None) == _lib.CS_ERR_BAD_ARG
    assert f(_p(a), _p(a), 1025, 8, 8, 192, 0, _p(out), 8, None) == _lib.CS_ERR_BAD_ARG
    assert f(_p(a), _p(a), 2, 0, 8, 192, 0, _p(out), 8, None) == _lib.CS_ERR_BAD_ARG
    assert f(_p(a), _p(a), 2, 8, 0, 192, 0, _p(out), 8, None) == _lib.CS_ERR_BAD_ARG
    assert f(_p(a), _p(a), 2, 8, 8, 191, 0, _p(out), 8, None) == _lib.CS_ERR_BAD_ARG and b"stride" in lib.cs_last_error()
    assert f(_p(a), _p(a), 2, 8, 8, 192, 1, _p(out), 7, None) == _lib.CS_ERR_BAD_ARG and b"row" in lib.cs_last_error()
    assert f(None, _p(a), 2, 8, 8, 192, 0, _p(out), 8, None) == _lib.CS_ERR_BAD_ARG
    assert f(_p(a), None, 2, 8, 8, 192, 0, _p(out), 8, None) == _lib.CS_ERR_BAD_ARG
    assert f(_p(a), _p(a), 2, 8, 8, 192, 0, None, 8, None) == _lib.CS_ERR_BAD_ARG
    assert f(_p(a), _p(a), 2, 8, 8, 192, 0, C.c_void_p(out.data_ptr() + 1), 8, None) == _lib.CS_ERR_BAD_ARG
    assert f(_p(a), _p(a), 1, 70000, 8, 70000 * 24, 0, _p(out), 8, None) == _lib.CS_ERR_UNSUPPORTED
    check("output of rejected calls")  # (the view holds the sentinel too: nothing was launched)
    assert bool((out.cpu().to(torch.int64) & 0xFFFF == 0xA5A5).all())


# ---- the Python layers ------------------------------------------------------------------------------------------------------------------------
def _stage(short=-1, patches=True):
    from crossscore_amd.data import InputStage

    return InputStage(torch.device("cuda", 0), resize_short_side=short, integer_patches=patches)


@pytest.mark.gpu
def test_input_stage_groups_sizes_and_takes_host_or_device_images():
    from crossscore_amd import _lib

    stage = _stage()
    rng = np.random.default_rng(2)
    shapes = [(60, 84), (30, 40), (60, 84), (60, 84), (30, 40)]
    a = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
    b = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
    for kind in (_lib.GTMAP_SSIM, _lib.GTMAP_MAE):
        host = stage.gt_metric_maps(a, b, kind)
        mixed = stage.gt_metric_maps([torch.from_numpy(x).cuda() if i % 2 else x for i, x in enumerate(a)],
                                     [torch.from_numpy(x).cuda() for x in b], kind)
        for i in range(len(a)):
            want = _op([a[i]], [b[i]], kind)[0]
            assert host[i].dtype == torch.int16 and tuple(host[i].shape) == shapes[i]
            assert torch.equal(host[i].cpu().to(torch.int64) & 0xFFFF, want) and torch.equal(mixed[i], host[i]), (kind, i)
    with pytest.raises(ValueError, match="differ in size"):
        stage.gt_metric_maps([a[0]], [b[1]], 0)
    # metric_maps takes the device maps where they are: the bits of the host-array path, with and without a resize, placeholders between
    from crossscore_amd.data import metric_mode
    for short in (-1, 56):
        st = _stage(short)
        idx = [0, 2, 3]
        dev = stage.gt_metric_maps([a[i] for i in idx], [b[i] for i in idx], _lib.GTMAP_SSIM)
        oh, ow = st.geometry(60, 84)[1][2:]
        for mode in (metric_mode("ssim", 0), metric_mode("ssim", -1)):
            got = torch.empty((4, oh, ow), device="cuda")
            want = torch.empty((4, oh, ow), device="cuda")
            st.metric_maps([dev[0], None, dev[2], dev[1]], [(60, 84)] * 4, mode, got)  # (not consecutive slices: gathered)
            st.metric_maps([dev[0].cpu().numpy().view(np.uint16), None, dev[2].cpu().numpy().view(np.uint16), dev[1].cpu().numpy().view(np.uint16)],
                           [(60, 84)] * 4, mode, want)
            assert torch.equal(got, want)
            st.metric_maps(dev, [(60, 84)] * 3, mode, got[:3])  # consecutive slices of one tensor: used in place
            st.metric_maps([d.cpu().numpy().view(np.uint16) for d in dev], [(60, 84)] * 3, mode, want[:3])
            assert torch.equal(got[:3], want[:3])


@pytest.mark.gpu
def test_compute_mode_gt_stage_does_not_wait_for_the_stream():
    """The pattern of test_metric_maps_do_not_wait_for_the_stream: the images go up from pinned memory and both stages only queue work."""
    from crossscore_amd import _lib

    if not hasattr(torch.cuda, "_sleep"):
        pytest.skip("torch.cuda._sleep is not available")
    rng = np.random.default_rng(4)
    a = [rng.integers(0, 256, (60, 84, 3), dtype=np.uint8) for _ in range(4)]
    b = [rng.integers(0, 256, (60, 84, 3), dtype=np.uint8) for _ in range(4)]
    stage = _stage(56)
    out = torch.empty((4, 56, 70), device="cuda")
    stage.metric_maps(stage.gt_metric_maps(a, b, _lib.GTMAP_SSIM), [(60, 84)] * 4, 1, out)  # tables, pinned blocks and kernels exist from here on
    torch.cuda.synchronize()
    ref = out.clone()
    out.zero_()
    torch.cuda._sleep(200_000_000)  # ~0.1 s of device time ahead of the stage on the current stream
    stage.metric_maps(stage.gt_metric_maps(a, b, _lib.GTMAP_SSIM), [(60, 84)] * 4, 1, out)
    assert not torch.cuda.current_stream().query()  # the host is back while the stream is still busy
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------------
def _strip(tree):
    n = 0
    for root, dirs, _ in os.walk(tree):
        if "metric_map" in dirs:
            shutil.rmtree(os.path.join(root, "metric_map"))
            dirs.remove("metric_map")
            n += 1
    return n


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """(bare, filled): the tree of tests/nvs_tree.py without any metric_map/, and a copy the generator filled (splits test and val)"""
    from crossscore_amd.config import load_config
    from crossscore_amd.metric_maps import generate

    # the score summary names its files after the two directories above res_540: both trees end in nvs/tree
    bare = make_tree(tmp_path_factory.mktemp("bare") / "nvs" / "tree")
    assert _strip(bare) > 0
    filled = str(tmp_path_factory.mktemp("filled") / "nvs" / "tree")
    shutil.copytree(bare, filled)
    res = [generate(load_config("default_test", [f"data.dataset.path={filled}", f"this_main.data_split={s}"])) for s in ("test", "val")]
    return bare, filled, res


def _png_files(tree):
    out = []
    for root, _, files in os.walk(tree):
        if os.sep + "metric_map" + os.sep in root + os.sep:
            out += [os.path.join(root, f) for f in files]
    return sorted(out)


@pytest.mark.gpu
def test_generator_fills_a_bare_tree(trees):
    from PIL import Image

    from crossscore_amd import _lib
    from crossscore_amd.config import load_config
    from crossscore_amd.decode import read_image_u8, read_metric_map_u16
    from crossscore_amd.metric_maps import generate

    bare, filled, res = trees
    assert not _png_files(bare)
    renders = []
    for root, _, files in os.walk(filled):
        if os.path.basename(root) == "renders":
            renders += [os.path.join(root, f) for f in files]
    assert len(renders) == 3 * 3 + 3 * 2 + 2 + 2  # scene_a (3 iterations: 3 train + 2 test images each), scene_b, scene_c
    written = sorted(p for r in res for p in r["written"])
    assert written == _png_files(filled) and len(written) == 2 * len(renders) and not any(r["skipped"] for r in res)
    assert sum(r["png_gpu_files"] for r in res) == len(written) and sum(r["png_host_files"] for r in res) == 0
    stage = _stage()
    for rp in renders:
        a, b = read_image_u8(rp), read_image_u8(rp.replace(os.sep + "renders" + os.sep, os.sep + "gt" + os.sep))
        for sub, kind in (("ssim", _lib.GTMAP_SSIM), ("mae", _lib.GTMAP_MAE)):
            f = rp.replace(os.sep + "renders" + os.sep, os.sep + os.path.join("metric_map", sub) + os.sep)
            im = Image.open(f)
            assert im.mode in ("I;16", "I") and im.size == (a.shape[1], a.shape[0]), f
            dev = stage.gt_metric_maps([a], [b], kind)[0].cpu().numpy().view(np.uint16)
            assert np.array_equal(read_metric_map_u16(f), dev), f
            if kind == _lib.GTMAP_MAE:
                assert np.array_equal(dev.astype(np.int64), orc.mae_codes(a, b).numpy()), f
    # a second run writes nothing; overwrite=True writes the same bytes again
    before = {p: open(p, "rb").read() for p in written}
    again = generate(load_config("default_test", [f"data.dataset.path={filled}"]))
    assert not again["written"] and len(again["skipped"]) == sum(len(r["written"]) for r in res[:1])
    over = generate(load_config("default_test", [f"data.dataset.path={filled}", "this_main.overwrite=True"]))
    assert sorted(over["written"]) == sorted(res[0]["written"]) and not over["skipped"]
    assert all(open(p, "rb").read() == before[p] for p in written)


def _pair(trees, tmp_path, tag, extra, back="synthetic/dinov2-small-2l"):
    """evaluate in compute mode on the bare tree and in files mode on the filled one, same weights -> (compute, files) results and captures"""
    bare, filled, _ = trees
    extra = list(extra) + ["logger.test.write.flag.score_map_gt=True"]
    comp = run_evaluate(bare, tmp_path, f"{tag}_compute", extra + ["this_main.gt_metric_maps=compute"], back=back)
    files = run_evaluate(filled, tmp_path, f"{tag}_files", extra + ["this_main.gt_metric_maps=files"], back=back)
    assert comp[0]["gt_metric_maps"] == "compute" and files[0]["gt_metric_maps"] == "files"
    return comp, files


def _assert_same_run(comp, files):
    from PIL import Image

    (rc, cc, _, _), (rf, cf, _, _) = comp, files
    assert len(cc) == len(cf) > 0
    for x, y in zip(sorted(cc, key=lambda c: c["batch_idx"]), sorted(cf, key=lambda c: c["batch_idx"])):
        assert x["gt"].tobytes() == y["gt"].tobytes() and x["stats"].tobytes() == y["stats"].tobytes(), x["batch_idx"]  # bit-identical
        assert np.array_equal(x["score"], y["score"])
        assert np.isfinite(x["gt"]).all()
    assert open(os.path.join(rc["version_dir"], "metrics.csv")).read() == open(os.path.join(rf["version_dir"], "metrics.csv")).read()
    assert read_csv_dicts(os.path.join(rc["out_dir"], "test_batches.csv")) == read_csv_dicts(os.path.join(rf["out_dir"], "test_batches.csv"))
    rel = lambda r: sorted(os.path.relpath(f, r["out_dir"]) for f in r["files"] if f.startswith(r["out_dir"]))  # noqa: E731
    assert rel(rc) == rel(rf) and any(f.startswith(os.path.join("batch", "score_map_gt")) for f in rel(rc))
    for f in rel(rc):
        if f.endswith(".png"):
            assert np.array_equal(np.array(Image.open(os.path.join(rc["out_dir"], f))), np.array(Image.open(os.path.join(rf["out_dir"], f)))), f


@pytest.mark.gpu
@pytest.mark.parametrize("cache", [True, False])
@pytest.mark.parametrize("fused", [True, False])
def test_evaluate_compute_equals_files_on_the_generated_tree(trees, tmp_path, cache, fused):
    extra = [f"this_main.cache_reference_tokens={cache}", f"this_main.fused_input_stage={fused}"]
    comp, files = _pair(trees, tmp_path, "r", extra)  # 60 x 84 renders, short side 56: the GT stage resizes
    assert comp[0]["input_stage"].startswith("one-pass" if fused else "two-launch")
    _assert_same_run(comp, files)
    comp, files = _pair(trees, tmp_path, "n", extra + ["this_main.resize_short_side=-1"])  # no resize: crop only
    _assert_same_run(comp, files)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [("ssim", 0), ("ssim", -1), ("mae", 0), ("mse", 0)])
def test_evaluate_compute_equals_files_for_every_metric_type_at_540x720(trees, tmp_path, metric):
    extra = [f"model.predict.metric.type={metric[0]}", f"model.predict.metric.min={metric[1]}"]
    comp, files = _pair(trees, tmp_path, "c", extra + ["this_main.data_split=val"])  # scene_c: 540 x 720, resized
    _assert_same_run(comp, files)
    comp, files = _pair(trees, tmp_path, "a", extra + ["this_main.fused_input_stage=False"], back="synthetic/dinov2-tiny")
    _assert_same_run(comp, files)


@pytest.mark.gpu
def test_compute_mode_scores_a_scene_without_metric_maps(tmp_path):
    """scene_b has no metric_map/: files mode scores it against the placeholder (a zero map: no correlation), compute mode for real."""
    tree = make_tree(tmp_path / "t", scenes=["scene_b"])
    files, _, _, _ = run_evaluate(tree, tmp_path, "files", [])
    comp, cap, _, _ = run_evaluate(tree, tmp_path, "compute", ["this_main.gt_metric_maps=compute"])
    assert not np.isfinite(files["metrics"]["test/corr_cross"])
    assert all(np.isfinite(v) for v in comp["metrics"].values())
    assert all(c["gt"].std() > 0 for c in cap)
    assert not os.path.exists(os.path.join(tree, "res_540", "scene_b", "test", "ours_1000", "metric_map"))
    # mae: the placeholder is NaN in files mode
    files, _, _, _ = run_evaluate(tree, tmp_path, "files_mae", ["model.predict.metric.type=mae"])
    comp, _, _, _ = run_evaluate(tree, tmp_path, "compute_mae", ["model.predict.metric.type=mae", "this_main.gt_metric_maps=compute"])
    assert all(np.isnan(v) for v in files["metrics"].values()) and all(np.isfinite(v) for v in comp["metrics"].values())


@pytest.mark.gpu
def test_a_render_and_a_captured_image_of_different_sizes_raise(tmp_path):
    from PIL import Image

    from crossscore_amd.config import load_config
    from crossscore_amd.metric_maps import generate

    tree = make_tree(tmp_path / "t", scenes=["scene_b"])
    g = os.path.join(tree, "res_540", "scene_b", "test", "ours_1000", "gt", "frame_00000.png")
    Image.fromarray(np.zeros((60, 80, 3), np.uint8)).save(g)
    with pytest.raises(ValueError, match=r"renders/frame_00000\.png is 60x84 and .*gt/frame_00000\.png is 60x80"):
        run_evaluate(tree, tmp_path, "bad", ["this_main.gt_metric_maps=compute"])
    with pytest.raises(ValueError, match=r"renders/frame_00000\.png is 60x84 and .*gt/frame_00000\.png is 60x80"):
        generate(load_config("default_test", [f"data.dataset.path={tree}"]))
    with pytest.raises(ValueError, match="gt_metric_maps"):
        run_evaluate(tree, tmp_path, "bad2", ["this_main.gt_metric_maps=both"])
