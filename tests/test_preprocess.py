"""Input stage: oracle vs torch-generated goldens (CPU), HIP kernel vs oracle and goldens (GPU)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import preprocess_oracle as po  # noqa: E402

GOLD = os.path.join(HERE, "golden")
CASES = ["p0_down_45x60_s37", "p1_down_120x90_s40_crop", "p2_up_20x30_s28", "p3_noresize_33x47", "p4_540x720_s518"]


def _image(g):
    h, w, seed = int(g["h"]), int(g["w"]), int(g["seed"])
    rng = np.random.Generator(np.random.PCG64(seed))
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    img[..., 1] = ((np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 2) % 256).astype(np.uint8)
    return img


def _check_against_golden(g, y, tol):
    if "out" in g.files:
        assert y.shape == g["out"].shape
        assert np.abs(y - g["out"]).max() <= tol
    else:
        assert np.abs(y[:, ::97, :] - g["rows"]).max() <= tol
        assert np.abs(y[:, :, ::101] - g["cols"]).max() <= tol
        assert np.abs(y.mean(axis=(1, 2), dtype=np.float64) - g["mean"]).max() <= 1e-6


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_reference_transforms(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    img = _image(g)
    crop = tuple(int(v) for v in g["crop"])
    y = po.preprocess_u8(img, tuple(int(v) for v in g["rs"]), crop if crop[0] >= 0 else None)
    _check_against_golden(g, y, 1.5e-6)  # fp32 vs fp32: differences are summation-order ulps of values of magnitude <= 2.7


def test_resized_output_size_rule():
    assert po.resized_output_size(540, 720, 518) == (518, 690)
    assert po.resized_output_size(720, 540, 518) == (690, 518)
    assert po.resized_output_size(518, 518, 518) == (518, 518)
    assert po.resized_output_size(45, 60, 37) == (37, 49)


def test_filter_table_rows_sum_to_one():
    for n_in, n_out in ((720, 690), (60, 49), (20, 28), (90, 40)):
        xmin, xsize, w = po.aa_axis_table(n_in, n_out)
        assert np.allclose(w.sum(axis=1), 1.0, atol=1e-6)
        assert (xmin >= 0).all() and (xmin + xsize <= n_in).all() and (xsize >= 1).all()


# ------------------------------------------------------------------------------------------------------------------- GPU
def _hip_preprocess(img, rs, crop, mean=po.IMAGENET_MEAN, std=po.IMAGENET_STD, pad_row=0):
    import ctypes as C
    import torch
    from crossscore_amd import _lib

    lib = _lib.load()
    h, w, _ = img.shape
    row = w * 3 + pad_row
    buf = np.zeros((h, row), np.uint8)
    buf[:, : w * 3] = img.reshape(h, w * 3)
    d_img = torch.from_numpy(buf).cuda()
    y0, x0, oh, ow = crop if crop is not None else (0, 0, rs[0], rs[1])
    out = torch.empty((3, oh, ow), dtype=torch.float32, device="cuda")
    scratch = torch.empty((h * rs[1] * 3,), dtype=torch.float32, device="cuda") if tuple(rs) != (h, w) else None
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    _lib.check(lib.cs_op_preprocess_u8(C.c_void_p(d_img.data_ptr()), h, w, row, rs[0], rs[1], y0, x0, oh, ow, m, s, C.c_void_p(out.data_ptr()),
                                      C.c_void_p(scratch.data_ptr()) if scratch is not None else None,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_preprocess_vs_golden_and_oracle(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    img = _image(g)
    rs = tuple(int(v) for v in g["rs"])
    crop = tuple(int(v) for v in g["crop"])
    crop = crop if crop[0] >= 0 else None
    y = _hip_preprocess(img, rs, crop, pad_row=5)
    _check_against_golden(g, y, 2e-6)
    ref = po.preprocess_u8(img, rs, crop)
    assert np.abs(y - ref).max() <= 2e-6
    if rs == img.shape[:2]:  # no resize: the same two IEEE divisions and one subtraction -> bit identical
        assert np.array_equal(y, ref)


@pytest.mark.gpu
def test_hip_preprocess_feeds_forward_bit_identically():
    """Without a resize the kernel's output IS the reference's input tensor, so the score map does not change by a bit."""
    import torch
    from crossscore_amd import synth
    from crossscore_amd.config import model_config
    from crossscore_amd.model import CrossScoreNet

    net = CrossScoreNet(model_config(**{"backbone.from_pretrained": "synthetic/dinov2-tiny"}))
    net.load_numpy_state_dict(synth.make_state_dict(net.arch, 3))
    net = net.cuda()
    rng = np.random.Generator(np.random.PCG64(5))
    imgs = rng.integers(0, 256, size=(3, 70, 84, 3), dtype=np.uint8)  # 1 query + 2 refs
    ref_in = np.stack([po.preprocess_u8(im) for im in imgs])
    hip_in = np.stack([_hip_preprocess(im, (70, 84), None) for im in imgs])
    assert np.array_equal(ref_in, hip_in)
    a = net(torch.from_numpy(ref_in[:1]).cuda(), torch.from_numpy(ref_in[None, 1:]).cuda(), False, 0, False)["score_map_ref_cross"]
    b = net(torch.from_numpy(hip_in[:1]).cuda(), torch.from_numpy(hip_in[None, 1:]).cuda(), False, 0, False)["score_map_ref_cross"]
    assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("backbone,dtype", [("synthetic/dinov2-small-2l", "fp16"), ("synthetic/dinov2-small-2l", "bf16"), ("synthetic/dinov2-base-2l", "fp16")])
def test_forwards_fed_from_uint8_are_bit_identical(backbone, dtype):
    """cs_forward_u8 / cs_encode_references_u8 / cs_forward_cached_u8 (uint8 in, tokens out: the input stage inside the patch-embedding launch)
    against cs_op_preprocess_u8 + the fp32 entry points: score maps, means, attention-weight maps and reference tokens bit for bit; images of
    different decoded sizes in one call, a placeholder reference (data = NULL = zeros before T.Normalize), a geometry the one-pass form refuses."""
    import torch
    from crossscore_amd.config import model_config
    from crossscore_amd.data import InputStage
    from crossscore_amd.model import CrossScoreNet, U8Image
    from crossscore_amd import synth

    net = CrossScoreNet(model_config(**{"backbone.from_pretrained": backbone}))
    net.load_numpy_state_dict(synth.make_state_dict(net.arch, 3))
    net.operand_dtype = dtype
    net = net.cuda()
    dev = torch.device("cuda:0")
    stage = InputStage(dev, resize_short_side=70, integer_patches=True)
    rng = np.random.Generator(np.random.PCG64(11))
    B, N = 2, 2
    # 4:3 images of two decoded sizes, both -> 70 x 93 -> the 70 x 84 window
    sizes = [(120, 160), (90, 120), (120, 160), (150, 200), (90, 120), (120, 160)]
    imgs = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
    size = stage.geometry(*sizes[0])[1][2:]
    assert all(stage.geometry(h, w)[1][2:] == size for h, w in sizes) and size == (70, 84)
    q32 = torch.empty((B, 3) + size, device=dev)
    r32 = torch.empty((B, N, 3) + size, device=dev)
    for b in range(B):
        stage(imgs[b], q32[b])
    refs_u8 = []
    for b in range(B):
        for n in range(N):
            if (b, n) == (1, 1):  # a placeholder of a short reference list
                r32[b, n] = stage.zero_image_value[:, None, None]
                refs_u8.append(stage.placeholder(size))
            else:
                stage(imgs[B + b * N + n], r32[b, n])
                refs_u8.append(stage.describe(imgs[B + b * N + n]))
    q_u8 = stage.batch([stage.describe(imgs[b]) for b in range(B)], size)
    r_u8 = stage.batch(refs_u8, size)
    assert net.u8_input_supported(q_u8.images[0], size)
    want = net(q32, r32, True, 3, False, return_mean=True)
    got = net.forward(q_u8, r_u8, True, 3, return_mean=True)
    torch.cuda.synchronize()
    for k in ("score_map_ref_cross", "score_mean_ref_cross", "attn_weights_map_ref_cross"):
        assert torch.equal(got[k], want[k]), k
    tok32 = net.encode_references(r32.reshape((B * N, 3) + size))
    tok_u8 = net.encode_references(r_u8)
    assert torch.equal(tok_u8, tok32)
    cached = net.forward_cached(q_u8, tok_u8.reshape((B, N) + tuple(tok_u8.shape[1:])), False, 0, True)
    torch.cuda.synchronize()
    assert torch.equal(cached["score_map_ref_cross"], want["score_map_ref_cross"]) and torch.equal(cached["score_mean_ref_cross"], want["score_mean_ref_cross"])
    stats = net.forward_stats()
    assert stats["kernels"].get("patch_u8", 0) >= 1 and "patch" not in stats["kernels"], stats["kernels"]
    # the filter-table cache holds 64 geometries and is dropped as a whole behind a device synchronisation when a 65th arrives: 70 other geometries
    # later the same call rebuilds what it needs and gives the same bits
    for k in range(70):
        net.u8_input_supported(U8Image(None, 200 + k, 260, (70 + 14 * (k % 3), 98), 0, 0), (70, 98), dev)
    again = net.forward(q_u8, r_u8, True, 3, return_mean=True)
    torch.cuda.synchronize()
    assert torch.equal(again["score_map_ref_cross"], want["score_map_ref_cross"])
    # a 114 x down-scale: 14 pixel rows reach 1 800 source rows, more than the launch holds for even one patch per run (1 170)
    far = U8Image(None, 8000, 9600, (70, 84), 0, 0)
    assert not net.u8_input_supported(far, size, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,short,crop,pad", [
    (70, 84, 0, None, 0),              # no resize (identity tables), 5 x 6 patches
    (90, 131, 70, None, 3),            # down 1.29 x, window 70 x 98 of the 70 x 101 image (integer patches), padded source rows
    (45, 60, 98, (5, 10, 84, 112), 0), # up 2.2 x, crop window off the corner
    (300, 410, 56, None, 1),           # down 5.4 x: 14 pixel rows reach 87 source rows
    (777, 1036, 518, None, 0),         # the BASELINE geometry from a 4:3 photo: 518 x 686 window, 37 x 49 patches -> two runs per patch row
    (2100, 2100, 518, None, 0),        # down 4.05 x at full width: the run is cut so that the source rows fit the LDS buffer
])
def test_patch_embedding_straight_from_uint8_is_bit_identical(h, w, short, crop, pad):
    """SURVEY.md 8f-4 as worded (uint8 in, tokens out; task/predict.py:68-93, nvs_dataset.py:218-241): the one-pass form repeats the operations of
    cs_op_preprocess_u8 inside the patch-embedding launch, so its token rows are those of the two-launch path bit for bit -- whatever the scale,
    the crop, the row padding and the number of runs a patch row is cut into."""
    rs = po.resized_output_size(h, w, short) if short else (h, w)
    if crop is None:
        crop = (0, 0, rs[0] - rs[0] % 14, rs[1] - rs[1] % 14)
    if crop[3] % 2:
        crop = (crop[0], crop[1], crop[2], crop[3] - 14)  # (the one-launch patch embedding takes even widths)
    _one_pass_against_two_launches(h, w, rs, crop, pad)


def _one_pass_against_two_launches(h, w, rs, crop, pad, bf16=False, Cc=384):
    """tokens of cs_op_patch_embed_fused_u8 == tokens of cs_op_preprocess_u8 + cs_op_patch_embed_fused, two images, bit for bit"""
    import torch
    import hip_helpers as hh

    P = 14
    rng = np.random.Generator(np.random.PCG64(h * 7 + w))
    imgs = rng.integers(0, 256, size=(2, h, w, 3), dtype=np.uint8)
    imgs[1, ..., 1] = ((np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 2) % 256).astype(np.uint8)
    y0, x0, H, W = crop
    two = np.stack([_hip_preprocess(im, rs, crop, pad_row=pad) for im in imgs])
    wgt = torch.from_numpy((rng.standard_normal((Cc, 3, P, P)) / 24).astype(np.float32)).cuda()
    bias = torch.from_numpy(rng.standard_normal(Cc).astype(np.float32)).cuda()
    pos = torch.from_numpy(rng.standard_normal((1 + (H // P) * (W // P), Cc)).astype(np.float32)).cuda()
    buf = np.zeros((2, h, w * 3 + pad), np.uint8)
    buf[:, :, : w * 3] = imgs.reshape(2, h, w * 3)
    with hh.switches(bf16=bf16):
        ref = hh.patch_embed_fused(torch.from_numpy(two).cuda(), wgt, bias, pos, P)
        got = hh.patch_embed_fused_u8(torch.from_numpy(buf).cuda(), rs, (y0, x0, H, W, w), po.IMAGENET_MEAN, po.IMAGENET_STD, wgt, bias, pos, P)
        torch.cuda.synchronize()
    assert torch.isfinite(got[1:1 + (H // P) * (W // P)]).all()
    assert torch.equal(got, ref)


U8_TMP_BYTES, U8_MAX_RUN = 64 * 1024, 48  # csrc/patch.hip: the one-pass form's horizontal-pass buffer in LDS, patches per workgroup


def _row_span(in_h, rs_h, crop_y, H, P=14):
    """source rows a patch row reaches (first tap of its first pixel row .. last tap of its last), the largest over the window's patch rows"""
    ymin, ysize, _ = po.aa_axis_table(in_h, rs_h)
    return max(int((ymin[r0:r0 + P] + ysize[r0:r0 + P]).max() - ymin[r0]) for r0 in range(crop_y, crop_y + H - P + 1, P))


def _u8_runs(W, span, P=14):
    """patches per run of a patch row: as few runs as hold span source rows x run width fp32 in the buffer, of near-equal size; None: not even one patch"""
    gw = W // P
    for nsx in range(-(-gw // U8_MAX_RUN), gw + 1):
        if span * -(-gw // nsx) * P * 4 <= U8_TMP_BYTES:
            return [gw // nsx + (1 if k < gw % nsx else 0) for k in range(nsx)]
    return None


def _xsize_max(in_w, rs_w, crop_x, W):
    return int(po.aa_axis_table(in_w, rs_w)[1][crop_x:crop_x + W].max())


# name: (h, w, rs, window (y, x, H, W), pad, bf16, the property the case is there for: f(span, runs) -> bool)
_wide = {37: [37], 38: [38], 48: [48], 49: [25, 24], 95: [48, 47], 96: [48, 48], 97: [33, 32, 32]}
U8_EDGES = {
    # 14 pixel rows reach all 1 170 source rows: one patch per run, the x / 255 table exactly 64 KiB into LDS
    "at_the_limit": (1170, 60, (14, 28), (0, 0, 14, 28), 0, False, lambda span, runs: span == 1170 and runs == [1, 1] and (span * 14 * 4 + 255) // 256 * 256 == U8_TMP_BYTES),
    "unequal_runs": (500, 120, (14, 98), (0, 0, 14, 98), 1, False, lambda span, runs: 390 < span <= 585 and runs == [2, 2, 2, 1]),
    "unequal_runs_bf16": (500, 120, (14, 98), (0, 0, 14, 98), 1, True, lambda span, runs: runs == [2, 2, 2, 1]),
    # the width pass keeps up to 8 weights in registers and loops over the table from 9 taps on.  A scale s reaches floor(2 s) + 1 taps (2 s when
    # that is an integer): 343 -> 98 (3.5 x) has 7, 350 -> 98 has 8 (the register path at its limit), 393 -> 98 (4.01 x) has columns of 8 and of 9
    # taps side by side, so both paths run in one launch
    "taps_7": (20, 343, (14, 98), (0, 0, 14, 98), 0, False, lambda span, runs: _xsize_max(343, 98, 0, 98) == 7),
    "register_path": (20, 350, (14, 98), (0, 0, 14, 98), 0, False, lambda span, runs: _xsize_max(350, 98, 0, 98) == 8),
    "loop_path": (20, 393, (14, 98), (0, 0, 14, 98), 0, False, lambda span, runs: _xsize_max(393, 98, 0, 98) == 9),
    "loop_path_bf16": (20, 393, (14, 98), (0, 0, 14, 98), 5, True, lambda span, runs: _xsize_max(393, 98, 0, 98) == 9),
    # 3 x up: consecutive resized rows start at the same source row
    "up_3x": (10, 20, (30, 60), (0, 0, 28, 56), 0, False, lambda span, runs: (np.diff(po.aa_axis_table(10, 30)[0][:28]) == 0).any()),
    # the window ends on the last resized row and column: the clamped last taps
    "bottom_right": (100, 160, (45, 72), (17, 16, 28, 56), 3, False, lambda span, runs: 17 + 28 == 45 and 16 + 56 == 72),
}
for _gw, _runs in _wide.items():  # no resize, one patch row: the LDS layout changes between 37 and 38 patches per run, a run holds 48
    U8_EDGES[f"wide_{_gw}"] = (14, 14 * _gw, (14, 14 * _gw), (0, 0, 14, 14 * _gw), 0, False, lambda span, runs, want=_runs: span == 14 and runs == want)
# C = 768: the uint8 form's second 384-column pass (it shares phases B and C with the float form), on two unequal runs
U8_EDGES["wide_49_two_passes"] = U8_EDGES["wide_49"]
U8_EDGE_WIDTH = {"wide_49_two_passes": 768}  # every other case: 384


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(U8_EDGES))
def test_patch_embedding_straight_from_uint8_at_its_edges(name):
    """The one-pass form where its code changes path: the largest row span it holds, runs of unequal length, 8 and 9 taps (registers / loop), an
    up-scale, a window in the bottom-right corner, patch rows of 37 .. 97 patches.  Each case first proves, from the oracle's table, that it is
    where it claims to be; the assertion is that of test_patch_embedding_straight_from_uint8_is_bit_identical."""
    h, w, rs, crop, pad, bf16, prop = U8_EDGES[name]
    span = _row_span(h, rs[0], crop[0], crop[2])
    assert prop(span, _u8_runs(crop[3], span)), (span, _u8_runs(crop[3], span))
    _one_pass_against_two_launches(h, w, rs, crop, pad, bf16, U8_EDGE_WIDTH.get(name, 384))


@pytest.mark.gpu
def test_patch_embedding_straight_from_uint8_refuses_one_row_past_the_limit():
    """1 171 source rows under one patch row do not fit even one patch per run: cs_op_patch_embed_fused_u8 says CS_ERR_UNSUPPORTED and writes
    nothing, cs_u8_input_supported says 0 (and 1 at 1 170)."""
    import ctypes as C
    import torch
    import guard
    from crossscore_amd import _lib, synth
    from crossscore_amd.config import model_config
    from crossscore_amd.model import CrossScoreNet, U8Image

    h, w, rs, P, Cc = 1171, 60, (14, 28), 14, 384
    span = _row_span(h, rs[0], 0, 14)
    assert span == 1171 and _u8_runs(28, span) is None and _u8_runs(28, span - 1) == [1, 1]
    rng = np.random.Generator(np.random.PCG64(1171))
    imgs = torch.from_numpy(rng.integers(0, 256, size=(2, h, w * 3), dtype=np.uint8)).cuda()
    wgt = torch.from_numpy((rng.standard_normal((Cc, 3, P, P)) / 24).astype(np.float32)).cuda()
    bias = torch.from_numpy(rng.standard_normal(Cc).astype(np.float32)).cuda()
    pos = torch.from_numpy(rng.standard_normal((1 + 2, Cc)).astype(np.float32)).cuda()
    gg = guard.guarded((2 * (1 + 2), Cc), torch.float32)
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.cs_op_patch_embed_fused_u8(p(imgs), 2, h, w, w * 3, rs[0], rs[1], 0, 0, 14, 28, (C.c_float * 3)(*po.IMAGENET_MEAN),
                                        (C.c_float * 3)(*po.IMAGENET_STD), p(wgt), p(bias), p(pos), P, Cc, p(gg.view),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.CS_ERR_UNSUPPORTED, (rc, _lib.last_error())
    gg.check("refused launch")
    assert (gg.view.view(torch.int32) == gg.sentinel).all()
    net = CrossScoreNet(model_config(**{"backbone.from_pretrained": "synthetic/dinov2-small-2l"}))
    net.load_numpy_state_dict(synth.make_state_dict(net.arch, 3))
    net = net.cuda()
    dev = torch.device("cuda:0")
    assert not net.u8_input_supported(U8Image(None, 1171, 60, rs, 0, 0), (14, 28), dev)
    assert net.u8_input_supported(U8Image(None, 1170, 60, rs, 0, 0), (14, 28), dev)


@pytest.mark.gpu
def test_hip_preprocess_bad_arguments():
    img = np.zeros((20, 30, 3), np.uint8)
    with pytest.raises(Exception):
        _hip_preprocess(img, (20, 30), (0, 0, 21, 30))  # crop window outside the image
    with pytest.raises(Exception):
        _hip_preprocess(img, (20, 30), None, std=(0.2, 0.0, 0.2))
