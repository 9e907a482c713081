"""The constructions of tests/patch_tile_data.py have the properties tests/test_hip_patch_tiles.py relies on (no GPU): the run lists of the
geometry table, exactness of the integer case in fp16, bf16 and fp32, slot coverage of the one-hot maps, and the sensitivity of the bit-exact and
the bounded test to the faults they are there for."""
import numpy as np
import pytest
import torch

import patch_tile_data as ptd

F32 = np.float32


def test_run_lists_of_the_geometry_table():
    """runs, first patches, LDS layout and row tiles by the arithmetic of cs_patch_fused_launch and the kernel's block decoding"""
    for gw, want in ptd.GW_TABLE.items():
        assert ptd.runs(gw) == want, (gw, ptd.runs(gw))
        st = ptd.run_starts(gw)
        assert st[0] == 0 and all(st[i] + want[i] == (st[i + 1] if i + 1 < len(st) else gw) for i in range(len(st)))
    assert ptd.row_tiles(1) == (1, 15)
    assert [ptd.row_tiles(n) for n in (15, 16, 17)] == [(1, 1), (1, 0), (2, 15)]
    assert [ptd.row_tiles(n) for n in (31, 32, 33)] == [(2, 1), (2, 0), (3, 15)]
    assert ptd.row_tiles(37) == (3, 11) and ptd.row_tiles(48) == (3, 0)
    # the layout switches between 37 and 38 patches per run; at 37 the dead rows 37..47 of tile 2 lie in the waves' epilogue patches
    assert ptd.layout(37) == (37, 37, 37 * 1296) and ptd.layout(38) == (38, 48, 48 * 1296) and ptd.layout(48)[1] == 48
    assert ptd.layout(49) == (25, 37, 37 * 1296) and ptd.layout(97) == (33, 37, 37 * 1296)
    assert ptd.run_starts(49) == [0, 25] and ptd.run_starts(97) == [0, 33, 65]
    assert all(max(ptd.runs(gw)) <= ptd.MAXNP for gw in range(1, 400))


@pytest.mark.parametrize("gw", list(ptd.GW_TABLE))
def test_integer_case_is_exact_in_every_format(gw):
    I, gh = 3, 2
    x = ptd.integer_images(I, gh, gw, 100 + gw)
    H, W = ptd.image_size(gh, gw, 5, 2)
    assert x.shape == (I, 3, H, W) and W % 2 == 0
    assert np.isnan(x[:, :, gh * 14:, :]).all() and np.isnan(x[:, :, :, gw * 14:]).all()
    pt = ptd.patches(x, gh, gw).astype(np.float64)
    assert np.isfinite(pt).all() and (pt == np.round(pt)).all() and np.abs(pt).max() <= 13
    sums = pt.reshape(I, gh * gw, 3, 196).sum(-1)
    assert (sums % 49 == 0).all()
    mu = sums / 196.0
    assert (4 * mu == np.round(4 * mu)).all()
    cen = pt - np.repeat(mu, 196, axis=2)
    # multiples of 1/4 below 16: six significant bits, exact in bf16 (8) and fp16 (11)
    assert np.abs(cen).max() < 16 and (4 * cen == np.round(4 * cen)).all()
    # the fixed-order fp32 mean is the exact one; the centred values survive the round trip through both operand types
    assert np.array_equal(ptd.mean_f32(x, gh, gw).astype(np.float64), mu)
    c32 = cen.astype(F32)
    assert np.array_equal(c32.astype(np.float64), cen)
    for bf16 in (False, True):
        assert np.array_equal(ptd.round16(c32, bf16), c32)
    t = torch.from_numpy(c32)
    assert torch.equal(t.to(torch.float16).float(), t) and torch.equal(t.to(torch.bfloat16).float(), t)
    for C in (384, 768):
        w, b, pos = ptd.integer_operands(C, 1 + gh * gw, 7 + C)
        assert set(np.unique(w).tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
        assert (4 * b == np.round(4 * b)).all() and (4 * pos == np.round(4 * pos)).all()
        assert np.unique(pos).size == pos.size  # a different value at every (token row, column)
        for bf16 in (False, True):
            assert np.array_equal(ptd.round16(w, bf16), w)
        big = ptd.largest_partial_sum(x, w, b, pos, gh, gw)
        assert big < 2.0 ** 22, big
        ref = ptd.conv64(x, w, b, pos, gh, gw)
        assert np.array_equal(ref.astype(F32).astype(np.float64), ref)
        if gw in (17, 49):  # the host model of the contract gives the reference bit for bit
            for bf16 in (False, True):
                assert np.array_equal(ptd.emulate(x, w, b, pos, gh, gw, bf16), ref.astype(F32))


def test_round16_is_the_operand_types_rounding():
    g = np.random.Generator(np.random.PCG64(3))
    a = np.concatenate([g.standard_normal(20000).astype(F32) * s for s in (1e-6, 1e-3, 1.0, 300.0)])
    t = torch.from_numpy(a)
    assert np.array_equal(ptd.round16(a, False), t.to(torch.float16).float().numpy())
    assert np.array_equal(ptd.round16(a, True), t.to(torch.bfloat16).float().numpy())
    for bf16 in (False, True):
        z = ptd.round16(a, bf16, toward_zero=True)
        assert (np.abs(z) <= np.abs(a)).all() and np.array_equal(ptd.round16(z, bf16), z)
        assert (np.abs(z - a) <= np.abs(a) * 2.0 ** (-7 if bf16 else -10) + 2.0 ** -24).all()


@pytest.mark.parametrize("C,tiles", [(768, 912), (384, 456)])
def test_one_hot_maps_cover_every_slot(C, tiles):
    """the four maps k = (37 n + b) mod 588 of a width hit every contraction index, every (16-column tile of a wave and pass, k-step) pair and
    every (n mod 16, k mod 32) pair: every lane and element slot of a packed weight fragment"""
    ks, tl, slots = ptd.onehot_coverage(C)
    assert ks == set(range(588))
    assert tl == {(t, s) for t in range(C // 16) for s in range(19)} and len(tl) == tiles
    assert slots == {(n, k) for n in range(16) for k in range(32)} and len(slots) == 512
    for b in ptd.ONEHOT_B[C]:
        w = ptd.onehot_weights(C, b).reshape(C, 588)
        assert (w.sum(1) == 1).all() and (w.max(1) == 1).all()
        ws = ptd.wsum_f32(w)
        assert np.array_equal(ws[ptd.onehot_k(C, b) // 196, np.arange(C)], np.ones(C, F32)) and ws.sum() == C


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
def test_one_hot_bits_move_under_every_fault(bf16):
    """the expected bits of test 2 change in nearly half of the elements when the packing truncates or the mean is summed in another order, and
    in all of them when nothing is centred"""
    gh, gw, I, C = 2, 17, 2, 768
    x = ptd.generic_images(I, gh, gw, 2000 + gw)
    want = np.concatenate([ptd.onehot_expected(x, gh, gw, ptd.onehot_k(C, b), bf16) for b in ptd.ONEHOT_B[C]]).view(np.int32)
    frac = {}
    for name, kw in (("toward_zero", dict(toward_zero=True)), ("order", dict(order="columns")), ("uncentred", dict(centred=False))):
        got = np.concatenate([ptd.onehot_expected(x, gh, gw, ptd.onehot_k(C, b), bf16, **kw) for b in ptd.ONEHOT_B[C]]).view(np.int32)
        frac[name] = float((got != want).mean())
    print("one-hot bits changed:", {k: f"{v:.2%}" for k, v in frac.items()})
    assert 0.45 < frac["toward_zero"] < 0.55 and frac["order"] > 0.4 and frac["uncentred"] > 0.999, frac


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
def test_constant_patches_bound_separates_centred_from_uncentred(bf16):
    """test 3 on the host model: the centred form sits far inside the bound, the uncentred one misses it"""
    I, gh, gw, C = 2, 1, 33, 768
    x, c = ptd.constant_images(I, gh, gw, 31)
    assert (ptd.patches(x, gh, gw).reshape(I, gh * gw, 3, 196) == c[..., None]).all()
    w, b, pos = ptd.random_operands(C, 1 + gh * gw, 32)
    ref, bound = ptd.conv64(x, w, b, pos, gh, gw), ptd.constant_bound(c, w, b, pos)
    ratio = {cen: float((np.abs(ptd.emulate(x, w, b, pos, gh, gw, bf16, cen).astype(np.float64) - ref) / bound).max()) for cen in (True, False)}
    print("constant patches, worst error / bound:", ratio)
    assert ratio[True] < 0.05 and ratio[False] > 2.0, ratio
