"""Tile-level tests of the one-launch patch embedding (csrc/patch.hip, cs_patch_fused_kernel<BF, false>) and of the two-kernel form it replaced
(im2col_rows_kernel + the CS_EPI_PATCH_F32 GEMM with pmean / wsum: the forward's fallback for ln_fold, C not a multiple of 384, patch != 14).

Geometry of the one-launch kernel: a workgroup of four waves owns one run of np <= 48 consecutive patches of one patch row; a row of gw patches
is cut into ceil(gw / 48) runs of near-equal length, blocks are numbered image-fastest.  Phase A: thread t owns the 14-pixel row segments t,
t + 256, .. (channel, dy, patch); their sums go through LDS to the per-(patch, channel) means (14 pixels left to right, 14 rows top to bottom,
one division by 196), the centred values are rounded once to the operand type into the A tile [np][648] (1296-byte rows).  Phase B: wave w
computes columns 96 w .. 96 w + 95 of a 384-column pass as six 16-column tiles on up to three 16-row tiles, 19 k-steps of 32 on
v_mfma_f32_16x16x32 with the weights as first operand; the weight fragments come from a fragment-ordered copy (patch_pack_kernel: lane l of
piece (pass, wave, k-step s, tile j) holds k = 32 s + 8 (l >> 4) .. + 7 of column 16 j + (l & 15)) through four register sets, three k-steps
ahead.  Phase C: per row tile through a wave-private LDS patch to 384-byte pieces of token rows, + bias + position row + sum_ch mean * wsum.
Behind the A tile lie the four epilogue patches and the means, at 37 * 1296 bytes when no run is longer than 37 patches, else at 48 * 1296.

Entry points: hh.patch_embed_fused (`fused`) and hh.patch_embed(..., centred=1) (`two`), in fp16 and in bf16 operand mode
(cs_debug_set_op_operand_dtype, restored in any case).

Shape -> branch of the kernel (patches per run, on two patch rows and three images unless a test says otherwise):
    gw = 1            one row tile with 15 dead rows, which read whatever the LDS holds and are never stored
    gw = 15 / 16 / 17 the edge of row tile 0: one dead row / a full tile / a second tile with one live row
    gw = 31 / 32 / 33 the edge of row tile 1: the same with the third tile
    gw = 37           the 37-row layout at its limit: the dead rows 37..47 of tile 2 are the waves' epilogue patches
    gw = 38 / 48      the 48-row layout, with 10 dead rows / full
    gw = 49           two runs, 25 + 24: unequal, the second starts at patch 25
    gw = 97           three runs, 33 + 32 + 32: rem = 1
    I = 3             an odd image count against the image-fastest block numbering, the position-table slice and the output offset
    C = 384 / 768     one pass / two: the second restarts its accumulators and reads its own weight pieces, bias and position columns
    one-hot W (n, k)  n mod 16 = lane within a fragment, n // 16 = (pass, wave, tile); k mod 32 = (lane quarter, element), k // 32 = k-step
                      and with it the register set (s mod 4) the fragment travels through
    H, W              5 rows and 2 columns of NaN past the last whole patch (test 1): never read

What the tests assert: 1, 2, 4 and 5 bit equality (torch.equal against the fp64 convolution, whose result is exact in fp32, or equality of the
fp32 bit patterns); 3 the one stated fp32 bound.  Figures printed by the tests (worst per test and mode) and the record of the kernel mutations
run against this file: EXPERIMENTS.md.
"""
import functools

import numpy as np
import pytest
import torch

import hip_helpers as hh
import patch_tile_data as ptd
from bits16 import MODES, Worst, bits, same_bits, to_dev

gpu = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
P = 14
FORMS = pytest.mark.parametrize("form", ["fused", "two"])

_worst = Worst("test_hip_patch_tiles", "patch tiles")


def setup_module(module):
    _worst.start()


def teardown_module(module):
    _worst.report()


def _run(form, x, w, b, pos, out=None):
    """(I, 3, H, W) images -> (I, 1 + Np, C) fp32 token rows; the CLS rows are not written"""
    o = hh.patch_embed_fused(x, w, b, pos, P, out=out) if form == "fused" else hh.patch_embed(x, w, b, pos, P, 1, out=out)
    torch.cuda.synchronize()
    return o.reshape(x.shape[0], -1, w.shape[0])


# ---- 1. exact integers --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _integer_case(gw, C):
    """(images, w, b, pos, fp64 convolution cast to fp32) on the host, once per (gw, C); shared by both forms and modes and never changed"""
    I, gh = 3, 2
    x = ptd.integer_images(I, gh, gw, 100 + gw)
    w, b, pos = ptd.integer_operands(C, 1 + gh * gw, 7 + C)
    ref = ptd.conv64(x, w, b, pos, gh, gw)
    ref32 = ref.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref)
    return x, w, b, pos, torch.from_numpy(ref32)


@gpu
@MODES
@FORMS
@pytest.mark.parametrize("C", [384, 768])
@pytest.mark.parametrize("gw", list(ptd.GW_TABLE))
def test_exact_integers(gw, C, form, bf16):
    """Integer pixels whose patch means are multiples of 1/4, integer weights, bias and position table in quarters: every operand is exact in
    fp16 and bf16 and every partial sum is a multiple of 1/4 far below 2^22 (tests/test_patch_tiles_host.py), so the result IS the fp64
    convolution, whatever the summation order.  A wrong slot, row, run offset, token row, pass or a dropped term changes an integer.  The
    images carry 5 rows and 2 columns of NaN past the last whole patch and sit in poison; the output sits in guard bands; CLS rows keep the
    sentinel."""
    import guard

    I, gh = 3, 2
    x, w, b, pos, ref32 = _integer_case(gw, C)
    Np = gh * gw
    gg = guard.guarded((I * (1 + Np), C), F32)
    with hh.switches(bf16=bf16):
        out = _run(form, guard.poisoned_in(to_dev(x)), to_dev(w), to_dev(b), to_dev(pos), out=gg.view)
    gg.check(f"{form} gw={gw} C={C}")
    assert bool((bits(out[:, 0]) == gg.sentinel).all()), "a CLS row was written"
    got = out[:, 1:].cpu()
    if not torch.equal(got, ref32):
        bad = torch.nonzero(got != ref32)
        i, m, n = bad[0].tolist()
        raise AssertionError(f"{form} gw={gw} C={C} bf16={bf16}: {bad.shape[0]} of {got.numel()} elements differ from the fp64 convolution; the first "
                             f"at image {i}, patch row {m // gw}, patch {m % gw}, column {n}: {float(got[i, m, n])} against {float(ref32[i, m, n])}; "
                             f"rows hit {sorted(set((bad[:, 1] % gw).tolist()))[:12]}, columns hit {sorted(set(bad[:, 2].tolist()))[:12]}")


# ---- 2. one-hot weights, single rounding --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _generic_images(gw):
    return ptd.generic_images(2, 2, gw, 2000 + gw)


@gpu
@MODES
@FORMS
@pytest.mark.parametrize("C", [384, 768])
@pytest.mark.parametrize("gw", [17, 49])
def test_one_hot_weights_single_rounding(gw, C, form, bf16):
    """A single 1.0 per output column n at k = (37 n + b) mod 588, four maps per width that together reach every contraction index, every
    (16-column tile, k-step) pair and every (lane, element) slot of a weight fragment (asserted on the host).  Bias and position table zero,
    generic float pixels: out[m][n] = fl32(round16(fl32(v[m][k] - mu)) + mu) with mu summed in the kernel's fixed order, bit for bit (numpy
    float32 emulation).  A second rounding, a truncating pack, another order of the mean or a fragment element in a wrong slot changes bits
    in about half of the elements."""
    I, gh = 2, 2
    x = _generic_images(gw)
    xd = to_dev(x)
    zb, zpos = torch.zeros(C, device=DEV), torch.zeros(1 + gh * gw, C, device=DEV)
    with hh.switches(bf16=bf16):
        for b in ptd.ONEHOT_B[C]:
            out = _run(form, xd, to_dev(ptd.onehot_weights(C, b)), zb, zpos)
            want = torch.from_numpy(ptd.onehot_expected(x, gh, gw, ptd.onehot_k(C, b), bf16))
            same_bits(out[:, 1:].cpu(), want, f"{form} gw={gw} C={C} b={b} bf16={bf16}")
            assert bool((out[:, 0] == 7.0).all())


# ---- 3. constant patches ------------------------------------------------------------------------------------------------------------------
@gpu
@MODES
@FORMS
def test_constant_patches_mean_term(form, bf16):
    """Every patch constant per channel, at normalised uint8 levels: the 16-bit operand is the rounding error of the mean and the result is
    b + pos + sum_ch mu_ch wsum[ch][n] in fp32.  Against the fp64 convolution: |err| <= 256 * 2^-24 * (sum_k |W| |c| + |b| + |pos|), the fp32
    bound of two 196-term sums plus the epilogue.  A form that does not centre misses it 6-fold in fp16 and 50-fold in bf16 (host model), a
    dropped mean term by O(1)."""
    I, gh, gw, C = 2, 1, 33, 768
    x, c = ptd.constant_images(I, gh, gw, 31)
    w, b, pos = ptd.random_operands(C, 1 + gh * gw, 32)
    ref, bound = ptd.conv64(x, w, b, pos, gh, gw), ptd.constant_bound(c, w, b, pos)
    with hh.switches(bf16=bf16):
        out = _run(form, to_dev(x), to_dev(w), to_dev(b), to_dev(pos))
    got = out[:, 1:].cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err / bound).max())
    print(f"patch tiles constant patches {form} bf16={bf16}: max |out - fp64| {err.max():.3e}, worst error / bound {ratio:.3e}")
    _worst.note(f"constant_patches {form}", bf16, err=err.max(), over_bound=ratio)
    assert (err <= bound).all(), ratio


# ---- 4. patch independence ----------------------------------------------------------------------------------------------------------------
# (gw, [(image, patch row, patch)]): the last patch of run 0 and the first of run 1, local rows 15 and 16 of a run (run 0, and 16 of run 1), the
# last patch of the last patch row, one on image 1; at gw = 37 the last live row, whose dead neighbours 37..47 are the epilogue patches
INDEP = [(49, [(0, 0, 24), (0, 0, 25), (0, 1, 15), (0, 1, 16), (0, 0, 41), (0, 1, 48), (1, 1, 25)]), (37, [(0, 1, 36), (1, 0, 36)])]


@gpu
@MODES
@FORMS
@pytest.mark.parametrize("gw,where", INDEP, ids=["gw49", "gw37"])
def test_a_patch_reaches_its_own_row_only(gw, where, form, bf16):
    """All 588 pixels of one patch replaced by NaN, by +Inf, by fresh finite values: every other token row of every image keeps every bit (the
    means are indexed per patch, the row sums stay with their patch, a 16-row MFMA tile never mixes rows); the row itself is NaN in every
    column for NaN and Inf (the mean term alone sees to that) and finite again after the finite replacement."""
    I, gh, C = 2, 2, 384
    x = to_dev(ptd.normal_images(I, gh, gw, 4000 + gw))
    w, b, pos = (to_dev(a) for a in ptd.random_operands(C, 1 + gh * gw, 4100 + gw))
    fresh = to_dev(np.random.Generator(np.random.PCG64(4200)).standard_normal((3, P, P)).astype(np.float32) * 1.5 + 0.25)
    with hh.switches(bf16=bf16):
        base = _run(form, x, w, b, pos).clone()
        assert torch.isfinite(base[:, 1:]).all()
        for img, pi, pj in where:
            tok = 1 + pi * gw + pj
            others = torch.ones(I, 1 + gh * gw, dtype=torch.bool, device=DEV)
            others[img, tok] = False
            for name, val in (("nan", float("nan")), ("inf", float("inf")), ("finite", fresh)):
                xv = x.clone()
                xv[img, :, pi * P:(pi + 1) * P, pj * P:(pj + 1) * P] = val
                got = _run(form, xv, w, b, pos)
                same = (bits(got) == bits(base)).all(-1)
                assert bool(same[others].all()), (form, gw, (img, pi, pj), name, "rows changed (image, token):", torch.nonzero(~same & others)[:8].tolist())
                row = got[img, tok]
                if name == "finite":
                    assert bool(torch.isfinite(row).all()) and not torch.equal(row, base[img, tok])
                else:
                    assert bool(torch.isnan(row).all()), (form, gw, (img, pi, pj), name)


# ---- 5. both passes, both widths ----------------------------------------------------------------------------------------------------------
@gpu
@MODES
def test_two_passes_equal_two_one_pass_launches(bf16):
    """C = 768 with weight rows, bias and position columns (Wa | Wb) equals, bit for bit, the two C = 384 launches on (Wa, ba, posa) and
    (Wb, bb, posb): pass 1 restarts its accumulators and reads its own weight pieces, bias, wsum and position columns.  gw = 38: the 48-row
    layout with ten dead rows."""
    I, gh, gw = 2, 2, 38
    x = to_dev(ptd.normal_images(I, gh, gw, 5000))
    w, b, pos = ptd.random_operands(768, 1 + gh * gw, 5001)
    with hh.switches(bf16=bf16):
        wide = _run("fused", x, to_dev(w), to_dev(b), to_dev(pos))
        for h in (0, 1):
            s = slice(384 * h, 384 * h + 384)
            half = _run("fused", x, to_dev(w[s]), to_dev(b[s]), to_dev(pos[:, s]))
            same_bits(wide[:, 1:, s], half[:, 1:], f"columns {s.start}..{s.stop - 1} bf16={bf16}")
    assert torch.isfinite(wide[:, 1:]).all()
