"""Tile-level tests of the decoder's row-complete kernel (csrc/rowln.hip, cs_rowln_kernel) on its v_mfma_f32_32x32x16 tiles with D transposed:
a workgroup owns 64 complete rows (two 32-row blocks rb), wave w the output columns [96 w, 96 w + 96) as three column tiles ct; the WEIGHT
fragment is the A operand, so register e of tile ct of lane (j, h) is feature 96 w + 32 ct + (e & 3) + 8 (e >> 2) + 4 h of row 32 rb + j.  The
weights arrive as six 64-wide K slices, double buffered in LDS (slice s2 in buffer s2 & 1), four k-steps of 16 per slice; lane half h reads
contraction slots 8 h .. 8 h + 7 of a k-step.  The second stage (n2 = C or 3 C) runs the same K loop once per group of C output columns on
the normalised rows, rounded to the operand type and handed over through LDS; its accumulators restart at each group's first slice.
Entry points: cs_op_linear_layernorm / cs_op_linear_layernorm_linear through tests/hip_helpers.py; every case is one or a few launches of at
most 257 rows at C = 384, in fp16 and in bf16 operand mode (the <384, false, G2> and <384, true, G2> instantiations, G2 = 0 / 1 / 3).

Shape -> branch of the kernel:
    M = 1             one workgroup, one live row: 63 rows are the clamped re-read of row 0, computed and dropped
    M = 31 / 32 / 33  the edge of row block rb = 0: rb = 1 all dropped / all dropped / one live row
    M = 63 / 64 / 65  the edge of the workgroup: one dropped row / a full block / a second workgroup with one live row
    M = 127 / 129     two workgroups less a row / a third one with one live row (128: the row-independence test)
    resid null / set  the `if (p.resid)` branch of the epilogue
    n2 = 0 / C / 3 C  the three instantiations per type: no second stage / 6 slices, both LDS weight buffers three times / 18 slices, a group
                      boundary at s2 = 6 and 12 (buffer parity continues across it: group 1 starts in buffer 0 again, after six slices)
    act2 = 0 / 1 / 2  the run-time activation of the second stage: none / ReLU / LeakyReLU(0.01)
    one-hot W (n, k)  n: residue mod 32 = (e, h) slot of a tile, n // 32 = (wave, ct); k: residue mod 16 = (h, slot of the 16-byte read),
                      (k % 64) // 16 = k-step, k // 64 = slice and its LDS buffer
    one-hot W2        the same for the second stage, plus n // C = the group: a nonzero of group 0 must not survive into groups 1 and 2
    +-v rows          mean 0 and variance v^2 / 64 exactly: v = 16 puts the normalised value at +-7.99999, which is +-8 in both operand types
                      (second stage exact); v = 2^-6 puts the variance at 3.8e-6, below, at and above the three eps values
    constant rows     variance 0: the result is beta plus the rounding of the mean, scaled by 1 / sqrt(eps)
    offset + N(0, 1)  mean-to-sigma ratios of about 60 and 600: the centred second pass against E[x^2] - mean^2

Figures printed by the tests (worst per test and mode) and the record of the kernel mutations run against this file: EXPERIMENTS.md.
"""
import math

import numpy as np
import pytest
import torch

import hip_helpers as hh
from bits16 import MODES, Worst, bits16, ordered16, same_bits, spacing16, vals16

gpu = pytest.mark.gpu

C = 384
DEV = "cuda"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
TOL32 = 2e-4  # out_f32 against fp64: the bound of test_hip_ops.py::test_linear_layernorm_one_launch

_worst = Worst("test_hip_rowln_tiles", "rowln tiles")


def setup_module(module):
    _worst.start()


def teardown_module(module):
    _worst.report()


def _ln64(pre, gam, bet, eps):
    return torch.nn.functional.layer_norm(pre.double(), (C,), gam.double(), bet.double(), eps)


def _act64(y, act2):
    """second-stage activation of the fp64 pre-activation; leaky: the kernel's constant is fp32(0.01)"""
    if act2 == 1:
        return torch.relu(y)
    if act2 == 2:
        return torch.where(y >= 0, y, float(np.float32(0.01)) * y)
    return y


def _rand_case(M, seed, bf16, with_resid=True, n2=0, offset=0.0, dev=None):
    """random operands, PCG64(seed), generated on the host: A, W, W2 rounded to the operand type; resid = offset + N(0, sigma)"""
    g = np.random.Generator(np.random.PCG64(seed))
    n = lambda *s: torch.from_numpy(g.standard_normal(s, dtype=np.float32))
    d = dict(A=bits16(n(M, C), bf16), W=bits16(n(C, C) / math.sqrt(C), bf16), b=n(C),
             res=(offset + (1.0 if offset else 2.0) * n(M, C)) if with_resid else None, gam=1.0 + 0.3 * n(C), bet=0.2 * n(C))
    if n2:
        d["W2"], d["b2"] = bits16(n(n2, C) / math.sqrt(C), bf16), 0.5 * n(n2)
    return {k: (v.to(dev or DEV) if v is not None else None) for k, v in d.items()}


def _pre64(d, bf16):
    pre = vals16(d["A"], bf16, F64) @ vals16(d["W"], bf16, F64).t() + d["b"].double()
    return pre + d["res"].double() if d["res"] is not None else pre


# ---- host-side constructions (no GPU: test_host_side_constructions runs them all) -------------------------------------------------------
def _ragged_grid():
    """(M, with_resid, n2, act2): every M with and without a residual; n2 and act2 spread so that each n2 meets both residual settings and each
    (n2 > 0, act2) pair occurs"""
    out = []
    for i, M in enumerate((1, 31, 32, 33, 63, 64, 65, 127, 129)):
        for r in (0, 1):
            n2 = (0, C, 3 * C)[(i + r) % 3]
            out.append((M, bool(r), n2, (i // 3 + 2 * r + i) % 3 if n2 else 0))
    assert {(n2, r) for _, r, n2, _ in out} == {(n2, r) for n2 in (0, C, 3 * C) for r in (False, True)}
    assert {(n2, a) for _, _, n2, a in out if n2} == {(n2, a) for n2 in (C, 3 * C) for a in (0, 1, 2)}
    return out


def _positions():
    """51 (output feature n, contraction index k) pairs.  n: every residue mod 32 (the (e, h) slots of a tile: all four 8-column groups, both h
    halves of each), each of the 12 column tiles (4 waves x 3 ct), the corners.  k: every residue mod 16, every (slice, k-step) pair -- so all
    four k-steps, the first and the last slice, even and odd slices (the two LDS weight buffers) -- and the corners."""
    out = []
    for i in range(48):
        n = 32 * (i % 12) + (5 * i) % 32
        sl, ks = divmod(i % 24, 4)
        out.append((n, 64 * sl + 16 * ks + (7 * i) % 16))
    out += [(C - 1, C - 1), (0, C - 1), (C - 1, 0)]  # ((0, 0) is pair 0)
    ns, ks_ = [n for n, _ in out], [k for _, k in out]
    assert all(0 <= n < C and 0 <= k < C for n, k in out) and len(set(out)) == len(out)
    assert {n % 32 for n in ns} == set(range(32)) and {n // 32 for n in ns} == set(range(12))
    assert {((n % 32) >> 3, (n >> 2) & 1) for n in ns} == {(g, h) for g in range(4) for h in range(2)}
    assert {k % 16 for k in ks_} == set(range(16))
    assert {(k // 64, (k % 64) // 16) for k in ks_} == {(s, t) for s in range(6) for t in range(4)}
    assert {0, 5} <= {k // 64 for k in ks_} and {(k // 64) % 2 for k in ks_} == {0, 1}
    return out


def _positions2(n2):
    """(n, k, act2) of the second stage: _positions() with n spread over the n2 / C groups (its coverage holds within a group: n % C), the first
    and last column of every group, every (group, act2) pair"""
    G = n2 // C
    base = _positions()
    out = [(C * (i % G) + n, k, (i // 3) % 3) for i, (n, k) in enumerate(base)]
    have = {n for n, _, _ in out}
    for i, n in enumerate(c for g in range(G) for c in (g * C, g * C + C - 1)):
        if n not in have:
            out.append((n, base[(11 * i + 5) % 48][1], i % 3))
    assert {0, C - 1, C, 2 * C - 1, 2 * C, 3 * C - 1}.intersection(range(n2)) <= {n for n, _, _ in out}
    assert {(n // C, a) for n, _, a in out} == {(g, a) for g in range(G) for a in range(3)}
    assert {(n % C) % 32 for n, _, _ in out} == set(range(32)) and {(n % C) // 32 for n, _, _ in out} == set(range(12))
    return out


def _signed_ints(M):
    """(M, C) small nonzero integers (exact in both operand types) that differ by row and column.  LayerNorm of a row with one nonzero a is
    sign(a) sqrt(C - 1) whatever |a| is (to eps / a^2), so a wrong contraction slot shows through the SIGNS: the sign of (r, c) is bit r % 9
    of c, which makes the sign patterns of any two columns differ inside every nine consecutive rows.  Magnitudes 1 .. 8."""
    r, c = torch.arange(M)[:, None], torch.arange(C)[None, :]
    a = (torch.where(((c >> (r % 9)) & 1) == 1, 1, -1) * (1 + (5 * r + 3 * c) % 8)).float()
    assert (a != 0).all() and a.abs().max() == 8
    if M >= 9:
        assert torch.unique(torch.sign(a[:9]), dim=1).shape[1] == C
    return a


def _pm_rows(M, v):
    """(rows (M, C) fp32, signs (M, C) in {-1, 0, +1}): +v at three columns, -v at three others, zero elsewhere.  Row m's six columns are one per
    K slice, 64 s + (m + 11 s) % 64: six different residues mod 16 per row, all 16 between the rows, and column k is nonzero in exactly the
    rows m = k - 11 (k // 64) mod 64 -- no two columns share their set of rows for M <= 64 + the repeat at row 64.  mean = 0, variance v^2 / 64."""
    m, s = torch.arange(M)[:, None], torch.arange(6)[None, :]
    cols = 64 * s + (m + 11 * s) % 64
    sg = (1 - 2 * ((m + s) % 2)).float()
    assert (sg.sum(1) == 0).all() and (cols // 64 == s).all()
    assert all(len({int(c) % 16 for c in row}) == 6 for row in cols) and {int(c) % 16 for c in cols.flatten()} == set(range(16))
    sign = torch.zeros(M, C).scatter_(1, cols, sg)
    if M >= 64:
        assert (sign != 0).any(0).all()  # every contraction index carries a nonzero in some row
    return sign * v, sign


def _boundary_margin(x, bf16):
    """relative distance of x > 0 from the nearest rounding boundary (midpoint of two neighbouring values) of the operand type, in fp64"""
    bits = 8 if bf16 else 11
    ulp = lambda y: 2.0 ** (math.frexp(y)[1] - 1 - (bits - 1))
    lo = math.floor(x / ulp(x)) * ulp(x)
    mids = [lo + ulp(x) / 2, lo - ulp(lo * (1 - 2.0 ** -12)) / 2, lo + ulp(x) + ulp(lo + ulp(x)) / 2]
    return min(abs(x - m) for m in mids) / x


def _normalised_pm(v, eps):
    """|LayerNorm| (gamma 1, beta 0) of the nonzero columns of _pm_rows(., v), fp64"""
    return v / math.sqrt(v * v / 64.0 + eps)


def _check_margin_of_eight(bf16):
    """v = 16, eps = 1e-5: the normalised value 7.99999 must round to 8 with room to spare.  The room is asked as 2^-12 relative to the nearest
    rounding boundary; a value that rounds UP to a power of two cannot have more than that in fp16 (half an ulp of the binade below, 2^-9, over
    8), and 7.99999 has 0.995 of it (2.429e-4; bf16: 1.95e-3), so the assertion stands at 0.99 x 2^-12: about 4000 fp32 ulps either way."""
    x = _normalised_pm(16.0, 1e-5)
    assert float(vals16(bits16(torch.tensor([x], dtype=torch.float64).float(), bf16), bf16, F64)[0]) == 8.0
    margin = _boundary_margin(x, bf16)
    assert margin >= 0.99 * 2.0 ** -12, margin
    assert 8.0 - x < 0.01 * 2.0 ** -9  # and it sits within 1 % of half an fp16 ulp of the value it rounds to
    return margin


EPS_SET = (1e-3, 1e-5, 1e-6)


def _eps_refs():
    """fp64 LayerNorm at the +v columns of the v = 2^-6 rows for the three eps: 0.4932, 4.2039, 7.1209; pairwise more than 100 tolerances apart"""
    refs = [_normalised_pm(2.0 ** -6, e) for e in EPS_SET]
    assert all(abs(a - b) > 100 * TOL32 for i, a in enumerate(refs) for b in refs[i + 1:]), refs
    return refs


MEAN_SEED = 20250  # test_large_common_mean: kept from the host check below (PCG64)


def _mean_case(offset, bf16, dev):
    """-> (operands, fp64 reference, elementwise bound): rows offset + N(0, 1) through the residual plus a random A W^T + b.
    Bound: 2e-4 + |gamma| |offset| 2^-23 rstd -- the fp32 rounding of a value of size |offset| and of the mean, scaled as the kernel scales them."""
    d = _rand_case(65, MEAN_SEED + int(abs(offset)), bf16, True, 0, offset=offset, dev=dev)
    pre = _pre64(d, bf16)
    rstd = 1.0 / torch.sqrt(pre.var(1, unbiased=False, keepdim=True) + 1e-5)
    return d, pre, _ln64(pre, d["gam"], d["bet"], 1e-5), TOL32 + d["gam"].double().abs() * abs(offset) * 2.0 ** -23 * rstd


def _single_pass_misses(offset, bf16):
    """the same rows normalised in fp32 with var = E[x^2] - mean^2 (numpy on the host): the fraction of elements outside the bound"""
    d, pre, ref, bound = _mean_case(offset, bf16, "cpu")
    x = pre.numpy().astype(np.float32)
    mu = x.mean(1, dtype=np.float32, keepdims=True)
    var = (x * x).mean(1, dtype=np.float32, keepdims=True) - mu * mu
    with np.errstate(invalid="ignore"):
        out = (x - mu) / np.sqrt(var + np.float32(1e-5)) * d["gam"].numpy() + d["bet"].numpy()
    return float((~((torch.from_numpy(out).double() - ref).abs() <= bound)).double().mean())


def test_host_side_constructions():
    """Everything above that a kernel test relies on, without a GPU: the coverage of the position sets, the rounding margin of +-8, the
    separation of the three eps references, and that single-pass statistics in fp32 FAIL the bound of test_large_common_mean at offset -1000."""
    _ragged_grid()
    assert len(_positions()) == 51 and len(_positions2(C)) == 51 and len(_positions2(3 * C)) > 51
    _signed_ints(65)
    rows, sign = _pm_rows(65, 16.0)
    assert (rows.sum(1) == 0).all() and ((rows * rows).sum(1) == 6 * 256).all()
    assert abs(_check_margin_of_eight(False) - 2.429e-4) < 1e-7 and abs(_check_margin_of_eight(True) - 1.952e-3) < 1e-6
    refs = _eps_refs()
    assert [round(r, 4) for r in refs] == [0.4932, 4.2039, 7.1209], refs
    for bf16 in (False, True):
        assert _single_pass_misses(-1000.0, bf16) > 0.5


# ---- 1. ragged rows ---------------------------------------------------------------------------------------------------------------------
@gpu
@MODES
@pytest.mark.parametrize("M,with_resid,n2,act2", _ragged_grid(), ids=lambda v: str(v))
def test_ragged_rows_on_random_data(M, with_resid, n2, act2, bf16):
    """Row counts around the 32-row block and the 64-row workgroup.  A and the residual are exactly M rows inside poison, all outputs inside
    guard bands.  out_f32 against fp64 on the same rounded operands; out_f16 = out_f32 rounded once, bit for bit; out2 against fp64 on the
    kernel's own 16-bit rows, within half an ulp of the operand type plus the fp32 accumulation bound of test_hip_bounds.py::_gemm_case."""
    from guard import guarded_out, poisoned_in

    d = _rand_case(M, 1000 + 7 * M + n2 + act2 + int(with_resid), bf16, with_resid, n2)
    A = poisoned_in(d["A"])
    res = poisoned_in(d["res"]) if with_resid else None
    of, cf = guarded_out((M, C), F32)
    oh, ch = guarded_out((M, C), F16)
    with hh.switches(bf16=bf16):
        if n2:
            o2, c2 = guarded_out((M, n2), F16)
            hh.linear_layernorm_linear(A, d["W"], d["b"], res, d["gam"], d["bet"], 1e-5, d["W2"], d["b2"], act2, of=of, oh=oh, out2=o2)
        else:
            hh.linear_layernorm(A, d["W"], d["b"], res, d["gam"], d["bet"], 1e-5, of=of, oh=oh)
        torch.cuda.synchronize()
    cf("out_f32")
    ch("out_f16")
    ref = _ln64(_pre64(d, bf16), d["gam"], d["bet"], 1e-5)
    e1 = float((of.double() - ref).abs().max())
    print(f"rowln tiles M={M} resid={with_resid} n2={n2} act2={act2} bf16={bf16}: max |out_f32 - ref| {e1:.2e}", end="")
    _worst.note("ragged", bf16, out_f32=e1)
    assert torch.isfinite(of).all() and e1 < TOL32, e1
    same_bits(oh, bits16(of, bf16), "out_f16 = out_f32 rounded once")
    if n2:
        c2("out2")
        rows, W2 = vals16(oh, bf16, F64), vals16(d["W2"], bf16, F64)
        r2 = _act64(rows @ W2.t() + d["b2"].double(), act2)
        S = rows.abs() @ W2.abs().t()
        half = 2.0 ** -8 if bf16 else 2.0 ** -11
        bound = half * r2.abs() + 1.001 * C * 2.0 ** -24 * S + 2.0 ** -24
        if act2 == 2:
            bound = bound + 2.0 ** -24 * r2.abs()  # the product with 0.01 is one more fp32 rounding
        e2 = (vals16(o2, bf16, F64) - r2).abs()
        print(f", max |out2 - ref| {float(e2.max()):.2e} (worst error / bound {float((e2 / bound).max()):.3f})", end="")
        _worst.note("ragged", bf16, out2=e2.max(), out2_over_bound=(e2 / bound).max())
        assert (e2 <= bound).all(), (float(e2.max()), float((e2 / bound).max()))
    print()


# ---- 2. one-hot W -----------------------------------------------------------------------------------------------------------------------
@gpu
@MODES
def test_one_hot_weight_first_stage(bf16):
    """A single 1 at W[n, k], bias 0, no residual, gamma 1, beta 0, eps 1e-6: the accumulators are exact, column n of the pre-norm rows is
    column k of A and everything else 0.  The normalised signal is +-19.6 at column n and -+0.05 elsewhere: a weight element in a wrong
    feature slot is off by O(1) at two columns, one in a wrong contraction slot by 39 in the rows where the two columns of A differ in sign.
    M = 65: both row blocks, a second workgroup."""
    M = 65
    a = _signed_ints(M).to(DEV)
    A = bits16(a, bf16)
    zero, one = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    worst = 0.0
    with hh.switches(bf16=bf16):
        for n, k in _positions():
            wf = torch.zeros(C, C, device=DEV)
            wf[n, k] = 1.0
            of, oh = hh.linear_layernorm(A, bits16(wf, bf16), zero, None, one, zero, 1e-6)
            torch.cuda.synchronize()
            pre = torch.zeros(M, C, dtype=torch.float64, device=DEV)
            pre[:, n] = a[:, k].double()
            err = float((of.double() - _ln64(pre, one, zero, 1e-6)).abs().max())
            worst = max(worst, err)
            assert err < TOL32, (n, k, err)
            same_bits(oh, bits16(of, bf16), (n, k))
    print(f"rowln tiles one-hot W bf16={bf16}: max |out_f32 - ref| {worst:.2e} over {len(_positions())} positions")
    _worst.note("one_hot_w", bf16, out_f32=worst)


# ---- 3. one-hot W2 ----------------------------------------------------------------------------------------------------------------------
def _act32(y, act2):
    """the second stage's activation as the kernel evaluates it, fp32"""
    if act2 == 1:
        return torch.relu(y)
    if act2 == 2:
        return torch.where(y >= 0, y, torch.tensor(0.01, dtype=F32, device=y.device) * y)
    return y


@gpu
@MODES
@pytest.mark.parametrize("n2", [C, 3 * C])
def test_one_hot_weight_second_stage_exact(n2, bf16):
    """W = 0 and b = 0: the first stage is the residual alone, rows of +-16 at six columns (_pm_rows).  mean 0, variance 4, normalised value
    +-7.99999 = +-8 in both operand types (margin asserted on the host), every other column 0.  With a single 1 at W2[n, k] and integer b2,
    out2 = round16(act2(b2 + (+-8 or 0 at column n))) bit for bit: the hand-off of the normalised rows through LDS, the slice and buffer a weight
    element travels through, the group its result lands in, and the accumulator reset of each group (a nonzero of group 0 stays out of 1, 2)."""
    _check_margin_of_eight(bf16)
    M = 65
    rows, sign = _pm_rows(M, 16.0)
    rows, norm = rows.to(DEV), (8.0 * sign).to(DEV)
    A, W = torch.zeros(M, C, dtype=F16, device=DEV), torch.zeros(C, C, dtype=F16, device=DEV)
    zero, one = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    b2 = ((torch.arange(n2, device=DEV) * 7) % 11 - 5).float()
    with hh.switches(bf16=bf16):
        for i, (n, k, act2) in enumerate(_positions2(n2)):
            w2 = torch.zeros(n2, C, device=DEV)
            w2[n, k] = 1.0
            _, oh, o2 = hh.linear_layernorm_linear(A, W, zero, rows, one, zero, 1e-5, bits16(w2, bf16), b2, act2, want_f32=False, want_f16=(i == 0))
            torch.cuda.synchronize()
            y = b2[None, :].repeat(M, 1)
            y[:, n] += norm[:, k]
            same_bits(o2, bits16(_act32(y, act2), bf16), (n, k, act2))
            if i == 0:
                same_bits(oh, bits16(norm, bf16), "normalised rows")


# ---- 4. eps -----------------------------------------------------------------------------------------------------------------------------
@gpu
@MODES
@pytest.mark.parametrize("eps", EPS_SET)
def test_eps_is_observable(eps, bf16):
    """Rows of +-2^-6 at six columns: variance 3.8e-6, so eps = 1e-3 / 1e-5 / 1e-6 dominates, matches or is below it and the result at the +v
    columns is 0.4932 / 4.2039 / 7.1209: any fixed eps fails two of the three cases by more than 100 tolerances (asserted by _eps_refs)."""
    ref_v = _eps_refs()[EPS_SET.index(eps)]
    M = 65
    rows, sign = _pm_rows(M, 2.0 ** -6)
    rows = rows.to(DEV)
    A, W = torch.zeros(M, C, dtype=F16, device=DEV), torch.zeros(C, C, dtype=F16, device=DEV)
    zero, one = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    with hh.switches(bf16=bf16):
        of, oh = hh.linear_layernorm(A, W, zero, rows, one, zero, eps)
        torch.cuda.synchronize()
    ref = _ln64(rows, one, zero, eps)
    assert float((ref - sign.to(DEV).double() * ref_v).abs().max()) < 1e-12
    err = float((of.double() - ref).abs().max())
    print(f"rowln tiles eps={eps} bf16={bf16}: max |out_f32 - ref| {err:.2e} at |ref| {ref_v:.4f}")
    _worst.note("eps", bf16, out_f32=err)
    assert err < TOL32, err
    same_bits(oh, bits16(of, bf16))


# ---- 5. zero variance -------------------------------------------------------------------------------------------------------------------
@gpu
@MODES
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_zero_variance_rows(eps, bf16):
    """Every row a constant c in {0, 1, 7.3, 30, 1000} (through the residual, W = 0), random gamma and beta.  c = 0: exactly beta.  Otherwise the
    centred value is the rounding error of the mean -- mean = s * fl(1 / C): one rounding in fl(1 / C), one in the product, and the sum s of
    384 equal fp32 values -- at most |c| 2^-23, and the variance is its square, far below eps: |out - beta| <= |gamma| |c| 2^-23 / sqrt(eps)."""
    M = 65
    g = np.random.Generator(np.random.PCG64(55))
    gam = torch.from_numpy(1.0 + 0.3 * g.standard_normal(C, dtype=np.float32)).to(DEV)
    bet = torch.from_numpy(0.2 * g.standard_normal(C, dtype=np.float32)).to(DEV)
    c = torch.tensor([0.0, 1.0, 7.3, 30.0, 1000.0], device=DEV)[torch.arange(M, device=DEV) % 5]
    rows = c[:, None].repeat(1, C)
    A, W = torch.zeros(M, C, dtype=F16, device=DEV), torch.zeros(C, C, dtype=F16, device=DEV)
    with hh.switches(bf16=bf16):
        of, oh = hh.linear_layernorm(A, W, torch.zeros(C, device=DEV), rows, gam, bet, eps)
        torch.cuda.synchronize()
    assert torch.isfinite(of).all()
    dev_ = (of.double() - bet.double()[None, :]).abs()
    bound = gam.double().abs()[None, :] * c.double().abs()[:, None] * 2.0 ** -23 / math.sqrt(eps)
    for j, cv in enumerate((0.0, 1.0, 7.3, 30.0, 1000.0)):
        print(f"rowln tiles constant rows c={cv} eps={eps} bf16={bf16}: max |out - beta| {float(dev_[j::5].max()):.2e} (bound at gamma = 1: "
              f"{cv * 2.0 ** -23 / math.sqrt(eps):.2e})")
    _worst.note("zero_variance", bf16, out_minus_beta=dev_.max(), over_bound=(dev_[c != 0] / bound[c != 0]).max())
    assert (dev_ <= bound).all(), float((dev_ - bound).max())
    zr = c == 0
    assert torch.equal(of[zr], bet[None, :].expand(int(zr.sum()), C))
    same_bits(oh[zr], bits16(bet, bf16)[None, :].expand(int(zr.sum()), C), "beta rounded once")
    same_bits(oh, bits16(of, bf16))


# ---- 6. large common mean ---------------------------------------------------------------------------------------------------------------
@gpu
@MODES
@pytest.mark.parametrize("offset", [100.0, -1000.0])
def test_large_common_mean(offset, bf16):
    """Rows offset + N(0, 1) (residual) + A W^T + b: the statistics are two passes over the registers (mean, then the centred squares), so the
    error is the fp32 rounding of values of size |offset| and of their mean.  E[x^2] - mean^2 in fp32 on the same rows misses this bound at
    offset -1000 (checked on the host with the same seed, here and in test_host_side_constructions: the variance of about 3 is the difference of
    two numbers of 1e6 whose fp32 spacing is 0.06)."""
    d, _, ref, bound = _mean_case(offset, bf16, DEV)
    if offset == -1000.0:
        assert _single_pass_misses(offset, bf16) > 0.5
    with hh.switches(bf16=bf16):
        of, oh = hh.linear_layernorm(d["A"], d["W"], d["b"], d["res"], d["gam"], d["bet"], 1e-5)
        torch.cuda.synchronize()
    err = (of.double() - ref).abs()
    print(f"rowln tiles offset={offset} bf16={bf16}: max |out_f32 - ref| {float(err.max()):.2e} (worst error / bound {float((err / bound).max()):.3f})")
    _worst.note("common_mean", bf16, out_f32=err.max(), over_bound=(err / bound).max())
    assert torch.isfinite(of).all() and (err <= bound).all(), float(err.max())
    same_bits(oh, bits16(of, bf16))


# ---- 7. row independence ----------------------------------------------------------------------------------------------------------------
@gpu
@MODES
@pytest.mark.parametrize("M,rs", [(128, (0, 31, 32, 63, 64, 127)), (65, (64,))], ids=["M128", "M65-last"])
def test_rows_are_independent_bit_for_bit(M, rs, bf16):
    """A lane holds 48 values of ONE row per row block and the row sums meet other rows only as neighbours in the LDS exchange: perturbing row r
    (activations and residual) changes row r of out_f32, out_f16 and out2 (n2 = 3 C) and not one bit of any other row.  M = 65, r = 64: the
    workgroup's 63 rows past M re-read row 64 (min(row, M - 1)); they are computed and dropped."""
    d = _rand_case(M, 4242 + M, bf16, True, 3 * C)
    run = lambda A, res: hh.linear_layernorm_linear(A, d["W"], d["b"], res, d["gam"], d["bet"], 1e-5, d["W2"], d["b2"], 2, want_f32=True, want_f16=True)
    with hh.switches(bf16=bf16):
        base = run(d["A"], d["res"])
        for r in rs:
            A, res = d["A"].clone(), d["res"].clone()
            A[r] = d["A"][(r + 1) % M]
            res[r] = res[r] * 1.25 + 0.5
            got = run(A, res)
            torch.cuda.synchronize()
            others = torch.arange(M, device=DEV) != r
            for name, g_, b_ in zip(("out_f32", "out_f16", "out2"), got, base):
                gb, bb = g_.view(torch.int32 if g_.dtype == F32 else torch.int16), b_.view(torch.int32 if b_.dtype == F32 else torch.int16)
                assert torch.equal(gb[others], bb[others]), (name, r, torch.nonzero((gb != bb).any(1)).flatten().tolist())
                assert not torch.equal(gb[r], bb[r]), (name, r)


# ---- 8. the two-launch form -------------------------------------------------------------------------------------------------------------
@gpu
@MODES
def test_same_answer_as_the_two_launch_form(bf16):
    """GEMM with the fp32 residual epilogue, then the LayerNorm kernel, on the same operands in the same mode (the forward's other form):
    out_f32 within 2e-4, the 16-bit rows at most one ulp of the operand type apart.  "One ulp" is what rounding two nearby fp32 values can
    give: where the two fp32 results differ by d, their roundings differ by at most 1 + floor(d / spacing) steps of the 16-bit grid (one
    rounding boundary, plus one more per whole spacing that fits into d).  d is a few fp32 ulps of the row's largest values, so the second
    term is 0 -- a single step at most -- everywhere but at values so close to zero that the 16-bit grid is finer than d (fp16 keeps 2^-24
    there); the spacing is taken at the smaller of the two magnitudes, halved for a binade edge between them."""
    from crossscore_amd import _lib

    M = 129
    d = _rand_case(M, 808, bf16, True, 0)
    with hh.switches(bf16=bf16):
        of, oh = hh.linear_layernorm(d["A"], d["W"], d["b"], d["res"], d["gam"], d["bet"], 1e-5)
        y = hh.gemm(d["A"], d["W"], d["b"], _lib.EPI_RESID_F32, resid=d["res"])
        of2, oh2 = hh.layernorm(y, d["gam"], d["bet"], 1e-5)
        torch.cuda.synchronize()
    e = float((of - of2).abs().max())
    ulps = (ordered16(oh) - ordered16(oh2)).abs()
    dd = (of.double() - of2.double()).abs()
    small = torch.minimum(vals16(oh, bf16, F64).abs(), vals16(oh2, bf16, F64).abs())
    allowed = 1 + torch.floor(dd / (0.5 * spacing16(small, bf16)))
    multi = ulps > 1
    print(f"rowln tiles two-launch form bf16={bf16}: max |out_f32 difference| {e:.2e}, 16-bit rows differ in {float((ulps > 0).float().mean()):.2%} "
          f"of the elements; more than one step apart: {int(multi.sum())} element(s), at most {int(ulps.max())} steps, the largest of them "
          f"|{float(small[multi].max()) if bool(multi.any()) else 0.0:.2e}|")
    _worst.note("two_launch", bf16, out_f32=e, steps=ulps.max(), largest_multi_step_value=small[multi].max() if bool(multi.any()) else 0.0)
    assert e < TOL32 and bool((ulps <= allowed).all()), (e, int(ulps.max()))
    assert bool((ulps[dd < 0.5 * spacing16(small, bf16)] <= 1).all())


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------
@gpu
@MODES
def test_refusals_leave_outputs_untouched(bf16):
    """Every argument set cs_rowln_check refuses raises ValueError before anything is launched: all three outputs, guard-filled, still hold the
    sentinel everywhere.  Inputs carry a spare row and the outputs their guard bands, so a call that were NOT refused would stay inside the
    test's own allocations.  The unshifted arguments are accepted at the end."""
    import ctypes as ct

    import guard
    from crossscore_amd import _lib

    lib = _lib.load()
    M, n2 = 33, C
    d = _rand_case(M + 1, 99, bf16, True, 2 * C)
    st = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    gf, gh, g2 = guard.guarded((M, C), F32), guard.guarded((M, C), F16), guard.guarded((M, 2 * C), F16)
    for k in ("b", "b2"):  # (a spare 16 bytes behind the shifted bias as well)
        d[k] = torch.cat([d[k], torch.zeros(4, device=DEV)])
    ptr = {k: (v.data_ptr() if v is not None else None) for k, v in d.items()}
    ptr.update(of=gf.view.data_ptr(), oh=gh.view.data_ptr(), o2=g2.view.data_ptr())

    def call(M=M, n2=n2, **over):
        q = dict(ptr, **over)
        if n2 == 0:
            return lib.cs_op_linear_layernorm(q["A"], q["W"], q["b"], q["res"], q["gam"], q["bet"], 1e-5, q["of"], q["oh"], M, C, st)
        return lib.cs_op_linear_layernorm_linear(q["A"], q["W"], q["b"], q["res"], q["gam"], q["bet"], 1e-5, q["of"], q["oh"], q["W2"], q["b2"], n2, 1,
                                                 q["o2"], M, C, st)

    refused = {
        "A + 8 bytes": dict(A=ptr["A"] + 8), "W2 + 8 bytes": dict(W2=ptr["W2"] + 8), "bias + 8 bytes": dict(b=ptr["b"] + 8),
        "out2 + 4 bytes": dict(o2=ptr["o2"] + 4), "M = 0": dict(M=0), "M = -1": dict(M=-1), "n2 = 2 C": dict(n2=2 * C),
        "no output, n2 = 0": dict(n2=0, of=None, oh=None), "W2 null": dict(W2=None),
    }
    with hh.switches(bf16=bf16):
        for what, over in refused.items():
            with pytest.raises(ValueError):
                _lib.check(call(**over))
            torch.cuda.synchronize()
            for g in (gf, gh, g2):
                assert bool((g.ibase == g.sentinel).all()), what
        _lib.check(call())
        torch.cuda.synchronize()
    assert torch.isfinite(gf.view).all()
    gf.check("out_f32")
    gh.check("out_f16")
