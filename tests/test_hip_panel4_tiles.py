"""Tile-level tests of the four-wave form of the encoder token-panel kernel (csrc/panel4.hip), the counterpart of test_hip_panel_tiles.py (which
pins the 8-wave kernel's 16-row tiles).  What differs here and is pinned here: wave w owns output columns 96 w .. 96 w + 95 in three 32 x 32
tiles for all four 32-row blocks (panel4_perm maps MFMA row i to a feature of its tile); the weight image holds two contraction layouts (natural
for the out-projection, tiled for fc1 / fc2); fc1 is split by row block and the activated slice crosses the waves through two LDS hand-off
buffers; b1 and b2 enter through the matrix pipe, split hi + lo; the bf16 instantiation alternates two fc1 accumulator buffers; the first and
last ticks are instantiations of their own.  Same op entry points (cs_op_panel_pack / cs_op_encoder_panel) behind cs_debug_panel_impl(1); every
case is one or a few launches of at most 257 rows; every test runs with fp16 and with bf16 operands.

Measured against the fp64 reference on the same rounded operands (panel_data.reference64), worst over the cases of the test:
  test_ragged_rows_at_row_block_granularity (all M, both out-projection settings; bounds: panel_data.BOUNDS)
    fp16: max |dx| 2.36e-3, mean |dx| 2.83e-4, max |du| 1.96e-3
    bf16: max |dx| 4.85e-3, mean |dx| 3.70e-4, max |du| 1.56e-2
  (the 8-wave kernel's figures on its own row counts, test_hip_panel_tiles.py: 2.36e-3 / 2.83e-4 / 1.95e-3 and 4.63e-3 / 3.69e-4 / 1.56e-2)
  test_random_b2_is_its_hi_plus_lo: x_out is the host split hi + lo bit for bit in both types, the fp16 features of magnitude below 2^-3 included:
  a subnormal half lo passes through v_mfma_f32_32x32x16_f16 unflushed.  max |x_out - b2| 2.38e-7 (fp16), 1.45e-5 (bf16).
  test_b2_on_random_residual (|x_out - (x + b2)| in fp64, both out-projection settings alike; bound: the split's own error + two fp32 ulps)
    fp16: max 7.15e-7; closest to its bound 9.55e-9 of 1.12e-8
    bf16: max 1.50e-5; closest to its bound 1.477e-5 of 1.502e-5
"""
import numpy as np
import pytest
import torch

import hip_helpers as hh
from bits16 import MODES, bits16, r16, vals16
from guard import guarded_out
from kernel_data import gelu_compiled, gelu_kernel_constants, gelu_tool
from panel_data import BOUNDS, C, F, make, reference64, zero_weights

pytestmark = pytest.mark.gpu

HT, NTICK = 64, 24  # hidden units per tick of the MLP loop, ticks
DEV = "cuda:0"


def _perm4(i):
    """panel4_perm: MFMA row i of a 32-feature tile -> feature of the tile"""
    return 16 * ((i >> 2) & 1) + (i & 3) + 4 * (i >> 3)


assert sorted(_perm4(i) for i in range(32)) == list(range(32))


# ---- 1. ragged rows ---------------------------------------------------------------------------------------------------------------------
def _nan_backed16(t16, extra=128):
    """a 16-bit operand tensor as the leading rows of a larger buffer whose other rows are NaN in both operand types (bits 0x7FFF)"""
    M = t16.shape[0]
    buf = torch.full((M + extra, t16.shape[1]), 0x7FFF, dtype=torch.int16, device=t16.device).view(torch.float16)
    buf[:M] = t16
    return buf[:M]


def _ragged_case(M, outproj, bf16, want_u=True):
    """-> (max |dx|, mean |dx|, max |du| or None) of one launch against panel_data.reference64.  x and u lie between guard bands of NaN bits (x's rows
    behind M are therefore NaN, as are the attention output's): the kernel clamps its reads to row M - 1 and must neither let those rows in nor
    write to them."""
    dev = torch.device(DEV)
    x, o, w = make(M, 900 + M, dev)
    with hh.switches(bf16=bf16, panel_impl=1):
        o16 = _nan_backed16(bits16(o.float(), bf16))
        img = hh.panel_pack(w["wo"] if outproj else None, w["ls1"] if outproj else None, w["w1"], w["g2"], w["w2"], w["ls2"])
        xk, cx = guarded_out((M, C), torch.float32, init=x)
        u, cu = guarded_out((M, C), torch.float16) if want_u else (None, None)
        hh.encoder_panel(xk, o16 if outproj else None, img, w["bo"] if outproj else None, w["b1"], w["b2"], want_u=want_u, u=u)
        torch.cuda.synchronize()
    cx("x")
    if want_u:
        cu("u")
    ref_x, ref_u = reference64(x, vals16(o16, bf16), w, outproj, bf16)
    assert torch.isfinite(xk).all()
    dx = (xk.double() - ref_x).abs()
    du = (vals16(u, bf16).double() - ref_u).abs() if want_u else None
    if want_u:
        assert torch.isfinite(du).all()
    return float(dx.max()), float(dx.mean()), (float(du.max()) if want_u else None)


RAGGED_M = [1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 161, 257]


@MODES
@pytest.mark.parametrize("outproj", [True, False], ids=["outproj", "mlp"])
@pytest.mark.parametrize("M", RAGGED_M)
def test_ragged_rows_at_row_block_granularity(M, outproj, bf16):
    """Row counts around the 32-row block (one wave's fc1 rows), the 128-row panel and a second and third workgroup: every row right, rows
    behind M neither read into a result nor written."""
    mx, mean, mu = _ragged_case(M, outproj, bf16)
    print(f"panel4 tiles M={M} outproj={outproj} bf16={bf16}: max |dx| {mx:.2e} mean |dx| {mean:.2e} max |du| {mu:.2e}")
    bx, bm, bu = BOUNDS[bf16]
    assert mx < bx and mean < bm and mu < bu, (mx, mean, mu)


@MODES
def test_ragged_rows_without_the_normalised_output(bf16):
    """u_out = null: the same x, no second statistics pass, nothing else written (M = 97: three full row blocks and one row of the fourth)."""
    mx, mean, _ = _ragged_case(97, True, bf16, want_u=False)
    print(f"panel4 tiles M=97 outproj=True bf16={bf16} want_u=False: max |dx| {mx:.2e} mean |dx| {mean:.2e}")
    bx, bm, _ = BOUNDS[bf16]
    assert mx < bx and mean < bm, (mx, mean)


# ---- 2. one-hot weight layouts ----------------------------------------------------------------------------------------------------------
def _tiled_kstep(k):
    """the k-step of contraction index k in the tiled order 32 (ks >> 1) + 16 h + 8 (ks & 1) + e of fc1 / fc2"""
    return 2 * (k >> 5) + ((k >> 3) & 1)


def _positions():
    """64 (output feature n, contraction index k over C, hidden unit hid) triples.
      n   every residue mod 32 (every panel4_perm slot) and all 12 output tiles (every wave x column tile)
      k   Wo, natural order: every residue mod 16 (lane half h, element e) and all 24 k-steps -- hence every ks % 6 slot of the weight pool,
          both B-fragment buffers (ks & 1) and all six LDS planes (ks / 4);
          W1, tiled order: every residue mod 32 and all 24 k-steps of that order
      hid every residue mod 64 (both hidden tiles of a tick, every perm slot; as the contraction of fc2 every (kk, h, e) slot of a tick) and all
          24 ticks, the ticks with instantiations of their own (0, 1, 22, 23: iterations -1 .. 1 and NTICK - 2 .. NTICK) more than once"""
    out = []
    for i in range(64):
        n = 32 * ((5 * i + i // 12) % 12) + (13 * i + 7) % 32
        k = 32 * (i % 12) + (i + 8 * (i // 32)) % 32
        tick = i // 2 if i < 48 else (0, 23, 1, 22)[i % 4]
        hid = HT * tick + (29 * i + 3) % 64
        out.append((n, k, hid))
    ns, ks, hs = [p[0] for p in out], [p[1] for p in out], [p[2] for p in out]
    assert all(0 <= n < C for n in ns) and all(0 <= k < C for k in ks) and all(0 <= h < F for h in hs)
    assert {n % 32 for n in ns} == set(range(32)) and {_perm4(n % 32) for n in ns} == set(range(32)) and {n // 32 for n in ns} == set(range(12))
    assert {k % 16 for k in ks} == set(range(16)) and {k // 16 for k in ks} == set(range(24))
    assert {(k // 16) % 6 for k in ks} == set(range(6)) and {(k // 16) & 1 for k in ks} == {0, 1} and {k // 64 for k in ks} == set(range(6))
    assert {k % 32 for k in ks} == set(range(32)) and {_tiled_kstep(k) for k in ks} == set(range(24))
    assert {h % 64 for h in hs} == set(range(64)) and {h // HT for h in hs} == set(range(NTICK))
    ticks = [h // HT for h in hs]
    assert all(ticks.count(t) > 1 for t in (0, 1, NTICK - 2, NTICK - 1))
    assert len(set(out)) == 64
    return out


_POSITIONS = _positions()  # (at import: a wrong set fails at collection, without a GPU)


@MODES
@pytest.mark.parametrize("stage", ["wo", "w1", "w2"])
def test_one_hot_weight_layouts(stage, bf16):
    """A single nonzero in Wo, in W1 (observed through one nonzero of W2 on the same hidden unit) or in W2, everything else zero: the output is
    exact in 16 bits, one column changes and nothing else.  Pins cs_panel4_pack_kernel's row permutation, its two contraction layouts and the
    (wave, k-step, tile) order of its sections independently of the kernel's arithmetic.  M = 129: all four row blocks and a second workgroup
    with one row, so every position passes through every wave's fc1 and every hand-off read.
    Scale folding in the same launches: ls1, g2 and ls2 are 3.0 everywhere but at the position's own index, where they are a power of two
    (ls1[n] = 0.5, g2[k] = 0.25, ls2[n] = 2.0); a scale taken from another row or column shows as a factor 3.
      wo: x = 0, attention output = small integers that differ by row and column  ->  column n of x is 0.5 x column k of the attention output
      w2: b1[hid] = 8, GELU(8) = 8 in both modes (8 - 1.3e-4 rounds to 8)          ->  column n of x is 2 x 8 in every row
      w1: rows (+4 at column k, -4 at column k + 192, else 0) have mean 0 and norm2 = +-sqrt(192) = 13.8564 there, which rounds to 13.859375
          (half; boundary 13.85547) / 13.875 (bfloat16; boundary 13.84375).  gamma is folded into the WEIGHT (W1' = W1 g2), not into norm2(x),
          so the scaling moves nothing towards a rounding boundary; but a folded weight of 0.25 would bring the pre-activation to 3.46, where
          GELU is no longer the identity in 16 bits.  The constant that moves is therefore W1[hid, k] = 4 (not 1): the folded weight is
          exactly 1, the pre-activation 13.859375 / 13.875 as in the 8-wave test, and a g2 from another column gives 12 times that
          ->  column n is x + 2 x that value."""
    dev = torch.device(DEV)
    M = 129
    rows = torch.arange(M, device=dev)
    o = ((rows[:, None] * 7 + torch.arange(C, device=dev)[None, :] * 3) % 17 - 8).float()
    with hh.switches(bf16=bf16, panel_impl=1):
        o16 = bits16(o, bf16)
        w = zero_weights(dev)
        for n, k, hid in _POSITIONS:
            for name, idx, v in (("ls1", n, 0.5), ("g2", k, 0.25), ("ls2", n, 2.0)):
                w[name].fill_(3.0)
                w[name][idx] = v
            x = torch.zeros(M, C, device=dev)
            outproj = stage == "wo"
            if stage == "wo":
                w["wo"][n, k] = 1.0
                expect = torch.zeros(M, C, device=dev)
                expect[:, n] = 0.5 * o[:, k]
            elif stage == "w2":
                w["w2"][n, hid] = 1.0
                w["b1"][hid] = 8.0
                expect = torch.zeros(M, C, device=dev)
                expect[:, n] = 16.0
            else:
                k2 = (k + 192) % C
                x[:, k], x[:, k2] = 4.0, -4.0
                w["w1"][hid, k] = 4.0
                w["w2"][n, hid] = 1.0
                expect = x.clone()
                expect[:, n] += 2.0 * (13.875 if bf16 else 13.859375)
            img = hh.panel_pack(w["wo"] if outproj else None, w["ls1"] if outproj else None, w["w1"], w["g2"], w["w2"], w["ls2"])
            hh.encoder_panel(x, o16 if outproj else None, img, w["bo"] if outproj else None, w["b1"], w["b2"], want_u=False)
            torch.cuda.synchronize()
            assert torch.equal(x, expect), (stage, n, k, hid, torch.nonzero(x != expect)[:4].tolist())
            w["wo"][n, k] = w["w1"][hid, k] = w["w2"][n, hid] = w["b1"][hid] = 0.0


# ---- 3. rows across row blocks and waves --------------------------------------------------------------------------------------------------
@MODES
def test_rows_are_independent_across_row_blocks_and_waves(bf16):
    """Rows meet in LDS three times: the LayerNorm exchange red[wave][row], fc1 by row block (wave w runs rows 32 w .. 32 w + 31 for everybody)
    and the hand-off buffers every wave reads all sixteen fragments of.  With different data in every row, perturbing one row (its residual and
    its attention output) changes that row's x and u and no other bit: first and last row of every row block, and of a second workgroup."""
    dev = torch.device(DEV)
    M = 160
    x, o, w = make(M, 77, dev)
    with hh.switches(bf16=bf16, panel_impl=1):
        o16 = bits16(o.float(), bf16)
        img = hh.panel_pack(w["wo"], w["ls1"], w["w1"], w["g2"], w["w2"], w["ls2"])
        x0 = x.clone()
        u0 = hh.encoder_panel(x0, o16, img, w["bo"], w["b1"], w["b2"])
        for r in (0, 31, 32, 63, 64, 95, 96, 127, 128, 159):
            xp, op = x.clone(), o16.clone()
            xp[r] = xp[r] * 1.25 + 0.5
            op[r] = o16[(r + 1) % M]
            up = hh.encoder_panel(xp, op, img, w["bo"], w["b1"], w["b2"])
            torch.cuda.synchronize()
            others = torch.arange(M, device=dev) != r
            assert torch.equal(xp[others], x0[others]) and torch.equal(up[others], u0[others]), r
            assert not torch.equal(xp[r], x0[r]) and not torch.equal(up[r], u0[r]), r


# ---- 4. GELU hand-off -------------------------------------------------------------------------------------------------------------------
def _extreme_units():
    """hidden units of the six extreme biases: (tick, hidden tile) over even and odd ticks x both tiles, ticks 0 and NTICK - 1 among them"""
    where = [(0, 1), (5, 0), (10, 1), (15, 1), (18, 0), (NTICK - 1, 0)]
    assert {(t % 2, ht) for t, ht in where} == {(a, b) for a in range(2) for b in range(2)} and {0, NTICK - 1} <= {t for t, _ in where}
    return [HT * t + 32 * ht + 5 * i + 3 for i, (t, ht) in enumerate(where)]


_EXTREME_UNITS = _extreme_units()


@MODES
def test_gelu_hand_off_reaches_every_branch_on_all_four_row_blocks(bf16):
    """The fc1 pre-activations are a ramp over the hidden units (b1 = -6 .. 6 in steps of 1/128, plus +-8, +-1000, +-60000 on even and odd ticks,
    both hidden tiles, the first and the last tick: the fitted range, both clamps, the sign of the relu, values whose half is far from their
    fp32), one of them moved by a one-hot W1 on rows whose norm2 is +-13.86.  M = 128: wave w activates row block w of every slice and hands it
    to the other three through hand-off buffer t & 1; in the bf16 form even and odd ticks also use different accumulator buffers (hA / hB).
    W2 routes hidden unit 4 n + j to output feature n (j = 0 .. 3: four launches), so x[:, n] is the activated value itself: compared with
    panel_shared.h's GELU evaluated on the host (tools/gelu_pk16_fit.py, the model test_gelu_pk16.py checks against the compiled constants) --
    exactly in fp16 mode, to the one final bfloat16 rounding in bf16 mode.
    Every hidden unit has a bias of its own, so the test also pins the b1 lookup (b1g + (t + 1) * HT * 4, offset 128 for the second tile,
    panel4_perm).  Not observable here: the hi + lo split of b1 -- the pre-activation is rounded to the operand type before the GELU, and every
    bias of this test is hi + lo exactly (the fp32 sums the MFMA forms are exact in any order)."""
    t = gelu_tool()
    consts = gelu_compiled(gelu_kernel_constants())
    dev = torch.device(DEV)
    M = 128
    k0, hid0 = 37, HT * 7 + 32 + 21
    b1 = (torch.arange(F, dtype=torch.float32) - 768.0) / 128.0
    for hid, v in zip(_EXTREME_UNITS, [-60000.0, -1000.0, -8.0, 8.0, 1000.0, 60000.0]):
        b1[hid] = v
    assert hid0 not in _EXTREME_UNITS
    pre = b1.clone()
    pre[hid0] += 13.875 if bf16 else 13.859375  # fp32 sum, as the MFMA forms it (one product on the two bias terms): exact
    pre = pre.numpy().astype(np.float32)
    with np.errstate(over="ignore"):
        h = t.kernel_gelu_bf16(pre, consts) if bf16 else t.kernel_gelu(pre, consts)
    h = torch.from_numpy(np.asarray(h, dtype=np.float64)).to(dev)
    with hh.switches(bf16=bf16, panel_impl=1):
        for j in range(4):
            w = zero_weights(dev)
            w["b1"] = b1.to(dev)
            w["w1"][hid0, k0] = 1.0
            for n in range(C):
                w["w2"][n, 4 * n + j] = 1.0
            x = torch.zeros(M, C, device=dev)
            x[:, k0], x[:, k0 + 192] = 4.0, -4.0
            img = hh.panel_pack(None, None, w["w1"], w["g2"], w["w2"], w["ls2"])
            hh.encoder_panel(x, None, img, None, w["b1"], w["b2"], want_u=False)
            torch.cuda.synchronize()
            got = x.double()
            got[:, k0] -= 4.0   # (these two columns carry the residual as well: their sums are rounded once more in fp32)
            got[:, k0 + 192] += 4.0
            want = h[torch.arange(C, device=dev) * 4 + j][None, :].expand(M, C)
            free = torch.ones(C, dtype=torch.bool, device=dev)
            free[k0] = free[k0 + 192] = False
            if bf16:
                ulp = torch.clamp(want.abs(), min=2.0 ** -126) * 2.0 ** -7
                assert ((got - want).abs() <= ulp)[:, free].all(), j
            else:
                assert torch.equal(got[:, free], want[:, free]), (j, torch.nonzero(got[:, free] != want[:, free])[:4].tolist())
            assert ((got - want).abs() <= 1e-5 + 2.0 ** -7 * want.abs())[:, ~free].all()


# ---- 5. b2 through the matrix pipe --------------------------------------------------------------------------------------------------------
def _split16(b, bf16):
    """the kernel's split of an fp32 bias: hi = rnd16(b), lo = rnd16(b - hi) -> (hi, lo) as fp32 values"""
    hi = r16(b, bf16)
    lo = r16(b - hi, bf16)
    return hi, lo


def _exact_b2(bf16):
    """(a): b2[n] = hi[n] + lo[n] from values of the operand type: hi distinct per feature with a 7-bit mantissa (a value of both types),
    |hi| in [2^-3, 4); lo a NORMAL value of the type of at most half an ulp of hi (fp16: 2^-14 is the smallest, so the binade of 2^-3 gets
    exactly half an ulp -- a tie in the kernel's rnd16(b2), whose split (hi + ulp, -lo) has the same sum).  hi + lo needs at most 22 / 16 bits."""
    n = torch.arange(C, dtype=torch.float64)
    e = n % 5 - 3                                     # |hi| in [2^e, 2^(e+1))
    hi = (1.0 + ((37 * n + 11) % 128) / 128.0) * 2.0 ** e * (1.0 - 2.0 * ((n // 5) % 2))
    ulp = 2.0 ** (e - (7 if bf16 else 10))
    frac = torch.tensor([0.5, 0.375, 0.3125, 0.4375, 0.25], dtype=torch.float64)[(n // 3).long() % 5]
    lo = ulp * frac
    if not bf16:
        lo = torch.clamp(lo, min=2.0 ** -14)
    lo = lo * (1.0 - 2.0 * ((n // 7) % 2))
    assert len(set(hi.tolist())) == C and float(hi.abs().min()) >= 0.125 and float(hi.abs().max()) < 4.0
    assert torch.equal(r16(hi, bf16), hi) and torch.equal(r16(lo, bf16), lo)
    assert bool((lo.abs() <= ulp / 2).all()) and float(lo.abs().min()) >= (2.0 ** -126 if bf16 else 2.0 ** -14)
    b = hi + lo
    assert torch.equal(b.float().double(), b)          # exactly an fp32 value
    h2, l2 = _split16(b.float(), bf16)
    assert torch.equal(h2 + l2, b.float())             # the split reproduces it (fp32 sum of the two parts: exact)
    return b.float()


_EXACT_B2 = {bf: _exact_b2(bf) for bf in (False, True)}  # (at import, on the CPU: the construction's own claims)


def _b2_launch(x, b2, outproj, bf16):
    """all weights zero, b1 = 0 -> x after one launch"""
    dev = x.device
    w = zero_weights(dev)
    w["b2"] = b2.to(dev)
    with hh.switches(bf16=bf16, panel_impl=1):
        img = hh.panel_pack(w["wo"] if outproj else None, w["ls1"] if outproj else None, w["w1"], w["g2"], w["w2"], w["ls2"])
        o16 = torch.zeros(x.shape[0], C, dtype=torch.float16, device=dev) if outproj else None
        xk = x.clone()
        hh.encoder_panel(xk, o16, img, w["bo"] if outproj else None, w["b1"], w["b2"], want_u=False)
        torch.cuda.synchronize()
    return xk


def _random_b2():
    """fp32 values in +-4 with full mantissas (drawn in fp64: torch.rand's fp32 values are multiples of 2^-24, most of them hi + lo exactly)"""
    g = torch.Generator(device="cpu").manual_seed(4242)
    return (torch.rand(C, generator=g, dtype=torch.float64) * 8.0 - 4.0).float()


def _claim(b2, bf16):
    """the source's own claim for the split bias: 2^-16 |b2| in bf16; 2^-22 |b2| + 2^-25 in fp16 (an unflushed subnormal lo)"""
    return b2.double().abs() * (2.0 ** -16 if bf16 else 2.0 ** -22) + (0.0 if bf16 else 2.0 ** -25)


@MODES
@pytest.mark.parametrize("outproj", [True, False], ids=["outproj", "mlp"])
def test_b2_exactly_representable_as_hi_plus_lo(outproj, bf16):
    """(a) x = 0, all weights zero: x_out[:, n] = b2[n] bit for bit in every row of both workgroups.  Distinct values per feature pin the permuted
    lookup p.b2[96 w + 32 ct + panel4_perm(jb)]."""
    dev = torch.device(DEV)
    M = 129
    b2 = _EXACT_B2[bf16]
    xk = _b2_launch(torch.zeros(M, C, device=dev), b2, outproj, bf16)
    expect = b2.to(dev)[None, :].expand(M, C)
    assert torch.equal(xk, expect), torch.nonzero(xk != expect)[:4].tolist()


@MODES
def test_random_b2_is_its_hi_plus_lo(bf16):
    """(b) random fp32 b2 in +-4 (about a dozen of magnitude below 2^-3, whose fp16 lo is subnormal): x_out is float(hi) + float(lo) of the host
    split exactly -- the MFMA adds the two products to a zero accumulator without a rounding and takes a subnormal half operand as it is -- and
    within the source's claim against b2 itself."""
    dev = torch.device(DEV)
    M = 129
    b2 = _random_b2()
    hi, lo = _split16(b2, bf16)
    if not bf16:
        assert int(((lo != 0) & (lo.abs() < 2.0 ** -14)).sum()) >= 4   # the subnormal case is in the set
    model = hi + lo
    assert torch.equal(model.double(), hi.double() + lo.double())
    assert bool(((model.double() - b2.double()).abs() <= _claim(b2, bf16)).all())   # (the model itself meets the claim)
    xk = _b2_launch(torch.zeros(M, C, device=dev), b2, False, bf16)
    err = (xk.double() - b2.double().to(dev)[None, :]).abs()
    print(f"panel4 b2 split bf16={bf16}: max |x_out - b2| {float(err.max()):.3e}, max relative {float((err / b2.double().abs().to(dev)).max()):.3e}")
    expect = model.to(dev)[None, :].expand(M, C)
    assert torch.equal(xk, expect), torch.nonzero(xk != expect)[:4].tolist()
    assert bool((err <= _claim(b2, bf16).to(dev)[None, :]).all())


def _ulp32(v):
    """the fp32 ulp of the binade of |v| (fp64 tensor)"""
    return 2.0 ** (torch.floor(torch.log2(torch.clamp(v.abs(), min=2.0 ** -126))) - 23)


@MODES
@pytest.mark.parametrize("outproj", [True, False], ids=["outproj", "mlp"])
def test_b2_on_random_residual(outproj, bf16):
    """(c) the random b2 of (b) on the random residual of panel_data.make, all weights zero: against fp64 x + b2 the error is the split's own
    (|hi + lo - b2| per feature, known exactly) plus two fp32 ulps of the largest of |x|, |b2|, |x + b2| -- the accumulator takes two products,
    with two roundings at most."""
    dev = torch.device(DEV)
    M = 129
    x, _, _ = make(M, 31, dev)
    b2 = _random_b2()
    hi, lo = _split16(b2, bf16)
    split_err = ((hi.double() + lo.double()) - b2.double()).abs().to(dev)
    xk = _b2_launch(x, b2, outproj, bf16)
    ref = x.double() + b2.double().to(dev)[None, :]
    big = torch.maximum(torch.maximum(x.double().abs(), b2.double().abs().to(dev)[None, :].expand(M, C)), ref.abs())
    bound = split_err[None, :] + 2.0 * _ulp32(big)
    err = (xk.double() - ref).abs()
    worst = int((err / bound).argmax())
    print(f"panel4 b2 on random x outproj={outproj} bf16={bf16}: max |d| {float(err.max()):.3e}; worst against its bound {float(err.flatten()[worst]):.3e} "
          f"of {float(bound.flatten()[worst]):.3e} (split error {float(split_err.max()):.3e} at most)")
    assert bool((err <= bound).all()), (worst // C, worst % C)
