"""Tile-level tests of the encoder token-panel kernel (csrc/panel.hip) on its 16x16x32 MFMA tiles: a wave pair's 32 rows are two row tiles of
16, a weight fragment is 16 output features x 32 contraction slots, a D tile hands lane (li, g) token li and features 4g .. 4g+3.
Same op entry points as test_hip_panel.py (cs_op_panel_pack / cs_op_encoder_panel); every case is one or a few launches of at most 257 rows.
The 8-wave kernel (the default) throughout; the four-wave form (csrc/panel4.hip: 32-row blocks, column-split waves, its own weight image) has
its own module, test_hip_panel4_tiles.py; the reference, the operand helpers and the bounds are shared (tests/panel_data.py, tests/bits16.py).

Parent kernel (32x32x16 tiles) on the inputs of test_ragged_rows_at_tile_granularity, measured once with the parent library; the bounds of the
test are the ones test_hip_panel.py carries (fp16: test_panel_vs_torch; bf16: the concurrent-streams test), not these figures:
    fp16: worst over all M and both out-projection settings  max |dx| 2.36e-3, mean |dx| 2.83e-4, max |du| 1.95e-3
    bf16:                                                    max |dx| 4.63e-3, mean |dx| 3.69e-4, max |du| 1.56e-2
(the re-tiled kernel on the same inputs gives the same figures to three digits: the worst cases are the packed-half GELU's, whose arithmetic
is unchanged; the summation order inside a k-step moves the results by fp32 roundings only)
"""
import numpy as np
import pytest
import torch

import hip_helpers as hh
from bits16 import MODES, bits16, vals16
from guard import guarded_out
from kernel_data import gelu_compiled, gelu_kernel_constants, gelu_tool
from panel_data import BOUNDS, C, F, make, reference64, zero_weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ragged_case(M, outproj, bf16, guarded=True):
    """-> (max |dx|, mean |dx|, max |du|) of one launch against panel_data.reference64; guard bands around x and u checked"""
    dev = torch.device(DEV)
    x, o, w = make(M, 900 + M, dev)
    with hh.switches(bf16=bf16, panel_impl=0):
        o16 = bits16(o.float(), bf16)
        img = hh.panel_pack(w["wo"] if outproj else None, w["ls1"] if outproj else None, w["w1"], w["g2"], w["w2"], w["ls2"])
        xk, cx = guarded_out((M, C), torch.float32, init=x)
        u, cu = guarded_out((M, C), torch.float16)
        hh.encoder_panel(xk, o16 if outproj else None, img, w["bo"] if outproj else None, w["b1"], w["b2"], u=u)
        torch.cuda.synchronize()
    if guarded:
        cx("x")
        cu("u")
    ref_x, ref_u = reference64(x, vals16(o16, bf16), w, outproj, bf16)
    assert torch.isfinite(xk).all()
    dx = (xk.double() - ref_x).abs()
    du = (vals16(u, bf16).double() - ref_u).abs()
    return float(dx.max()), float(dx.mean()), float(du.max())




@MODES
@pytest.mark.parametrize("outproj", [True, False], ids=["outproj", "mlp"])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257])
def test_ragged_rows_at_tile_granularity(M, outproj, bf16):
    """Row counts around the 16-row tile, the 32-row pair and the 128-row panel: every row right, nothing written past row M."""
    mx, mean, mu = _ragged_case(M, outproj, bf16)
    print(f"panel tiles M={M} outproj={outproj} bf16={bf16}: max |dx| {mx:.2e} mean |dx| {mean:.2e} max |du| {mu:.2e}")
    bx, bm, bu = BOUNDS[bf16]
    assert mx < bx and mean < bm and mu < bu, (mx, mean, mu)


# ---- one-hot weight layouts -------------------------------------------------------------------------------------------------------------
def _positions():
    """32 (output feature, contraction index over C, hidden unit) triples: output features reach every residue mod 16 on an even and on an odd
    feature tile; contraction indices (and hidden units, the contraction of fc2) every residue mod 32, i.e. every (g, e) slot and both
    accumulator tiles a B fragment is made of; hidden units both feature tiles of a slice, even and odd slices, slices 0 and 47."""
    out = []
    for i in range(32):
        n = 16 * ((5 * i + (i >> 4)) % 24) + i % 16
        k = 32 * (i % 12) + i
        s = i // 2 if i % 2 == 0 else 47 - i // 2
        out.append((n, k, 32 * s + i))
    assert {(n % 16, (n // 16) % 2) for n, _, _ in out} == {(a, b) for a in range(16) for b in range(2)}
    assert {k % 32 for _, k, _ in out} == set(range(32)) and {h % 32 for _, _, h in out} == set(range(32))
    assert {0, 47} <= {h // 32 for _, _, h in out} and {(h // 32) % 2 for _, _, h in out} == {0, 1}
    return out


@MODES
@pytest.mark.parametrize("stage", ["wo", "w1", "w2"])
def test_one_hot_weight_layouts(stage, bf16):
    """A single nonzero in Wo, in W1 (observed through one nonzero of W2 on the same hidden unit) or in W2, everything else zero, LayerScale and
    gamma 1: the output is exact in 16 bits, one column changes and nothing else.  Pins cs_panel_pack_kernel's permutation of rows and
    contraction slots independently of the kernel's arithmetic.
      wo: x = 0, attention output = small integers that differ by row and column  ->  column n of x is column k of the attention output
      w2: b1[hid] = 8, GELU(8) = 8 in both modes (8 - 1.3e-4 rounds to 8)          ->  column n of x is 8 in every row
      w1: rows (+4 at column k, -4 at column k + 192, else 0) have mean 0 and norm2 = +-sqrt(192) = 13.8564 there, far from a rounding
          boundary of either type (13.859375 half, 13.875 bfloat16), and GELU leaves that value as it is  ->  column n is x + that value."""
    dev = torch.device(DEV)
    M = 33  # both row tiles of a pair and a second pair
    rows = torch.arange(M, device=dev)
    with hh.switches(bf16=bf16, panel_impl=0):
        for n, k, hid in _positions():
            w = zero_weights(dev)
            x = torch.zeros(M, C, device=dev)
            o = None
            if stage == "wo":
                w["wo"][n, k] = 1.0
                o = ((rows[:, None] * 7 + torch.arange(C, device=dev)[None, :] * 3) % 17 - 8).float()
                expect = torch.zeros(M, C, device=dev)
                expect[:, n] = o[:, k]
            elif stage == "w2":
                w["w2"][n, hid] = 1.0
                w["b1"][hid] = 8.0
                expect = torch.zeros(M, C, device=dev)
                expect[:, n] = 8.0
            else:
                k2 = (k + 192) % C
                x[:, k], x[:, k2] = 4.0, -4.0
                w["w1"][hid, k] = 1.0
                w["w2"][n, hid] = 1.0
                expect = x.clone()
                expect[:, n] += 13.875 if bf16 else 13.859375
            img = hh.panel_pack(w["wo"] if o is not None else None, w["ls1"] if o is not None else None, w["w1"], w["g2"], w["w2"], w["ls2"])
            hh.encoder_panel(x, bits16(o, bf16) if o is not None else None, img, w["bo"] if o is not None else None, w["b1"], w["b2"], want_u=False)
            torch.cuda.synchronize()
            assert torch.equal(x, expect), (stage, n, k, hid, torch.nonzero(x != expect)[:4].tolist())


# ---- row tiles ------------------------------------------------------------------------------------------------------------------------
@MODES
def test_row_tiles_are_independent(bf16):
    """Rows 0-15 and 16-31 of a pair are two MFMA row tiles that share every weight fragment.  With different data in every row, perturbing one
    row (its residual and its attention output) changes that row's outputs and no other bit."""
    dev = torch.device(DEV)
    M = 64
    x, o, w = make(M, 77, dev)
    with hh.switches(bf16=bf16, panel_impl=0):
        o16 = bits16(o.float(), bf16)
        img = hh.panel_pack(w["wo"], w["ls1"], w["w1"], w["g2"], w["w2"], w["ls2"])
        x0 = x.clone()
        u0 = hh.encoder_panel(x0, o16, img, w["bo"], w["b1"], w["b2"])
        for r in (0, 15, 16, 31, 37, 63):  # both row tiles of the first pair, their edges, the second pair
            xp, op = x.clone(), o16.clone()
            xp[r] = xp[r] * 1.25 + 0.5
            op[r] = o16[(r + 1) % M]
            up = hh.encoder_panel(xp, op, img, w["bo"], w["b1"], w["b2"])
            torch.cuda.synchronize()
            others = torch.arange(M, device=dev) != r
            assert torch.equal(xp[others], x0[others]) and torch.equal(up[others], u0[others]), r
            assert not torch.equal(xp[r], x0[r]) and not torch.equal(up[r], u0[r]), r


# ---- GELU hand-off ---------------------------------------------------------------------------------------------------------------------
@MODES
def test_gelu_hand_off_reaches_every_branch_on_both_row_tiles(bf16):
    """The fc1 pre-activations are a ramp over the hidden units (b1 = -6 .. 6 in steps of 1/128, plus +-8, +-1000, +-60000: the fitted range, both
    clamps, the sign of the relu, values whose half is far from their fp32), one of them moved by a one-hot W1 on rows whose norm2 is +-13.86.
    Rows 0-15 are the A wave's half of every slice (row tile 0), rows 16-31 the B wave's (row tile 1, activated one tick later from the raw
    hand-off); even and odd slices use different hand-off slots.  W2 routes hidden unit 4 n + j to output feature n (j = 0 .. 3: four
    launches), so x[:, n] is the activated value itself: compared with panel_shared.h's GELU evaluated on the host (tools/gelu_pk16_fit.py,
    the model test_gelu_pk16.py checks against the compiled constants) -- exactly in fp16 mode, to the one final bfloat16 rounding in bf16 mode."""
    t = gelu_tool()
    consts = gelu_compiled(gelu_kernel_constants())
    dev = torch.device(DEV)
    M = 32
    k0, hid0 = 37, 32 * 5 + 21
    b1 = (torch.arange(F, dtype=torch.float32) - 768.0) / 128.0
    extremes = [-60000.0, -1000.0, -8.0, 8.0, 1000.0, 60000.0]
    for i, v in enumerate(extremes):  # spread over even and odd slices and both feature tiles of a slice
        b1[32 * (3 + 7 * i) + 5 * i] = v
    pre = b1.clone()
    pre[hid0] += 13.875 if bf16 else 13.859375  # fp32 sum, as the MFMA forms it (one product on the bias)
    pre = pre.numpy().astype(np.float32)
    with np.errstate(over="ignore"):
        h = t.kernel_gelu_bf16(pre, consts) if bf16 else t.kernel_gelu(pre, consts)
    h = torch.from_numpy(np.asarray(h, dtype=np.float64)).to(dev)
    with hh.switches(bf16=bf16, panel_impl=0):
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
