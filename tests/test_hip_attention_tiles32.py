"""The attention kernel's 32x32x16 tile loop (dh = 16, 96, 128, 192: the tiny test net's, ViT-B's, dinov2-large's and dinov2-giant's decoder heads) and
the one-head weights kernel at the same head dims (csrc/attention.hip from "MFMA 32x32x16 tile loop" on, csrc/elementwise.hip attn_weights_kernel).
The sibling tests/test_hip_attention_tiles.py does the same for the 16x16x32 loop (dh = 64, 48); the two loops share no code below the staging macros.

Geometry.  A workgroup is 4 waves of 32 query rows; lane (r = lane & 31, hh = lane >> 5) owns query q0 + r, and in the 32-key half k2 of a 64-key
tile its accumulator e holds key 4 hh + (e & 3) + 8 (e >> 2): keys with key % 8 < 4 live in lane r, the others in lane r + 32, and a row's maximum and
sum cross the two through one shfl_xor 32.  What this makes possible to get wrong: the key order of the packed P operand pf[k2][s2] against the two
transposed V reads, a reference move that does not reach the partner lane, the threshold of the skipped second half (`two`), the ragged mask, and dead
waves (`live_w`) that must still stage tiles and meet the barriers.

Which shape takes which branch (t = tile index, nt = ceil(Lk / 64); LAST = the ragged instance of the tile body, run for t = nt - 1):

  branch                                   shapes
  live_w false (whole wave beyond Lq)      Lq = 1, 31, 32 (waves 1..3), 33, 64 (2, 3), 65, 96 (3), 129 (second block: 1..3), 300 (third block: 2, 3)
  clamped rows inside a live wave          Lq = 1, 31, 33, 65, 97, 129, 300 (12 live rows in wave 1 of the third block)
  two false, t == 0                        Lk = 1, 4, 5, 31, 32
  two false, t > 0                         Lk = 65, 96 (t = 1), 129 (t = 2), 276 (t = 4: four full tiles + 20); 532 in the reference-move test (t = 8)
  two true in LAST, second half ragged     Lk = 33, 36, 63 (t = 0), 97 (t = 1), 296 (t = 4: four full tiles + 40)
  two true in LAST, no mask (Lk % 64 == 0) Lk = 64, 128
  LAST mask with only hh = 0 live          Lk = 1, 4 (t = 0), 65 (t = 1), 129 (t = 2); first key group of the second half: Lk = 33, 36, 97
  both LDS buffers used again              Lk = 129, 276, 296 (nt >= 3)
  move_reference in a full tile            one-hot shapes with nt >= 3 (Lk = 129, 276, 296); tile 8 of Lk = 640 in the reference-move test (ONE row decides)
  move_reference in the LAST tile          one-hot shapes with nt >= 2; tile 8 of Lk = 532 in the reference-move test (ONE row decides, two == false)

The bounds of the random-data checks are those of test_hip_ops.py::test_attention_matches_fp32 (fp16 operands: P rounded to fp16 before PV, O to fp16
on store, fp32 statistics), which runs these head dims already at six fixed shapes."""
import math

import numpy as np
import pytest
import torch

from crossscore_amd import _lib  # noqa: E402
import guard  # noqa: E402
import hip_helpers as hh  # noqa: E402
import bits16 as b16  # noqa: E402
from bits16 import rng, to_dev  # noqa: E402
from kernel_data import attn_code, attn_ref  # noqa: E402

DEV = "cuda"
F16 = torch.float16
DHS = (16, 96, 128, 192)

# hh = 1 without a live key (1, 4), both sides of the 32-key half, tile boundaries, multi-tile runs with a dead (276) / ragged (296) second half
LKS32 = (1, 4, 5, 31, 32, 33, 36, 63, 64, 65, 96, 97, 128, 129, 276, 296)
# dead waves 1..3, clamped rows inside a live wave, a second and a third block
LQS32 = (1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 300)


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("dh", DHS)
def test_one_hot_layout_every_position_and_every_ragged_shape(dh, bf16):
    """One-hot softmax: O[q] == V[key(q)] exactly.  Batch item b selects key (37 q + 11 + b) mod Lk for query q, and there are min(64, Lk) batch
    items, so EVERY query row (all four waves, every block, both lane halves) hits 64 consecutive keys = every position of a 64-key tile, for each
    Lq x Lk of the grid.

    The codes are +-32 on dims 0..10 (the sibling's +-16 would not do at dh = 192).  The kernel multiplies Q by c = log2(e)/sqrt(dh) and rounds it
    to 16 bits, qs = round16(32 c); the matching key's logit is 11 * 32 * qs base-2 units and the nearest other key (one bit differs) has
    9 * 32 * qs, a gap of 64 qs:
        dh = 192: 32 c = 3.3319 -> qs = 3.3320 (fp16), 3.3281 (bf16): gap >= 213
        dh = 128: 32 c = 4.0807 -> gap >= 261;   dh = 96: 32 c = 4.7120 -> gap >= 301
        dh = 16:  32 c = 11.542 -> qs = 11.539 (fp16), 11.5625 (bf16): gap >= 738, peak logit 11 * 32 * 11.5625 = 4070 (harmless in fp32)
    so all losing keys together carry less than 296 * 2^-213 of the weight: nothing of them survives the fp32 sums or shows in a 16-bit output of a
    zero V entry (at +-16 and dh = 192 the gap would be 53 and a bf16 zero would show ~1e-13 on a correct kernel)."""
    rd, fl = b16.rd(bf16), b16.fl(bf16)
    bad = []
    with hh.switches(bf16=bf16):
        for Lk in LKS32:
            B = min(64, Lk)
            K = torch.zeros((B, Lk, dh), device=DEV)
            K[:, :, :11] = 2 * attn_code(torch.arange(Lk, device=DEV))[None]
            V = (torch.arange(Lk * dh, device=DEV).float().view(1, Lk, dh) * 7 % 251 - 125).expand(B, Lk, dh).contiguous()  # exact in 16 bits
            for Lq in LQS32:
                sel = (torch.arange(Lq, device=DEV)[None, :] * 37 + 11 + torch.arange(B, device=DEV)[:, None]) % Lk  # (B, Lq)
                Q = torch.zeros((B, Lq, dh), device=DEV)
                Q[:, :, :11] = 2 * attn_code(sel)
                O = hh.attention(rd(Q), rd(K), rd(V), 1, dh)  # raw Q: the kernel applies log2(e)/sqrt(dh) itself
                want = torch.gather(V, 1, sel[:, :, None].expand(B, Lq, dh))
                err = float((fl(O) - want).abs().max())
                if not err < 1e-20:
                    bad.append((Lq, Lk, err))
    torch.cuda.synchronize()
    assert not bad, bad[:20]


@pytest.mark.gpu
@pytest.mark.parametrize("dh,heads", [(16, 2), (96, 1), (96, 2), (128, 1), (192, 1)])
def test_ragged_grid_matches_fp32_with_poison_behind_keys_and_columns(dh, heads):
    """The Lq x Lk grid on random data against the fp32 softmax (max 4e-3, mean 4e-4, lse 5e-4: test_attention_matches_fp32's).  K and V are views
    into buffers whose rows behind key Lk - 1 AND whose 16 columns behind the last head hold NaN / Inf / 65504: a masked key has p = 0 and 0 x NaN
    would reach O, a dead second half must not reach O at all, and the poison columns sit right behind the last head's last 16-byte chunk, where a
    row read of more than dh elements would land."""
    Cc = heads * dh
    pad, B = 70, 2
    poison = torch.tensor([float("nan"), float("inf"), -float("inf"), 65504.0], device=DEV).to(F16)
    bad, worst, at = [], [0.0, 0.0, 0.0], [None, None, None]
    for Lk in LKS32:
        g = rng(dh * 100 + heads * 10000 + Lk)
        kb = poison[torch.arange(B * (Lk + pad) * (Cc + 16), device=DEV) % 4].view(B, Lk + pad, Cc + 16).clone()
        vb = kb.clone()
        kb[:, :Lk, :Cc] = to_dev(1.5 * g.standard_normal((B, Lk, Cc), dtype=np.float32)).to(F16)
        vb[:, :Lk, :Cc] = to_dev(g.standard_normal((B, Lk, Cc), dtype=np.float32)).to(F16)
        K, V = kb[:, :Lk, :Cc], vb[:, :Lk, :Cc]
        for Lq in LQS32:
            Q = hh.prescale_q(to_dev(1.5 * g.standard_normal((B, Lq, Cc), dtype=np.float32)).to(F16), dh)
            O, lse = hh.attention(Q, K, V, heads, dh, lse=True, q_scale=1.0)
            ref, lse_ref = attn_ref(Q, K.contiguous(), V.contiguous(), heads, dh)
            err = (O.float() - ref).abs()
            fig = (float(err.max()), float(err.mean()), float((lse * math.log(2.0) - lse_ref).abs().max()))
            for i in range(3):
                if worst[i] == worst[i] and not fig[i] <= worst[i]:  # (a NaN figure is kept)
                    worst[i], at[i] = fig[i], (Lq, Lk)
            finite = bool(torch.isfinite(O.float()).all()) and bool(torch.isfinite(lse).all())
            if not (finite and fig[0] < 4e-3 and fig[1] < 4e-4 and fig[2] < 5e-4):
                bad.append((Lq, Lk) + fig)
    torch.cuda.synchronize()
    print(f"dh {dh} heads {heads} fp16: worst max {worst[0]:.2e} at (Lq, Lk) = {at[0]}, mean {worst[1]:.2e} at {at[1]}, lse {worst[2]:.2e} at {at[2]}")
    assert not bad, bad[:20]


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("dh", DHS)
def test_reference_move_needed_by_one_row_only(dh, bf16):
    """A spike of +32 base-2 units on ONE key for ONE query, in tile 8: on a key of either lane half (key % 8 = 1: lane r, 6: lane r + 32), in
    either 32-key half of the tile, for a row of each of the four waves.  The move is decided by the lane that holds the key and must reach its
    partner lane r ^ 32, which holds the other half of the row's sum and of O -- and every row of the wave -- by each row's own amount.  Once more
    with Lk = 8 * 64 + 20 and the spike in the live half of the last tile: the move then runs in the LAST instance of the body with two == false.
    Only dimension 0 carries the spike, so no other (query, key) pair sees it; the random part has a standard deviation of 2 base-2 units at every
    head dim (Q is drawn at 0.5 sqrt(64 / dh)), the sibling's."""
    rd, fl = b16.rd(bf16), b16.fl(bf16)
    heads, Lq = 1, 128
    # fp16: the bounds of test_attention_matches_fp32.  bf16: P and O carry 8 bits instead of 11 (2^3 times the fp16 bound); the statistics are fp32 in both
    tol = (3.2e-2 if bf16 else 4e-3, 5e-4)
    cases = [(640, 32 * half + off) for half in (0, 1) for off in (9, 22)] + [(8 * 64 + 20, off) for off in (9, 14)]  # off % 8 in {1, 6}
    worst = [0.0, 0.0]
    with hh.switches(bf16=bf16):
        for Lk, off in cases:
            key = 64 * 8 + off
            assert key % 8 in (1, 6) and key < Lk
            for q in (5, 32 + 30, 64 + 17, 96 + 31):  # one row of each wave
                g = rng(1000 * off + q + dh + Lk)
                Q = 0.5 * math.sqrt(64 / dh) * g.standard_normal((1, Lq, dh), dtype=np.float32)
                K = 0.5 * g.standard_normal((1, Lk, dh), dtype=np.float32)
                V = g.standard_normal((1, Lk, dh), dtype=np.float32)
                Q[:, :, 0] = 0.0
                K[:, :, 0] = 0.0
                Q[0, q, 0] = 4.0
                K[0, key, 0] = 8.0  # +32 in base-2 units for (q, key) alone: far above kTau = 8
                Qs, Kb, Vb = rd(to_dev(Q)), rd(to_dev(K)), rd(to_dev(V))  # Q taken as already scaled: q_scale = 1
                O, lse = hh.attention(Qs, Kb, Vb, heads, dh, lse=True, q_scale=1.0)
                ref, lse_ref = attn_ref(fl(Qs), fl(Kb), fl(Vb), heads, dh)
                err = float((fl(O) - ref).abs().max())
                lerr = float((lse * math.log(2.0) - lse_ref).abs().max())
                worst = [max(worst[0], err) if err == err else err, max(worst[1], lerr) if lerr == lerr else lerr]
                assert err < tol[0] and lerr < tol[1], (Lk, q, key, err, lerr)
                assert float((fl(O)[0, q] - fl(Vb)[0, key]).abs().max()) < tol[0]  # the spiked row is (all but) that key's V row
    print(f"dh {dh} {'bf16' if bf16 else 'fp16'}: worst max {worst[0]:.2e} lse {worst[1]:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("step,tiles", [(0.9, 8), (1.0, 24), (-1.5, 12)])
@pytest.mark.parametrize("dh", DHS)
def test_lazy_reference_point(dh, step, tiles):
    """test_hip_ops.py::test_attention_lazy_reference_point on this loop: logits that climb by `step` base-2 units per 64-key tile stay below kTau for
    several tiles (P grows up to 256 with no rescale), then cross it; falling logits never move the reference.  Same data recipe (q.u ~ 1, so the
    logits do not depend on dh), same bounds."""
    heads, Lq = 1, 64
    Lk = 64 * tiles
    g = rng(int(10 * abs(step)) + tiles + dh)
    u = g.standard_normal(dh).astype(np.float32)
    u /= np.linalg.norm(u)
    Q = to_dev(np.tile(u[None, None, :], (1, Lq, 1)) * (1 + 0.05 * g.standard_normal((1, Lq, 1)).astype(np.float32)))  # q.u ~ 1 in base-2 units
    ramp = (np.arange(Lk) // 64).astype(np.float32) * step
    K = to_dev(ramp[None, :, None] * u[None, None, :] + 0.3 * g.standard_normal((1, Lk, dh)).astype(np.float32))
    V = to_dev(g.standard_normal((1, Lk, dh), dtype=np.float32))
    Qs, Kb, Vb = Q.to(F16), K.to(F16), V.to(F16)  # Q taken as already scaled: q_scale = 1
    O, lse = hh.attention(Qs, Kb, Vb, heads, dh, lse=True, q_scale=1.0)
    ref, lse_ref = attn_ref(Qs, Kb, Vb, heads, dh)
    torch.cuda.synchronize()
    err, lerr = float((O.float() - ref).abs().max()), float((lse * math.log(2.0) - lse_ref).abs().max())
    print(f"dh {dh} step {step} tiles {tiles}: max {err:.2e} lse {lerr:.2e}")
    assert err < 4e-3
    assert lerr < 5e-4


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("dh,Lk", [(96, 1369), (16, 90), (128, 200), (192, 97)])
def test_rows_are_bitwise_independent_of_their_position(dh, Lk, bf16):
    """The same (Q row, K, V) gives the same bits in any lane of either half, wave, block, head-of-grid position and batch item -- also in the wave
    with 12 live rows (288..299 of Lq = 300) beside two dead ones."""
    rd = b16.rd(bf16)
    heads, Lq, B = 2, 300, 2
    g = rng(dh + Lk)
    Cc = heads * dh
    q1 = 1.5 * g.standard_normal((1, 1, Cc), dtype=np.float32)
    Q = hh.prescale_q(to_dev(np.tile(q1, (B, Lq, 1))), dh)
    K = to_dev(np.tile(1.5 * g.standard_normal((1, Lk, Cc), dtype=np.float32), (B, 1, 1)))
    V = to_dev(np.tile(g.standard_normal((1, Lk, Cc), dtype=np.float32), (B, 1, 1)))
    with hh.switches(bf16=bf16):
        O, lse = hh.attention(rd(Q.float()), rd(K), rd(V), heads, dh, lse=True, q_scale=1.0)
    torch.cuda.synchronize()
    Oi = O.view(torch.int16)
    assert torch.equal(Oi, Oi[:1, :1].expand_as(Oi))
    assert torch.equal(lse, lse[:1, :, :1].expand_as(lse))
    assert bool(torch.isfinite(lse).all())


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("dh", DHS)
def test_attention_weights_one_middle_head(dh, bf16):
    """cs_op_attention_weights at these head dims: lse from the fused kernel (prescaled Q), then P[b][q][k] = exp2(q.k - lse) for head 1 of 3 at a
    ragged shape (Lk = 210: the fourth wave of the only key block has 18 live lanes).  Rows sum to 1 and match the fp32 softmax within 1e-4, the
    bounds of test_attention_weights_one_head; in bf16 too, because the kernel's dot product and the fused kernel's statistics are fp32 on the
    same 16-bit operands.  K is a view with poison rows behind key Lk - 1, which lanes beyond Lk must not read into the output."""
    rd, fl = b16.rd(bf16), b16.fl(bf16)
    heads, head, Lq, Lk, B, pad = 3, 1, 70, 210, 2, 70
    g = rng(8 + dh)
    Cc = heads * dh
    Q = rd(hh.prescale_q(to_dev(1.5 * g.standard_normal((B, Lq, Cc), dtype=np.float32)), dh).float())
    poison = torch.tensor([float("nan"), float("inf"), -float("inf"), 65504.0], device=DEV)
    kb = poison[torch.arange(B * (Lk + pad) * Cc, device=DEV) % 4].view(B, Lk + pad, Cc).clone()
    kb[:, :Lk] = to_dev(1.5 * g.standard_normal((B, Lk, Cc), dtype=np.float32))
    kb = rd(kb)
    assert bool(torch.isnan(fl(kb[:, Lk:])).any())
    K = kb[:, :Lk]
    V = rd(to_dev(g.standard_normal((B, Lk, Cc), dtype=np.float32)))
    with hh.switches(bf16=bf16):
        _, lse = hh.attention(Q, K, V, heads, dh, lse=True, q_scale=1.0)
        Pw = hh.attention_weights(Q, K, heads, dh, lse, head=head, q_scale=1.0)
    torch.cuda.synchronize()
    q = fl(Q).view(B, Lq, heads, dh)[:, :, head]
    k = fl(K.contiguous()).view(B, Lk, heads, dh)[:, :, head]
    p_ref = torch.softmax((q @ k.transpose(-1, -2)) * math.log(2.0), dim=-1)
    assert bool(torch.isfinite(Pw).all())
    err, serr = float((Pw - p_ref).abs().max()), float((Pw.sum(-1) - 1).abs().max())
    print(f"dh {dh} {'bf16' if bf16 else 'fp16'}: weights max {err:.2e} row sum {serr:.2e}")
    assert err < 1e-4
    assert serr < 1e-4


def _untouched(g):
    """every element of a guarded allocation, the view included, still holds the sentinel"""
    torch.cuda.synchronize()
    assert bool((g.ibase == g.sentinel).all())


def _row_misaligned(B, L, Cc, by):
    """(B, L, Cc) zeros whose rows are Cc + by elements apart"""
    return torch.zeros((B, L, Cc + by), dtype=F16, device=DEV)[:, :, :Cc]


def _batch_misaligned(B, L, Cc, by):
    """(B, L, Cc) zeros with contiguous rows whose batch items are L * Cc + by elements apart"""
    return torch.zeros((B * (L * Cc + by),), dtype=F16, device=DEV).as_strided((B, L, Cc), (L * Cc + by, Cc, 1))


@pytest.mark.gpu
def test_attention_entry_points_refuse_misaligned_strides_and_long_key_spans():
    """cs_op_attention and cs_op_attention_weights read Q / K (/ V) rows in 16-byte chunks and (the fused kernel) address a key tile with 32-bit
    offsets: row and batch strides that are no multiple of 8 elements (O: 4), and Lk * row stride >= 2^30 elements, are a ValueError before any
    launch, and the guard-filled outputs keep every sentinel.  Every refused operand is a view inside its own allocation; the long key spans
    exist as numbers only (the call returns before anything is dereferenced)."""
    B, heads, dh, Lq, Lk = 2, 2, 16, 8, 24
    Cc = heads * dh
    lib = _lib.load()
    ok = lambda L: torch.zeros((B, L, Cc), dtype=F16, device=DEV)  # noqa: E731
    lse_in = torch.zeros((B, heads, Lq), dtype=torch.float32, device=DEV)

    # ---- cs_op_attention_weights
    gw = guard.guarded((B, Lq, Lk), torch.float32)
    for Q, K in [(_row_misaligned(B, Lq, Cc, 4), ok(Lk)), (ok(Lq), _row_misaligned(B, Lk, Cc, 4)),
                 (_batch_misaligned(B, Lq, Cc, 4), ok(Lk)), (ok(Lq), _batch_misaligned(B, Lk, Cc, 4))]:
        with pytest.raises(ValueError):
            hh.attention_weights(Q, K, heads, dh, lse_in, 1, q_scale=1.0, out=gw.view)
        _untouched(gw)
    Q, K = ok(Lq), ok(Lk)
    for big_lk, ldk in [(1 << 20, 1 << 10), ((1 << 30) // Cc, Cc)]:
        rc = lib.cs_op_attention_weights(hh._p(Q), hh._p(K), Cc, ldk, Lq * Cc, Lk * Cc, B, heads, Lq, big_lk, dh, 1.0, hh._p(lse_in), 1,
                                         hh._p(gw.view), hh._stream())
        with pytest.raises(ValueError):
            _lib.check(rc)
        _untouched(gw)

    # ---- cs_op_attention
    go = guard.guarded((B, Lq, Cc), F16)
    gl = guard.guarded((B, heads, Lq), torch.float32)
    refused = [dict(Q=_row_misaligned(B, Lq, Cc, 4)), dict(K=_row_misaligned(B, Lk, Cc, 4)), dict(V=_row_misaligned(B, Lk, Cc, 4)),
               dict(Q=_batch_misaligned(B, Lq, Cc, 4)), dict(K=_batch_misaligned(B, Lk, Cc, 4)), dict(V=_batch_misaligned(B, Lk, Cc, 4))]
    for kw in refused:
        a = dict(Q=ok(Lq), K=ok(Lk), V=ok(Lk))
        a.update(kw)
        with pytest.raises(ValueError):
            hh.attention(a["Q"], a["K"], a["V"], heads, dh, q_scale=1.0, O=go.view, L=gl.view)
        _untouched(go)
        _untouched(gl)
    # O rows / batch items 2 elements off a multiple of 4: views into guarded flat allocations
    g_row = guard.guarded((B * Lq * (Cc + 2),), F16)
    g_bat = guard.guarded((B * (Lq * Cc + 2),), F16)
    for g, strides in [(g_row, (Lq * (Cc + 2), Cc + 2, 1)), (g_bat, (Lq * Cc + 2, Cc, 1))]:
        O = g.base.as_strided((B, Lq, Cc), strides, g.front)
        with pytest.raises(ValueError):
            hh.attention(ok(Lq), ok(Lk), ok(Lk), heads, dh, q_scale=1.0, O=O, L=gl.view)
        _untouched(g)
        _untouched(gl)
    Q, K, V = ok(Lq), ok(Lk), ok(Lk)
    for big_lk, ldk, ldv in [(1 << 20, 1 << 10, Cc), (1 << 20, Cc, 1 << 10), ((1 << 30) // Cc, Cc, Cc)]:
        rc = lib.cs_op_attention(hh._p(Q), hh._p(K), hh._p(V), hh._p(go.view), Cc, ldk, ldv, Cc, Lq * Cc, Lk * Cc, Lk * Cc, Lq * Cc, B, heads, Lq, big_lk, dh,
                                 1.0, hh._p(gl.view), hh._stream())
        with pytest.raises(ValueError):
            _lib.check(rc)
        _untouched(go)
        _untouched(gl)
