"""The attention kernel's 16x16x32 tile loop (dh = 64, 48) and its skipping of rows and keys that do not exist (csrc/attention.hip).

What the layout makes possible to get wrong, beyond tests/test_hip_ops.py: the key order inside the packed P operand against the two transposed
V reads, the four lanes that share a query row's softmax statistics, the zero half of the second QK^T k-step at dh = 48, and every combination of
dead query tile / dead wave / dead 16-key tile / dead PV k-step in the ragged last tile.  The bounds of the random-data checks are those of
test_hip_ops.py::test_attention_matches_fp32 (fp16 operands: P rounded to fp16 before PV, O to fp16 on store, fp32 statistics)."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import hip_helpers as hh  # noqa: E402
import bits16 as b16  # noqa: E402
from bits16 import rng, to_dev  # noqa: E402
from kernel_data import attn_code, attn_ref  # noqa: E402

DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16 = torch.float16

# every dead-tile / dead-k-step combination of a 64-key tile, and dead second query tiles / dead waves of a 128-row block
LKS = (1, 15, 16, 17, 26, 31, 32, 33, 47, 48, 49, 63, 64, 65, 1370)
LQS = (1, 16, 17, 90, 112, 113, 128, 129, 1370)


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("dh", [64, 48])
def test_one_hot_layout_every_position_and_every_ragged_shape(dh, bf16):
    """One-hot softmax: O[q] == V[key(q)] exactly.  Batch item b selects key (37 q + 11 + b) mod Lk for query q, and there are min(64, Lk) batch
    items, so EVERY query row (both query tiles of a wave, all four waves, every block) hits 64 consecutive keys = every position of a 64-key tile,
    for each Lq x Lk of the grid.  The losing keys are at least 2^-92 down: nothing of them survives the fp32 sums."""
    rd, fl = b16.rd(bf16), b16.fl(bf16)
    bad = []
    with hh.switches(bf16=bf16):
        for Lk in LKS:
            B = min(64, Lk)
            K = torch.zeros((B, Lk, dh), device=DEV)
            K[:, :, :11] = attn_code(torch.arange(Lk, device=DEV))[None]
            V = (torch.arange(Lk * dh, device=DEV).float().view(1, Lk, dh) * 7 % 251 - 125).expand(B, Lk, dh).contiguous()  # exact in 16 bits
            for Lq in LQS:
                sel = (torch.arange(Lq, device=DEV)[None, :] * 37 + 11 + torch.arange(B, device=DEV)[:, None]) % Lk  # (B, Lq)
                Q = torch.zeros((B, Lq, dh), device=DEV)
                Q[:, :, :11] = attn_code(sel)
                O = hh.attention(rd(Q), rd(K), rd(V), 1, dh)  # raw Q: the kernel applies log2(e)/sqrt(dh) itself
                want = torch.gather(V, 1, sel[:, :, None].expand(B, Lq, dh))
                err = float((fl(O) - want).abs().max())
                if not err < 1e-20:
                    bad.append((Lq, Lk, err))
    torch.cuda.synchronize()
    assert not bad, bad[:20]


@pytest.mark.gpu
@pytest.mark.parametrize("dh,heads", [(64, 2), (48, 1), (48, 2)])
def test_ragged_grid_matches_fp32_with_poison_behind_keys_and_columns(dh, heads):
    """The Lq x Lk grid on random data against the fp32 softmax (max 4e-3, mean 4e-4, lse 5e-4).  K and V are views into buffers whose rows behind
    key Lk - 1 AND whose 16 columns behind the last head hold NaN / Inf bit patterns: with one head of 48 the poison sits right where the
    zero-padded second k-step of QK^T would read if it took its d = 48..63 from memory (0 x NaN), and a dead key tile must not reach O."""
    Cc = heads * dh
    pad, B = 70, 2
    poison = torch.tensor([float("nan"), float("inf"), -float("inf"), 65504.0], device=DEV).to(F16)
    bad, worst = [], [0.0, 0.0, 0.0]
    for Lk in LKS:
        g = rng(dh * 100 + heads * 10000 + Lk)
        kb = poison[torch.arange(B * (Lk + pad) * (Cc + 16), device=DEV) % 4].view(B, Lk + pad, Cc + 16).clone()
        vb = kb.clone()
        kb[:, :Lk, :Cc] = to_dev(1.5 * g.standard_normal((B, Lk, Cc), dtype=np.float32)).to(F16)
        vb[:, :Lk, :Cc] = to_dev(g.standard_normal((B, Lk, Cc), dtype=np.float32)).to(F16)
        K, V = kb[:, :Lk, :Cc], vb[:, :Lk, :Cc]
        for Lq in LQS:
            Q = hh.prescale_q(to_dev(1.5 * g.standard_normal((B, Lq, Cc), dtype=np.float32)).to(F16), dh)
            O, lse = hh.attention(Q, K, V, heads, dh, lse=True, q_scale=1.0)
            ref, lse_ref = attn_ref(Q, K.contiguous(), V.contiguous(), heads, dh)
            err = (O.float() - ref).abs()
            fig = (float(err.max()), float(err.mean()), float((lse * math.log(2.0) - lse_ref).abs().max()))
            worst = [max(a, b) if b == b else float("nan") for a, b in zip(worst, fig)]
            if not (bool(torch.isfinite(O.float()).all()) and fig[0] < 4e-3 and fig[1] < 4e-4 and fig[2] < 5e-4):
                bad.append((Lq, Lk) + fig)
    torch.cuda.synchronize()
    print(f"dh {dh} heads {heads}: worst max {worst[0]:.2e} mean {worst[1]:.2e} lse {worst[2]:.2e}")
    assert not bad, bad[:20]


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("dh", [64, 48])
def test_reference_move_needed_by_one_row_only(dh, bf16):
    """A spike on ONE key for ONE query, late in the key sequence, in each of the four lane groups that share a query row (keys 4 g .. 4 g + 3 of a
    16-key tile) and for a row of either query tile: the move is decided by one lane and must reach all four lanes of that row -- and every row
    of the wave -- by the same amount.  Only dimension 0 carries the spike, so no other (query, key) pair sees it."""
    rd, fl = b16.rd(bf16), b16.fl(bf16)
    heads, Lq, Lk = 1, 128, 640
    # fp16: the bounds of test_attention_matches_fp32.  bf16: P and O carry 8 bits instead of 11 (2^3 times the fp16 bound); the statistics are fp32 in both
    tol = (3.2e-2 if bf16 else 4e-3, 5e-4)
    with hh.switches(bf16=bf16):
        for g4 in range(4):
            for q in (5, 16 + 9, 64 + 3, 96 + 16 + 14):  # query tiles 0 / 1 of waves 0, 0, 2, 3
                g = rng(1000 * g4 + q + dh)
                Q = 0.5 * g.standard_normal((1, Lq, dh), dtype=np.float32)
                K = 0.5 * g.standard_normal((1, Lk, dh), dtype=np.float32)
                V = g.standard_normal((1, Lk, dh), dtype=np.float32)
                key = 64 * 8 + 16 * (q % 4) + 4 * g4 + (q % 3)  # tile 8, every 16-key tile in turn
                Q[:, :, 0] = 0.0
                K[:, :, 0] = 0.0
                Q[0, q, 0] = 4.0
                K[0, key, 0] = 8.0  # +32 in base-2 units for (q, key) alone: far above kTau = 8
                Qs, Kb, Vb = rd(to_dev(Q)), rd(to_dev(K)), rd(to_dev(V))  # Q taken as already scaled: q_scale = 1
                O, lse = hh.attention(Qs, Kb, Vb, heads, dh, lse=True, q_scale=1.0)
                ref, lse_ref = attn_ref(fl(Qs), fl(Kb), fl(Vb), heads, dh)
                err = float((fl(O) - ref).abs().max())
                lerr = float((lse * math.log(2.0) - lse_ref).abs().max())
                assert err < tol[0] and lerr < tol[1], (g4, q, key, err, lerr)
                assert float((fl(O)[0, q] - fl(Vb)[0, key]).abs().max()) < tol[0]  # the spiked row is (all but) that key's V row


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("dh,Lk", [(64, 1370), (48, 1369), (64, 200), (48, 90)])
def test_rows_are_bitwise_independent_of_their_position(dh, Lk, bf16):
    """The same (Q row, K, V) gives the same bits in any lane, query tile, wave, block and batch item -- also in the wave whose second query tile
    is dead (rows 288..299 of Lq = 300) and which therefore runs the ragged instance of the tile body on every tile."""
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
def test_encoder_shape_is_bit_identical_from_run_to_run():
    """cfg-2's encoder launch (48 images x 6 heads, 1370 tokens, dh 64, read in place from the packed [T][3C] projection), twice."""
    dh, heads, T, B = 64, 6, 1370, 48
    Cc = heads * dh
    g = rng(2)
    qkv = to_dev(g.standard_normal((B, T, 3 * Cc), dtype=np.float32)).to(F16)
    qkv[:, :, :Cc] = hh.prescale_q(1.5 * qkv[:, :, :Cc].float(), dh)
    args = (qkv[:, :, :Cc], qkv[:, :, Cc:2 * Cc], qkv[:, :, 2 * Cc:], heads, dh)
    O1, l1 = hh.attention(*args, lse=True, q_scale=1.0)
    O2, l2 = hh.attention(*args, lse=True, q_scale=1.0)
    torch.cuda.synchronize()
    assert torch.equal(O1.view(torch.int16), O2.view(torch.int16)) and torch.equal(l1, l2)
    assert bool(torch.isfinite(O1.float()).all()) and float(O1.float().abs().max()) > 0


def test_attention_kernels_have_no_private_segment_and_keep_three_waves(tmp_path):
    """Every cs_attn_kernel instantiation builds with no private segment and no spilled register, and the two on the 16x16x32 tile loop
    (dh = 64, 48: the benchmark's) need at most 168 vector registers = three waves per SIMD at the allocation granularity of 8."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    from crossscore_amd import build as b
    out = str(tmp_path / "attention.s")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value"] + b.EXTRA_FLAGS.get("attention.hip", []) + [
        "-S", "--cuda-device-only", "-o", out, os.path.join(REPO, "crossscore_amd", "csrc", "attention.hip")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:]
    name, seen = None, {}
    for ln in open(out):
        ln = ln.strip()
        if ln.startswith(".name:"):
            name = ln.split()[-1]
        elif name and "cs_attn_kernel" in name and ln.split(":")[0] in (".private_segment_fixed_size", ".vgpr_count", ".vgpr_spill_count"):
            seen.setdefault(name, {})[ln.split(":")[0]] = int(ln.split()[-1])
    assert len(seen) == 12, sorted(seen)  # 6 head dims x 2 operand types
    for name, d in seen.items():
        assert d[".private_segment_fixed_size"] == 0 and d[".vgpr_spill_count"] == 0, (name, d)
        if "ILi64E" in name or "ILi48E" in name:
            assert d[".vgpr_count"] <= 168, (name, d)
    assert sum("ILi64E" in n or "ILi48E" in n for n in seen) == 4
