"""cs_op_attention_backward (csrc/attnbwd.hip) and cs_op_cross_backward (csrc/crossfit.hip) against tests/crossfit_oracle.py, in
both operand types.  O and lse are cs_op_attention's on the same inputs, never the oracle's.  Every bound is assembled from the number formats and the case's own tensors
(crossfit_helpers.attn_fro_bounds), never from what the kernel returns; outputs sit inside tests/guard.py bands, the operands are strided views
of poisoned buffers (K and V side by side in rows of 4 C elements, as the forward's packed projection leaves them; dK | dV in one buffer)."""
import ctypes as C
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import crossfit_helpers as ch  # noqa: E402
import crossfit_oracle as co  # noqa: E402
import headfit_helpers as hh  # noqa: E402
from bits16 import MODES, bits16, r16, same_bits, vals16  # noqa: E402
from guard import guarded_out, poisoned_in  # noqa: E402
from hip_helpers import attention, switches  # noqa: E402
from crossscore_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
B, HEADS = ch.BATCH, ch.HEADS


def _rows(t):
    """(B, h, L, dh) values -> (B, L, h dh) rows"""
    return co.merge_heads(t)


def _place(Qp, K, V, dO, bf16):
    """the operands on the device, each a strided view of a poisoned buffer: Q and dO in rows of C + 8 / C + 16 elements, K and V in the column
    blocks [2C, 3C) and [3C, 4C) of one (B, Lk, 4C) buffer whose other columns hold NaNs"""
    Cc = Qp.shape[1] * Qp.shape[3]
    dev = lambda t: bits16(_rows(t).float().cuda(), bf16)  # noqa: E731
    Qd = poisoned_in(dev(Qp), ld=Cc + 8)
    dOd = poisoned_in(dev(dO), ld=Cc + 16)
    kv = torch.full((K.shape[0], K.shape[2], 4 * Cc), float("nan"), dtype=torch.float16, device="cuda")
    kv[:, :, 2 * Cc:3 * Cc] = dev(K)
    kv[:, :, 3 * Cc:] = dev(V)
    kv = poisoned_in(kv, ld=4 * Cc)
    return Qd, kv[:, :, 2 * Cc:3 * Cc], kv[:, :, 3 * Cc:], dOd


def _run(Qp, K, V, dO, bf16, q_scale=1.0, Qraw=None):
    """-> (O, lse as cs_op_attention gave them (fp64 values, (B, h, L, dh) / (B, h, Lq)), dQu, dKu, dV values (B, h, L, dh), the raw outputs)"""
    h, dh = Qp.shape[1], Qp.shape[3]
    Cc = h * dh
    Lq, Lk = Qp.shape[2], K.shape[2]
    Qd, Kd, Vd, dOd = _place(Qp if Qraw is None else Qraw, K, V, dO, bf16)
    with switches(bf16=bf16):
        Od, chk_o = guarded_out((B, Lq, Cc), torch.float16, ld=Cc + 8)
        lse = torch.full((B, h, Lq), float("nan"), device="cuda")
        attention(Qd, Kd, Vd, h, dh, q_scale=q_scale, O=Od, L=lse)
        chk_o("O")
        dQ, chk_q = guarded_out((B, Lq, Cc), torch.float16, ld=Cc + 8)
        dKV, chk_kv = guarded_out((B, Lk, 2 * Cc), torch.float16)
        ch.attention_backward(Qd, Kd, Vd, Od, dOd, lse, h, dh, q_scale, dQ, dKV[:, :, :Cc], dKV[:, :, Cc:])
        chk_q("dQ")
        chk_kv("dK | dV")
    val = lambda t: co.heads_of(vals16(t.contiguous(), bf16, F64).cpu(), h)  # noqa: E731
    raw = (dQ.contiguous().clone(), dKV.contiguous().clone())
    return val(Od), lse.double().cpu(), val(dQ), val(dKV[:, :, :Cc]), val(dKV[:, :, Cc:]), raw


def _check(Lq, Lk, dh, bf16, seed, kind, tag, twice=False, floor=None):
    Qp, K, V, dO = ch.attn_case(Lq, Lk, dh, bf16, seed, kind)
    O, lse, dQ, dK, dV, raw = _run(Qp, K, V, dO, bf16)
    assert bool(torch.isfinite(lse).all())
    ref = co.attention_backward(Qp, K, V, O, dO, lse, rnd=lambda t: r16(t, bf16))
    bounds = ch.attn_fro_bounds(ref, Qp, K, V, O, dO, lse, bf16)
    for name, got in (("dQu", dQ), ("dKu", dK), ("dV", dV)):
        assert bool(torch.isfinite(got).all()), name
        err, nrm = float((got - ref[name]).norm()), float(ref[name].norm())
        print(f"attention_backward {tag} Lq {Lq} Lk {Lk} dh {dh} {'bf16' if bf16 else 'fp16'} {name}: |err| {err:.3e}, |ref| {nrm:.3e}, "
              f"err/bound {err / bounds[name]:.4f}, bound/|ref| {bounds[name] / max(nrm, 1e-300):.2e}")
        assert err <= bounds[name], name
        if floor is not None and name in floor:
            assert bounds[name] <= floor[name] * nrm, name  # (the bound stays a small part of the gradient: a condition on the case)
    if twice:
        raw2 = _run(Qp, K, V, dO, bf16)[5]
        same_bits(raw2[0], raw[0], "second run, dQ")
        same_bits(raw2[1], raw[1], "second run, dK | dV")


def test_head_dims():
    """16, 48 and 96 are built, with 64-row tiles on both axes; the forward's other head dims are refused"""
    lib = _lib.load()
    for dh in ch.DHS:
        assert ch.tiles(dh) == (64, 64)
        assert lib.cs_attention_backward_workspace_bytes(2, 2, 65, 3, dh) >= 2 * 2 * 65 * 4
    for dh in ch.DHS_UNSUPPORTED + (8, 32):
        assert lib.cs_attention_backward_tiles(dh, None, None) == _lib.CS_ERR_UNSUPPORTED
        assert lib.cs_attention_backward_workspace_bytes(2, 2, 65, 3, dh) == 0


@MODES
@pytest.mark.parametrize("dh", ch.DHS)
@pytest.mark.parametrize("pair", range(5))
def test_attention_backward(pair, dh, bf16):
    tq, tk = ch.tiles(dh)
    Lq, Lk = ch.shape_pairs(tq, tk)[pair]
    # (Lk = 1: P = 1 and dz = 0, dQu and dKu are rounding residue; elsewhere the bound is a few spacings' worth of the gradient)
    floor = None if Lk == 1 else {k: 0.03 if bf16 else 0.004 for k in co.ATTN}
    _check(Lq, Lk, dh, bf16, seed=1000 * pair + dh, kind="random", tag="grid", twice=True, floor=floor)


@MODES
@pytest.mark.parametrize("dh", ch.DHS)
def test_attention_backward_peaky(dh, bf16):
    """key 0 takes P ~ 1 for every query: dP - D cancels in its column"""
    Lq, Lk, so = ch.SPECIAL_CASES["peaky"]
    Qp, K, V, dO = ch.attn_case(Lq, Lk, dh, bf16, so + dh, "peaky")
    P = co.attention_forward(Qp, K, V)[2]
    assert float(P[..., 0].min()) > 0.9
    _check(Lq, Lk, dh, bf16, seed=so + dh, kind="peaky", tag="peaky")


@MODES
@pytest.mark.parametrize("dh", ch.DHS)
def test_attention_backward_underflow(dh, bf16):
    """|S2| of some hundreds: P underflows to zero for most keys, in fp32 already"""
    Lq, Lk, so = ch.SPECIAL_CASES["underflow"]
    Qp, K, V, dO = ch.attn_case(Lq, Lk, dh, bf16, so + dh, "underflow")
    S2 = Qp @ K.transpose(-1, -2)
    P = co.attention_forward(Qp, K, V)[2]
    assert float(S2.abs().max()) > 150 and float((P < 2.0 ** -126).double().mean()) > 0.5
    _check(Lq, Lk, dh, bf16, seed=so + dh, kind="underflow", tag="underflow")


@MODES
@pytest.mark.parametrize("dh", ch.DHS)
def test_attention_backward_negative_logits(dh, bf16):
    """Every logit near -200 with ragged last tiles on both axes: lse < -128, so a key of the ragged tile that does not exist would take
    P = 2^(0 - lse) = inf in fp32 and, against its zero K row, put a NaN into every row of dQ.  The rows that do not exist contribute exact
    zeros instead: the outputs are finite and inside the bounds (tests/test_crossfit_host.py plants the defect into the oracle on this case)."""
    Lq, Lk, so = ch.SPECIAL_CASES["negative"]
    Qp, K, V, dO = ch.attn_case(Lq, Lk, dh, bf16, so + dh, "negative")
    tq, tk = ch.tiles(dh)
    assert Lq % tq and Lk % tk and float(co.attention_forward(Qp, K, V)[1].max()) < -128.0
    _check(Lq, Lk, dh, bf16, seed=so + dh, kind="negative", tag="negative")


@MODES
def test_attention_backward_raw_q(bf16):
    """q_scale = 0: the kernel scales raw Q by log2(e) / sqrt(dh) in fp32 and rounds once, as cs_op_attention does; dK is taken against that Q'"""
    Qraw, Qp, K, V, dO = ch.raw_q_case(bf16)
    O, lse, dQ, dK, dV, _ = _run(Qp, K, V, dO, bf16, q_scale=0.0, Qraw=Qraw)
    ref = co.attention_backward(Qp, K, V, O, dO, lse, rnd=lambda t: r16(t, bf16))
    bounds = ch.attn_fro_bounds(ref, Qp, K, V, O, dO, lse, bf16)
    for name, got in (("dQu", dQ), ("dKu", dK), ("dV", dV)):
        err = float((got - ref[name]).norm())
        print(f"attention_backward raw q {'bf16' if bf16 else 'fp16'} {name}: err/bound {err / bounds[name]:.4f}")
        assert err <= bounds[name], name


def test_attention_backward_rejections():
    """every rejection returns before any launch: the poisoned outputs keep their bits"""
    dh, Lq, Lk = 16, 5, 7
    Cc = HEADS * dh
    lib = _lib.load()
    mk = lambda L, w=Cc: torch.zeros((B, L, w), dtype=torch.float16, device="cuda")  # noqa: E731
    Q, K, V, O, dO = mk(Lq), mk(Lk), mk(Lk), mk(Lq), mk(Lq)
    lse = torch.zeros((B, HEADS, Lq), device="cuda")
    outs = [torch.full((B, L, Cc), 7.0, dtype=torch.float16, device="cuda") for L in (Lq, Lk, Lk)]
    ws = hh.workspace(lib.cs_attention_backward_workspace_bytes(B, HEADS, Lq, Lk, dh))
    good = ch.attention_backward_args(Q, K, V, O, dO, lse, HEADS, dh, 1.0, outs[0], outs[1], outs[2], ws)
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)  # noqa: E731
    edits = {"null Q": (0, None), "null K": (1, None), "null V": (2, None), "null O": (3, None), "null dO": (4, None), "null lse": (5, None),
             "null dQ": (22, None), "null dK": (25, None), "null dV": (28, None), "null workspace": (31, None),
             "misaligned Q": (0, off(Q, 8)), "misaligned K": (1, off(K, 2)), "misaligned dO": (4, off(dO, 4)), "misaligned dV": (28, off(outs[2], 8)),
             "misaligned lse": (5, off(lse, 2)), "misaligned workspace": (31, off(ws, 16)),
             "ldq 36": (6, Cc + 4), "ldk 33": (7, Cc + 1), "ldv 0": (8, 0), "ldo 36": (9, Cc + 4), "lddo 34": (10, Cc + 2), "lddq 36": (23, Cc + 4),
             "lddk 36": (26, Cc + 4), "lddv 36": (29, Cc + 4), "q_bs 4": (11, Lq * Cc + 4), "dk_bs 4": (27, Lk * Cc + 4),
             "Lk ldk 2^30": (7, 1 << 28), "batch 0": (16, 0), "heads 0": (17, 0), "Lq 0": (18, 0), "Lk 0": (19, 0), "q_scale -1": (21, -1.0)}
    for what, (i, v) in edits.items():
        args = list(good)
        args[i] = v
        assert lib.cs_op_attention_backward(*args) == _lib.CS_ERR_BAD_ARG, what
        assert _lib.last_error(), what
    for dh_bad in ch.DHS_UNSUPPORTED:
        args = list(good)
        args[20] = dh_bad
        assert lib.cs_op_attention_backward(*args) == _lib.CS_ERR_UNSUPPORTED, dh_bad
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 7.0).all())
    assert lib.cs_op_attention_backward(*good) == 0
    torch.cuda.synchronize()


# ---- the whole block: cs_op_cross_backward ----
import headfit_oracle as ho  # noqa: E402
import tailfit_helpers as th  # noqa: E402

P, PP = 14, 196


def _gpu_attention(bf16):
    """(Qp, K, V) fp64 (B, h, L, dh) -> (O, lse) as cs_op_attention gives them for those operands (q_scale = 1), fp64 on the CPU"""
    def run(Qp, K, V):
        h = Qp.shape[1]
        dev = lambda t: bits16(_rows(t).float().cuda(), bf16).contiguous()  # noqa: E731
        with switches(bf16=bf16):
            O, lse = attention(dev(Qp), dev(K), dev(V), h, Qp.shape[3], lse=True, q_scale=1.0)
        torch.cuda.synchronize()
        return co.heads_of(vals16(O, bf16, F64).cpu(), h), lse.double().cpu()
    return run


def _cross_device(c, bf16):
    """the operands of a cross_case on the device, the 16-bit ones strided views of poisoned buffers (K and V in the last 2 C columns of rows of 4 C)"""
    Cc = c["C"]
    d16 = lambda t: bits16(t.float().cuda(), bf16)  # noqa: E731
    f32 = lambda t: t.float().cuda()  # noqa: E731
    kv = torch.full((c["mem"].shape[0], 4 * Cc), float("nan"), dtype=torch.float16, device="cuda")
    kv[:, 2 * Cc:3 * Cc] = d16(c["K"])
    kv[:, 3 * Cc:] = d16(c["V"])
    kv = poisoned_in(kv, ld=4 * Cc)
    gt = ho.to_image(c["gt_rows"], c["B"], c["gh"], c["gw"], P).contiguous().cuda()
    return dict(x1=f32(c["x1"]), Qp=poisoned_in(d16(c["Qp"]), ld=Cc + 8), K=kv[:, 2 * Cc:3 * Cc], V=kv[:, 3 * Cc:], O=poisoned_in(d16(c["O"]), ld=Cc + 16),
                lse=f32(c["lse"]).contiguous(), mem=poisoned_in(d16(c["mem"]), ld=Cc + 8), W1=poisoned_in(d16(c["W1"]), ld=Cc + 8),
                Wo=poisoned_in(d16(c["Wo"]), ld=Cc + 24), bo=f32(c["bo"]), g2=f32(c["g2"]), x2=f32(c["x2"]), H=poisoned_in(d16(c["H"]), ld=Cc + 8),
                X=poisoned_in(d16(c["X"]), ld=Cc + 16), A=poisoned_in(d16(c["A"]), ld=Cc + 8), W2=poisoned_in(d16(c["W2"]), ld=Cc + 8), b2=f32(c["b2"]),
                g3=f32(c["g3"]), Wa=poisoned_in(d16(c["Wa"]), ld=Cc + 24), Wb=poisoned_in(d16(c["Wb"]), ld=Cc + 8), bb=f32(c["bb"]), gt=gt)


def _cross_args(c, d, outs, ws, accumulate=0):
    return ch.cross_backward_args(d["x1"], d["Qp"], d["K"], d["V"], d["O"], d["lse"], d["mem"], d["W1"], d["Wo"], d["bo"], d["g2"], c["N"], c["h"],
                                  c["short_cut"], d["x2"], d["H"], d["X"], d["A"], d["W2"], d["b2"], d["g3"], d["Wa"], d["Wb"], d["bb"], d["gt"], c["B"],
                                  c["gh"], c["gw"], P, c["act"], c["p"], c["inv"], accumulate, outs, ws)


def _cross_shapes(Cc):
    return ((3 * Cc, Cc), (3 * Cc,), (Cc, Cc), (Cc,), (Cc,), (Cc,), (Cc, Cc), (Cc,), (Cc, Cc), (Cc,), (Cc,), (Cc,), (Cc, Cc), (Cc,), (PP, Cc), (PP,))


@MODES
@pytest.mark.parametrize("Cc,h", [(128, 8), (384, 8)])
@pytest.mark.parametrize("B,N,gh,gw,short_cut", ch.CROSS_OP_CASES)
def test_cross_backward(B, N, gh, gw, short_cut, Cc, h, bf16):
    lib = _lib.load()
    c = ch.cross_case(B, N, gh, gw, Cc, h, 0, 1.0, bf16, seed=B * 100 + Cc + gh, attn=_gpu_attention(bf16), short_cut=short_cut)
    ref = ch.cross_oracle(c, bf16)
    bounds = ch.cross_fro_bounds(ref, c, bf16)
    d = _cross_device(c, bf16)
    M = B * gh * gw
    with switches(bf16=bf16):
        def run():
            outs = [guarded_out(s, torch.float32) for s in _cross_shapes(Cc)]
            loss = torch.full((), 7.0, dtype=F64, device="cuda")
            ws = hh.workspace(lib.cs_cross_backward_workspace_bytes(B, gh * gw, N, Cc, P, h))
            _lib.check(lib.cs_op_cross_backward(*_cross_args(c, d, [o[0] for o in outs] + [loss], ws)))
            torch.cuda.synchronize()
            for (_, chk), name in zip(outs, co.KEYS):
                chk(name)
            return [o[0].contiguous().clone() for o in outs], loss
        got, loss = run()
        tail = th.tail_backward(d["x2"], d["H"], d["X"], d["A"], d["W2"], d["b2"], d["g3"], d["Wa"], d["Wb"], d["bb"], d["gt"], B, gh, gw, P, c["act"], c["p"],
                                c["inv"])
        again, loss2 = run()
    for o, t, name in zip(got[6:], tail[:10], co.KEYS[6:]):
        assert torch.equal(o, t), f"{name}: the tail's and the head's gradients are cs_op_tail_backward's bit for bit"
    assert float(loss) == float(tail[10]) == float(loss2)
    for a, b, name in zip(got, again, co.KEYS):
        assert torch.equal(a, b), f"{name}: two identical calls give identical bits"
    have = {**ch.split_in_proj((got[0].double().cpu(), got[1].double().cpu()), Cc), "dWo": got[2].double().cpu(), "dbo": got[3].double().cpu(),
            "dgamma2": got[4].double().cpu(), "dbeta2": got[5].double().cpu()}
    want = {**ch.split_in_proj(ref, Cc), **{k: ref[k] for k in ("dWo", "dbo", "dgamma2", "dbeta2")}}
    tag = f"M {M} Mk {M * N} C {Cc} {'bf16' if bf16 else 'fp16'}{'' if short_cut else ' no short cut'}"
    for name in ch.CROSS_PARTS:
        err, nrm = float((have[name] - want[name]).norm()), float(want[name].norm())
        print(f"cross_backward {tag} {name}: rel Frobenius {err / nrm:.3e}, err/bound {err / bounds[name]:.4f}, bound/|ref| {bounds[name] / nrm:.2e}")
        assert err <= bounds[name], name
        if name != "dbk":
            assert bounds[name] <= 0.06 * nrm, name  # (the bound stays a small part of the gradient: a condition on the case)
    # the K bias gradient: zero in exact arithmetic; the op returns no more than the residue the oracle with roundings on predicts, plus its bound
    assert float(have["dbk"].norm()) <= float(want["dbk"].norm()) + bounds["dbk"]
    assert float(want["dbk"].norm()) <= 0.05 * float(want["dbv"].norm())


def test_cross_backward_rejections():
    """every rejection returns before any launch: the poisoned outputs keep their bits"""
    B, N, gh, gw, Cc, h = 1, 2, 2, 3, 128, 8
    c = ch.cross_case(B, N, gh, gw, Cc, h, 0, 1.0, False, seed=3)
    lib = _lib.load()
    d = _cross_device(c, False)
    outs = ch.cross_outs(Cc)
    ws = hh.workspace(lib.cs_cross_backward_workspace_bytes(B, gh * gw, N, Cc, P, h))
    good = _cross_args(c, d, outs, ws)
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)  # noqa: E731
    edits = {"null x1": (0, None), "null Qp": (1, None), "null K": (3, None), "null V": (4, None), "null O": (6, None), "null lse": (8, None),
             "null mem": (9, None), "null W1": (11, None), "null Wo": (13, None), "null bo": (15, None), "null gamma2": (16, None),
             "null dWin": (47, None), "null dbeta2": (52, None), "null x2": (20, None), "null loss": (63, None), "null workspace": (64, None),
             "short Qp pitch": (2, Cc - 8), "odd K|V pitch": (5, 4 * Cc + 4), "odd O pitch": (7, Cc + 4), "odd mem pitch": (10, Cc + 2),
             "short W1 pitch": (12, Cc - 8), "odd Wo pitch": (14, Cc + 4), "misaligned x1": (0, off(d["x1"], 4)), "misaligned Qp": (1, off(d["Qp"], 8)),
             "misaligned K": (3, off(d["K"], 2)), "misaligned lse": (8, off(d["lse"], 2)), "misaligned dWo": (49, off(outs[2], 2)),
             "misaligned workspace": (64, off(ws, 16)), "N 0": (17, 0), "heads 0": (18, 0), "heads 7": (18, 7), "empty batch": (38, 0),
             "patch 16": (41, 16), "hidden 96": (42, 96), "inv_count 0": (45, 0.0)}
    for what, (i, v) in edits.items():
        args = list(good)
        args[i] = v
        assert lib.cs_op_cross_backward(*args) != 0, what
        assert _lib.last_error(), what
    for heads in (2, 1):  # head dims 64 and 128: the forward runs them, the backward is not built for them
        args = list(good)
        args[18] = heads
        assert lib.cs_op_cross_backward(*args) == _lib.CS_ERR_UNSUPPORTED, heads
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 7.0).all())
    assert lib.cs_cross_backward_workspace_bytes(B, gh * gw, N, Cc, P, 2) == 0 and lib.cs_cross_backward_workspace_bytes(B, gh * gw, N, Cc, 16, h) == 0
    assert lib.cs_op_cross_backward(*good) == 0
    torch.cuda.synchronize()
