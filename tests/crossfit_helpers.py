"""Support of the cross-attention fit's tests: torch-tensor wrappers over the attention backward's entry points of the C ABI
(row and batch pitches are the tensors' own strides), the cases the op tests and the host test share, and the bounds the op tests assemble."""
import ctypes as C
import math

import torch

import crossfit_oracle as co
from bits16 import r16, spacing16
from crossscore_amd import _lib
from headfit_helpers import _p, _st, workspace

F64 = torch.float64
U32 = 2.0 ** -24
DHS = (16, 48, 96)                 # the head dims the backward is built for
DHS_UNSUPPORTED = (64, 128, 192)   # the forward's other head dims: CS_ERR_UNSUPPORTED
BATCH, HEADS = 2, 2


def tiles(dh):
    """(query rows of a workgroup of the dQ kernel, keys of a workgroup of the dK / dV kernel) as the library reports them"""
    q, k = C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().cs_attention_backward_tiles(dh, C.byref(q), C.byref(k)))
    return q.value, k.value


def shape_pairs(tq=64, tk=64):
    """(Lq, Lk) pairs in which every Lq of {1, tq - 1, tq, tq + 1, 2 tq + 3} and every Lk of {1, tk - 1, tk + 1, 3 tk + 5} appears"""
    return [(1, 3 * tk + 5), (tq - 1, 1), (tq, tk - 1), (tq + 1, tk + 1), (2 * tq + 3, 3 * tk + 5)]


def attention_backward_args(Q, K, V, O, dO, lse, heads, dh, q_scale, dQ, dK, dV, ws):
    """the argument list of cs_op_attention_backward from (B, L, >= heads dh) views; the rejection tests edit single entries"""
    B, Lq, _ = Q.shape
    return [_p(Q), _p(K), _p(V), _p(O), _p(dO), _p(lse), Q.stride(1), K.stride(1), V.stride(1), O.stride(1), dO.stride(1), Q.stride(0), K.stride(0),
            V.stride(0), O.stride(0), dO.stride(0), B, heads, Lq, K.shape[1], dh, float(q_scale), _p(dQ), dQ.stride(1), dQ.stride(0), _p(dK),
            dK.stride(1), dK.stride(0), _p(dV), dV.stride(1), dV.stride(0), _p(ws), _st()]


def attention_backward(Q, K, V, O, dO, lse, heads, dh, q_scale, dQ, dK, dV):
    lib = _lib.load()
    ws = workspace(lib.cs_attention_backward_workspace_bytes(Q.shape[0], heads, Q.shape[1], K.shape[1], dh), Q.device)
    _lib.check(lib.cs_op_attention_backward(*attention_backward_args(Q, K, V, O, dO, lse, heads, dh, q_scale, dQ, dK, dV, ws)))
    torch.cuda.synchronize()  # (the workspace is this call's)


def attn_case(Lq, Lk, dh, bf16, seed, kind="random", B=BATCH, h=HEADS):
    """-> (Qp, K, V, dO): fp64 tensors (B, h, L, dh) that hold values of the operand type; Qp is the pre-scaled query (q_scale = 1).
    random: logits S2 of a few units;  peaky: key 0 of every (batch, head) takes P ~ 1, so dP - D cancels;  underflow: |S2| of some hundreds,
    P underflows to zero for most keys;  negative: every S2 near -200"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g, dtype=F64)  # noqa: E731
    c = co.LOG2E / math.sqrt(dh)
    q, K, V, dO = rn(B, h, Lq, dh), rn(B, h, Lk, dh), rn(B, h, Lk, dh), 0.1 * rn(B, h, Lq, dh)
    if kind == "peaky":
        u = rn(B, h, 1, dh)
        u = u / u.norm(dim=-1, keepdim=True)
        q = 0.3 * q + 3.0 * math.sqrt(dh) ** 0.5 * u
        K[:, :, :1] = 3.0 * math.sqrt(dh) ** 0.5 * u
    if kind == "negative":  # every logit near -200: lse < -128, so 2^(0 - lse) of a key that does not exist overflows fp32
        u = rn(B, h, 1, dh)
        u = math.sqrt(200.0) * u / u.norm(dim=-1, keepdim=True)
        return r16(u + 0.3 * q, bf16), r16(-u + 0.3 * K, bf16), r16(V, bf16), r16(dO, bf16)
    scale = {"random": 1.5, "peaky": 1.0, "underflow": 60.0}[kind]
    return r16(scale * c * q, bf16), r16(K, bf16), r16(V, bf16), r16(dO, bf16)


# the cases of tests/test_crossfit_ops.py beside its grid (shape_pairs, kind "random", seed 1000 pair + dh): kind -> (Lq, Lk, seed offset); the
# host test plants its defects into every one of them
SPECIAL_CASES = {"peaky": (70, 67, 5), "underflow": (66, 130, 9), "negative": (67, 70, 13)}
RAW_Q_SHAPE = (65, 70, 48)  # (Lq, Lk, dh) of the q_scale = 0 case


def raw_q_case(bf16):
    """the q_scale = 0 case -> (Qraw, Qp, K, V, dO): raw queries and the Q' = round16(fp32(Qraw) * fp32(log2(e) / sqrt(dh))) both kernels form"""
    Lq, Lk, dh = RAW_Q_SHAPE
    g = torch.Generator().manual_seed(4)
    Qraw = r16(1.5 * torch.randn((BATCH, HEADS, Lq, dh), generator=g, dtype=F64), bf16)
    _, K, V, dO = attn_case(Lq, Lk, dh, bf16, 11)
    sc = torch.tensor(co.LOG2E, dtype=torch.float32) / torch.sqrt(torch.tensor(float(dh), dtype=torch.float32))
    return Qraw, r16((Qraw.float() * sc).double(), bf16), K, V, dO


def attn_fro_bounds(r, Qp, K, V, O, dO, lse, bf16):
    """Per-tensor bounds on the Frobenius norm of the error of dQu, dKu and dV, cs_op_attention_backward against
    crossfit_oracle.attention_backward (r, run with the operand roundings on), built as tailfit_helpers.tail_fro_bounds builds its own: from the
    number formats, the shapes and the case's own tensors (fp64, CPU), never from what the kernel returns.

    Rounded to the operand type are Ph, dzh and the three stored outputs.  Kernel and oracle round the same values from fp32 and fp64
    pre-images; an element differs only where the two straddle a rounding boundary, and then by one spacing of the type at that value.  The
    bound grants that EVERY element of every one of them is off by a full spacing, with signs that do not conspire: a perturbation d of the
    factor G of a sum S = sum_m G_m (x) X_m with |d_mn| <= spacing(G_mn) and independent signs has E |dS|_F^2 <= sum spacing(G_mn)^2 |X_m|^2, and
    the stages (the factor, the stored output) add in quadrature.  On top, rigorously (signs aligned): the fp32 evaluation of P and dz in front
    of their rounding -- (dh + 4) 2^-24 of the sums of magnitudes of S2, dP and D, the subtraction S2 - lse and the exp2 (through ln2 P), the
    product P (dP - D) with its cancellation priced in by |dP - D| -- carried through the output product, and that product's own fp32
    accumulation, (terms + 4) 2^-24 of the sum of magnitudes."""
    Qp, K, V, O, dO, lse = (t.to(F64) for t in (Qp, K, V, O, dO, lse))
    Lq, Lk, dh = Qp.shape[-2], K.shape[-2], Qp.shape[-1]
    P, Ph, dz, dzh, dP, D, S2 = (r[k] for k in ("P", "Ph", "dz", "dzh", "dP", "D", "S2"))
    T = lambda t: t.transpose(-1, -2)  # noqa: E731
    rows = lambda t: t.pow(2).sum(-1)  # noqa: E731
    us = (dh + 4) * U32
    rel_p = co.LN2 * (us * (Qp.abs() @ T(K.abs())) + 2 * U32 * (S2.abs() + lse.abs()[..., None])) + 4 * U32
    e_p = P * rel_p
    e_dp = us * (dO.abs() @ T(V.abs())) + 2 * U32 * (dP.abs() + D.abs()[..., None]) + us * (dO.abs() * O.abs()).sum(-1)[..., None]
    e_dz = e_p * (dP - D[..., None]).abs() + P * e_dp + 2 * U32 * dz.abs()
    sp_p, sp_z = spacing16(Ph, bf16), spacing16(dzh, bf16)
    quad = lambda a, b: math.sqrt(float(a) + float(b))  # noqa: E731
    out = {}
    out["dV"] = quad((sp_p.pow(2) * rows(dO)[..., :, None]).sum(), spacing16(r["dV"], bf16).pow(2).sum()) + \
        float((T(e_p) @ dO.abs()).norm()) + (Lq + 4) * U32 * float((T(Ph.abs()) @ dO.abs()).norm())
    out["dKu"] = quad((sp_z.pow(2) * rows(Qp)[..., :, None]).sum(), spacing16(r["dKu"], bf16).pow(2).sum()) + \
        float((T(e_dz) @ Qp.abs()).norm()) + (Lq + 4) * U32 * float((T(dzh.abs()) @ Qp.abs()).norm())
    out["dQu"] = quad((sp_z.pow(2) * rows(K)[..., None, :]).sum(), spacing16(r["dQu"], bf16).pow(2).sum()) + \
        float((e_dz @ K.abs()).norm()) + (Lk + 4) * U32 * float((dzh.abs() @ K.abs()).norm())
    return out


# ---- the whole block: cs_op_cross_backward ----
# (B, N, gh, gw, do_short_cut) of test_crossfit_ops.test_cross_backward: M = 30 and 12; the last without the residual around the attention
CROSS_OP_CASES = [(2, 2, 3, 5, True), (2, 2, 2, 3, True), (2, 2, 2, 3, False)]
CROSS_PARTS = ("dWq", "dWk", "dWv", "dbq", "dbk", "dbv", "dWo", "dbo", "dgamma2", "dbeta2")  # in_proj split into its three C-row blocks


def cross_case(B, N, gh, gw, Cc, h, act, p, bf16, seed, attn=None, short_cut=True, P=14):
    """A whole case of the block on the CPU (fp64 tensors that hold fp32 / operand-type values): x1, mem, the block's weights, Q', K, V, then O and
    lse from `attn` (Qp, K, V as (B, h, L, dh) -> (O, lse); default: the oracle's forward), y2 -> x2, the tail's weights and stored rows, and a
    gt at least 0.05 away from the score.  -> dict"""
    import headfit_oracle as ho
    import tailfit_oracle as to
    g = torch.Generator().manual_seed(seed)
    M, Mk, PP = B * gh * gw, B * N * gh * gw, P * P
    rn = lambda *s: torch.randn(s, generator=g, dtype=F64)  # noqa: E731
    f32 = lambda t: t.float().double()  # noqa: E731
    rnd = lambda t: r16(t, bf16)  # noqa: E731
    x1, mem = f32(rn(M, Cc)), rnd(rn(Mk, Cc))
    Win = torch.cat([2.0 * rn(Cc, Cc), 2.0 * rn(Cc, Cc), rn(Cc, Cc)]) / Cc ** 0.5
    Win[Cc:] = rnd(Win[Cc:])
    bin_ = f32(0.1 * rn(3 * Cc))
    Wo, W1, W2, Wa = (rnd(rn(Cc, Cc) / Cc ** 0.5) for _ in range(4))
    bo, b1, b2, ba = (f32(0.1 * rn(Cc)) for _ in range(4))
    g2, be2, g3, b3 = f32(1.0 + 0.2 * rn(Cc)), f32(0.1 * rn(Cc)), f32(1.0 + 0.2 * rn(Cc)), f32(0.1 * rn(Cc))
    Wb, bb = rnd(rn(PP, Cc) * (1.5 / Cc ** 0.5)), f32(rn(PP) * 0.3)
    blk = co.block_forward(x1, mem, Win, bin_, Wo, bo, g2, be2, B, h, short_cut, rnd=rnd)
    Qp, K, V = blk["Qp"], blk["K"], blk["V"]
    sp = lambda t: co.heads_of(t.reshape(B, -1, Cc), h)  # noqa: E731
    if attn is None:
        O4, lse, _ = co.attention_forward(sp(Qp), sp(K), sp(V), rnd)
        lse = lse.float().double()
    else:
        O4, lse = attn(sp(Qp), sp(K), sp(V))
    O = co.merge_heads(O4).reshape(M, Cc)
    y2 = (x1 if short_cut else 0.0) + O @ Wo.T + bo
    x2 = f32(to.ln_stats(y2)[2] * g2 + be2)
    H, _, X, A = to.tail_forward(x2, W1, b1, W2, b2, g3, b3, Wa, ba, rnd=rnd)
    s, _ = ho.scores(A, Wb, bb, act, p)
    off = (0.05 + 0.25 * torch.rand(s.shape, generator=g, dtype=F64)) * torch.where(torch.rand(s.shape, generator=g) < 0.5, -1.0, 1.0)
    return dict(x1=x1, mem=mem, Win=Win, bin=bin_, Wo=Wo, bo=bo, g2=g2, be2=be2, W1=W1, b1=b1, W2=W2, b2=b2, g3=g3, b3=b3, Wa=Wa, ba=ba, Wb=Wb, bb=bb,
                Qp=Qp, K=K, V=V, O=O, lse=lse, x2=x2, H=H, X=X, A=A, gt_rows=(s + off).float(), B=B, N=N, gh=gh, gw=gw, C=Cc, h=h, act=act, p=p,
                short_cut=short_cut, inv=1.0 / s.numel())


def cross_oracle(c, bf16, mutate=None):
    """crossfit_oracle.backward on a cross_case, roundings on"""
    return co.backward(c["x1"], c["Qp"], c["K"], c["V"], c["O"], c["lse"], c["mem"], c["W1"], c["Wo"], c["bo"], c["g2"], c["x2"], c["H"], c["X"], c["A"],
                       c["W2"], c["b2"], c["g3"], c["Wa"], c["Wb"], c["bb"], c["gt_rows"], c["act"], c["p"], c["inv"], c["B"], c["h"], c["short_cut"],
                       rnd=lambda t: r16(t, bf16), mutate=mutate)


def split_in_proj(r, Cc):
    """dWin / dbin of a result dict (or of a (dWin, dbin) pair) as their three blocks, under CROSS_PARTS' names"""
    dW, db = (r["dWin"], r["dbin"]) if isinstance(r, dict) else r
    return {"dWq": dW[:Cc], "dWk": dW[Cc:2 * Cc], "dWv": dW[2 * Cc:], "dbq": db[:Cc], "dbk": db[Cc:2 * Cc], "dbv": db[2 * Cc:]}


def cross_backward_args(x1, Qp, K, V, O, lse, mem, W1, Wo, bo, g2, N, heads, short_cut, x2, H, X, A, W2, b2, g3, Wa, Wb, bb, gt, B, gh, gw, P, act, powp,
                        inv_count, accumulate, outs, ws, eps=co.EPS):
    """the argument list of cs_op_cross_backward (outs: the sixteen gradients in crossfit_oracle.KEYS order, then the loss); K and V are views of
    one packed buffer (the same row pitch)"""
    assert K.stride(0) == V.stride(0)
    return [_p(x1), _p(Qp), Qp.stride(0), _p(K), _p(V), K.stride(0), _p(O), O.stride(0), _p(lse), _p(mem), mem.stride(0), _p(W1), W1.stride(0), _p(Wo),
            Wo.stride(0), _p(bo), _p(g2), N, heads, int(short_cut), _p(x2), _p(H), H.stride(0), _p(X), X.stride(0), _p(A), A.stride(0), _p(W2),
            W2.stride(0), _p(b2), _p(g3), float(eps), _p(Wa), Wa.stride(0), _p(Wb), Wb.stride(0), _p(bb), _p(gt), B, gh, gw, P, A.shape[1], act, powp,
            float(inv_count), int(accumulate)] + [_p(t) for t in outs] + [_p(ws), _st()]


def cross_outs(Cc, P=14, dev="cuda", fill=7.0):
    shapes = ((3 * Cc, Cc), (3 * Cc,), (Cc, Cc), (Cc,), (Cc,), (Cc,), (Cc, Cc), (Cc,), (Cc, Cc), (Cc,), (Cc,), (Cc,), (Cc, Cc), (Cc,), (P * P, Cc), (P * P,))
    return [torch.full(s, fill, device=dev) for s in shapes] + [torch.full((), fill, dtype=F64, device=dev)]


def cross_fro_bounds(r, c, bf16):
    """Per-part bounds (CROSS_PARTS) on the Frobenius norm of the error of the block's six gradients, cs_op_cross_backward against
    crossfit_oracle.backward (r, roundings on), in the manner of tailfit_helpers.tail_fro_bounds.  The chain of rounded intermediates in front of a
    reduction sum_m G_m (x) X_m: g, dpre, dyh, dHh (the tail's four) reach dx2, so dgamma2 / dbeta2 see 4 stages; dy2h is the fifth (dWo, dbo);
    dOh the sixth; the in_proj blocks see those six as a perturbation of their factor G = dQu | dKu | dV -- every element off by one spacing e16 of
    its value, signs that do not conspire, the stages in quadrature: sqrt(stages) e16 Q with Q^2 = sum_m |G_m|^2 |X_m|^2 -- and, on top of them,
    the attention backward's own three roundings (Ph, dzh, the stored output) through attn_fro_bounds, carried into the reduction with signs that
    do not conspire either: its Frobenius bound times the largest row norm of X.  Rigorously on top: the fp32 accumulations, (rows + 2 C + 12)
    2^-24 of the Frobenius norm of the sum of magnitudes, and three roundings of the fp32 scale of the in_proj reductions."""
    e16 = 2.0 ** -7 if bf16 else 2.0 ** -10
    Cc, h, B, inv = c["C"], c["h"], c["B"], c["inv"]
    dh = Cc // h
    M, Mk = c["x1"].shape[0], c["mem"].shape[0]
    rows = lambda t: t.pow(2).sum(1)  # noqa: E731
    one = lambda n: torch.ones((n, 1), dtype=F64)  # noqa: E731
    sp = lambda t: co.heads_of(t.reshape(B, -1, Cc), h)  # noqa: E731
    ab = attn_fro_bounds(r["attn"], sp(c["Qp"]), sp(c["K"]), sp(c["V"]), sp(c["O"]), sp(r["dOh"]), c["lse"], bf16)
    out = {}

    def red(name, G, X, stages, scale, nrows, attn_b=0.0):
        u = (nrows + 2 * Cc + 12 + 3) * U32
        q = float((rows(G) * rows(X)).sum().sqrt())
        out[name] = inv * scale * (math.sqrt(stages * (e16 * q) ** 2 + (attn_b * float(rows(X).max().sqrt())) ** 2) + u * float((G.abs().T @ X.abs()).norm()))

    rs = 1.0 / math.sqrt(dh)
    red("dWq", r["dQu"], r["x1h"], 6, rs, M, ab["dQu"])
    red("dbq", r["dQu"], one(M), 6, rs, M, ab["dQu"])
    red("dWk", r["dKu"], c["mem"], 6, co.LN2, Mk, ab["dKu"])
    red("dbk", r["dKu"], one(Mk), 6, co.LN2, Mk, ab["dKu"])
    red("dWv", r["dV"], c["mem"], 6, 1.0, Mk, ab["dV"])
    red("dbv", r["dV"], one(Mk), 6, 1.0, Mk, ab["dV"])
    red("dWo", r["dy2h"], c["O"], 5, 1.0, M)
    red("dbo", r["dy2h"], one(M), 5, 1.0, M)
    u = (M + 2 * Cc + 12) * U32
    dx, xh = r["dx2"], r["xhat2"]
    out["dgamma2"] = inv * (2.0 * e16 * float((dx * xh).norm()) + u * float((dx * xh).abs().sum(0).norm()))
    out["dbeta2"] = inv * (2.0 * e16 * float(dx.norm()) + u * float(dx.abs().sum(0).norm()))
    return out


def autograd_block(c, autocast=None, loss_scale=1.0, eps=co.EPS):
    """The block and the tail as the reference's modules execute them (F.multi_head_attention_forward, the residual, F.layer_norm, then the tail of
    tailfit_helpers.autograd_tail) under torch.autograd on x1 and mem of a cross_case, in the dtype of its tensors -> (loss, the sixteen gradients
    in crossfit_oracle.KEYS order).  autocast: a 16-bit dtype to run it under torch.autocast on the CPU, the loss scaled by loss_scale."""
    import torch.nn.functional as F

    import headfit_oracle as ho
    names = ("Win", "bin", "Wo", "bo", "g2", "be2", "W1", "b1", "W2", "b2", "g3", "b3", "Wa", "ba", "Wb", "bb")
    prm = [c[k].detach().clone().requires_grad_(True) for k in names]
    Win, bin_, Wo, bo, g2, be2, W1, b1, W2, b2, g3, b3, Wa, ba, Wb, bb = prm
    B, Cc, h, gh, gw = c["B"], c["C"], c["h"], c["gh"], c["gw"]
    x1, mem, gt_rows = c["x1"].to(Win.dtype), c["mem"].to(Win.dtype), c["gt_rows"].to(Win.dtype)
    P = int(round(Wb.shape[0] ** 0.5))

    def run():
        q = x1.reshape(B, -1, Cc).transpose(0, 1)
        m = mem.reshape(B, -1, Cc).transpose(0, 1)
        a, _ = F.multi_head_attention_forward(q, m, m, Cc, h, Win, bin_, None, None, False, 0.0, Wo, bo, training=False, need_weights=False)
        a = a.transpose(0, 1).reshape(-1, Cc)
        x2 = F.layer_norm((x1 + a) if c["short_cut"] else a, (Cc,), g2, be2, eps)
        H = F.relu(F.linear(x2, W1, b1))
        X = F.layer_norm(x2 + F.linear(H, W2, b2), (Cc,), g3, b3, eps)
        z = F.linear(F.leaky_relu(F.linear(X, Wa, ba), ho.LEAKY), Wb, bb)
        sg = torch.sigmoid(z) if c["act"] == 0 else torch.tanh(z)
        s = sg if c["p"] == 1 else sg ** c["p"]
        return torch.nn.L1Loss()(ho.to_image(s, B, gh, gw, P), ho.to_image(gt_rows, B, gh, gw, P))

    if autocast is None:
        loss = run()
    else:
        with torch.autocast("cpu", dtype=autocast):
            loss = run()
    (loss * loss_scale).backward()
    return loss.detach(), [t.grad.detach() / loss_scale for t in prm]
