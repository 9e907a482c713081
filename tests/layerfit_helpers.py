"""Support of the whole-layer fit's tests: the cases the op test and the host test share, the argument list of
cs_op_layer_backward, the bounds the op test assembles, and the block under torch.autograd."""
import math

import torch

import crossfit_helpers as ch
import crossfit_oracle as co
import layerfit_oracle as lo
from bits16 import r16
from headfit_helpers import _p, _st

F64 = torch.float64
U32 = ch.U32
# (B, N, gh, gw, do_short_cut) of test_layerfit_ops.test_layer_backward: M = 30 and 12, the latter also without the residuals; 5 x 13 patches
# (Np = 65) put one ragged row AND one ragged key behind the attention backward's 64-row tiles inside the composition
LAYER_OP_CASES = [(2, 2, 3, 5, True), (2, 2, 2, 3, True), (2, 2, 2, 3, False), (2, 2, 5, 13, True)]
WIDTHS = [(128, 8), (384, 8)]  # (C, heads): head dims 16 and 48
LAYER_PARTS = ("dWq_s", "dWk_s", "dWv_s", "dbq_s", "dbk_s", "dbv_s", "dWo_s", "dbo_s", "dgamma1", "dbeta1")  # in_proj split into its three C-row blocks
IN_PROJ = LAYER_PARTS[:6]
# which parts a planted defect of layerfit_oracle.MUTATIONS reaches.  dbk_s is zero in exact arithmetic (sum_k dz = 0) and is left out everywhere;
# dbeta1 = inv_count sum_m dx1 does not see y1; a wrong lse or a wider key range only enters the attention backward; the in_proj scalars sit
# on single blocks; the wrong input rows do not enter the biases' column sums.  The stale O is counted where Os is read itself: as the reduction's
# second factor (dWo_s), in D = sum_d dOsh Os of the attention backward (the Q and K blocks) and as xhat1 (dgamma1).  dV_s = Ph^T dOsh, dbv_s and
# dbo_s = sum_m dy1h see it only through xhat1 inside the LayerNorm backward, where the residual x0 dominates y1: too weak a path to count on.
_ALL = tuple(k for k in LAYER_PARTS if k != "dbk_s")
_ATTN = tuple(k for k in IN_PROJ if k != "dbk_s")
REACH = {"dx1_no_residual": _ALL, "dx1_no_q": _ALL, "dx1_no_ln2": _ALL, "y1_no_residual": tuple(k for k in _ALL if k != "dbeta1"),
         "cross_O": ("dWq_s", "dWk_s", "dbq_s", "dWo_s", "dgamma1"), "cross_lse": _ATTN, "all_keys": _ATTN, "no_rsqrt_s": ("dWq_s", "dbq_s"),
         "no_ln2_s": ("dWk_s",), "x1h_for_x0h": ("dWq_s", "dWk_s", "dWv_s")}
NEEDS_SHORT_CUT = ("dx1_no_residual", "y1_no_residual")  # without do_short_cut these two have nothing to change


def case_seed(B, gh, gw, Cc):
    return B * 1000 + Cc + 7 * gh + gw


def layer_case(B, N, gh, gw, Cc, h, act, p, bf16, seed, attn=None, short_cut=True, P=14):
    """A whole case of the layer on the CPU (fp64 tensors that hold fp32 / operand-type values): x0, the self-attention block's weights, Qs', Ks,
    Vs, then Os and lse_s from `attn` ((Qp, K, V) as (B, h, L, dh) -> (O, lse); default: the oracle's forward), y1 -> x1; then the cross-attention
    block on that x1, the tail and a gt at least 0.05 away from the score, as crossfit_helpers.cross_case builds them.  -> dict with cross_case's
    keys and x0, Win_s, bin_s, Wo_s, bo_s, g1, be1, Qs, Ks, Vs, Os, lse_s, Wqp (the packed c Wq of the cross-attention, operand-type values)"""
    import headfit_oracle as ho
    import tailfit_oracle as to
    g = torch.Generator().manual_seed(seed)
    M, Mk, PP = B * gh * gw, B * N * gh * gw, P * P
    rn = lambda *s: torch.randn(s, generator=g, dtype=F64)  # noqa: E731
    f32 = lambda t: t.float().double()  # noqa: E731
    rnd = lambda t: r16(t, bf16)  # noqa: E731
    x0, mem = f32(rn(M, Cc)), rnd(rn(Mk, Cc))
    Win_s = torch.cat([2.0 * rn(Cc, Cc), 2.0 * rn(Cc, Cc), rn(Cc, Cc)]) / Cc ** 0.5
    Win_s[Cc:] = rnd(Win_s[Cc:])
    bin_s = f32(0.1 * rn(3 * Cc))
    Wo_s = rnd(rn(Cc, Cc) / Cc ** 0.5)
    bo_s, g1, be1 = f32(0.1 * rn(Cc)), f32(1.0 + 0.2 * rn(Cc)), f32(0.1 * rn(Cc))
    sf = lo.self_forward(x0, Win_s, bin_s, Wo_s, bo_s, g1, be1, B, h, short_cut, rnd=rnd, attn=attn)
    lse_s = sf["lse_s"].float().double()
    x1 = f32(sf["x1"])
    # the cross-attention block, the tail and the head: crossfit_helpers.cross_case with this x1 in place of a random one
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
    # the packed query projection as cs_finalize forms it: fp32 weight times the fp32 scale, rounded once
    cq = (torch.tensor(co.LOG2E, dtype=torch.float32) / torch.sqrt(torch.tensor(float(Cc // h), dtype=torch.float32)))
    Wqp = rnd((Win[:Cc].float() * cq).double())
    return dict(x0=x0, Win_s=Win_s, bin_s=bin_s, Wo_s=Wo_s, bo_s=bo_s, g1=g1, be1=be1, Qs=sf["Qs"], Ks=sf["Ks"], Vs=sf["Vs"], Os=sf["Os"], lse_s=lse_s,
                Wqp=Wqp, x1=x1, mem=mem, Win=Win, bin=bin_, Wo=Wo, bo=bo, g2=g2, be2=be2, W1=W1, b1=b1, W2=W2, b2=b2, g3=g3, b3=b3, Wa=Wa, ba=ba,
                Wb=Wb, bb=bb, Qp=Qp, K=K, V=V, O=O, lse=lse, x2=x2, H=H, X=X, A=A, gt_rows=(s + off).float(), B=B, N=N, gh=gh, gw=gw, C=Cc, h=h,
                act=act, p=p, short_cut=short_cut, inv=1.0 / s.numel())


def cross_args_of(c):
    """the positional arguments of crossfit_oracle.backward (up to h) from a layer_case"""
    return (c["x1"], c["Qp"], c["K"], c["V"], c["O"], c["lse"], c["mem"], c["W1"], c["Wo"], c["bo"], c["g2"], c["x2"], c["H"], c["X"], c["A"], c["W2"],
            c["b2"], c["g3"], c["Wa"], c["Wb"], c["bb"], c["gt_rows"], c["act"], c["p"], c["inv"], c["B"], c["h"])


def layer_oracle(c, bf16, mutate=None, rounded=True):
    """layerfit_oracle.backward on a layer_case, roundings on (or off: the fp64 definition on the same stored operands)"""
    return lo.backward(c["x0"], c["Qs"], c["Ks"], c["Vs"], c["Os"], c["lse_s"], c["Wqp"], c["Wo_s"], c["bo_s"], c["g1"], cross_args_of(c), c["inv"], c["B"],
                       c["h"], c["short_cut"], rnd=(lambda t: r16(t, bf16)) if rounded else None, mutate=mutate)


def params_of(c):
    """the twenty-two tensors of a layer_case in layerfit_oracle.PARAMS order"""
    return [c[k] for k in lo.PARAMS]


def split_layer(r, Cc):
    """the six gradients of a result dict (or of a list in layerfit_oracle.LAYER order) under LAYER_PARTS' names"""
    dW, db, dWo, dbo, dg, dbe = [r[k] for k in lo.LAYER] if isinstance(r, dict) else r
    return {"dWq_s": dW[:Cc], "dWk_s": dW[Cc:2 * Cc], "dWv_s": dW[2 * Cc:], "dbq_s": db[:Cc], "dbk_s": db[Cc:2 * Cc], "dbv_s": db[2 * Cc:], "dWo_s": dWo,
            "dbo_s": dbo, "dgamma1": dg, "dbeta1": dbe}


def layer_backward_args(d, c, P, accumulate, outs, ws, eps=co.EPS):
    """the argument list of cs_op_layer_backward: d the device tensors by layer_case's names (Qs, Ks, Vs views of one packed buffer; K, V too), outs
    the twenty-two gradients in layerfit_oracle.KEYS order then the loss.  The rejection test edits single entries."""
    assert d["Qs"].stride(0) == d["Ks"].stride(0) == d["Vs"].stride(0)
    head = [_p(d["x0"]), _p(d["Qs"]), _p(d["Ks"]), _p(d["Vs"]), d["Qs"].stride(0), _p(d["Os"]), d["Os"].stride(0), _p(d["lse_s"]), _p(d["Wqp"]),
            d["Wqp"].stride(0), _p(d["Wo_s"]), d["Wo_s"].stride(0), _p(d["bo_s"]), _p(d["g1"])]
    cross = ch.cross_backward_args(d["x1"], d["Qp"], d["K"], d["V"], d["O"], d["lse"], d["mem"], d["W1"], d["Wo"], d["bo"], d["g2"], c["N"], c["h"],
                                   c["short_cut"], d["x2"], d["H"], d["X"], d["A"], d["W2"], d["b2"], d["g3"], d["Wa"], d["Wb"], d["bb"], d["gt"], c["B"],
                                   c["gh"], c["gw"], P, c["act"], c["p"], c["inv"], accumulate, outs, ws, eps)
    return head + cross


def layer_shapes(Cc, PP=196):
    return ((3 * Cc, Cc), (3 * Cc,), (Cc, Cc), (Cc,), (Cc,), (Cc,),
            (3 * Cc, Cc), (3 * Cc,), (Cc, Cc), (Cc,), (Cc,), (Cc,), (Cc, Cc), (Cc,), (Cc, Cc), (Cc,), (Cc,), (Cc,), (Cc, Cc), (Cc,), (PP, Cc), (PP,))


def layer_fro_bounds(r, c, bf16):
    """Per-part bounds (LAYER_PARTS) on the Frobenius norm of the error of the block's six gradients, cs_op_layer_backward against
    layerfit_oracle.backward (r, roundings on), built as crossfit_helpers.cross_fro_bounds builds its own: from the number formats, the shapes and
    the case's own tensors, never from what the kernel returns.

    The rounded intermediates in front of dx1 = dy2h + ln2 dQu Wq': the six of the cross-attention fit (g, dpre, dyh, dHh, dy2h, dOh) and dQu's own
    store, seven stages; each grants every element of dx1 a full spacing e16 of its value with signs that do not conspire, the stages in
    quadrature.  dQu also carries the cross-attention backward's inner roundings (Ph, dzh), bounded in Frobenius norm by
    crossfit_helpers.attn_fro_bounds and carried through ln2 Wq' with its spectral norm; and the fp32 GEMM behind it, (C + 4) 2^-24 of the sum of
    magnitudes.  So dgamma1 / dbeta1 see sqrt(7) e16 of their summands plus that Frobenius error times the largest |xhat1| (or 1).  dy1h is the
    eighth stage (dWo_s, dbo_s), dOsh the ninth; the in_proj blocks see those nine as a perturbation of their factor G = dQu_s | dKu_s | dV_s and,
    on top, the self-attention backward's own three roundings through attn_fro_bounds times the largest row norm of x0h -- and the Frobenius
    error of dx1 above, which reaches them through the LayerNorm backward (whose Jacobian has norm at most |gamma1|_max rstd_max: a projection
    scaled by gamma and rstd), Wo_s (spectral norm) and the attention backward (linear in dO; priced by the ratio |G|_F / |dOsh|_F of the case).
    Rigorously on top: the fp32 accumulations, (rows + 2 C + 12) 2^-24 of the Frobenius norm of the sum of magnitudes, and three roundings of the
    fp32 scale of the in_proj reductions."""
    e16 = 2.0 ** -7 if bf16 else 2.0 ** -10
    Cc, h, B, inv = c["C"], c["h"], c["B"], c["inv"]
    dh = Cc // h
    M = c["x0"].shape[0]
    rows = lambda t: t.pow(2).sum(1)  # noqa: E731
    one = lambda n: torch.ones((n, 1), dtype=F64)  # noqa: E731
    sp = lambda t: co.heads_of(t.reshape(B, -1, Cc), h)  # noqa: E731
    spec = lambda t: float(torch.linalg.matrix_norm(t.to(F64), 2))  # noqa: E731
    ab_x = ch.attn_fro_bounds(r["attn"], sp(c["Qp"]), sp(c["K"]), sp(c["V"]), sp(c["O"]), sp(r["dOh"]), c["lse"], bf16)
    ab_s = ch.attn_fro_bounds(r["attn_s"], sp(c["Qs"]), sp(c["Ks"]), sp(c["Vs"]), sp(c["Os"]), sp(r["dOsh"]), c["lse_s"], bf16)
    # the error of dx1 that is not a relative perturbation of its elements: the cross-attention backward's inner roundings and the fp32 GEMM
    e_dx1 = co.LN2 * (ab_x["dQu"] * spec(c["Wqp"]) + (Cc + 4) * U32 * float((r["dQu"].abs() @ c["Wqp"].abs()).norm()))
    dx, xh = r["dx1"], r["xhat1"]
    u = (M + 2 * Cc + 12) * U32
    out = {}
    out["dgamma1"] = inv * (math.sqrt(7.0) * e16 * float((dx * xh).norm()) + e_dx1 * float(xh.abs().max()) + u * float((dx * xh).abs().sum(0).norm()))
    out["dbeta1"] = inv * (math.sqrt(7.0) * e16 * float(dx.norm()) + e_dx1 + u * float(dx.abs().sum(0).norm()))
    rstd = 1.0 / torch.sqrt(c_var(r["y1"]) + co.EPS)
    e_dy1 = e_dx1 * float(c["g1"].abs().max()) * float(rstd.max())  # what e_dx1 becomes behind the LayerNorm backward
    e_dOs = e_dy1 * spec(c["Wo_s"])

    def red(name, G, X, stages, scale, extra):
        uu = (M + 2 * Cc + 12 + 3) * U32
        q = float((rows(G) * rows(X)).sum().sqrt())
        out[name] = inv * scale * (math.sqrt(stages * (e16 * q) ** 2 + (extra * float(rows(X).max().sqrt())) ** 2) + uu * float((G.abs().T @ X.abs()).norm()))

    nd = float(r["dOsh"].norm())
    rs = 1.0 / math.sqrt(dh)
    for nm, key, scale in (("q", "dQu_s", rs), ("k", "dKu_s", co.LN2), ("v", "dV_s", 1.0)):
        G = r[key]
        extra = ab_s[key[:-2]] + e_dOs * float(G.norm()) / nd
        red(f"dW{nm}_s", G, r["x0h"], 9, scale, extra)
        red(f"db{nm}_s", G, one(M), 9, scale, extra)
    red("dWo_s", r["dy1h"], c["Os"], 8, 1.0, e_dy1)
    red("dbo_s", r["dy1h"], one(M), 8, 1.0, e_dy1)
    return out


def c_var(y):
    """biased variance of every row, (M, 1)"""
    return y.to(F64).var(1, unbiased=False, keepdim=True)


def autograd_layer(c, autocast=None, loss_scale=1.0, eps=co.EPS):
    """The last decoder layer, the tail and the head as the reference's modules execute them (F.multi_head_attention_forward over the rows
    themselves, the residual, F.layer_norm, then the cross-attention block and the tail of crossfit_helpers.autograd_block) under torch.autograd
    on x0 and mem of a layer_case, in the dtype of its tensors -> (loss, the twenty-two gradients in layerfit_oracle.KEYS order).  autocast: a
    16-bit dtype to run it under torch.autocast on the CPU, the loss scaled by loss_scale."""
    import torch.nn.functional as F

    import headfit_oracle as ho
    prm = [c[k].detach().clone().requires_grad_(True) for k in lo.PARAMS]
    Win_s, bin_s, Wo_s, bo_s, g1, be1, Win, bin_, Wo, bo, g2, be2, W1, b1, W2, b2, g3, b3, Wa, ba, Wb, bb = prm
    B, Cc, h, gh, gw = c["B"], c["C"], c["h"], c["gh"], c["gw"]
    x0, mem, gt_rows = c["x0"].to(Win.dtype), c["mem"].to(Win.dtype), c["gt_rows"].to(Win.dtype)
    P = int(round(Wb.shape[0] ** 0.5))

    def run():
        q0 = x0.reshape(B, -1, Cc).transpose(0, 1)
        a0, _ = F.multi_head_attention_forward(q0, q0, q0, Cc, h, Win_s, bin_s, None, None, False, 0.0, Wo_s, bo_s, training=False, need_weights=False)
        a0 = a0.transpose(0, 1).reshape(-1, Cc)
        x1 = F.layer_norm((x0 + a0) if c["short_cut"] else a0, (Cc,), g1, be1, eps)
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


# ---- the device side of a case (GPU tests) ----
def gpu_attention(bf16):
    """(Qp, K, V) fp64 (B, h, L, dh) -> (O, lse) as cs_op_attention gives them for those operands (q_scale = 1), fp64 on the CPU"""
    from bits16 import bits16, vals16
    from hip_helpers import attention, switches

    def run(Qp, K, V):
        h = Qp.shape[1]
        dev = lambda t: bits16(co.merge_heads(t).float().cuda(), bf16).contiguous()  # noqa: E731
        with switches(bf16=bf16):
            O, lse = attention(dev(Qp), dev(K), dev(V), h, Qp.shape[3], lse=True, q_scale=1.0)
        torch.cuda.synchronize()
        return co.heads_of(vals16(O, bf16, F64).cpu(), h), lse.double().cpu()
    return run


def layer_device(c, bf16, P=14):
    """the operands of a layer_case on the device under its own names, the 16-bit ones strided views of poisoned buffers: Qs' | Ks | Vs in the
    first 3 C columns of rows of 3 C + 8 (the forward's packed rows, with a pitch of their own), K and V in the last 2 C columns of rows of 4 C"""
    import headfit_oracle as ho
    from bits16 import bits16
    from guard import poisoned_in
    Cc = c["C"]
    d16 = lambda t: bits16(t.float().cuda(), bf16)  # noqa: E731
    f32 = lambda t: t.float().cuda().contiguous()  # noqa: E731
    pin = lambda k, pad: poisoned_in(d16(c[k]), ld=Cc + pad)  # noqa: E731
    qkv = poisoned_in(torch.cat([d16(c["Qs"]), d16(c["Ks"]), d16(c["Vs"])], 1), ld=3 * Cc + 8)
    kv = torch.full((c["mem"].shape[0], 4 * Cc), float("nan"), dtype=torch.float16, device="cuda")
    kv[:, 2 * Cc:3 * Cc] = d16(c["K"])
    kv[:, 3 * Cc:] = d16(c["V"])
    kv = poisoned_in(kv, ld=4 * Cc)
    gt = ho.to_image(c["gt_rows"], c["B"], c["gh"], c["gw"], P).contiguous().cuda()
    return dict(x0=f32(c["x0"]), Qs=qkv[:, :Cc], Ks=qkv[:, Cc:2 * Cc], Vs=qkv[:, 2 * Cc:], Os=pin("Os", 24), lse_s=f32(c["lse_s"]), Wqp=pin("Wqp", 16),
                Wo_s=pin("Wo_s", 8), bo_s=f32(c["bo_s"]), g1=f32(c["g1"]),
                x1=f32(c["x1"]), Qp=pin("Qp", 8), K=kv[:, 2 * Cc:3 * Cc], V=kv[:, 3 * Cc:], O=pin("O", 16), lse=f32(c["lse"]), mem=pin("mem", 8),
                W1=pin("W1", 8), Wo=pin("Wo", 24), bo=f32(c["bo"]), g2=f32(c["g2"]), x2=f32(c["x2"]), H=pin("H", 8), X=pin("X", 16), A=pin("A", 8),
                W2=pin("W2", 8), b2=f32(c["b2"]), g3=f32(c["g3"]), Wa=pin("Wa", 24), Wb=pin("Wb", 8), bb=f32(c["bb"]), gt=gt)


def cross_args_device(d, c, P, accumulate, outs, ws):
    """the argument list of cs_op_cross_backward on the same device tensors (outs: its sixteen gradients, then the loss)"""
    return ch.cross_backward_args(d["x1"], d["Qp"], d["K"], d["V"], d["O"], d["lse"], d["mem"], d["W1"], d["Wo"], d["bo"], d["g2"], c["N"], c["h"],
                                  c["short_cut"], d["x2"], d["H"], d["X"], d["A"], d["W2"], d["b2"], d["g3"], d["Wa"], d["Wb"], d["bb"], d["gt"], c["B"],
                                  c["gh"], c["gw"], P, c["act"], c["p"], c["inv"], accumulate, outs, ws)
