"""fp64 restatement of the whole-layer fit for the tests, on top of tests/crossfit_oracle.py: the backward of the last decoder
layer's self-attention block (in_proj -> attention -> out_proj -> + residual -> norm1) in front of the cross-attention fit's.  torch on the CPU,
no autograd: every formula is written out.

Forward of the block, as the kernels run it (M = B Np rows, h heads of dh = C / h columns, c = log2(e) / sqrt(dh); x0 the rows that enter the layer):
    x0h = round16(x0);  Qs' = c (x0h Wq_s^T + bq_s),  Ks = x0h Wk_s^T + bk_s,  Vs = x0h Wv_s^T + bv_s  (16 bit; c folded into the packed weights)
    per batch item and head, over that item's own Np rows:  S2 = Qs' Ks^T,  lse_s = log2 sum_k 2^S2,  P = 2^(S2 - lse_s),  Os = P Vs  (16 bit)
    y1 = (do_short_cut ? x0 : 0) + Os Wo_s^T + bo_s,  x1 = LayerNorm(y1; gamma1, beta1, eps)
x1 then enters the cross-attention block twice: as the residual around it and, rounded, as the input of its query projection
    Q' = c (x1h Wq^T + bq) = x1h Wq'^T + bq'  with the packed Wq' = c Wq.

Backward (backward below), continuing crossfit_oracle.backward, whose sixteen gradients and loss stay as they are.  That chain leaves dy2h (the
gradient at y2, the cross block's pre-norm rows) and dQu with d loss / d Q' = ln2 dQu (its module docstring).  So
    dx1 = (do_short_cut ? dy2h : 0) + ln2 dQu Wq'            -- no new factor: Wq' carries c, and c ln2 = 1 / sqrt(dh)
    y1 recomputed from x0, the stored Os, Wo_s, bo_s;  (dgamma1, dbeta1, dy1h) = tailfit_oracle.ln_backward(y1, dx1, gamma1)
    dbo_s = inv_count sum_m dy1h;  dWo_s = inv_count dy1h^T Os;  dOsh = dy1h Wo_s rounded once
    (dQu_s, dKu_s, dV_s) = crossfit_oracle.attention_backward(Qs', Ks, Vs, Os, dOsh, lse_s), Lq = Lk = Np per batch item
    in_proj rows [0, C): inv_count / sqrt(dh) dQu_s^T x0h;  [C, 2C): inv_count ln2 dKu_s^T x0h;  [2C, 3C): inv_count dV_s^T x0h;  biases: column sums
The gradient stops at x0.  `rnd` (fp64 -> fp64, or None) rounds where the kernels round to the 16-bit operand type.

`mutate` (a string, tests only) plants one defect (MUTATIONS); tests/test_layerfit_host.py checks that each one exceeds the bounds of the op tests."""
import math

import torch

import crossfit_oracle as co
import tailfit_oracle as to

F64 = co.F64
EPS = co.EPS
LN2 = co.LN2
LOG2E = co.LOG2E
LAYER = ("dWin_s", "dbin_s", "dWo_s", "dbo_s", "dgamma1", "dbeta1")   # the six gradients of the block, in cs_layer_backward's order
KEYS = LAYER + co.KEYS
# the planted defects: what each one is, in the words of the issue
MUTATIONS = ("dx1_no_residual", "dx1_no_q", "dx1_no_ln2", "y1_no_residual", "cross_lse", "cross_O", "all_keys", "no_rsqrt_s", "no_ln2_s", "x1h_for_x0h")


def self_forward(x0, Win, bin_, Wo, bo, g1, b1, B, h, short_cut=True, eps=EPS, rnd=None, attn=None):
    """the block in fp64 from the module's own tensors (Win (3C, C) unscaled) -> dict(x0h, Qs, Ks, Vs, Os, lse_s, y1, x1): 16-bit rows as `rnd`
    left them.  x0 (B Np, C).  attn: (Qs, Ks, Vs as (B, h, Np, dh)) -> (Os, lse_s) in place of the oracle's attention"""
    rnd = rnd or (lambda t: t)
    x0, Win, bin_, Wo = (t.to(F64) for t in (x0, Win, bin_, Wo))
    Cc = x0.shape[1]
    c = LOG2E / math.sqrt(Cc // h)
    x0h = rnd(x0)
    Qs = rnd(c * (x0h @ Win[:Cc].T + bin_[:Cc]))
    Ks = rnd(x0h @ Win[Cc:2 * Cc].T + bin_[Cc:2 * Cc])
    Vs = rnd(x0h @ Win[2 * Cc:].T + bin_[2 * Cc:])
    sp = lambda t: co.heads_of(t.reshape(B, -1, Cc), h)  # noqa: E731
    if attn is None:
        O4, lse, _ = co.attention_forward(sp(Qs), sp(Ks), sp(Vs), rnd)
    else:
        O4, lse = attn(sp(Qs), sp(Ks), sp(Vs))
    Os = co.merge_heads(O4).reshape(-1, Cc)
    y1 = (x0 if short_cut else 0.0) + Os @ Wo.T + bo.to(F64)
    x1 = to.ln_stats(y1, eps)[2] * g1.to(F64) + b1.to(F64)
    return {"x0h": x0h, "Qs": Qs, "Ks": Ks, "Vs": Vs, "Os": Os, "lse_s": lse, "y1": y1, "x1": x1}


def backward(x0, Qs, Ks, Vs, Os, lse_s, Wqp, Wo_s, bo_s, g1, cross_args, inv_count, B, h, short_cut=True, rnd=None, eps=EPS, mutate=None):
    """-> dict of the twenty-two gradients (KEYS), loss and the intermediates.  Wqp: the cross-attention's PACKED query projection c Wq (C, C);
    cross_args: the positional arguments of crossfit_oracle.backward up to and including h (x1, Qp, K, V, O, lse, mem, ..., inv_count, B, h)."""
    rnd = rnd or (lambda t: t)
    x0, Qs, Ks, Vs, Os, Wqp, Wo_s = (t.to(F64) for t in (x0, Qs, Ks, Vs, Os, Wqp, Wo_s))
    Cc = x0.shape[1]
    dh = Cc // h
    r = co.backward(*cross_args, short_cut, rnd=rnd, eps=eps)
    x1, O_cross, lse_cross = cross_args[0].to(F64), cross_args[4].to(F64), cross_args[5].to(F64)
    if mutate == "cross_O":       # the stale buffer: p.dob holds the cross-attention's output by the time the backward runs
        Os = O_cross
    if mutate == "cross_lse":     # ... and p.lse that attention's log-sum-exp
        lse_s = lse_cross
    dq = (0.0 if mutate == "dx1_no_q" else (1.0 if mutate == "dx1_no_ln2" else LN2) * (r["dQu"] @ Wqp))
    dx1 = (r["dy2h"] if short_cut and mutate != "dx1_no_residual" else torch.zeros_like(x0)) + dq
    y1 = (x0 if short_cut and mutate != "y1_no_residual" else 0.0) + Os @ Wo_s.T + bo_s.to(F64)
    ln = to.ln_backward(y1, dx1, g1, inv_count, eps, rnd)
    dy1h = ln["dyh"]
    dOsh = rnd(dy1h @ Wo_s)
    sp = lambda t: co.heads_of(t.reshape(B, -1, Cc), h)  # noqa: E731
    if mutate == "all_keys":      # one launch over all B Np rows: every query also attends to the other batch items' keys
        al = lambda t: co.heads_of(t.reshape(1, -1, Cc), h).expand(B, -1, -1, -1)  # noqa: E731
        a = co.attention_backward(sp(Qs), al(Ks), al(Vs), sp(Os), sp(dOsh), lse_s, rnd)
        fold = lambda t: rnd(co.merge_heads(t.sum(0, keepdim=True)).reshape(-1, Cc))  # noqa: E731
        dQu, dKu, dV = co.merge_heads(a["dQu"]).reshape(-1, Cc), fold(a["dKu"]), fold(a["dV"])
    else:
        a = co.attention_backward(sp(Qs), sp(Ks), sp(Vs), sp(Os), sp(dOsh), lse_s, rnd)
        dQu, dKu, dV = (co.merge_heads(a[k]).reshape(-1, Cc) for k in co.ATTN)
    xin = rnd(x1) if mutate == "x1h_for_x0h" else rnd(x0)
    dWin, dbin = co.in_proj_gradients(dQu, dKu, dV, xin, xin, dh, inv_count, ln2=1.0 if mutate == "no_ln2_s" else LN2,
                                      rsqrt=1.0 if mutate == "no_rsqrt_s" else None)
    r.update({"dWin_s": dWin, "dbin_s": dbin, "dWo_s": inv_count * (dy1h.T @ Os), "dbo_s": inv_count * dy1h.sum(0), "dgamma1": ln["dgamma"],
              "dbeta1": ln["dbeta"], "dx1": dx1, "y1": y1, "dy1h": dy1h, "dOsh": dOsh, "xhat1": ln["xhat"], "dQu_s": dQu, "dKu_s": dKu, "dV_s": dV,
              "attn_s": a, "x0h": rnd(x0)})
    return r


PARAMS = ("Win_s", "bin_s", "Wo_s", "bo_s", "g1", "be1") + co.PARAMS  # the twenty-two tensors, in KEYS order


def forward_backward(x0, mem, params, gt_rows, act, p, B, h, short_cut=True, rnd=None, mutate=None):
    """the layer, the tail and the head forward from the twenty-two tensors, then backward() -> its dict"""
    rnd_ = rnd or (lambda t: t)
    Win_s, bin_s, Wo_s, bo_s, g1, be1 = params[:6]
    Win, bin_, Wo, bo, g2, be2, W1, b1, W2, b2, g3, b3, Wa, ba, Wb, bb = params[6:]
    sf = self_forward(x0, Win_s, bin_s, Wo_s, bo_s, g1, be1, B, h, short_cut, rnd=rnd)
    x1 = sf["x1"]
    blk = co.block_forward(x1, mem, Win, bin_, Wo, bo, g2, be2, B, h, short_cut, rnd=rnd)
    H, _, X, A = to.tail_forward(blk["x2"], W1, b1, W2, b2, g3, b3, Wa, ba, rnd=rnd)
    Cc = x0.shape[1]
    inv = 1.0 / gt_rows.numel()
    cross_args = (x1, blk["Qp"], blk["K"], blk["V"], blk["O"], blk["lse"], mem, W1, Wo, bo, g2, blk["x2"], H, X, A, W2, b2, g3, Wa, Wb, bb, gt_rows,
                  act, p, inv, B, h)
    Wqp = rnd_(LOG2E / math.sqrt(Cc // h) * Win[:Cc].to(F64))
    return backward(x0, sf["Qs"], sf["Ks"], sf["Vs"], sf["Os"], sf["lse_s"], Wqp, Wo_s, bo_s, g1, cross_args, inv, B, h, short_cut, rnd=rnd, mutate=mutate)


def fit(x0, mem, params, gt_rows, act, p, B, h, steps, short_cut=True, lr=5e-4, **adam):
    """`steps` AdamW steps of the twenty-two tensors on one fixed batch in fp64 (x0 and mem fixed: everything in front of the last layer is
    frozen) -> (losses before each step, final params in PARAMS order)"""
    import headfit_oracle as ho
    params = [t.to(F64).clone() for t in params]
    m = [torch.zeros_like(t) for t in params]
    v = [torch.zeros_like(t) for t in params]
    losses = []
    for t in range(1, steps + 1):
        r = forward_backward(x0, mem, params, gt_rows, act, p, B, h, short_cut)
        losses.append(float(r["loss"]))
        for k, key in enumerate(KEYS):
            params[k], m[k], v[k] = ho.adamw_step(params[k], m[k], v[k], r[key], t, lr=lr, **adam)
    return losses, params
