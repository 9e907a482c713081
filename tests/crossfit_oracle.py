"""fp64 restatement of the cross-attention fit for the tests, on top of tests/tailfit_oracle.py: the backward of the last
decoder layer's cross-attention block (in_proj -> attention -> out_proj -> + residual -> norm2) in front of the tail's.  torch on the CPU, no
autograd: every formula is written out.

Forward of the block, as the kernels run it (M = B Np query rows, Mk = B N Np memory rows, h heads of dh = C / h columns, c = log2(e) / sqrt(dh)):
    Q' = c (x1h Wq^T + bq) (16 bit: the forward folds c into the packed Wq / bq),  K = mem Wk^T + bk,  V = mem Wv^T + bv  (16 bit)
    per batch item and head:  S2 = Q' K^T,  lse = log2 sum_k 2^S2,  P = 2^(S2 - lse),  O = P V  (16 bit)
    y2 = (do_short_cut ? x1 : 0) + O Wo^T + bo,  x2 = LayerNorm(y2; gamma2, beta2, eps)
2^S2 = e^(S2 ln2) and S2 ln2 = (q . k) / sqrt(dh) for the unscaled projection q = Q' / c, so P is exactly the softmax the reference computes.

Backward of the attention (attention_backward below; everything per batch item and head):
    D[q] = sum_d dO[q, d] O[q, d];   dP = dO V^T;   dz = P (dP - D)          -- dz is d loss / d (S2 ln2), the gradient at the NATURAL logits
    dV = Ph^T dO;   dKu = dzh^T Q';   dQu = dzh K                             -- Ph, dzh: P and dz rounded once
Scaling derivation.  With a = S2 ln2 the natural logits, d loss / d S2 = ln2 dz.  S2 = Q' K^T gives d loss / d K = ln2 dz^T Q' = ln2 dKu and
d loss / d Q' = ln2 dz K = ln2 dQu.  The unscaled projection q = Q' / c has d loss / d q = c ln2 dQu = dQu / sqrt(dh), because
c ln2 = log2(e) ln2 / sqrt(dh) = 1 / sqrt(dh).  So the in_proj gradients are
    rows [0, C):   inv_count / sqrt(dh) dQu^T x1h,  bias inv_count / sqrt(dh) sum_m dQu
    rows [C, 2C):  inv_count ln2 dKu^T mem,         bias inv_count ln2 sum dKu     (zero in exact arithmetic: sum_k dz[q, k] = 0)
    rows [2C, 3C): inv_count dV^T mem,              bias inv_count sum dV
and dKu / dQu carry no scalar themselves (the two factors go into the fp32 scale of the reductions; no extra 16-bit rounding is spent on them).

The chain in front of it (backward below), continuing tailfit_oracle.backward, whose ten gradients and loss stay as they are:
    dx2 = dyh + dHh W1                              (the residual around the feed-forward block plus linear1's input gradient)
    y2 recomputed from x1, the stored O, Wo, bo;  (dgamma2, dbeta2, dy2h) = tailfit_oracle.ln_backward(y2, dx2, gamma2)
    dbo = inv_count sum_m dy2h;  dWo = inv_count dy2h^T O;  dOh = dy2h Wo rounded once
The gradient stops at x1 and at mem.  `rnd` (fp64 -> fp64, or None) rounds where the kernels round to the 16-bit operand type.

`mutate` (a string, tests only) plants one defect; tests/test_crossfit_host.py checks that each one exceeds the bounds of the op tests."""
import math

import torch

import tailfit_oracle as to

F64 = to.F64
EPS = to.EPS
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
ATTN = ("dQu", "dKu", "dV")
CROSS = ("dWin", "dbin", "dWo", "dbo", "dgamma2", "dbeta2")   # the six gradients of the block, in cs_cross_backward's order
KEYS = CROSS + to.KEYS
MUTATIONS = ("no_D", "dP_for_dz", "natural_exp", "wrong_head_lse", "skip_ragged_keys", "skip_ragged_queries", "swap_kq", "padded_keys")


def heads_of(t, h):
    """(B, L, h dh) -> (B, h, L, dh)"""
    B, L, Cc = t.shape
    return t.reshape(B, L, h, Cc // h).permute(0, 2, 1, 3)


def merge_heads(t):
    """(B, h, L, dh) -> (B, L, h dh)"""
    B, h, L, dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, L, h * dh)


def attention_forward(Qp, K, V, rnd=None):
    """Qp (pre-scaled by c), K, V: (B, h, L, dh) -> (O as `rnd` left it, lse (B, h, Lq) base 2, P)"""
    rnd = rnd or (lambda t: t)
    S2 = Qp.to(F64) @ K.to(F64).transpose(-1, -2)
    m = S2.max(-1, keepdim=True)[0]
    lse = m[..., 0] + torch.log2(torch.exp2(S2 - m).sum(-1))
    P = torch.exp2(S2 - lse[..., None])
    return rnd(P @ V.to(F64)), lse, P


def attention_backward(Qp, K, V, O, dO, lse, rnd=None, mutate=None, tile=64):
    """Qp, O, dO: (B, h, Lq, dh); K, V: (B, h, Lk, dh); lse (B, h, Lq) -> dict(dQu, dKu, dV as `rnd` left them, and S2, P, Ph, D, dP, dz, dzh)"""
    rnd = rnd or (lambda t: t)
    Qp, K, V, O, dO, lse = (t.to(F64) for t in (Qp, K, V, O, dO, lse))
    Lq, Lk = Qp.shape[-2], K.shape[-2]
    if mutate == "wrong_head_lse":
        lse = lse.roll(1, dims=1)
    S2 = Qp @ K.transpose(-1, -2)
    P = torch.exp(S2 - lse[..., None]) if mutate == "natural_exp" else torch.exp2(S2 - lse[..., None])
    D = (dO * O).sum(-1)
    if mutate == "no_D":
        D = torch.zeros_like(D)
    dP = dO @ V.transpose(-1, -2)
    dz = dP if mutate == "dP_for_dz" else P * (dP - D[..., None])
    if mutate == "skip_ragged_keys" and Lk % tile:      # the last, ragged key tile contributes nothing
        P, dz = P.clone(), dz.clone()
        P[..., Lk - Lk % tile:] = 0
        dz[..., Lk - Lk % tile:] = 0
    if mutate == "skip_ragged_queries" and Lq % tile:   # the last, ragged query tile contributes nothing
        P, dz = P.clone(), dz.clone()
        P[..., Lq - Lq % tile:, :] = 0
        dz[..., Lq - Lq % tile:, :] = 0
    Ph, dzh = rnd(P), rnd(dz)
    dQ = dzh @ K
    if mutate == "padded_keys" and Lk % tile:
        # the keys that fill the ragged last tile do not exist: their K and V rows arrive as zeros.  Counted all the same, each takes
        # P = 2^(0 - lse) and dz = P (0 - D), rounded like every other, and meets a zero K row in dQu: nothing, unless 2^(-lse) leaves the operand
        # type's range (lse < -16 in fp16, < -128 in bf16 and in the kernel's fp32) -- then inf x 0 puts a NaN into the query's whole row
        pad = tile - Lk % tile
        dz_pad = rnd(torch.exp2(-lse) * (0.0 - D))[..., None].expand(*D.shape, pad)
        dQ = dQ + dz_pad @ torch.zeros((pad, K.shape[-1]), dtype=F64)
    dKu = dzh @ K if mutate == "swap_kq" and Lq == Lk else dzh.transpose(-1, -2) @ Qp  # (K and Q swapped: the shapes allow it where Lq = Lk)
    return {"dQu": rnd(dQ), "dKu": rnd(dKu), "dV": rnd(Ph.transpose(-1, -2) @ dO), "S2": S2, "P": P, "Ph": Ph, "D": D,
            "dP": dP, "dz": dz, "dzh": dzh}


def in_proj_gradients(dQu, dKu, dV, x1h, mem, dh, inv_count, ln2=LN2, rsqrt=None):
    """dQu (M, C), dKu, dV (Mk, C), x1h (M, C), mem (Mk, C) -> (dWin (3C, C), dbin (3C)): the scalars of the module docstring in the reductions"""
    rs = 1.0 / math.sqrt(dh) if rsqrt is None else rsqrt
    dW = torch.cat([inv_count * rs * (dQu.T @ x1h), inv_count * ln2 * (dKu.T @ mem), inv_count * (dV.T @ mem)])
    db = torch.cat([inv_count * rs * dQu.sum(0), inv_count * ln2 * dKu.sum(0), inv_count * dV.sum(0)])
    return dW, db


def block_forward(x1, mem, Win, bin_, Wo, bo, g2, b2, B, h, short_cut=True, eps=EPS, rnd=None):
    """the block in fp64 from the module's own tensors (Win (3C, C) unscaled) -> dict(x1h, Qp, K, V, O, lse, y2, x2): 16-bit rows as `rnd` left them.
    x1 (B Np, C), mem (B N Np, C)"""
    rnd = rnd or (lambda t: t)
    x1, mem, Win, bin_, Wo = (t.to(F64) for t in (x1, mem, Win, bin_, Wo))
    Cc = x1.shape[1]
    dh = Cc // h
    c = LOG2E / math.sqrt(dh)
    x1h = rnd(x1)
    Qp = rnd(c * (x1h @ Win[:Cc].T + bin_[:Cc]))
    K = rnd(mem @ Win[Cc:2 * Cc].T + bin_[Cc:2 * Cc])
    V = rnd(mem @ Win[2 * Cc:].T + bin_[2 * Cc:])
    O4, lse, _ = attention_forward(heads_of(Qp.reshape(B, -1, Cc), h), heads_of(K.reshape(B, -1, Cc), h), heads_of(V.reshape(B, -1, Cc), h), rnd)
    O = merge_heads(O4).reshape(-1, Cc)
    y2 = (x1 if short_cut else 0.0) + O @ Wo.T + bo.to(F64)
    x2 = to.ln_stats(y2, eps)[2] * g2.to(F64) + b2.to(F64)
    return {"x1h": x1h, "Qp": Qp, "K": K, "V": V, "O": O, "lse": lse, "y2": y2, "x2": x2}


def backward(x1, Qp, K, V, O, lse, mem, W1, Wo, bo, g2, x2, H, X, A, W2, b2, g3, Wa, Wb, bb, gt_rows, act, p, inv_count, B, h, short_cut=True,
             rnd=None, eps=EPS, mutate=None):
    """-> dict of the sixteen gradients (KEYS), loss and the intermediates; rows (M, C) / (Mk, C), lse (B, h, Np).  mutate: MUTATIONS, or
    "no_ln2" | "no_rsqrt" | "y2_no_residual" | "dx2_no_ffn" """
    rnd = rnd or (lambda t: t)
    x1, Qp, K, V, O, mem, W1, Wo = (t.to(F64) for t in (x1, Qp, K, V, O, mem, W1, Wo))
    Cc = x1.shape[1]
    dh = Cc // h
    r = to.backward(x2, H, X, A, W2, b2, g3, Wa, Wb, bb, gt_rows, act, p, inv_count, rnd, eps)
    dx2 = r["dyh"] + (0.0 if mutate == "dx2_no_ffn" else r["dHh"] @ W1)
    y2 = (x1 if short_cut and mutate != "y2_no_residual" else 0.0) + O @ Wo.T + bo.to(F64)
    ln = to.ln_backward(y2, dx2, g2, inv_count, eps, rnd)
    dy2h = ln["dyh"]
    dOh = rnd(dy2h @ Wo)
    sp = lambda t: heads_of(t.reshape(B, -1, Cc), h)  # noqa: E731
    a = attention_backward(sp(Qp), sp(K), sp(V), sp(O), sp(dOh), lse, rnd, mutate if mutate in MUTATIONS else None)
    dQu, dKu, dV = (merge_heads(a[k]).reshape(-1, Cc) for k in ATTN)
    dWin, dbin = in_proj_gradients(dQu, dKu, dV, rnd(x1), mem, dh, inv_count, ln2=1.0 if mutate == "no_ln2" else LN2,
                                   rsqrt=1.0 if mutate == "no_rsqrt" else None)
    r.update({"dWin": dWin, "dbin": dbin, "dWo": inv_count * (dy2h.T @ O), "dbo": inv_count * dy2h.sum(0), "dgamma2": ln["dgamma"], "dbeta2": ln["dbeta"],
              "dx2": dx2, "y2": y2, "dy2h": dy2h, "dOh": dOh, "xhat2": ln["xhat"], "dQu": dQu, "dKu": dKu, "dV": dV, "attn": a, "x1h": rnd(x1)})
    return r


PARAMS = ("Win", "bin", "Wo", "bo", "g2", "be2", "W1", "b1", "W2", "b2", "g3", "b3", "Wa", "ba", "Wb", "bb")  # the sixteen tensors, in KEYS order


def forward_backward(x1, mem, params, gt_rows, act, p, B, h, short_cut=True, rnd=None):
    """the block, the tail and the head forward from the sixteen tensors, then backward() -> its dict"""
    Win, bin_, Wo, bo, g2, be2, W1, b1, W2, b2, g3, b3, Wa, ba, Wb, bb = params
    blk = block_forward(x1, mem, Win, bin_, Wo, bo, g2, be2, B, h, short_cut, rnd=rnd)
    H, _, X, A = to.tail_forward(blk["x2"], W1, b1, W2, b2, g3, b3, Wa, ba, rnd=rnd)
    return backward(x1, blk["Qp"], blk["K"], blk["V"], blk["O"], blk["lse"], mem, W1, Wo, bo, g2, blk["x2"], H, X, A, W2, b2, g3, Wa, Wb, bb, gt_rows,
                    act, p, 1.0 / gt_rows.numel(), B, h, short_cut, rnd=rnd)


def fit(x1, mem, params, gt_rows, act, p, B, h, steps, short_cut=True, lr=5e-4, step_size=None, gamma=1.0, **adam):
    """`steps` AdamW steps of the sixteen tensors on one fixed batch in fp64 (x1 and mem fixed: everything in front of the last cross-attention
    is frozen) -> (losses before each step, final params in PARAMS order); StepLR as in headfit_oracle.fit"""
    import headfit_oracle as ho
    params = [t.to(F64).clone() for t in params]
    m = [torch.zeros_like(t) for t in params]
    v = [torch.zeros_like(t) for t in params]
    losses = []
    for t in range(1, steps + 1):
        r = forward_backward(x1, mem, params, gt_rows, act, p, B, h, short_cut)
        losses.append(float(r["loss"]))
        rate = ho.step_lr(lr, step_size, gamma, t - 1) if step_size else lr
        for k, key in enumerate(KEYS):
            params[k], m[k], v[k] = ho.adamw_step(params[k], m[k], v[k], r[key], t, lr=rate, **adam)
    return losses, params
