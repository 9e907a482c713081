"""fp64 restatement of the tail fit for the tests, on top of tests/headfit_oracle.py: the backward of the last decoder layer's
linear1 -> ReLU -> linear2 -> + residual -> norm3 in front of the head's.  torch on the CPU, no autograd: every formula is written out.

Tail forward: H = relu(x2h W1^T + b1), y = x2 + H W2^T + b2, mu = mean_c y, rstd = 1 / sqrt(mean_c (y - mu)^2 + eps), xhat = (y - mu) rstd,
X = xhat gamma + beta, then the head (headfit_oracle).  The FFN is always closed with the residual, whatever do_short_cut says.  No dropout.

Backward (this build owns the definition; n = the pixel count of the whole batch, inv_count = 1 / n):
    the head part is headfit_oracle.backward on the forward's STORED X and A: dWa, dba, dWb, dbb, loss and dpre (rounded once)
    dX = dpre Wa
    y is RECOMPUTED from x2, the stored H, W2 and b2 (the forward never stores its pre-LayerNorm sum; its fused kernel adds the same products in
      another order); mu, rstd and xhat come from that y
    dgamma = inv_count sum_m dX xhat;  dbeta = inv_count sum_m dX
    dy = rstd (gamma dX - mean_c(gamma dX) - xhat mean_c(gamma dX xhat)), rounded once -> dyh
    db2 = inv_count sum_m dyh;  dW2 = inv_count dyh^T H
    dH = (dyh W2) [H > 0], rounded once -> dHh (the mask reads the stored activation; H == 0 takes 0, as relu's backward does)
    db1 = inv_count sum_m dHh;  dW1 = inv_count dHh^T x2h,  x2h = x2 rounded once
    dx2 is not formed: the gradient stops there.
`rnd` (a function fp64 -> fp64, or None) rounds where the kernels round to the 16-bit operand type."""
import torch

import headfit_oracle as ho

F64 = ho.F64
EPS = 1e-5
TAIL = ("dW1", "db1", "dW2", "db2", "dg3", "db3")       # the six gradients below the head, in cs_tail_backward's order
KEYS = TAIL + ("dWa", "dba", "dWb", "dbb")


def ln_stats(y, eps=EPS):
    """-> (mu, rstd, xhat) of the rows of y: biased variance, two-pass"""
    mu = y.mean(1, keepdim=True)
    rstd = 1.0 / ((y - mu).pow(2).mean(1, keepdim=True) + eps).sqrt()
    return mu, rstd, (y - mu) * rstd


def ln_backward(y, dX, gamma, inv_count, eps=EPS, rnd=None):
    """-> dict(dy (unrounded), dyh, dgamma, dbeta, xhat, rstd)"""
    rnd = rnd or (lambda t: t)
    y, dX, gamma = y.to(F64), dX.to(F64), gamma.to(F64)
    _, rstd, xhat = ln_stats(y, eps)
    gd = gamma * dX
    dy = rstd * (gd - gd.mean(1, keepdim=True) - xhat * (gd * xhat).mean(1, keepdim=True))
    return {"dy": dy, "dyh": rnd(dy), "dgamma": inv_count * (dX * xhat).sum(0), "dbeta": inv_count * dX.sum(0), "xhat": xhat, "rstd": rstd}


def tail_forward(x2, W1, b1, W2, b2, g3, b3, Wa, ba, eps=EPS, rnd=None):
    """-> (H, y, X, A) of the tail in fp64, rounded by `rnd` where the forward stores 16-bit rows (x2h, H, the head's operand X, A)"""
    rnd = rnd or (lambda t: t)
    x2 = x2.to(F64)
    H = rnd(torch.relu(rnd(x2) @ W1.to(F64).T + b1.to(F64)))
    y = x2 + H @ W2.to(F64).T + b2.to(F64)
    X = rnd(ln_stats(y, eps)[2] * g3.to(F64) + b3.to(F64))
    A = rnd(ho.leaky(X @ Wa.to(F64).T + ba.to(F64)))
    return H, y, X, A


def backward(x2, H, X, A, W2, b2, g3, Wa, Wb, bb, gt_rows, act, p, inv_count, rnd=None, eps=EPS):
    """-> dict of the ten gradients (KEYS), loss, and the intermediates dpre, dX, y, dy, dyh, dH (unrounded), dHh, x2h, xhat"""
    rnd = rnd or (lambda t: t)
    x2, H, W2, Wa = x2.to(F64), H.to(F64), W2.to(F64), Wa.to(F64)
    r = ho.backward(X, A, Wb, bb, gt_rows, act, p, inv_count, rnd)
    dX = r["dpre"] @ Wa
    y = x2 + H @ W2.T + b2.to(F64)
    ln = ln_backward(y, dX, g3, inv_count, eps, rnd)
    dyh = ln["dyh"]
    dH = (dyh @ W2) * (H > 0).to(F64)
    dHh = rnd(dH)
    x2h = rnd(x2)
    r.update({"dW1": inv_count * (dHh.T @ x2h), "db1": inv_count * dHh.sum(0), "dW2": inv_count * (dyh.T @ H), "db2": inv_count * dyh.sum(0),
              "dg3": ln["dgamma"], "db3": ln["dbeta"], "dX": dX, "y": y, "dy": ln["dy"], "dyh": dyh, "dH": dH, "dHh": dHh, "x2h": x2h,
              "xhat": ln["xhat"], "rstd": ln["rstd"]})
    return r


def fit(x2, params, gt_rows, act, p, steps, lr=5e-4, step_size=None, gamma=1.0, **adam):
    """`steps` AdamW steps of the tail on one fixed batch in fp64 (x2 fixed: everything below the last norm2 is frozen) -> (losses before each
    step, final params); params = [W1, b1, W2, b2, g3, b3, Wa, ba, Wb, bb]; StepLR as in headfit_oracle.fit"""
    x2 = x2.to(F64)
    params = [t.to(F64).clone() for t in params]
    m = [torch.zeros_like(t) for t in params]
    v = [torch.zeros_like(t) for t in params]
    inv = 1.0 / gt_rows.numel()
    losses = []
    for t in range(1, steps + 1):
        W1, b1, W2, b2, g3, b3, Wa, ba, Wb, bb = params
        H, _, X, A = tail_forward(x2, W1, b1, W2, b2, g3, b3, Wa, ba)
        r = backward(x2, H, X, A, W2, b2, g3, Wa, Wb, bb, gt_rows, act, p, inv)
        losses.append(float(r["loss"]))
        rate = ho.step_lr(lr, step_size, gamma, t - 1) if step_size else lr
        for k, key in enumerate(KEYS):
            params[k], m[k], v[k] = ho.adamw_step(params[k], m[k], v[k], r[key], t, lr=rate, **adam)
    return losses, params
