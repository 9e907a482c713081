"""Support of the tail-fit tests: torch-tensor wrappers over the tail's entry points of the C ABI (row pitches are the
tensors' own strides, as in headfit_helpers), the autograd tail the reference's modules execute, and the bounds the op tests assemble."""
import torch
import torch.nn.functional as F

import headfit_oracle as ho
import select_oracle as so
import tailfit_oracle as to
from crossscore_amd import _lib
from headfit_helpers import _p, _st, workspace

F64 = torch.float64
U32 = 2.0 ** -24


def ln_row_tile():
    return _lib.load().cs_tail_fit_ln_row_tile()


def ln_backward_args(y, dX, gamma, eps, bf16, inv_count, accumulate, dyh, dgamma, dbeta, ws):
    """the argument list of cs_op_ln_backward; the rejection tests edit single entries"""
    M, Cc = y.shape
    return [_p(y), y.stride(0), _p(dX), dX.stride(0), _p(gamma), M, Cc, float(eps), int(bf16), float(inv_count), int(accumulate), _p(dyh),
            dyh.stride(0), _p(dgamma), _p(dbeta), _p(ws), _st()]


def ln_backward(y, dX, gamma, eps, bf16, inv_count, accumulate, dyh, dgamma, dbeta):
    lib = _lib.load()
    ws = workspace(lib.cs_ln_backward_workspace_bytes(*y.shape), y.device)
    _lib.check(lib.cs_op_ln_backward(*ln_backward_args(y, dX, gamma, eps, bf16, inv_count, accumulate, dyh, dgamma, dbeta, ws)))
    torch.cuda.synchronize()  # (the workspace is this call's)


def tail_backward_args(x2, H, X, A, W2, b2, g3, Wa, Wb, bb, gt, B, gh, gw, P, act, powp, inv_count, accumulate, outs, ws, eps=to.EPS):
    """the argument list of cs_op_tail_backward (outs: the ten gradients in tailfit_oracle.KEYS order, then the loss)"""
    return [_p(x2), _p(H), H.stride(0), _p(X), X.stride(0), _p(A), A.stride(0), _p(W2), W2.stride(0), _p(b2), _p(g3), float(eps), _p(Wa),
            Wa.stride(0), _p(Wb), Wb.stride(0), _p(bb), _p(gt), B, gh, gw, P, A.shape[1], act, powp, float(inv_count), int(accumulate)] + \
           [_p(t) for t in outs] + [_p(ws), _st()]


def fresh_outs(Cc, P=14, dev="cuda", fill=7.0):
    shapes = ((Cc, Cc), (Cc,), (Cc, Cc), (Cc,), (Cc,), (Cc,), (Cc, Cc), (Cc,), (P * P, Cc), (P * P,))
    return [torch.full(s, fill, device=dev) for s in shapes] + [torch.full((), fill, dtype=F64, device=dev)]


def tail_backward(x2, H, X, A, W2, b2, g3, Wa, Wb, bb, gt, B, gh, gw, P, act, powp, inv_count, accumulate=False, outs=None):
    lib = _lib.load()
    M, Cc = A.shape
    if outs is None:
        outs = fresh_outs(Cc, P, A.device)
    ws = workspace(lib.cs_tail_backward_workspace_bytes(M, Cc, P), A.device)
    _lib.check(lib.cs_op_tail_backward(*tail_backward_args(x2, H, X, A, W2, b2, g3, Wa, Wb, bb, gt, B, gh, gw, P, act, powp, inv_count,
                                                           accumulate, outs, ws)))
    torch.cuda.synchronize()
    return outs


def autograd_tail(x2, params, gt, act, p, gh, gw, P, autocast=None, loss_scale=1.0, eps=to.EPS):
    """The tail as the reference's modules execute it (F.linear, F.relu, F.layer_norm, F.leaky_relu, F.linear, sigmoid | tanh, pow, the jigsaw,
    L1Loss) under torch.autograd, in the dtype of its inputs -> (loss, the ten gradients in tailfit_oracle.KEYS order).  autocast: a 16-bit
    dtype to run it under torch.autocast on the CPU with the loss scaled by loss_scale and the gradients unscaled, as a GradScaler does."""
    prm = [t.detach().clone().requires_grad_(True) for t in params]
    W1, b1, W2, b2, g3, b3, Wa, ba, Wb, bb = prm
    B = gt.shape[0]

    def run():
        H = F.relu(F.linear(x2, W1, b1))
        X = F.layer_norm(x2 + F.linear(H, W2, b2), (x2.shape[1],), g3, b3, eps)
        z = F.linear(F.leaky_relu(F.linear(X, Wa, ba), ho.LEAKY), Wb, bb)
        sg = torch.sigmoid(z) if act == 0 else torch.tanh(z)
        s = sg if p == 1 else sg ** p
        return torch.nn.L1Loss()(ho.to_image(s, B, gh, gw, P), gt)

    if autocast is None:
        loss = run()
    else:
        with torch.autocast("cpu", dtype=autocast):
            loss = run()
    (loss * loss_scale).backward()
    return loss.detach(), [t.grad.detach() / loss_scale for t in prm]


def rel_fro(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def tail_params(net):
    """the ten tail tensors of a module, detached, in TAIL_KEYS order"""
    return [p.detach() for p in net.tail_parameters()]


def ln_backward_seq32(y, dX, gamma, inv_count, eps=to.EPS):
    """The fp32-sequential restatement of tailfit_oracle.ln_backward: the same formulas in fp32, every sum over the columns and over the rows
    added in index order -> (dy, dgamma, dbeta) fp32"""
    y, dX, gamma = y.float(), dX.float(), gamma.float()
    M, Cc = y.shape
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731

    def rowsum(t):
        acc = torch.zeros((M,), dtype=torch.float32)
        for c in range(Cc):
            acc = acc + t[:, c]
        return acc[:, None]

    mu = rowsum(y) / f32(Cc)
    d = y - mu
    rstd = f32(1.0) / torch.sqrt(rowsum(d * d) / f32(Cc) + f32(eps))
    xhat = d * rstd
    gd = gamma * dX
    m1, m2 = rowsum(gd) / f32(Cc), rowsum(gd * xhat) / f32(Cc)
    dy = rstd * (gd - m1 - xhat * m2)
    dg, db = torch.zeros((Cc,), dtype=torch.float32), torch.zeros((Cc,), dtype=torch.float32)
    for m in range(M):
        dg = dg + dX[m] * xhat[m]
        db = db + dX[m]
    return dy, f32(inv_count) * dg, f32(inv_count) * db


def ln_bounds(y, dX, gamma, inv_count, eps=to.EPS):
    """(bound of dy before its 16-bit rounding, of dgamma, of dbeta): select_oracle.tolerance of the restatement above against the fp64 oracle"""
    r = to.ln_backward(y, dX, gamma, inv_count, eps)
    dy, dg, db = ln_backward_seq32(y, dX, gamma, inv_count, eps)
    return (so.tolerance(r["dy"].numpy(), dy.numpy()), so.tolerance(r["dgamma"].numpy(), dg.numpy()), so.tolerance(r["dbeta"].numpy(), db.numpy()))


def tail_fro_bounds(r, H, M, Cc, inv_count, bf16):
    """Per-tensor bounds on the Frobenius norm of the error of the six gradients below the head, cs_op_tail_backward against
    tailfit_oracle.backward (r, run with the operand roundings on), from the number formats, M, C and the case's own tensors (fp64, CPU).

    The kernels and the oracle round the same four intermediates (g, dpre, dyh, dHh) to the operand type, from fp32 and fp64 pre-images; an
    element differs only where the two pre-images straddle a rounding boundary, and then by one spacing, at most e16 = 2^-10 (fp16) / 2^-7
    (bf16) of its value.  An element-wise worst case -- every element of every intermediate off by a spacing, all signs aligned through
    every product -- exceeds the gradients themselves and checks nothing.  The bound here grants the far-from-real event that EVERY element of
    ALL FOUR intermediates is off by a full spacing, but with signs that do not conspire (they are decided by the last bits of unrelated
    sums): a perturbation d of the factor G of a row sum S = sum_m G_m (x) X_m with |d_mn| <= e16 |G_mn| and independent signs has
    E |dS|_F^2 <= e16^2 sum_m |G_m|^2 |X_m|^2 =: (e16 Q)^2, and the four stages add in quadrature: 2 e16 Q.  Q is computed from the oracle's
    own factors, so a cancellation in S is priced in.  On top, rigorously: the fp32 accumulations, (M + 2 C + 12) 2^-24 of the Frobenius norm
    of the sum of magnitudes (M rows of the gemm_tn or the column sum, C products in each of the two GEMMs a factor went through, the
    LayerNorm's own sums).  A zero output, a missing ReLU mask or a missing mean term of the LayerNorm backward moves a gradient by tens of
    percents of its norm; these bounds are 2e-3 (fp16) and 1.6e-2 (bf16) of Q."""
    e16 = 2.0 ** -7 if bf16 else 2.0 ** -10
    H = H.double()
    dyh, dHh, dX, xhat, x2h = (r[k] for k in ("dyh", "dHh", "dX", "xhat", "x2h"))
    rows = lambda t: t.pow(2).sum(1)  # noqa: E731
    u = (M + 2 * Cc + 12) * U32
    one = torch.ones((M, 1), dtype=F64)
    out = {}
    for name, G, X in (("dW1", dHh, x2h), ("db1", dHh, one), ("dW2", dyh, H), ("db2", dyh, one), ("db3", dX, one)):
        out[name] = inv_count * (2.0 * e16 * float((rows(G) * rows(X)).sum().sqrt()) + u * float((G.abs().T @ X.abs()).norm()))
    out["dg3"] = inv_count * (2.0 * e16 * float((dX * xhat).norm()) + u * float((dX * xhat).abs().sum(0).norm()))
    return out
