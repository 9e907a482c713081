"""torch-tensor wrappers over the head-fit entry points of the C ABI (csrc/headfit.hip; tests only).  16-bit operands are raw bits in float16
tensors (tests/bits16.py); row pitches are the tensors' own strides, so guarded and poisoned views go through unchanged."""
import ctypes as C

import torch

from crossscore_amd import _lib


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sizes():
    """(rows per workgroup of head_grad_z, rows per partial of gemm_tn, columns of g) as the library reports them"""
    lib = _lib.load()
    return lib.cs_head_fit_row_tile(), lib.cs_head_fit_row_chunk(), lib.cs_head_fit_g_columns()


def workspace(nbytes, device="cuda"):
    return torch.empty((max(int(nbytes), 256),), dtype=torch.uint8, device=device)


def grad_z(A, Wb, bb, gt, B, gh, gw, P, act, powp, g, loss, colsum_part=None, s_tap=None, raw=False):
    """g (M, >= 224) and loss (fp64 scalar, +=) are the caller's; -> status code when raw, else checked"""
    lib = _lib.load()
    M, Cc = A.shape
    ws = workspace(lib.cs_head_backward_workspace_bytes(M, Cc, P), A.device)
    args = [_p(A), A.stride(0), _p(Wb), Wb.stride(0), _p(bb), _p(gt), B, gh, gw, P, Cc, act, powp, _p(g), g.stride(0), _p(loss), _p(colsum_part)]
    if s_tap is not None:
        rc = lib.cs_debug_op_head_grad_z_tap(*args, _p(s_tap), _p(ws), _st())
    else:
        rc = lib.cs_op_head_grad_z(*args, _p(ws), _st())
    if raw:
        return rc
    _lib.check(rc)
    torch.cuda.synchronize()  # (the workspace is this call's)


def gemm_tn(G, X, N, K, scale, accumulate, out, colsum=None):
    lib = _lib.load()
    M = G.shape[0]
    ws = workspace(lib.cs_gemm_tn_workspace_bytes(M, N, K), G.device)
    _lib.check(lib.cs_op_gemm_tn(_p(G), G.stride(0), _p(X), X.stride(0), M, N, K, scale, int(accumulate), _p(out), out.stride(0), _p(colsum),
                                 _p(ws), _st()))
    torch.cuda.synchronize()


def head_backward_args(X, A, Wb, bb, gt, B, gh, gw, P, act, powp, inv_count, accumulate, outs, ws):
    """the argument tuple of cs_op_head_backward (outs = dWa, dba, dWb, dbb, loss); the rejection tests edit single entries"""
    return [_p(X), X.stride(0), _p(A), A.stride(0), _p(Wb), Wb.stride(0), _p(bb), _p(gt), B, gh, gw, P, A.shape[1], act, powp, float(inv_count),
            int(accumulate)] + [_p(t) for t in outs] + [_p(ws), _st()]


def head_backward(X, A, Wb, bb, gt, B, gh, gw, P, act, powp, inv_count, accumulate=False, outs=None):
    lib = _lib.load()
    M, Cc = A.shape
    dev = A.device
    if outs is None:
        outs = (torch.full((Cc, Cc), 7.0, device=dev), torch.full((Cc,), 7.0, device=dev), torch.full((P * P, Cc), 7.0, device=dev),
                torch.full((P * P,), 7.0, device=dev), torch.full((), 7.0, dtype=torch.float64, device=dev))
    ws = workspace(lib.cs_head_backward_workspace_bytes(M, Cc, P), dev)
    _lib.check(lib.cs_op_head_backward(*head_backward_args(X, A, Wb, bb, gt, B, gh, gw, P, act, powp, inv_count, accumulate, outs, ws)))
    torch.cuda.synchronize()
    return outs


def adamw(p, m, v, g, step, lr, betas, eps, wd, p16=None):
    _lib.check(_lib.load().cs_op_adamw(_p(p), _p(m), _p(v), _p(g), p.numel(), lr, betas[0], betas[1], eps, wd, step, _p(p16), _st()))


def dz_bound(A, Wb, bb):
    """|dz| of z = A Wb^T + bb on this input: the fp32-sequential restatement of the product against fp64 (select_oracle.tolerance); A, Wb, bb
    fp64 CPU tensors holding the operands' values"""
    import select_oracle as so
    z = A @ Wb.T + bb
    seq = torch.zeros(z.shape, dtype=torch.float32)
    a32, w32 = A.float(), Wb.float()
    for k in range(A.shape[1]):
        seq = seq + a32[:, k:k + 1] * w32[:, k][None, :]
    seq = seq + bb.float()
    return so.tolerance(z.numpy(), seq.numpy())
