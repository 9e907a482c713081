"""The single-op entry points of the tail fit (csrc/tailfit.hip) against tests/tailfit_oracle.py, in both operand types.
Every bound is assembled in the test from the number formats and the case's own input (tailfit_helpers.ln_bounds / tail_fro_bounds), never from what
a kernel returns; outputs sit inside tests/guard.py bands, strided inputs inside poisoned padding."""
import ctypes as C
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import headfit_helpers as hh  # noqa: E402
import headfit_oracle as ho  # noqa: E402
import tailfit_helpers as th  # noqa: E402
import tailfit_oracle as to  # noqa: E402
from bits16 import MODES, bits16, r16, same_bits, spacing16, vals16  # noqa: E402
from guard import guarded_out, poisoned_in  # noqa: E402
from hip_helpers import switches  # noqa: E402
from crossscore_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

P, PP = 14, 196
F64 = torch.float64
U32 = 2.0 ** -24


def _ln_ms():
    t = th.ln_row_tile()
    return [1, t - 1, t, t + 1, 3 * t + 5]


def _ln_case(M, Cc, seed):
    """fp32 rows y (an offset and a spread per row), dX and gamma, as the fp64 tensors that hold their values"""
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn((M, Cc), generator=g) * (0.5 + torch.rand((M, 1), generator=g) * 3) + torch.randn((M, 1), generator=g)).float().double()
    dX = (torch.randn((M, Cc), generator=g) * 0.1).float().double()
    gamma = (1 + 0.3 * torch.randn((Cc,), generator=g)).float().double()
    return y, dX, gamma


def _run_ln(y, dX, gamma, inv, bf16, accumulate=0, init=None):
    """-> (dyh values fp64, dgamma, dbeta fp64, raw dyh) from guarded outputs and padded, poisoned inputs"""
    M, Cc = y.shape
    yd = poisoned_in(y.float().cuda(), ld=Cc + 4)
    dd = poisoned_in(dX.float().cuda(), ld=Cc + 8)
    dyh, chk = guarded_out((M, Cc), torch.float16, ld=Cc + 4)
    dg, chk_g = guarded_out((Cc,), torch.float32, init=init[0].cuda() if init else None)
    db, chk_b = guarded_out((Cc,), torch.float32, init=init[1].cuda() if init else None)
    th.ln_backward(yd, dd, gamma.float().cuda(), to.EPS, bf16, inv, accumulate, dyh, dg, db)
    chk("dyh")
    chk_g("dgamma")
    chk_b("dbeta")
    return vals16(dyh, bf16, F64).cpu(), dg.double().cpu(), db.double().cpu(), dyh.contiguous().clone()


@MODES
@pytest.mark.parametrize("Cc", [64, 128, 384, 768])
@pytest.mark.parametrize("mi", range(5))
def test_ln_backward(mi, Cc, bf16):
    M = _ln_ms()[mi]
    y, dX, gamma = _ln_case(M, Cc, seed=10 * mi + Cc)
    inv = float(torch.tensor(1.0 / (M * PP)).float())  # a number fp32 holds: the op takes inv_count as a float
    r = to.ln_backward(y, dX, gamma, inv)
    tol_dy, tol_g, tol_b = th.ln_bounds(y, dX, gamma, inv)
    got, dg, db, raw = _run_ln(y, dX, gamma, inv, bf16)
    # dyh: the fp32 evaluation (the restatement's tolerance) and one rounding step of the output type
    err = (got - r["dy"]).abs()
    bound = tol_dy + spacing16(r["dy"], bf16)
    eg, eb = float((dg - r["dgamma"]).abs().max()), float((db - r["dbeta"]).abs().max())
    print(f"ln_backward M {M} C {Cc} {'bf16' if bf16 else 'fp16'}: worst err/bound dyh {float((err / bound).max()):.3f}, dgamma {eg / tol_g:.3f}, dbeta {eb / tol_b:.3f}")
    assert float((err - bound).max()) <= 0
    assert eg <= tol_g and eb <= tol_b
    _, dg2, db2, raw2 = _run_ln(y, dX, gamma, inv, bf16)
    same_bits(raw2, raw, "second run, dyh")
    assert torch.equal(dg2, dg) and torch.equal(db2, db), "two identical calls give identical bits"


@MODES
def test_ln_backward_constant_row_and_zero_gamma(bf16):
    """row 4 is constant (2.5 in 64 columns: its fp32 mean is exact, so xhat is exactly 0 and rstd = 1 / sqrt(eps)); gamma[7] = 0 takes column 7
    of dX out of dyh bit for bit"""
    M, Cc = 9, 64
    y, dX, gamma = _ln_case(M, Cc, seed=3)
    y[4] = 2.5
    gamma[7] = 0.0
    inv = 0.25
    r = to.ln_backward(y, dX, gamma, inv)
    tol_dy, tol_g, tol_b = th.ln_bounds(y, dX, gamma, inv)
    got, dg, db, raw = _run_ln(y, dX, gamma, inv, bf16)
    assert bool(torch.isfinite(got).all())
    assert float(((got - r["dy"]).abs() - (tol_dy + spacing16(r["dy"], bf16))).max()) <= 0
    assert float((dg - r["dgamma"]).abs().max()) <= tol_g and float((db - r["dbeta"]).abs().max()) <= tol_b
    dX2 = dX.clone()
    dX2[:, 7] += 5.0
    _, dg2, db2, raw2 = _run_ln(y, dX2, gamma, inv, bf16)
    same_bits(raw2, raw, "dyh with another dX in the column of gamma = 0")
    assert not torch.equal(db2[7], db[7]) and torch.equal(db2[:7], db[:7]) and torch.equal(db2[8:], db[8:])


@MODES
def test_ln_backward_accumulate(bf16):
    """two halves of the rows with accumulate against one call: within the fp32 bounds of the three sums and the rounding of the stored sum (the
    partials' boundaries differ, so the bits may)"""
    t = th.ln_row_tile()
    M, Cc, inv = 2 * t + 6, 128, 0.125
    y, dX, gamma = _ln_case(M, Cc, seed=21)
    h = t + 3
    one = _run_ln(y, dX, gamma, inv, bf16)
    zero = (torch.zeros(Cc), torch.zeros(Cc))
    first = _run_ln(y[:h], dX[:h], gamma, inv, bf16, 1, zero)
    acc = _run_ln(y[h:], dX[h:], gamma, inv, bf16, 1, (first[1].float(), first[2].float()))
    same_bits(torch.cat([first[3], acc[3]]), one[3], "dyh is per row")
    tols = [th.ln_bounds(a, b, gamma, inv) for a, b in ((y, dX), (y[:h], dX[:h]), (y[h:], dX[h:]))]
    for k in (1, 2):
        bound = sum(tl[k] for tl in tols) + 2 * U32 * one[k].abs()
        assert float(((acc[k] - one[k]).abs() - bound).max()) <= 0


def test_ln_backward_rejections():
    M, Cc = 5, 64
    y, dX, gamma = _ln_case(M, Cc, seed=1)
    lib = _lib.load()
    yd, dd, gd = y.float().cuda(), dX.float().cuda(), gamma.float().cuda()
    outs = [torch.full((M, Cc), 7.0, dtype=torch.float16, device="cuda"), torch.full((Cc,), 7.0, device="cuda"), torch.full((Cc,), 7.0, device="cuda")]
    ws = hh.workspace(lib.cs_ln_backward_workspace_bytes(M, Cc))
    good = th.ln_backward_args(yd, dd, gd, to.EPS, 0, 0.5, 0, outs[0], outs[1], outs[2], ws)
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)  # noqa: E731
    edits = {"null y": (0, None), "null dX": (2, None), "null gamma": (4, None), "null dyh": (11, None), "null dgamma": (13, None), "null ws": (15, None),
             "short pitch": (1, Cc - 4), "odd pitch": (3, Cc + 2), "short dyh pitch": (12, Cc - 4), "misaligned y": (0, off(yd, 4)),
             "misaligned dyh": (11, off(outs[0], 2)), "misaligned ws": (15, off(ws, 16)), "C 96": (6, 96), "C 4096": (6, 4096), "M 0": (5, 0),
             "bf16 2": (8, 2), "inv_count 0": (9, 0.0), "eps -1": (7, -1.0)}
    for what, (i, v) in edits.items():
        args = list(good)
        args[i] = v
        assert lib.cs_op_ln_backward(*args) != 0, what
        assert _lib.last_error(), what
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 7.0).all())
    assert lib.cs_ln_backward_workspace_bytes(5, 96) == 0 and lib.cs_ln_backward_workspace_bytes(5, 1536) > 0
    assert lib.cs_op_ln_backward(*good) == 0
    torch.cuda.synchronize()


# ---- the whole backward ----
CONFIGS = [(0, 1.0), (0, 2.5), (1, 1.0)]


def _tail_case(B, gh, gw, Cc, act, p, bf16, seed):
    """x2 (fp32 values), the eight weights of the tail's forward as the handle holds them (matrices in the operand type, vectors fp32), the
    16-bit rows H, X, A the forward would store (exact zeros in H where the ReLU cut), and a gt at least 0.05 away from the score"""
    g = torch.Generator().manual_seed(seed)
    M = B * gh * gw
    rn = lambda *s: torch.randn(s, generator=g, dtype=F64)  # noqa: E731
    f32 = lambda t: t.float().double()  # noqa: E731
    x2 = f32(rn(M, Cc))
    W1, W2, Wa = (r16(rn(Cc, Cc) / Cc ** 0.5, bf16) for _ in range(3))
    b1, b2, ba = (f32(rn(Cc) * 0.1) for _ in range(3))
    g3, b3 = f32(1.0 + 0.2 * rn(Cc)), f32(0.1 * rn(Cc))
    Wb = r16(rn(PP, Cc) * (1.5 / Cc ** 0.5), bf16)
    bb = f32(rn(PP) * 0.3)
    H, _, X, A = to.tail_forward(x2, W1, b1, W2, b2, g3, b3, Wa, ba, rnd=lambda t: r16(t, bf16))
    assert int((H == 0).sum()) > 0 and int((H > 0).sum()) > 0
    s, _ = ho.scores(A, Wb, bb, act, p)
    off = (0.05 + 0.25 * torch.rand(s.shape, generator=g, dtype=F64)) * torch.where(torch.rand(s.shape, generator=g) < 0.5, -1.0, 1.0)
    return x2, H, X, A, W2, b2, g3, Wa, Wb, bb, (s + off).float()


def _dev16(t, bf16):
    return bits16(t.float().cuda(), bf16)


def _check_tail(B, gh, gw, Cc, act, p, bf16, seed, tag):
    M = B * gh * gw
    x2, H, X, A, W2, b2, g3, Wa, Wb, bb, gt_rows = _tail_case(B, gh, gw, Cc, act, p, bf16, seed)
    inv = 1.0 / gt_rows.numel()
    ref = to.backward(x2, H, X, A, W2, b2, g3, Wa, Wb, bb, gt_rows, act, p, inv, rnd=lambda t: r16(t, bf16))
    bounds = th.tail_fro_bounds(ref, H, M, Cc, inv, bf16)
    with switches(bf16=bf16):
        shapes = ((Cc, Cc), (Cc,), (Cc, Cc), (Cc,), (Cc,), (Cc,), (Cc, Cc), (Cc,), (PP, Cc), (PP,))
        outs = [guarded_out(s, torch.float32) for s in shapes]
        loss = torch.full((), 7.0, dtype=F64, device="cuda")
        gt = ho.to_image(gt_rows, B, gh, gw, P).contiguous().cuda()
        Hd, Xd, Ad = poisoned_in(_dev16(H, bf16), ld=Cc + 8), poisoned_in(_dev16(X, bf16), ld=Cc + 16), poisoned_in(_dev16(A, bf16), ld=Cc + 8)
        W2d, Wad, Wbd = poisoned_in(_dev16(W2, bf16), ld=Cc + 8), poisoned_in(_dev16(Wa, bf16), ld=Cc + 24), poisoned_in(_dev16(Wb, bf16), ld=Cc + 8)
        th.tail_backward(x2.float().cuda(), Hd, Xd, Ad, W2d, b2.float().cuda(), g3.float().cuda(), Wad, Wbd, bb.float().cuda(), gt, B, gh, gw, P,
                         act, p, inv, outs=[o[0] for o in outs] + [loss])
        for (_, chk), name in zip(outs, to.KEYS):
            chk(name)
        head = hh.head_backward(Xd, Ad, Wbd, bb.float().cuda(), gt, B, gh, gw, P, act, p, inv)
    for (o, _), h, name in zip(outs[6:], head[:4], to.KEYS[6:]):
        assert torch.equal(o.contiguous(), h), f"{name}: the head's gradients are cs_op_head_backward's bit for bit"
    assert float(loss) == float(head[4])
    for (o, _), name in zip(outs[:6], to.TAIL):
        err = float((o.double().cpu() - ref[name]).norm())
        print(f"tail_backward {tag} M {M} C {Cc} act {act} p {p} {'bf16' if bf16 else 'fp16'} {name}: rel Frobenius {err / float(ref[name].norm()):.3e}, "
              f"err/bound {err / bounds[name]:.4f}, bound/|ref| {bounds[name] / float(ref[name].norm()):.2e}")
        assert err <= bounds[name], name
        assert bounds[name] <= 0.02 * float(ref[name].norm()), name  # (the bound stays a small part of the gradient: a condition on the case)


@MODES
@pytest.mark.parametrize("act,p", CONFIGS)
@pytest.mark.parametrize("Cc", [128, 384])
@pytest.mark.parametrize("B,gh,gw", [(2, 3, 5), (1, 1, 1)])
def test_tail_backward(B, gh, gw, Cc, act, p, bf16):
    _check_tail(B, gh, gw, Cc, act, p, bf16, seed=B * 100 + Cc + int(10 * p) + act, tag="grid")


@MODES
def test_tail_backward_two_row_chunks(bf16):
    """M = one row chunk of gemm_tn + 1 (a prime times a prime would do; 1 x M keeps the grid non-square): every weight gradient reduces two chunks"""
    chunk = hh.sizes()[1]
    _check_tail(1, 1, chunk + 1, 128, 0, 1.0, bf16, seed=77, tag="chunks")


def test_tail_backward_rejections():
    """every rejection returns before any launch: the poisoned outputs keep their bits"""
    B, gh, gw, Cc, act, p = 1, 2, 3, 128, 0, 1.0
    x2, H, X, A, W2, b2, g3, Wa, Wb, bb, gt_rows = _tail_case(B, gh, gw, Cc, act, p, False, seed=3)
    lib = _lib.load()
    x2d, Hd, Xd, Ad, W2d, Wad, Wbd = x2.float().cuda(), _dev16(H, False), _dev16(X, False), _dev16(A, False), _dev16(W2, False), _dev16(Wa, False), _dev16(Wb, False)
    b2d, g3d, bbd = b2.float().cuda(), g3.float().cuda(), bb.float().cuda()
    gt = ho.to_image(gt_rows, B, gh, gw, P).contiguous().cuda()
    outs = th.fresh_outs(Cc)
    ws = hh.workspace(lib.cs_tail_backward_workspace_bytes(B * gh * gw, Cc, P))
    good = th.tail_backward_args(x2d, Hd, Xd, Ad, W2d, b2d, g3d, Wad, Wbd, bbd, gt, B, gh, gw, P, act, p, 1.0 / gt.numel(), 0, outs, ws)
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)  # noqa: E731
    edits = {"null x2": (0, None), "null H": (1, None), "null X": (3, None), "null A": (5, None), "null W2": (7, None), "null b2": (9, None),
             "null gamma": (10, None), "null Wa": (12, None), "null Wb": (14, None), "null bias": (16, None), "null gt": (17, None),
             "null dW1": (27, None), "null dg3": (31, None), "null dbb": (36, None), "null loss": (37, None), "null workspace": (38, None),
             "short H pitch": (2, Cc - 8), "odd X pitch": (4, Cc + 4), "odd W2 pitch": (8, Cc + 4), "short Wa pitch": (13, Cc - 8),
             "misaligned x2": (0, off(x2d, 4)), "misaligned H": (1, off(Hd, 8)), "misaligned dW2": (29, off(outs[2], 2)),
             "misaligned loss": (37, off(outs[10], 4)), "misaligned workspace": (38, off(ws, 16)), "empty batch": (18, 0), "patch 16": (21, 16),
             "hidden 96": (22, 96), "act 2": (23, 2), "power 0": (24, 0.0), "inv_count 0": (25, 0.0), "eps -1": (11, -1.0)}
    tanh_p2 = list(good)
    tanh_p2[23], tanh_p2[24] = 1, 2.0
    assert lib.cs_op_tail_backward(*tanh_p2) == _lib.CS_ERR_UNSUPPORTED
    for what, (i, v) in edits.items():
        args = list(good)
        args[i] = v
        assert lib.cs_op_tail_backward(*args) != 0, what
        assert _lib.last_error(), what
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 7.0).all())
    assert lib.cs_tail_backward_workspace_bytes(6, 96, 14) == 0 and lib.cs_tail_backward_workspace_bytes(6, 128, 16) == 0
    assert lib.cs_op_tail_backward(*good) == 0
    torch.cuda.synchronize()
