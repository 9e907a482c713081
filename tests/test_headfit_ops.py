"""The single-op entry points of the head fit (csrc/headfit.hip) against tests/headfit_oracle.py, in both operand types.
Every bound is assembled in the test from the number formats and the case's own input (never from what a kernel returns); outputs sit inside
tests/guard.py bands, strided inputs inside poisoned padding."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import headfit_helpers as hh  # noqa: E402
import headfit_oracle as ho  # noqa: E402
import select_oracle as so  # noqa: E402
from bits16 import MODES, bits16, r16, same_bits, spacing16, vals16  # noqa: E402
from guard import guarded, guarded_out, poisoned_in  # noqa: E402
from hip_helpers import switches  # noqa: E402
from crossscore_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

P, PP = 14, 196
F64 = torch.float64
U32 = 2.0 ** -24  # unit roundoff of fp32
CONFIGS = [(0, 1.0), (0, 2.0), (1, 1.0), (0, 4.0)]  # (act, p): the golden's three and p = 4


def _factor(m):
    """(gh, gw), gh < gw, gh the largest divisor of m below its square root (1 x m for a prime: still not square)"""
    gh = max(d for d in range(1, int(m ** 0.5) + 1) if m % d == 0 and d * d != m)
    return gh, m // gh


def _grids():
    """(B, gh, gw): M = 45 on a non-square grid, and one row tile of the kernel -1 / +1, the tile as the library reports it, non-square too"""
    tile = hh.sizes()[0]
    return [(3, 3, 5), (1,) + _factor(tile - 1), (1,) + _factor(tile + 1)]


def _head_case(B, gh, gw, Cc, act, p, bf16, seed):
    """hidden rows, second linear, bias (values the 16-bit type holds), the oracle's z / s and a gt at least 0.05 away from s everywhere"""
    g = torch.Generator().manual_seed(seed)
    M = B * gh * gw
    A = r16(torch.randn((M, Cc), generator=g, dtype=F64) * 0.7, bf16)
    A[::7, ::5] = 0.0
    Wb = r16(torch.randn((PP, Cc), generator=g, dtype=F64) * (1.5 / Cc ** 0.5), bf16)
    bb = (torch.randn((PP,), generator=g, dtype=F64) * 0.3).float().double()
    s, z = ho.scores(A, Wb, bb, act, p)
    off = (0.05 + 0.25 * torch.rand(s.shape, generator=g, dtype=F64)) * torch.where(torch.rand(s.shape, generator=g) < 0.5, -1.0, 1.0)
    gt_rows = (s + off).float()  # not clipped: a ground truth outside the activation's range is a legal input
    assert float((s - gt_rows.double()).abs().min()) >= 0.05  # a condition on the inputs: no sign is in doubt
    return A, Wb, bb, z, s, gt_rows


def _dz(A, Wb, bb, z):
    """|dz| of the case: the fp32-sequential restatement of z = A Wb^T + bb against fp64 (select_oracle.tolerance)"""
    prod = A.float()[:, None, :] * Wb.float()[None, :, :]
    seq = torch.zeros(prod.shape[:2], dtype=torch.float32)
    for k in range(prod.shape[2]):
        seq = seq + prod[:, :, k]
    seq = seq + bb.float()
    return so.tolerance(z.numpy(), seq.numpy())


@MODES
@pytest.mark.parametrize("act,p", CONFIGS)
@pytest.mark.parametrize("Cc", [64, 384])
@pytest.mark.parametrize("grid", [0, 1, 2])
def test_head_grad_z(grid, Cc, act, p, bf16):
    B, gh, gw = _grids()[grid]
    M = B * gh * gw
    A, Wb, bb, z, s, gt_rows = _head_case(B, gh, gw, Cc, act, p, bf16, seed=100 * grid + Cc + int(10 * p) + act)
    tile, _, NP = hh.sizes()
    dz = _dz(A, Wb, bb, z)
    g_ref, lsum_ref, _, _ = ho.grad_z(A, Wb, bb, gt_rows, act, p)
    _, _, d1, d2 = ho.activation(z, act, p)
    with switches(bf16=bf16):
        dev = "cuda"
        Ad = poisoned_in(bits16(A.float().to(dev), bf16), ld=Cc + 8)
        Wd = poisoned_in(bits16(Wb.float().to(dev), bf16), ld=Cc + 16)
        gt = ho.to_image(gt_rows, B, gh, gw, P).contiguous().to(dev)
        G = guarded((M, NP), torch.float16, ld=NP + 8, sentinel=0xFFFF)  # the canvas the padding columns must turn to zero on
        loss = torch.full((), 3.0, dtype=F64, device=dev)
        ntile = (M + tile - 1) // tile
        part, part_check = guarded_out((ntile, NP), torch.float32)
        tap, tap_check = guarded_out((M, PP), torch.float32)
        hh.grad_z(Ad, Wd, bb.float().to(dev), gt, B, gh, gw, P, act, p, G.view, loss, part, tap)
        G.check("g")
        part_check("column-sum partials")
        tap_check("s tap")
        got = vals16(G.view, bf16, F64).cpu()
        s_got = tap.double().cpu()
    # s: the product's fp32 accumulation through ds/dz, plus the fp32 evaluation of exp (|z| * 2^-24 in its exponent, |z| < 16 here) and pow: 2^-19
    assert float(z.abs().max()) < 16
    s_err = (s_got - s).abs()
    assert float((s_err - (d1.abs().max() * dz + 2.0 ** -19)).max()) <= 0, float(s_err.max())
    # g: one 16-bit ulp of the oracle's value + max |d2s/dz2| * |dz|
    err = (got[:, :PP] - g_ref).abs()
    bound = spacing16(g_ref, bf16) + float(d2.max()) * dz
    print(f"grad_z M {M} C {Cc} act {act} p {p} {'bf16' if bf16 else 'fp16'}: max err {float(err.max()):.3e}, least slack {float((bound - err).min()):.3e}, dz {dz:.2e}")
    assert float((err - bound).max()) <= 0
    assert int((G.view[:, PP:].view(torch.int16) != 0).sum()) == 0, "padding columns of g must be exactly zero"
    # loss: += of the fp64 sum of the fp32 terms |s - gt| over the kernel's own s; only the order of the fp64 additions differs
    want = 3.0 + float((s_got.float() - gt_rows).abs().double().sum())
    assert abs(float(loss) - want) <= M * PP * 2.0 ** -52 * want
    assert abs(float(loss) - 3.0 - float(lsum_ref)) <= float((d1.abs().max() * dz + 2.0 ** -19) * M * PP)
    # per-workgroup column sums of the rounded g: fp32 sums of at most `tile` values
    for t in range(ntile):
        rows = got[t * tile:(t + 1) * tile]
        assert float(((part[t].double().cpu() - rows.sum(0)).abs() - tile * U32 * rows.abs().sum(0)).max()) <= 0


@MODES
@pytest.mark.parametrize("act,p", [(0, 1.0), (0, 2.0), (1, 1.0)])
def test_head_grad_z_saturated(act, p, bf16):
    """z = +40 in the even columns, -40 in the odd ones (zero weights, the bias alone).  sigma = 1 or tanh = +-1 exactly in fp32, so ds/dz is
    exactly 0 there.  sigmoid(-40) = 4.2e-18 is NOT zero in fp32: its gradient p sigma^p rounds to zero in fp16 (smallest subnormal 6e-8) and is
    a representable 2^-58-sized number in bf16, where the definition (g rounded once to the operand type) keeps it."""
    B, gh, gw, Cc = 2, 3, 5, 64
    M = B * gh * gw
    NP = hh.sizes()[2]
    with switches(bf16=bf16):
        A = bits16(torch.randn((M, Cc), device="cuda"), bf16)
        Wb = torch.zeros((PP, Cc), dtype=torch.float16, device="cuda")
        bb = torch.where(torch.arange(PP, device="cuda") % 2 == 0, 40.0, -40.0).float()
        gt = torch.full((B, gh * P, gw * P), 0.5, device="cuda")
        g, check = guarded_out((M, NP), torch.float16, sentinel=0xFFFF)
        loss = torch.zeros((), dtype=F64, device="cuda")
        hh.grad_z(A, Wb, bb, gt, B, gh, gw, P, act, p, g, loss)
        check("g")
        got = vals16(g, bf16, F64)[:, :PP]
    assert int((got[:, 0::2] != 0).sum()) == 0, "z = +40 must give g = 0 exactly"
    if act == 1 or not bf16:
        assert int((got[:, 1::2] != 0).sum()) == 0, "z = -40 must give g = 0 exactly"
    else:
        want = -p * torch.sigmoid(torch.tensor(-40.0, dtype=F64)) ** p  # s < gt: the sign is -1
        assert float((got[:, 1::2] - want).abs().max()) <= float(spacing16(want, True))


@MODES
def test_head_grad_z_zero_at_own_score(bf16):
    """a pixel whose gt is the op's own s (read through the s tap) has zero gradient: sign(0) = 0"""
    B, gh, gw, Cc, act, p = 3, 3, 5, 64, 0, 2.0
    M = B * gh * gw
    A, Wb, bb, z, s, gt_rows = _head_case(B, gh, gw, Cc, act, p, bf16, seed=5)
    NP = hh.sizes()[2]
    m, n = 17, 101
    with switches(bf16=bf16):
        Ad, Wd, bd = bits16(A.float().cuda(), bf16), bits16(Wb.float().cuda(), bf16), bb.float().cuda()
        g = torch.zeros((M, NP), dtype=torch.float16, device="cuda")
        loss = torch.zeros((), dtype=F64, device="cuda")
        tap = torch.zeros((M, PP), device="cuda")
        hh.grad_z(Ad, Wd, bd, ho.to_image(gt_rows, B, gh, gw, P).contiguous().cuda(), B, gh, gw, P, act, p, g, loss, s_tap=tap)
        assert int(g[m, n].view(torch.int16)) & 0x7FFF != 0
        gt_rows = gt_rows.clone()
        gt_rows[m, n] = tap[m, n].cpu()
        g2 = torch.zeros_like(g)
        hh.grad_z(Ad, Wd, bd, ho.to_image(gt_rows, B, gh, gw, P).contiguous().cuda(), B, gh, gw, P, act, p, g2, loss)
        assert int(g2[m, n].view(torch.int16)) == 0
        g2[m, n] = g[m, n]
        same_bits(g2, g, "every other element")


def _tn_ms():
    chunk = hh.sizes()[1]
    return [1, chunk - 1, chunk, chunk + 1, 2 * chunk + 3]


@MODES
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("mi", range(5))
def test_gemm_tn(mi, accumulate, bf16):
    M = _tn_ms()[mi]
    scale = float(np.float32(1.37 * 2.0 ** -10))  # a number fp32 holds: the op takes its scale as a float
    gen = torch.Generator().manual_seed(7 + mi)
    for N in (196, 64, 384):
        for K in (64, 384):
            G = r16(torch.randn((M, N), generator=gen, dtype=F64), bf16)
            X = r16(torch.randn((M, K), generator=gen, dtype=F64), bf16)
            out0 = torch.randn((N, K), generator=gen).float()
            cs0 = torch.randn((N,), generator=gen).float()
            with switches(bf16=bf16):
                Gd = poisoned_in(bits16(G.float().cuda(), bf16), ld=(N + 15) // 8 * 8)
                Xd = poisoned_in(bits16(X.float().cuda(), bf16), ld=K + 8)
                out, check = guarded_out((N, K), torch.float32, ld=K + 3, init=out0.cuda())
                cs, cs_check = guarded_out((N,), torch.float32, init=cs0.cuda())
                hh.gemm_tn(Gd, Xd, N, K, scale, accumulate, out, cs)
                first = out.clone(), cs.clone()
                check("out")
                cs_check("colsum")
                out.copy_(out0.cuda())
                cs.copy_(cs0.cuda())
                hh.gemm_tn(Gd, Xd, N, K, scale, accumulate, out, cs)
                same_bits(out.contiguous(), first[0].contiguous(), "second run, products")
                same_bits(cs, first[1], "second run, column sums")
            # M * 2^-24 * (|G|^T |X|) * |scale|: the textbook bound of an fp32 accumulation of M exact products and the scaling; with accumulate
            # the stored sum out0 + scale * sum is rounded once more: 2^-24 of its magnitude
            want = scale * (G.T @ X) + (out0.double() if accumulate else 0)
            bound = M * U32 * (G.abs().T @ X.abs()) * scale + (U32 * want.abs() if accumulate else 0)
            err = (first[0].double().cpu() - want).abs()
            assert float((err - bound).max()) <= 0, (N, K, float(err.max()))
            want_c = scale * G.sum(0) + (cs0.double() if accumulate else 0)
            bound_c = M * U32 * G.abs().sum(0) * scale + (U32 * want_c.abs() if accumulate else 0)
            assert float(((first[1].double().cpu() - want_c).abs() - bound_c).max()) <= 0, (N, K)


@MODES
def test_gemm_tn_one_hot(bf16):
    """one-hot rows of G pick single rows of X exactly, across the chunk boundary; an asymmetric X shows a transposed output"""
    chunk = hh.sizes()[1]
    M, N, K = chunk + 90, 196, 64
    picks = {0: 5, chunk - 1: 195, chunk: 0, chunk + 89: 64}  # row m -> column n
    G = torch.zeros((M, N))
    for m, n in picks.items():
        G[m, n] = 1.0
    X = (torch.arange(M)[:, None] * 0.25 + torch.arange(K)[None, :] * 2.0)
    X = r16(X.double(), bf16).float()
    with switches(bf16=bf16):
        out, check = guarded_out((N, K), torch.float32)
        hh.gemm_tn(poisoned_in(bits16(G.cuda(), bf16), ld=N + 4), bits16(X.cuda(), bf16), N, K, 1.0, 0, out)
        check("out")
    want = torch.zeros((N, K))
    for m, n in picks.items():
        want[n] = X[m]
    same_bits(out.cpu(), want, "picked rows", by_value=True)


BWD_CASES = [(3, 3, 5, 64, 0, 1.0), (3, 3, 5, 384, 0, 2.0), (1, 5, 13, 64, 1, 1.0), (2, 3, 5, 64, 0, 4.0)]


def _bwd_case(B, gh, gw, Cc, act, p, bf16, seed):
    g = torch.Generator().manual_seed(seed)
    M = B * gh * gw
    X = r16(torch.randn((M, Cc), generator=g, dtype=F64), bf16)
    Wa = torch.randn((Cc, Cc), generator=g, dtype=F64) / Cc ** 0.5
    A = r16(ho.leaky(X @ Wa.T), bf16)
    A[::3, ::4] = 0.0  # exact zeros beside the negative values: the 0.01 side of the mask
    assert int((A < 0).sum()) > 0 and int((A == 0).sum()) > 0
    Wb = r16(torch.randn((PP, Cc), generator=g, dtype=F64) * (1.5 / Cc ** 0.5), bf16)
    bb = (torch.randn((PP,), generator=g, dtype=F64) * 0.3).float().double()
    s, _ = ho.scores(A, Wb, bb, act, p)
    off = (0.05 + 0.25 * torch.rand(s.shape, generator=g, dtype=F64)) * torch.where(torch.rand(s.shape, generator=g) < 0.5, -1.0, 1.0)
    return X, A, Wb, bb, (s + off).float()


def _dev16(t, bf16):
    return bits16(t.float().cuda(), bf16)


@MODES
@pytest.mark.parametrize("case", range(len(BWD_CASES)))
def test_head_backward(case, bf16):
    B, gh, gw, Cc, act, p = BWD_CASES[case]
    M = B * gh * gw
    X, A, Wb, bb, gt_rows = _bwd_case(B, gh, gw, Cc, act, p, bf16, seed=40 + case)
    inv = 1.0 / gt_rows.numel()
    ref = ho.backward(X, A, Wb, bb, gt_rows, act, p, inv, rnd=lambda t: r16(t, bf16))
    with switches(bf16=bf16):
        outs = [guarded_out(s, torch.float32) for s in ((Cc, Cc), (Cc,), (PP, Cc), (PP,))]
        loss = torch.full((), 7.0, dtype=F64, device="cuda")
        gt = ho.to_image(gt_rows, B, gh, gw, P).contiguous().cuda()
        hh.head_backward(_dev16(X, bf16), _dev16(A, bf16), _dev16(Wb, bf16), bb.float().cuda(), gt, B, gh, gw, P, act, p, inv,
                         outs=[o[0] for o in outs] + [loss])
        for (_, chk), name in zip(outs, ("dWa", "dba", "dWb", "dbb")):
            chk(name)
    # (u16 + M 2^-24) (|G|^T |.|) / n: u16 for the two 16-bit roundings the oracle shares with the kernels only up to their last bit, M 2^-24
    # for the fp32 accumulation over the rows
    f = ((2.0 ** -8 if bf16 else 2.0 ** -11) + M * U32) * inv
    g, dpre = ref["g"].abs(), ref["dpre"].abs()
    bounds = {"dWa": f * (dpre.T @ X.abs()), "dba": f * dpre.sum(0), "dWb": f * (g.T @ A.abs()), "dbb": f * g.sum(0)}
    for (o, _), name in zip(outs, ("dWa", "dba", "dWb", "dbb")):
        err = (o.double().cpu() - ref[name]).abs()
        rel = float(err.norm() / ref[name].norm())
        print(f"head_backward case {case} {'bf16' if bf16 else 'fp16'} {name}: rel Frobenius {rel:.3e}, worst err/bound {float((err / bounds[name].clamp_min(1e-300)).max()):.3f}")
        assert float((err - bounds[name]).max()) <= 0, name
    # the mean of fp32 terms |s - gt|: each carries the fp32 evaluation of s (2^-19, as in test_head_grad_z) and the product's fp32 accumulation
    # through ds/dz <= p / 4 <= 1 (a few 2^-20 at these widths): 2^-17 in all
    assert abs(float(loss) - float(ref["loss"])) <= 2.0 ** -17


@MODES
def test_head_backward_accumulate(bf16):
    """two halves of a batch with accumulate = the sum of the halves run alone, up to the one rounding of the stored sum"""
    B, gh, gw, Cc, act, p = 4, 3, 5, 64, 0, 2.0
    X, A, Wb, bb, gt_rows = _bwd_case(B, gh, gw, Cc, act, p, bf16, seed=77)
    inv = 1.0 / gt_rows.numel()
    h = B // 2 * gh * gw
    with switches(bf16=bf16):
        Xd, Ad, Wd, bd = _dev16(X, bf16), _dev16(A, bf16), _dev16(Wb, bf16), bb.float().cuda()
        gt = ho.to_image(gt_rows, B, gh, gw, P).contiguous().cuda()
        one = hh.head_backward(Xd[:h], Ad[:h], Wd, bd, gt[:B // 2], B // 2, gh, gw, P, act, p, inv)
        two = hh.head_backward(Xd[h:], Ad[h:], Wd, bd, gt[B // 2:], B // 2, gh, gw, P, act, p, inv)
        acc = hh.head_backward(Xd[:h], Ad[:h], Wd, bd, gt[:B // 2], B // 2, gh, gw, P, act, p, inv)
        acc = hh.head_backward(Xd[h:], Ad[h:], Wd, bd, gt[B // 2:], B // 2, gh, gw, P, act, p, inv, accumulate=True, outs=acc)
    for a, o, t in zip(acc, one, two):
        u = 2.0 ** -53 if a.dtype == F64 else U32
        want = o.double() + t.double()
        assert float(((a.double() - want).abs() - u * (want.abs() + t.double().abs())).max()) <= 0


def test_head_backward_rejections():
    """every rejection returns before any launch: the poisoned outputs keep their bits"""
    B, gh, gw, Cc, act, p = 1, 2, 3, 64, 0, 1.0
    X, A, Wb, bb, gt_rows = _bwd_case(B, gh, gw, Cc, act, p, False, seed=3)
    lib = _lib.load()
    Xd, Ad, Wd, bd = _dev16(X, False), _dev16(A, False), _dev16(Wb, False), bb.float().cuda()
    gt = ho.to_image(gt_rows, B, gh, gw, P).contiguous().cuda()
    outs = [torch.full(s, 7.0, device="cuda") for s in ((Cc, Cc), (Cc,), (PP, Cc), (PP,))] + [torch.full((), 7.0, dtype=F64, device="cuda")]
    ws = hh.workspace(lib.cs_head_backward_workspace_bytes(B * gh * gw, Cc, P))
    good = hh.head_backward_args(Xd, Ad, Wd, bd, gt, B, gh, gw, P, act, p, 1.0 / gt.numel(), 0, outs, ws)
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)  # noqa: E731
    edits = {"null X": (0, None), "null A": (2, None), "null Wb": (4, None), "null bias": (6, None), "null gt": (7, None), "null dWa": (17, None),
             "null loss": (21, None), "null workspace": (22, None), "misaligned X": (0, off(Xd, 2)), "misaligned A": (2, off(Ad, 8)),
             "misaligned dWb": (19, off(outs[2], 2)), "misaligned loss": (21, off(outs[4], 4)), "misaligned workspace": (22, off(ws, 16)),
             "odd row stride": (1, Cc + 4), "short row stride": (3, Cc - 8), "empty batch": (8, 0), "patch 16": (11, 16), "hidden 72": (12, 72),
             "act 2": (13, 2), "power 0": (14, 0.0), "inv_count 0": (15, 0.0)}
    tanh_p2 = list(good)
    tanh_p2[13], tanh_p2[14] = 1, 2.0  # tanh with a power: the reference forces p = 1 there
    assert lib.cs_op_head_backward(*tanh_p2) == _lib.CS_ERR_UNSUPPORTED
    for what, (i, v) in edits.items():
        args = list(good)
        args[i] = v
        assert lib.cs_op_head_backward(*args) != 0, what
        assert _lib.last_error(), what
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 7.0).all())
    assert lib.cs_head_fit_supported(384, 14) == 1 and lib.cs_head_fit_supported(64, 14) == 1 and lib.cs_head_fit_supported(768, 14) == 1
    assert lib.cs_head_fit_supported(1536, 14) == 1 and lib.cs_head_fit_supported(72, 14) == 0 and lib.cs_head_fit_supported(384, 16) == 0
    assert lib.cs_op_head_backward(*good) == 0
    torch.cuda.synchronize()


@MODES
@pytest.mark.parametrize("n", [1, 63, 64, 65, 75264])
@pytest.mark.parametrize("variant", ["plain", "no_decay", "zero_grad"])
def test_adamw(n, variant, bf16):
    """steps 1-3 against the fp64 oracle started from the kernel's own previous state.  Hyperparameters are the fp32 numbers the kernel receives,
    so 1 - beta is exact in both.  The bound counts the kernel's fp32 roundings at the unit roundoff u = 2^-24 each:
      m' = m + (g - m)(1 - b1)                       3 roundings:  u (|g - m| + |(g - m)(1 - b1)| + |m'|)
      v' = b2 v + ((1 - b2) g) g                     4 roundings:  u (|b2 v| + 2 (1 - b2) g^2 + |v'|)
      denom = sqrt(v') / sqrt(1 - b2^t) + eps        sqrt halves v's relative error; sqrt, the fp32 constant, the product, the sum: 4 u
      update = (lr / (1 - b1^t)) * (m' / denom)      the constant's rounding and division, the quotient, the product: 4 u
      p' = p (1 - lr wd) - update                    lr wd, 1 - x, the product: 3 u |p|; the difference: u |p'|"""
    gen = torch.Generator().manual_seed(n)
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    lr, b1, b2, eps, wd = f32(5e-4), f32(0.9), f32(0.999), f32(1e-8), f32(0.0 if variant == "no_decay" else 1e-2)
    p = torch.randn((n,), generator=gen).cuda()
    m = torch.zeros((n,), device="cuda")
    v = torch.zeros((n,), device="cuda")
    with switches(bf16=bf16):
        for step in (1, 2, 3):
            g = (torch.zeros((n,)) if variant == "zero_grad" else torch.randn((n,), generator=gen) * 10.0 ** float(torch.randint(-6, 1, (1,), generator=gen))).cuda()
            p0, m0, v0, gd = p.double(), m.double(), v.double(), g.double()
            P_, chk_p = guarded_out((n,), torch.float32, init=p)
            M_, chk_m = guarded_out((n,), torch.float32, init=m)
            V_, chk_v = guarded_out((n,), torch.float32, init=v)
            p16, chk_16 = guarded_out((n,), torch.float16)
            hh.adamw(P_, M_, V_, g, step, lr, (b1, b2), eps, wd, p16)
            for chk in (chk_p, chk_m, chk_v, chk_16):
                chk("adamw")
            pr, mr, vr = ho.adamw_step(p0, m0, v0, gd, step, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
            dm = U32 * ((gd - m0).abs() + ((gd - m0) * (1 - b1)).abs() + mr.abs())
            dv = U32 * ((b2 * v0).abs() + 2 * (1 - b2) * gd * gd + vr.abs())
            assert float(((M_.double() - mr).abs() - dm).max()) <= 0
            assert float(((V_.double() - vr).abs() - dv).max()) <= 0
            denom = (vr / (1 - b2 ** step)).sqrt() + eps
            rel_denom = 0.5 * dv / vr.clamp_min(1e-300) * (vr > 0) + 4 * U32
            size = lr / (1 - b1 ** step)
            upd = size * mr / denom
            dupd = size * dm / denom + upd.abs() * (rel_denom + 4 * U32)
            dp = 3 * U32 * p0.abs() + dupd + U32 * pr.abs()
            err = (P_.double() - pr).abs()
            assert float((err - dp).max()) <= 0, (step, float(err.max()))
            same_bits(p16, bits16(P_, bf16), "p16 = p rounded once")
            if variant == "zero_grad":
                assert bool((M_ == 0).all()) and bool((V_ == 0).all())
            p, m, v = P_.clone(), M_.clone(), V_.clone()
