"""Guard-band and tile-edge tests of every kernel entry point: each output lies inside guard bands of sentinel bits (tests/guard.py guarded_out)
that must come back untouched, each strided input is a view whose row padding and surroundings hold NaN / Inf / 65504 (poisoned_in), and the
values are compared with a high-precision reference of the same operation on the same rounded operands.  The shapes are the residues of each
kernel's own tiling (see the ids): rows and columns around tile edges, K around the GEMM's residual-prefetch threshold, persistent grids one
tile short of / at / one past a full round, query and key counts around the attention's 128-query blocks and 64-key tiles."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from crossscore_amd import _lib  # noqa: E402
from oracle import crossscore_oracle as orc  # noqa: E402
import guard  # noqa: E402
import hip_helpers as hh  # noqa: E402
import bits16 as b16  # noqa: E402
from guard import guarded_out, poisoned_in  # noqa: E402
from kernel_data import row_partials  # noqa: E402
from nets import make_net  # noqa: E402
from panel_data import make as panel_make  # noqa: E402
from panel_data import reference as panel_reference  # noqa: E402

DEV = "cuda"
F16, F32 = torch.float16, torch.float32
_same = functools.partial(b16.same_bits, by_value=True)  # 16-bit outputs by their bits, fp32 outputs by value (+0 equals -0)
_wall = b16.Worst("test_hip_bounds")


def setup_module(module):
    _wall.start()


def teardown_module(module):
    _wall.report()


def _ints(rows, cols, a, b, m, off):
    """small-integer operands: fp16 / bf16 hold them exactly, their products and fp32 sums are exact"""
    return ((torch.arange(rows, device=DEV)[:, None] * a + torch.arange(cols, device=DEV)[None, :] * b) % m - off).float()


# ================================================================================================ GEMM (both kernels)
def _gemm_case(M, N, K, epi, pad=0, inplace=False, bf16=False, g256=False, random=False):
    """one cs_op_gemm call with poisoned operands (rows K + pad apart), a guarded output (rows N + pad apart) and, for RESID_F32, a poisoned or
    in-place residual; integer operands: compared bit for bit; random ones: against the stated rounding bound"""
    rd, fl = b16.rd(bf16), b16.fl(bf16)
    if random:
        g = np.random.Generator(np.random.PCG64(M * 7 + N * 3 + K))
        A0 = rd(torch.from_numpy(g.standard_normal((M, K), dtype=np.float32)).to(DEV))
        W0 = rd(torch.from_numpy(g.standard_normal((N, K), dtype=np.float32) / math.sqrt(K)).to(DEV))
        b = torch.from_numpy(g.standard_normal((N,), dtype=np.float32)).to(DEV)
        r = torch.from_numpy(g.standard_normal((M, N), dtype=np.float32)).to(DEV)
    else:
        A0, W0 = rd(_ints(M, K, 5, 3, 7, 3)), rd(_ints(N, K, 3, 7, 5, 2))
        b = torch.arange(N, device=DEV) % 11 - 5.0
        r = _ints(M, N, 1, 2, 9, 4)
    A, W = poisoned_in(A0, ld=K + pad), poisoned_in(W0, ld=K + pad)
    y = fl(A0).double() @ fl(W0).double().t() + b.double()
    S = fl(A0).double().abs() @ fl(W0).double().abs().t()
    f32 = epi == _lib.EPI_RESID_F32
    resid = None
    with hh.switches(bf16=bf16, gemm256=g256):
        if f32:
            if inplace:
                out, chk = guarded_out((M, N), F32, ld=N + pad, init=r)
                resid = out
            else:
                resid = poisoned_in(r, ld=N + pad) if r is not None else None
                out, chk = guarded_out((M, N), F32, ld=N + pad)
            hh.gemm(A, W, b, epi, resid=resid, out=out)
        else:
            out, chk = guarded_out((M, N), F16, ld=N + pad)
            hh.gemm(A, W, b, epi, out=out)
        chk(f"gemm out epi {epi}")
    if f32:
        ref = y + r.double()
        if random:  # fp32 output: half an ulp + K 2^-24 sum|a w| of accumulation (+ the residual add)
            err = (out.double() - ref).abs()
            assert (err <= 2.0 ** -24 * ref.abs() + K * 2.0 ** -24 * (S + ref.abs()) + 1e-30).all(), float(err.max())
        else:
            _same(out, ref.float(), "resid")
        return
    o = fl(out).double()
    if epi == _lib.EPI_BIAS_GELU_F16:
        ref = orc.gelu_erf(y.float().cpu()).double().to(DEV)
        rel = 4.2e-3 if bf16 else 6e-4
        # + the GELU fit (<= 2.1e-4 on |y| <= 4.2, test_hip_ops); beyond it the fit clamps x to +-4.2 and keeps y * Phi_fit(-4.2) ~ 1.25e-4 |y|
        tail = torch.where(y.abs() > 4.2, 1.3e-4 * y.abs(), torch.zeros_like(y))
        assert ((o - ref).abs() <= rel * ref.abs() + 3e-4 + tail).all(), float((o - ref).abs().max())
        return
    if epi == _lib.EPI_BIAS_LEAKY_F16:
        ref = torch.where(y >= 0, y, 0.01 * y)
        rel = 4.2e-3 if bf16 else 6e-4
        assert ((o - ref).abs() <= rel * ref.abs() + 1e-4).all(), float((o - ref).abs().max())
        return
    ref = torch.relu(y) if epi == _lib.EPI_BIAS_RELU_F16 else y
    if random:  # half an ulp of the 16-bit output + K 2^-24 sum|a w|
        half = 2.0 ** -8 if bf16 else 2.0 ** -11
        err = (o - ref).abs()
        assert (err <= half * ref.abs() + 1.001 * K * 2.0 ** -24 * S + 2.0 ** -24).all(), float(err.max())
    else:
        _same(out, rd(ref.float()), f"epi {epi}")


_E = {"bias": _lib.EPI_BIAS_F16, "gelu": _lib.EPI_BIAS_GELU_F16, "relu": _lib.EPI_BIAS_RELU_F16, "leaky": _lib.EPI_BIAS_LEAKY_F16,
      "resid": _lib.EPI_RESID_F32}

# (M, N, K, epilogue, pad, in place): the 128-row kernel; 128- / 192-column tiles, BK = 32, residual prefetch (PIPE) at K / 32 >= 9 (K >= 320)
GEMM128 = [
    # rows: one row, a partial tile, one short of / at / one past a tile edge, many tiles; ragged N = 136 (128-column tiles)
    *[(M, 136, 64, "bias", 0, False) for M in (1, 17, 127, 128, 129, 1000)],
    # columns: ragged (136, 200), narrow 128-multiples (128, 256, 384), 192-multiples (576, 1152), > 1536 (1664: 128 tiles, 1728: 192 tiles)
    *[(129, N, 576, "resid", 0, False) for N in (136, 200, 128, 256, 384, 576, 1152, 1664, 1728)],
    # K below / at / above the residual-prefetch threshold (K = 256: 8 slices, the last without PIPE; K = 320: 10 slices, the first with it),
    # PIPE x ragged N, in place and with poisoned pitches
    *[(129, 200, K, "resid", 0, True) for K in (64, 256, 320, 512, 576, 1536)],
    (300, 136, 1536, "resid", 8, False), (17, 200, 576, "resid", 24, True), (1000, 1728, 576, "resid", 8, True),
    # tiles_m in {1, 7, 8, 9} with two or more column tiles
    *[(M, 256, 64, "bias", 0, False) for M in (100, 7 * 128 - 3, 8 * 128, 9 * 128 - 5)],
    # every 16-bit epilogue with row pitches above the minimum (lda / ldw / ldc)
    (129, 200, 128, "bias", 8, False), (129, 200, 128, "gelu", 16, False), (129, 136, 128, "relu", 8, False), (127, 1664, 64, "leaky", 8, False),
    (129, 576, 64, "gelu", 8, False),
]


@pytest.mark.parametrize("M,N,K,epi,pad,inplace", GEMM128, ids=[f"M{c[0]}-N{c[1]}-K{c[2]}-{c[3]}-pad{c[4]}{'-inplace' if c[5] else ''}" for c in GEMM128])
def test_gemm128_extents(M, N, K, epi, pad, inplace):
    _gemm_case(M, N, K, _E[epi], pad, inplace)


@pytest.mark.parametrize("case", ["bias-ragged", "resid-pipe-ragged", "resid-bf16", "bias-bf16"])
def test_gemm128_random_operands_within_the_rounding_bound(case):
    M, N, K, epi, bf16 = {"bias-ragged": (129, 200, 576, "bias", False), "resid-pipe-ragged": (257, 136, 1536, "resid", False),
                          "resid-bf16": (129, 200, 576, "resid", True), "bias-bf16": (17, 1664, 128, "bias", True)}[case]
    _gemm_case(M, N, K, _E[epi], 8, False, bf16=bf16, random=True)


@pytest.mark.parametrize("where", ["grid-1", "grid", "grid+1"])
def test_gemm128_persistent_grid_edges(where):
    """one 128-column tile per row panel: total tiles = grid - 1 / grid / grid + 1 of the persistent grid (2 blocks per CU, rounded to 8)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = (2 * cus // 8) * 8
    tiles = {"grid-1": grid - 1, "grid": grid, "grid+1": grid + 1}[where]
    M = tiles * 128 - 3 if where != "grid+1" else (tiles - 1) * 128 + 1
    assert (M + 127) // 128 == tiles
    _gemm_case(M, 128, 64, _lib.EPI_BIAS_F16, 8, False)


# the 256-tile kernel: M >= 256, N % 256 == 0 (<= 8192), K % 128 == 0, K >= 384; bias from memory when N > 3072
GEMM256 = [(M, 256, 384, "bias") for M in (256, 257, 511, 513)] + [(513, 3072, 512, "resid"), (257, 3328, 384, "bias"), (256, 8192, 512, "resid"),
                                                                   (511, 256, 512, "gelu")]
OUTSIDE256 = [(255, 256, 384, "resid"), (300, 256, 320, "resid"), (300, 1152, 384, "bias"), (257, 8448, 384, "bias")]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("M,N,K,epi", GEMM256 + OUTSIDE256,
                         ids=[f"M{c[0]}-N{c[1]}-K{c[2]}-{c[3]}" for c in GEMM256] + [f"outside-M{c[0]}-N{c[1]}-K{c[2]}-{c[3]}" for c in OUTSIDE256])
def test_gemm256_extents(M, N, K, epi, bf16):
    _gemm_case(M, N, K, _E[epi], 8, epi == "resid" and M % 2 == 1, bf16=bf16, g256=True)


@pytest.mark.parametrize("M,Cc,K,g256", [(1, 384, 256, False), (129, 128, 256, False), (127, 384, 576, False), (257, 768, 384, True),
                                         (513, 512, 512, True)], ids=lambda v: str(v))
def test_gemm_resid_layernorm_producer_extents(M, Cc, K, g256):
    """RESID_F32_LN: x += A W^T + b in place, plus the 16-bit copy of x and per-row partial sums (128-row kernel: 4 per column tile; 256-tile kernel:
    one per 64 columns), all three outputs guarded"""
    A0, W0 = _ints(M, K, 5, 3, 7, 3).half(), _ints(Cc, K, 3, 7, 5, 2).half()
    b = torch.arange(Cc, device=DEV) % 11 - 5.0
    r = _ints(M, Cc, 1, 2, 9, 4)
    sp = Cc // 64 if g256 else 4 * hh.column_tiles(Cc)
    x, cx = guarded_out((M, Cc), F32, ld=Cc, init=r)
    x16, c16 = guarded_out((M, Cc), F16)
    st, cst = guarded_out((M, sp, 2), F32)
    with hh.switches(bf16=False, gemm256=g256):
        hh.gemm(poisoned_in(A0, ld=K + 8), poisoned_in(W0, ld=K + 8), b, _lib.EPI_RESID_F32_LN, resid=x, out=x, out_f16=x16, stats_out=st)
    cx("x")
    c16("x16")
    cst("stats")
    ref = A0.double() @ W0.double().t() + b.double() + r.double()
    _same(x, ref.float(), "x")
    _same(x16, x.half(), "x16")
    want = row_partials(x, sp) if not g256 else torch.stack([x.view(M, sp, 64).sum(2), (x * x).view(M, sp, 64).sum(2)], dim=2)
    assert (st - want).abs().max() <= 2e-5 * float(want.abs().max()), float((st - want).abs().max())  # fp32 sums in another order


@pytest.mark.parametrize("M,Cc,N,epi,g256", [(1, 384, 1152, "ln", False), (129, 128, 136, "ln_gelu", False), (129, 384, 200, "ln", False),
                                             (257, 384, 1536, "ln_gelu", True), (511, 512, 256, "ln", True)], ids=lambda v: str(v))
def test_gemm_layernorm_consumer_extents(M, Cc, N, epi, g256):
    """LN(x) W^T + b as rstd * (16-bit(x) W'^T - mean * s) + c: 128-row kernel from partial sums (ln_sp = 4 / 8), 256-tile kernel from finalised
    rows (cs_op_ln_finalize, guarded past rows_padded); against the fp64 LayerNorm + projection at the tolerance of test_hip_ops"""
    g = np.random.Generator(np.random.PCG64(M + Cc + N))
    x = torch.from_numpy(2.0 * g.standard_normal((M, Cc), dtype=np.float32) + 0.7).to(DEV)
    gam = torch.from_numpy(1 + 0.2 * g.standard_normal((Cc,), dtype=np.float32)).to(DEV)
    bet = torch.from_numpy(0.1 * g.standard_normal((Cc,), dtype=np.float32)).to(DEV)
    Wf = torch.from_numpy(g.standard_normal((N, Cc), dtype=np.float32) / math.sqrt(Cc)).to(DEV)
    bb = torch.from_numpy(0.1 * g.standard_normal((N,), dtype=np.float32)).to(DEV)
    Wp = (Wf * gam[None, :]).half()
    s, c = Wp.float().sum(1), bb + Wf @ bet
    e = _lib.EPI_LN_F16 if epi == "ln" else _lib.EPI_LN_GELU_F16
    with hh.switches(bf16=False, gemm256=g256):
        if g256:
            part = torch.stack([x.view(M, Cc // 64, 64).sum(2), (x * x).view(M, Cc // 64, 64).sum(2)], dim=2)
            Mpad = (M + 255) // 256 * 256
            stat, cstat = guarded_out((Mpad, 1, 2), F32)
            hh.ln_finalize(part, Cc, stat=stat)
            cstat("ln_finalize stat")
            assert (stat[M:] == 0).all()
            ln = stat
        else:
            ln = row_partials(x, 4 * hh.column_tiles(Cc))
        out, chk = guarded_out((M, N), F16, ld=N + 8)
        hh.gemm(poisoned_in(x.half(), ld=Cc + 8), poisoned_in(Wp, ld=Cc + 8), c, e, out=out, ln_part=ln, col_s=s, ln_eps=1e-6)
        chk("LN consumer out")
    ref = torch.nn.functional.layer_norm(x.double(), (Cc,), gam.double(), bet.double(), 1e-6) @ Wf.double().t() + bb.double()
    if e == _lib.EPI_LN_GELU_F16:
        ref = orc.gelu_erf(ref.float().cpu()).double().to(DEV)
    err = (out.double() - ref).abs()
    assert err.max() < 3e-2 and err.mean() < 1.2e-3, (float(err.max()), float(err.mean()))


@pytest.mark.parametrize("I,gh,gw,pad", [(3, 5, 6, 0), (3, 43, 1, 8), (1, 1, 1, 0)], ids=lambda v: str(v))
def test_gemm_patch_epilogue_extents(I, gh, gw, pad):
    """PATCH_F32: patch row m -> token row img * (1 + Np) + 1 + p; the CLS rows and everything past the last token row stay untouched"""
    Np, Cc, K = gh * gw, 136, 128
    M = I * Np
    A0, W0 = _ints(M, K, 5, 3, 7, 3).half(), _ints(Cc, K, 3, 7, 5, 2).half()
    b = torch.arange(Cc, device=DEV) % 11 - 5.0
    pos = _ints(1 + Np, Cc, 2, 1, 13, 6)
    g = guard.guarded((I * (1 + Np), Cc), F32, ld=Cc + pad)
    with hh.switches(bf16=False, gemm256=False):
        hh.gemm(poisoned_in(A0, ld=K + pad), poisoned_in(W0, ld=K + pad), b, _lib.EPI_PATCH_F32, out=g.view, pos=pos, Np=Np, K=K)
    g.check("patch out")
    o3 = g.view.unflatten(0, (I, 1 + Np))
    ref = (A0.double() @ W0.double().t() + b.double()).reshape(I, Np, Cc) + pos[None, 1:].double()
    _same(o3[:, 1:], ref.float(), "patch rows")
    assert (o3[:, 0].contiguous().view(torch.int32) == g.sentinel).all()  # CLS rows untouched


@pytest.mark.parametrize("gh,gw,B", [(5, 6, 3), (3, 5, 9), (37, 37, 1), (1, 1, 1)], ids=lambda v: str(v))
def test_head_score_extents(gh, gw, B):
    """the head's jigsaw store, per-row partials, arrival counters and means: grids whose images straddle 128-row tiles, M < 128, B = 1"""
    P, Cc = 14, 128
    Np = gh * gw
    M = B * Np
    g = np.random.Generator(np.random.PCG64(gh * 100 + gw + B))
    A = poisoned_in(torch.from_numpy(g.standard_normal((M, Cc), dtype=np.float32)).to(DEV).half(), ld=Cc + 8)
    W = poisoned_in(torch.from_numpy(g.standard_normal((P * P, Cc), dtype=np.float32) / math.sqrt(Cc)).to(DEV).half(), ld=Cc + 8)
    b = torch.from_numpy(g.standard_normal((P * P,), dtype=np.float32)).to(DEV)
    score, cs = guarded_out((B, gh * P, gw * P), F32)
    part, cp = guarded_out((M, hh.head_sp(P)), F32)
    cnt, cc = guarded_out((B,), torch.int32, init=torch.zeros(B, dtype=torch.int32, device=DEV))
    mean, cm = guarded_out((B,), F32)
    with hh.switches(bf16=False, gemm256=False):
        hh.head_score(A, W, b, B, gh, gw, P, cnt=cnt, score=score, part=part, mean=mean)
    for chk, what in ((cs, "score"), (cp, "mean_part"), (cc, "counters"), (cm, "mean")):
        chk(what)
    y = torch.sigmoid(A.double() @ W.double().t() + b.double())
    ref = orc.jigsaw_to_image(y.float().cpu().view(B, Np, P, P), gh, gw).to(DEV)
    assert (score - ref).abs().max() < 1e-5
    assert int(cnt.abs().sum()) == 0
    assert float((mean.double() - score.double().mean(dim=(-1, -2))).abs().max()) < 2e-7 * max(1.0, math.sqrt(Np * P * P) / 64)


# ================================================================================================ attention
ATTN = [  # (dh, heads, B, Lq, Lk): every head dim, Lq around the 128-query block, Lk around the 64-key tile, batch * heads not a multiple of 8
    (64, 1, 3, 1, 1), (64, 3, 1, 63, 64), (48, 3, 1, 64, 63), (96, 1, 5, 65, 65), (16, 3, 3, 127, 129), (128, 1, 3, 128, 1),
    (192, 1, 1, 129, 63), (64, 5, 1, 129, 129), (48, 1, 3, 1, 129), (16, 1, 1, 65, 1),
]


def _attn_case(dh, heads, B, Lq, Lk, bf16):
    rd, fl = b16.rd(bf16), b16.fl(bf16)
    g = np.random.Generator(np.random.PCG64(dh * 1000 + Lq * 7 + Lk))
    Cc = heads * dh
    gap = 3  # rows of poison between batch items

    td = torch.bfloat16 if bf16 else F16

    def inp(L, sc, prescale=False):
        t = torch.from_numpy(sc * g.standard_normal((B, L, Cc), dtype=np.float32)).to(DEV)
        t = (t * (1.4426950408889634 / dh ** 0.5) if prescale else t).to(td)
        full = guard.poison_bits(td, B * (L + gap) * Cc, DEV).view(td).view(B, L + gap, Cc).clone()
        full[:, :L] = t
        return poisoned_in(full, ld=Cc + 8)[:, :L].view(F16), t.view(F16)

    Q, q0 = inp(Lq, 1.5, True)
    K, k0 = inp(Lk, 1.5)
    V, v0 = inp(Lk, 1.0)
    og = guard.guarded((B, Lq + gap, Cc), F16, ld=Cc + 16)
    O = og.view[:, :Lq]
    L, cl = guarded_out((B, heads, Lq), F32)
    Pw, cw = guarded_out((B, Lq, Lk), F32)
    with hh.switches(bf16=bf16, gemm256=True):
        hh.attention(Q, K, V, heads, dh, q_scale=1.0, O=O, L=L)
        hh.attention_weights(Q, K, heads, dh, L, heads - 1, q_scale=1.0, out=Pw)
    og.check("O")
    cl("lse")
    cw("weights")
    assert (og.view[:, Lq:].contiguous().view(torch.int16) == og.sentinel).all()  # the gap rows between O's batch items
    q = fl(q0).double().view(B, Lq, heads, dh).transpose(1, 2)
    k = fl(k0).double().view(B, Lk, heads, dh).transpose(1, 2)
    v = fl(v0).double().view(B, Lk, heads, dh).transpose(1, 2)
    s = (q @ k.transpose(-1, -2)) * math.log(2.0)
    p = torch.softmax(s, -1)
    ref = (p @ v).transpose(1, 2).reshape(B, Lq, Cc)
    err = (fl(O.contiguous()).double() - ref).abs()
    if bf16:
        assert err.max() < 3e-2 and err.mean() < 3e-3, (float(err.max()), float(err.mean()))
    else:
        assert err.max() < 4e-3 and err.mean() < 4e-4, (float(err.max()), float(err.mean()))
    assert (L.double() * math.log(2.0) - torch.logsumexp(s, -1)).abs().max() < (3e-3 if bf16 else 5e-4)
    assert (Pw.double() - p[:, heads - 1]).abs().max() < (2e-3 if bf16 else 1e-4)


@pytest.mark.parametrize("dh,heads,B,Lq,Lk", ATTN, ids=[f"dh{c[0]}-h{c[1]}-B{c[2]}-Lq{c[3]}-Lk{c[4]}" for c in ATTN])
def test_attention_extents(dh, heads, B, Lq, Lk):
    _attn_case(dh, heads, B, Lq, Lk, False)


@pytest.mark.parametrize("dh,heads,B,Lq,Lk", [(64, 3, 1, 129, 65), (48, 1, 3, 1, 63)], ids=lambda v: str(v))
def test_attention_extents_bf16(dh, heads, B, Lq, Lk):
    _attn_case(dh, heads, B, Lq, Lk, True)


# ================================================================================================ LayerNorm kernels
LN = [(4, 1, "both"), (252, 3, "f32"), (260, 4, "f16"), (1020, 5, "both"), (1024, 1, "f16"), (1028, 3, "both"), (1536, 4, "f32"),
      (2044, 5, "f16"), (2048, 3, "both"), (1536, 5, "bf16"), (1028, 1, "bf16")]


@pytest.mark.parametrize("Cc,M,mode", LN, ids=[f"C{c[0]}-M{c[1]}-{c[2]}" for c in LN])
def test_layernorm_extents(Cc, M, mode):
    """one wave per row, 4 rows per block, 4 (C <= 1024) or 8 (C <= 2048) float4 per lane: fp64 reference, fp32 only / 16-bit only / both"""
    g = np.random.Generator(np.random.PCG64(Cc + M))
    x = torch.from_numpy(3.0 * g.standard_normal((M, Cc), dtype=np.float32) + 1.0).to(DEV)
    gam = torch.from_numpy(1 + 0.2 * g.standard_normal((Cc,), dtype=np.float32)).to(DEV)
    bet = torch.from_numpy(0.1 * g.standard_normal((Cc,), dtype=np.float32)).to(DEV)
    bf16 = mode == "bf16"
    want32, want16 = mode in ("both", "f32", "bf16"), mode in ("both", "f16", "bf16")
    of, c32 = guarded_out((M, Cc), F32) if want32 else (None, None)
    ob, c16 = guarded_out((M, Cc), F16) if want16 else (None, None)
    with hh.switches(bf16=bf16, gemm256=True):
        hh.layernorm(x, gam, bet, 1e-6, want32, want16, of=of, ob=ob)
    ref = torch.nn.functional.layer_norm(x.double(), (Cc,), gam.double(), bet.double(), 1e-6)
    if want32:
        c32("out_f32")
        assert (of.double() - ref).abs().max() < 2e-5
    if want16:
        c16("out_f16")
        o16 = b16.fl(bf16)(ob).double()
        half = 2.0 ** -8 if bf16 else 2.0 ** -11
        assert ((o16 - ref).abs() <= half * ref.abs() + 2e-5).all()
        if want32:
            _same(ob, b16.rd(bf16)(of), "16-bit out = the fp32 out rounded once")


@pytest.mark.parametrize("M,with_resid,inplace", [(1, True, True), (63, False, False), (64, True, False), (65, True, True)], ids=lambda v: str(v))
def test_linear_layernorm_extents(M, with_resid, inplace):
    """csrc/rowln.hip, 64 rows per block at C = 384: both outputs guarded, the second stage's out2 guarded, and the in-place form (out2 = A)"""
    Cc = 384
    g = np.random.Generator(np.random.PCG64(M + 3))
    A0 = torch.from_numpy(g.standard_normal((M, Cc), dtype=np.float32)).to(DEV).half()
    W = torch.from_numpy(g.standard_normal((Cc, Cc), dtype=np.float32) / math.sqrt(Cc)).to(DEV).half()
    b = torch.from_numpy(g.standard_normal((Cc,), dtype=np.float32)).to(DEV)
    res = torch.from_numpy(2.0 * g.standard_normal((M, Cc), dtype=np.float32)).to(DEV) if with_resid else None
    gam = torch.from_numpy(1.0 + 0.3 * g.standard_normal((Cc,), dtype=np.float32)).to(DEV)
    bet = torch.from_numpy(0.2 * g.standard_normal((Cc,), dtype=np.float32)).to(DEV)
    W2 = torch.from_numpy(g.standard_normal((Cc, Cc), dtype=np.float32) / math.sqrt(Cc)).to(DEV).half()
    b2 = torch.from_numpy(0.5 * g.standard_normal((Cc,), dtype=np.float32)).to(DEV)
    of, cf = guarded_out((M, Cc), F32)
    oh, ch = guarded_out((M, Cc), F16)
    hh.linear_layernorm(A0, W, b, res, gam, bet, 1e-5, of=of, oh=oh)
    cf("out_f32")
    ch("out_f16")
    pre = A0.double() @ W.double().t() + b.double() + (res.double() if res is not None else 0.0)
    ref = torch.nn.functional.layer_norm(pre, (Cc,), gam.double(), bet.double(), 1e-5)
    assert (of.double() - ref).abs().max() < 2e-4
    e16 = (oh.double() - ref).abs()
    assert (e16 <= 6e-4 * ref.abs() + 2.5e-4).all(), float((e16 - 6e-4 * ref.abs()).max())
    if inplace:
        A, ca = guarded_out((M, Cc), F16, init=A0)
        _, _, o2 = hh.linear_layernorm_linear(A, W, b, res, gam, bet, 1e-5, W2, b2, 1, want_f32=False, want_f16=False, out2=A)
        ca("out2 = A")
    else:
        o2, c2 = guarded_out((M, Cc), F16)
        hh.linear_layernorm_linear(A0, W, b, res, gam, bet, 1e-5, W2, b2, 1, want_f32=False, want_f16=False, out2=o2)
        c2("out2")
    ref2 = torch.relu(oh.double() @ W2.double().t() + b2.double())
    assert ((o2.double() - ref2).abs() <= 6e-4 * ref2.abs() + 1e-4).all()


@pytest.mark.parametrize("impl", [0, 1], ids=["panel8", "panel4"])
@pytest.mark.parametrize("M", [1, 127, 128, 129])
def test_encoder_panel_extents(M, impl):
    """128 rows per workgroup: x (in place) and u guarded past row M; the packed weight image guarded with both byte sentinels"""
    lib = _lib.load()
    with hh.switches(panel_impl=impl):
        x, o, w = panel_make(M, 40 + M, torch.device(DEV))
        n = lib.cs_panel_image_bytes(1)
        imgs = []
        for s in (guard.SENTINEL[torch.uint8], guard.ALT_SENTINEL[torch.uint8]):
            img, ci = guarded_out((n,), torch.uint8, sentinel=s)
            hh.panel_pack(w["wo"], w["ls1"], w["w1"], w["g2"], w["w2"], w["ls2"], img=img)
            ci("panel image")
            imgs.append(img)
        _same(imgs[0], imgs[1], "panel image")
        xk, cx = guarded_out((M, 384), F32, init=x)
        u, cu = guarded_out((M, 384), F16)
        hh.encoder_panel(xk, o, imgs[0], w["bo"], w["b1"], w["b2"], u=u)
        cx("x")
        cu("u")
    ref_x, ref_u = panel_reference(x, o, w, True, emulate=True)
    assert (xk - ref_x).abs().max() < 4e-3
    assert (u.float() - ref_u).abs().max() < 6e-3


# ================================================================================================ the SwiGLU gate
@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("F,M,pad", [(8, 5, 8), (4096, 3, 0), (2048, 7, 16)], ids=["F8", "F4096", "F2048-swiglu-2l"])
def test_silu_mul(F, M, pad, bf16):
    """cs_op_silu_mul against fp64 silu(x1) * x2 rounded once, in place on rows ld >= 2 F apart: the second half of each row and the padding
    are unchanged; x1 far negative (the exp overflow side), +-0 and x2 = 0 included"""
    rd, fl = b16.rd(bf16), b16.fl(bf16)
    g = np.random.Generator(np.random.PCG64(F + M))
    x = torch.from_numpy(3.0 * g.standard_normal((M, 2 * F), dtype=np.float32)).to(DEV)
    x[0, :4] = torch.tensor([-100.0, -20000.0, 0.0, -0.0])
    x[0, 4:8] = torch.tensor([-90.0, 5.0, -3.0, 8.0])
    x[0, F + 5] = 0.0
    x[0, F + 6] = -0.0
    x0 = rd(x)
    gbuf = guard.guarded((M, 2 * F), F16, ld=2 * F + pad, init=x0)
    with hh.switches(bf16=bf16, gemm256=True):
        hh.silu_mul(gbuf.view)
    gbuf.check("silu_mul rows")  # the ld padding of every row and the guards
    out = gbuf.view
    _same(out[:, F:], x0[:, F:], "second half")
    x1, x2 = fl(x0[:, :F]).double(), fl(x0[:, F:]).double()
    ref = x1 / (1.0 + torch.exp(-x1)) * x2
    o = fl(out[:, :F].contiguous()).double()
    half = 2.0 ** -8 if bf16 else 2.0 ** -11
    err = (o - ref).abs()
    # one rounding of an fp32 evaluation (__expf and the division: a few fp32 ulps) + half an ulp of the 16-bit output
    assert (err <= (half + 2e-6) * ref.abs() + 2.0 ** -24).all(), float((err - half * ref.abs()).max())
    assert torch.isfinite(o).all()
    assert float(o[0, 0]) == 0.0 and float(o[0, 1]) == 0.0 and float(o[0, 2]) == 0.0


# ================================================================================================ patch embedding, im2col
def test_patch_embeddings_and_im2col_extents():
    """_patch_embed (im2col + GEMM), _fused and _fused_u8 write patch rows only: the CLS rows and everything past the last token row stay untouched;
    the u8 images' row padding holds 255 and the result is bit-identical to the unpadded call"""
    I, H, W, P, Cc = 3, 70, 84, 14, 384
    Np = (H // P) * (W // P)
    g = np.random.Generator(np.random.PCG64(5))
    x = torch.from_numpy(g.standard_normal((I, 3, H, W), dtype=np.float32)).to(DEV)
    wconv = torch.from_numpy(g.standard_normal((Cc, 3, P, P), dtype=np.float32) / math.sqrt(588)).to(DEV)
    b = torch.from_numpy(g.standard_normal((Cc,), dtype=np.float32)).to(DEV)
    pos = torch.from_numpy(g.standard_normal((1 + Np, Cc), dtype=np.float32)).to(DEV)
    ref = torch.nn.functional.conv2d(x.double(), wconv.double(), b.double(), stride=P).flatten(2).transpose(1, 2) + pos[None, 1:].double()
    outs = {}
    for name in ("two", "fused"):
        gg = guard.guarded((I * (1 + Np), Cc), F32)
        if name == "two":
            hh.patch_embed(x, wconv, b, pos, P, 1, out=gg.view)
        else:
            hh.patch_embed_fused(x, wconv, b, pos, P, out=gg.view)
        gg.check(name)
        o3 = gg.view.reshape(I, 1 + Np, Cc)
        assert (o3[:, 0].contiguous().view(torch.int32) == gg.sentinel).all()
        assert (o3[:, 1:].double() - ref).abs().mean() < 4e-4  # fp16 operands of N(0, 1) pixels: ~2e-4 expected
        outs[name] = o3
    assert (outs["two"][:, 1:] - outs["fused"][:, 1:]).abs().max() < 2e-5
    Kp = 640
    A, ca = guarded_out((I * Np, Kp), F16)
    hh.im2col(x, P, Kp, out=A)
    ca("im2col")
    xr = x.reshape(I, 3, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(I * Np, 588)
    _same(A[:, :588], xr.half(), "im2col")
    assert (A[:, 588:] == 0).all()
    # the one-pass form from uint8 rows with poisoned pitch padding, with and without a resize
    h, w = 80, 96
    imgs = torch.from_numpy(g.integers(0, 256, size=(I, h, w * 3), dtype=np.uint8)).to(DEV)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    for rs, crop in (((h, w), (3, 5, H, W, w)), ((75, 90), (2, 4, H, W, w))):
        plain = hh.patch_embed_fused_u8(imgs, rs, crop, mean, std, wconv, b, pos, P)
        gg = guard.guarded((I * (1 + Np), Cc), F32)
        hh.patch_embed_fused_u8(poisoned_in(imgs, ld=w * 3 + 13), rs, crop, mean, std, wconv, b, pos, P, out=gg.view)
        gg.check("patch_u8")
        o3, p3 = gg.view.reshape(I, 1 + Np, Cc), plain.reshape(I, 1 + Np, Cc)
        _same(o3[:, 1:], p3[:, 1:], "u8 patch rows, padded vs unpadded source rows")
        assert (o3[:, 0].contiguous().view(torch.int32) == gg.sentinel).all()


# ================================================================================================ input / output stages, tables, packing
@pytest.mark.parametrize("rs", [(40, 50), (30, 36)], ids=["noresize", "resize"])
def test_preprocess_u8_pitch(rs):
    h, w = 40, 50
    g = np.random.Generator(np.random.PCG64(rs[0]))
    img = torch.from_numpy(g.integers(0, 256, size=(h, w * 3), dtype=np.uint8)).to(DEV)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    crop, oh_ow = (1, 2), (rs[0] - 3, rs[1] - 5)
    plain = hh.preprocess_u8(img, w, rs, crop, oh_ow, mean, std)
    out, chk = guarded_out((3,) + oh_ow, F32)
    hh.preprocess_u8(poisoned_in(img, ld=w * 3 + 7), w, rs, crop, oh_ow, mean, std, out=out)
    chk("preprocess out")
    _same(out, plain, "padded vs unpadded source rows")
    if rs == (h, w):
        ref = (img.view(h, w, 3).permute(2, 0, 1).double() / 255.0 - torch.tensor(mean, device=DEV).double()[:, None, None]) / \
            torch.tensor(std, device=DEV).double()[:, None, None]
        assert (out.double() - ref[:, 1:1 + oh_ow[0], 2:2 + oh_ow[1]]).abs().max() < 1e-5


@pytest.mark.parametrize("mode", [_lib.METRIC_SSIM_M1_1, _lib.METRIC_MAE], ids=["ssim", "mae"])
@pytest.mark.parametrize("rs", [(30, 40), (24, 32)], ids=["noresize", "resize"])
def test_metric_map_u16_pitch_and_placeholders(rs, mode):
    B, h, w = 3, 30, 40
    g = np.random.Generator(np.random.PCG64(rs[0] + mode))
    maps = torch.from_numpy(g.integers(0, 65536, size=(B, h, w), dtype=np.uint16).view(np.int16)).to(DEV)
    crop, oh_ow = (1, 3), (rs[0] - 2, rs[1] - 4)
    plain = hh.metric_map_u16(maps, B, h, w, mode, rs, crop, oh_ow)
    out, chk = guarded_out((B,) + oh_ow, F32)
    hh.metric_map_u16(poisoned_in(maps, ld=w + 5), B, h, w, mode, rs, crop, oh_ow, out=out)
    chk("metric map out")
    _same(out, plain, "padded vs unpadded map rows")
    ph, cph = guarded_out((B,) + oh_ow, F32)
    hh.metric_map_u16(None, B, h, w, mode, rs, crop, oh_ow, out=ph)
    cph("placeholder maps")
    if mode == _lib.METRIC_MAE:
        assert torch.isnan(ph).all()
    else:
        assert (ph == 0).all()
    if rs == (h, w):
        m = maps.view(torch.int16).int() & 0xFFFF
        ref = m.double() / 32767 - 1 if mode == _lib.METRIC_SSIM_M1_1 else m.double() / 65535
        assert (out.double() - ref[:, 1:1 + oh_ow[0], 3:3 + oh_ow[1]]).abs().max() < 1e-6


@pytest.mark.parametrize("n", [1, 255, 257])
def test_elementwise_outputs_stay_inside(n):
    """score -> gray16 / rgb (integer outputs: both sentinels), the score-vs-GT sums, pack_f16 with ldo > K, the LayerNorm fold constants"""
    g = np.random.Generator(np.random.PCG64(n))
    score = torch.from_numpy(g.random((1, 1, n), dtype=np.float32)).to(DEV)
    for signed in (0, 1):
        outs = []
        for s in (guard.SENTINEL[torch.int16], guard.ALT_SENTINEL[torch.int16]):
            o, c = guarded_out((n,), torch.int16, sentinel=s)
            hh.score_to_gray16(score, signed, out=o)
            c("gray16")
            outs.append(o.clone())
        _same(outs[0], outs[1])
        v = score.double().view(-1)
        ref = torch.floor((v + 1) * 32767 if signed else v * 65535)
        assert ((outs[0].int() & 0xFFFF).double() - ref).abs().max() <= 1
    lut = torch.arange(768, device=DEV).view(256, 3).remainder(251).to(torch.uint8)
    outs = []
    for s in (guard.SENTINEL[torch.uint8], guard.ALT_SENTINEL[torch.uint8]):
        o, c = guarded_out((n, 3), torch.uint8, sentinel=s)
        hh.score_to_rgb(score, 0.0, 1.0, lut, out=o)
        c("rgb")
        outs.append(o.clone())
    _same(outs[0], outs[1])
    _same(outs[0], hh.score_to_rgb(score, 0.0, 1.0, lut), "rgb: guarded vs plain call")  # (values: test_predict_driver's writer goldens)
    B, H, W = 3, 1, n
    sc = torch.from_numpy(g.random((B, H, W), dtype=np.float32)).to(DEV)
    gt = torch.from_numpy(g.random((B, H, W), dtype=np.float32)).to(DEV)
    st, cst = guarded_out((B, 6), torch.float64)
    hh.score_gt_stats(sc, gt, out=st)
    cst("score_gt_stats")
    s64, g64 = sc.double().view(B, -1), gt.double().view(B, -1)
    ref = torch.stack([(s64 - g64).abs().sum(1), s64.sum(1), g64.sum(1), (s64 * s64).sum(1), (g64 * g64).sum(1), (s64 * g64).sum(1)], 1)
    assert (st - ref).abs().max() < 1e-9 * max(1, n)
    rows = 3
    wf = torch.from_numpy(g.standard_normal((rows, n), dtype=np.float32)).to(DEV)
    ldo = (n + 7) // 8 * 8 + 8
    pk, cpk = guarded_out((rows, ldo), F16)
    hh.pack_f16(wf, out=pk)
    cpk("pack_f16")
    _same(pk[:, :n], wf.half(), "packed")
    assert (pk[:, n:] == 0).all()
    s, cs_ = guarded_out((rows,), F32)
    c_, cc_ = guarded_out((rows,), F32)
    beta = torch.from_numpy(g.standard_normal((n,), dtype=np.float32)).to(DEV)
    bias = torch.from_numpy(g.standard_normal((rows,), dtype=np.float32)).to(DEV)
    hh.ln_fold_consts(pk[:, :n], wf, beta, bias, s=s, c=c_)
    cs_("ln_fold s")
    cc_("ln_fold c")
    assert (s.double() - pk[:, :n].double().sum(1)).abs().max() < 1e-4 * max(1, n / 64)
    assert (c_.double() - (bias.double() + wf.double() @ beta.double())).abs().max() < 1e-4 * max(1, n / 64)


@pytest.mark.parametrize("gh,gw", [(1, 1), (5, 51), (17, 15)], ids=lambda v: str(v))
def test_position_tables_extents(gh, gw):
    """pos_bicubic (both conventions) and the multi-view PE resize (both modes): guarded (1 + gh gw, C) / (gh gw, C) tables"""
    G, Cc = 5, 64
    g = np.random.Generator(np.random.PCG64(gh * gw))
    pos = torch.from_numpy(g.standard_normal((1 + G * G, Cc), dtype=np.float32)).to(DEV)
    for legacy in (None, True):
        out, chk = guarded_out((1 + gh * gw, Cc), F32)
        hh.pos_bicubic(pos, G, gh, gw, legacy=legacy, out=out)
        chk("pos_bicubic")
        if legacy is None:
            ref = torch.cat([pos[:1].cpu(), orc.bicubic_resize_grid(pos[1:].cpu().reshape(G, G, Cc), gh, gw).reshape(gh * gw, Cc)])
            assert (out.cpu() - ref).abs().max() < 3e-5
    pe = torch.from_numpy(g.standard_normal((40, 40, Cc), dtype=np.float32)).to(DEV)
    for mode in (0, 1):
        out, chk = guarded_out((gh * gw, Cc), F32)
        hh.pe_interp(pe, gh, gw, mode, out=out)
        chk("pe_interp")
        if mode:
            ref = orc.multiview_pe({"pos_enc_fn.PE": pe.cpu()[None]}, gh, gw, "bicubic")
        else:
            ref = orc.bilinear_resize_grid_align_corners(pe.cpu(), gh, gw)
        assert (out.cpu() - ref.reshape(gh * gw, Cc)).abs().max() < 3e-5


# ================================================================================================ forward-level extents and the all-placeholder batch


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize("back", ["synthetic/dinov2-tiny", "synthetic/dinov2-small-2l"], ids=["tiny", "vits-2l"])
def test_forward_outputs_stay_inside_their_buffers(back):
    """cs_forward, cs_encode_references, cs_forward_cached (and their _u8 forms at the ViT-S width): score, attention, mean and token outputs in
    guarded buffers; odd B and N, H and W not multiples of 14; the same bits as the unguarded call"""
    from crossscore_amd import synth
    from crossscore_amd.model import U8Batch, U8Image
    net = make_net(back, 3, device=DEV)[0]
    lib = _lib.load()
    B, N, H, W, P = 3, 3, 75, 90, 14
    h, w = H // P, W // P
    Cc = net.arch.hidden
    q, r = (torch.from_numpy(a).to(DEV) for a in synth.make_inputs(B, N, H, W, 5))
    handle = net._ensure_handle(torch.device("cuda", 0))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    shapes = {"score": (B, h * P, w * P), "attn": (B, h, w, N, h, w), "mean": (B,)}

    def outs(guarded):
        if not guarded:
            return {k: torch.empty(s, dtype=F32, device=DEV) for k, s in shapes.items()}, []
        gs = {k: guard.guarded(s, F32, guard_rows=64) for k, s in shapes.items()}
        return {k: g.view for k, g in gs.items()}, [g.check for g in gs.values()]

    def run(kind, guarded):
        o, checks = outs(guarded)
        if kind == "forward":
            _lib.check(lib.cs_forward(handle, _vp(q), _vp(r), B, N, H, W, _vp(o["score"]), _vp(o["attn"]), 1, _vp(o["mean"]), st))
        elif kind == "encode":
            if guarded:
                g = guard.guarded((B * N, h * w, Cc), F16, guard_rows=64)
                o, checks = {"tokens": g.view}, [g.check]
            else:
                o = {"tokens": torch.empty((B * N, h * w, Cc), dtype=F16, device=DEV)}
            _lib.check(lib.cs_encode_references(handle, _vp(r), B * N, H, W, _vp(o["tokens"]), st))
        else:
            tok = run("encode", False)["tokens"].view(B, N, h * w, Cc)
            _lib.check(lib.cs_forward_cached(handle, _vp(q), _vp(tok), B, N, H, W, _vp(o["score"]), _vp(o["attn"]), 1, _vp(o["mean"]), st))
        for c in checks:
            c(kind)
        torch.cuda.synchronize()
        return o

    for kind in ("forward", "encode", "cached"):
        a, b = run(kind, False), run(kind, True)
        for k in a:
            _same(b[k], a[k], f"{kind} {k}")
    if Cc % 384:
        return
    # the _u8 forms: decoded images of the window's size, rows padded
    g = np.random.Generator(np.random.PCG64(9))
    mk = lambda: U8Image(torch.from_numpy(g.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).to(DEV), H, W, (H, W))  # noqa: E731
    qb, rb = U8Batch([mk() for _ in range(B)], (H, W), device=DEV), U8Batch([mk() for _ in range(B * N)], (H, W), device=DEV)
    one = qb.images[0].c_struct()
    assert lib.cs_u8_input_supported(handle, C.byref(one), H, W) == 1
    res = {}
    for guarded in (False, True):
        o, checks = outs(guarded)
        _lib.check(lib.cs_forward_u8(handle, qb.c_array(0, B), rb.c_array(0, B * N), B, N, H, W, qb.mean, qb.std, _vp(o["score"]), _vp(o["attn"]), 1,
                                     _vp(o["mean"]), st))
        if guarded:
            gt = guard.guarded((B * N, h * w, Cc), F16, guard_rows=64)
            tok, checks = gt.view, checks + [gt.check]
        else:
            tok = torch.empty((B * N, h * w, Cc), dtype=F16, device=DEV)
        _lib.check(lib.cs_encode_references_u8(handle, rb.c_array(0, B * N), B * N, H, W, rb.mean, rb.std, _vp(tok), st))
        oc, cks = outs(guarded)
        _lib.check(lib.cs_forward_cached_u8(handle, qb.c_array(0, B), _vp(tok.contiguous()), B, N, H, W, qb.mean, qb.std, _vp(oc["score"]), _vp(oc["attn"]),
                                            1, _vp(oc["mean"]), st))
        for c in checks + cks:
            c("u8 forms")
        torch.cuda.synchronize()
        res[guarded] = (o, tok, oc)
    for (x, y) in zip(res[False], res[True]):
        if isinstance(x, dict):
            for k in x:
                _same(y[k], x[k], f"u8 {k}")
        else:
            _same(y, x, "u8 tokens")


def test_encode_references_u8_all_placeholders():
    """every image of the batch a placeholder (data NULL; U8Batch.device then comes from the stage): the same bits as cs_encode_references on
    images that hold zero_image_value; ReferenceTokenCache.gather with zero_reference gives the same tokens with from_u8 on and off"""
    from crossscore_amd.data import InputStage, ReferenceTokenCache
    net = make_net("synthetic/dinov2-small-2l", 3, device=DEV)[0]
    stage = InputStage(torch.device(DEV), resize_short_side=56)
    H, W, R = 56, 70, 3
    batch = stage.batch([stage.placeholder((H, W)) for _ in range(R)], (H, W))
    assert batch.device == torch.device(DEV)
    t_u8 = net.encode_references(batch)
    imgs = stage.zero_image_value[None, :, None, None].expand(R, 3, H, W).contiguous()
    t_f32 = net.encode_references(imgs)
    torch.cuda.synchronize()
    _same(t_u8, t_f32, "placeholder tokens")
    toks = {}
    for from_u8 in (True, False):
        cache = ReferenceTokenCache(net, stage, keep_images=False, from_u8=from_u8)
        toks[from_u8], _ = cache.gather([["a.png", "b.png"], ["c.png", "a.png"]], {}, (H, W), zero_reference=True)
    _same(toks[True], toks[False], "gather with zero_reference")


def test_predict_and_evaluate_with_zero_reference_on_the_one_pass_stage(tmp_path):
    """data.dataset.zero_reference=True, image writers off (fused_input_stage=auto takes the one-pass stage) and the reference-token cache on: every
    reference key is a placeholder.  predict and evaluate both complete and give the two-launch stage's outputs."""
    from PIL import Image
    from crossscore_amd import synth
    from crossscore_amd.config import load_config
    from crossscore_amd.predict import predict
    from nvs_tree import make_tree
    from scenes import make_scene, run_evaluate

    back = "synthetic/dinov2-small-2l"
    net = make_net(back, 6, device=DEV)[0]
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(net.arch, 6).items()}
    qd, rd = make_scene(str(tmp_path / "data"), n_query=3, n_ref=4, h=70, w=90)
    common = [f"data.dataset.query_dir={qd}", f"data.dataset.reference_dir={rd}", f"model.backbone.from_pretrained={back}",
              "this_main.resize_short_side=56", "data.neighbour_config.cross=3", "data.loader.validation.batch_size=2",
              "this_main.cache_reference_tokens=True", "data.dataset.zero_reference=True", "logger.predict.write.config.score_map_colour_mode=gray",
              "logger.predict.write.flag.image_query=False", "logger.predict.write.flag.image_reference=False"]
    outs = {}
    for mode in ("auto", False):
        np.random.seed(0)
        outs[mode] = predict(load_config("default_predict", common + [f"logger.predict.out_dir={tmp_path}/out_{mode}", f"this_main.fused_input_stage={mode}"]),
                             state_dict=sd, now="T")
    a, b = outs["auto"], outs[False]
    assert a["input_stage"].startswith("one-pass") and b["input_stage"].startswith("two-launch")
    assert [r[3] for r in a["rows"]] == [r[3] for r in b["rows"]]
    fa = sorted(f[len(a["out_dir"]):] for f in a["files"])
    assert fa == sorted(f[len(b["out_dir"]):] for f in b["files"])
    for rel in fa:
        if rel.endswith(".png"):
            assert np.array_equal(np.array(Image.open(a["out_dir"] + rel)), np.array(Image.open(b["out_dir"] + rel))), rel
    (tmp_path / "nvs").mkdir()
    tree = make_tree(tmp_path / "nvs")
    got = {}
    for fused in (True, False):
        res, cap, _, _ = run_evaluate(tree, tmp_path, f"z_{fused}", ["this_main.cache_reference_tokens=True", f"this_main.fused_input_stage={fused}",
                                                                     "data.dataset.zero_reference=True"], back=back)
        assert res["input_stage"].startswith("one-pass" if fused else "two-launch")
        got[fused] = (res["metrics"], [c["score"] for c in cap])
    assert got[True][0] == got[False][0]
    assert all(np.array_equal(x, y) for x, y in zip(got[True][1], got[False][1]))
