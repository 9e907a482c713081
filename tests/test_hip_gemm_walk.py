"""Walk tests of the two persistent GEMM kernels: every epilogue across tile hand-overs.

A block of csrc/gemm.hip or csrc/gemm256.hip walks more than one output tile only when the launch has more tiles than blocks, which on a whole
GPU needs more than 512 (256) tiles.  cs_debug_gemm_grid(8 / 16) shrinks the grid instead: with 8 blocks the one block of each XCD walks all of
the XCD's tiles, with 16 two blocks interleave and own different tile counts (one of them often a single tile: the bias then comes from LDS in
one block and from memory in its neighbour).  Everything between two tiles of a block runs at shapes of at most 2301 rows: the deferred epilogue
steps riding on the next tile's K slices (or outside any slice when the tile has fewer than 8), the counted vector-memory waits, the residual
prefetch and both arms of its flush, the LayerNorm stash, the head's cross-block mean finisher, blocks that own nothing and XCDs that own
different numbers of panels.

Operands come from tests/gemm_walk_data.py (aperiodic small integers: tests/test_gemm_walk_host.py shows on the CPU that a wrong panel, column
tile, K slice or epilogue step changes the expected output), are poisoned around their rows, outputs are guarded, the reference is fp64 on the
same rounded operands, and every output under the hook is bit-equal to the default grid's.

The ids name the hand-overs a case contains with 8 blocks: FF / FR / RF / RR = a full (F) or ragged (R) tile followed by a full or ragged one,
lastF / lastR = what a block's last tile is."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from crossscore_amd import _lib  # noqa: E402
from oracle import crossscore_oracle as orc  # noqa: E402
import bits16 as b16  # noqa: E402
import gemm_walk_data as wd  # noqa: E402
import hip_helpers as hh  # noqa: E402
from bits16 import to_dev  # noqa: E402
from guard import guarded, guarded_out, poisoned_in  # noqa: E402
from kernel_data import row_partials  # noqa: E402
from nets import make_net  # noqa: E402

DEV = "cuda"
F16, F32 = torch.float16, torch.float32
GRIDS = (0, 8, 16)  # 0: the default grid (one tile per block at these shapes)
_same = functools.partial(b16.same_bits, by_value=True)  # 16-bit outputs by their bits, fp32 outputs by value (+0 equals -0)
_wall = b16.Worst("test_hip_gemm_walk")


def setup_module(module):
    _wall.start()


def teardown_module(module):
    _wall.report()


def _per_grid(run, grids=GRIDS):
    """run() (fresh outputs each time) under each grid -> {blocks: tuple of outputs}"""
    outs = {}
    for blocks in grids:
        with hh.switches(grid=blocks):
            outs[blocks] = run()
    torch.cuda.synchronize()
    return outs


def _grid_invariant(outs, names):
    base = outs[GRIDS[0]]
    for blocks, o in outs.items():
        for a, b, name in zip(o, base, names):
            _same(a, b, f"{name}: {blocks} blocks against the default grid")


def _tag(M, N, BM, BN):
    seen, last = wd.orders(M, N, BM, BN, 8)
    ab = {"full": "F", "ragged": "R"}
    pairs = sorted(ab[s.split(">")[0]] + ab[s.split(">")[1]] for s in seen)
    return ".".join(pairs + sorted("last" + ab[s[5:]] for s in last))


def _exact_16bit(y, bf16):
    """the condition under which a 16-bit output is compared bit for bit: integers the type holds"""
    assert float(y.abs().max()) <= (256 if bf16 else 2048) and bool((y == y.round()).all())


# ================================================================================================ 128-row kernel: 16-bit epilogues
_E16 = {"bias": _lib.EPI_BIAS_F16, "relu": _lib.EPI_BIAS_RELU_F16, "leaky": _lib.EPI_BIAS_LEAKY_F16, "gelu": _lib.EPI_BIAS_GELU_F16}
# K = 64: 2 slices, six deferred steps run outside any slice; K = 256: exactly 8 slices; K = 320: 10 slices
HALF128 = wd.HALF128


def _half_case(M, N, K, epi, bf16=False):
    rd, fl = b16.rd(bf16), b16.fl(bf16)
    d = wd.operands(M, N, K)
    A0, W0, b = rd(to_dev(d["A"])), rd(to_dev(d["W"])), to_dev(d["b"])
    A, W = poisoned_in(A0, ld=K + 8), poisoned_in(W0, ld=K + 8)
    y = fl(A0).double() @ fl(W0).double().t() + b.double()
    _exact_16bit(y, bf16)

    def run():
        out, chk = guarded_out((M, N), F16, ld=N + 8)
        with hh.switches(bf16=bf16, gemm256=False):
            hh.gemm(A, W, b, _E16[epi], out=out)
        chk(f"{epi} out")
        return (out,)

    outs = _per_grid(run)
    for blocks, (out,) in outs.items():
        o = fl(out).double()
        rel = 4.2e-3 if bf16 else 6e-4
        if epi == "gelu":  # the bound of test_hip_bounds._gemm_case, tail term included
            ref = orc.gelu_erf(y.float().cpu()).double().to(DEV)
            tail = torch.where(y.abs() > 4.2, 1.3e-4 * y.abs(), torch.zeros_like(y))
            assert ((o - ref).abs() <= rel * ref.abs() + 3e-4 + tail).all(), (blocks, float((o - ref).abs().max()))
        elif epi == "leaky":
            ref = torch.where(y >= 0, y, 0.01 * y)
            assert ((o - ref).abs() <= rel * ref.abs() + 1e-4).all(), (blocks, float((o - ref).abs().max()))
            _same(out[y >= 0], rd(y.float())[y >= 0], f"leaky, y >= 0, {blocks} blocks")
        else:
            _same(out, rd((torch.relu(y) if epi == "relu" else y).float()), f"{epi}, {blocks} blocks")
    _grid_invariant(outs, ("out",))


@pytest.mark.parametrize("M,N,K,epi", HALF128, ids=[f"M{c[0]}-N{c[1]}-K{c[2]}-{c[3]}-{_tag(c[0], c[1], 128, wd.bn128(c[1]))}" for c in HALF128])
def test_gemm128_walk_16bit_epilogues(M, N, K, epi):
    _half_case(M, N, K, epi)


# ================================================================================================ 128-row kernel: RESID_F32
# K = 256: the last K without the residual prefetch (PIPE), 320: the first with it.  PIPE with a ragged last tile: N = 136 / M = 1147;
# with a full last tile: (2176, 384)
RESID128 = wd.RESID128


def _resid_case(M, N, K, mode, bf16=False, grids=GRIDS):
    rd, fl = b16.rd(bf16), b16.fl(bf16)
    d = wd.operands(M, N, K)
    A0, W0, b, r = rd(to_dev(d["A"])), rd(to_dev(d["W"])), to_dev(d["b"]), to_dev(d["r"])
    A, W = poisoned_in(A0, ld=K + 8), poisoned_in(W0, ld=K + 8)
    ref = fl(A0).double() @ fl(W0).double().t() + b.double() + (r.double() if mode != "none" else 0.0)
    assert float(ref.abs().max()) < 2 ** 24
    rsep = poisoned_in(r, ld=N + 24 if mode == "ldr" else N) if mode in ("sep", "ldr") else None

    def run():
        if mode == "inplace":
            out, chk = guarded_out((M, N), F32, ld=N + 8, init=r)
            resid = out
        else:
            out, chk = guarded_out((M, N), F32, ld=N + 8)
            resid = rsep
        with hh.switches(bf16=bf16, gemm256=False):
            hh.gemm(A, W, b, _lib.EPI_RESID_F32, resid=resid, out=out)
        chk("resid out")
        return (out,)

    outs = _per_grid(run, grids)
    for blocks, (out,) in outs.items():
        _same(out, ref.float(), f"resid {mode}, {blocks} blocks")
    _grid_invariant(outs, ("out",))


@pytest.mark.parametrize("M,N,K,mode", RESID128, ids=[f"M{c[0]}-N{c[1]}-K{c[2]}-{c[3]}-{_tag(c[0], c[1], 128, wd.bn128(c[1]))}" for c in RESID128])
def test_gemm128_walk_resid_f32(M, N, K, mode):
    _resid_case(M, N, K, mode)


def test_gemm128_walk_resid_f32_at_the_natural_grid():
    """no hook: grid + 9 tiles of one 128-column tile each at K = 320 (PIPE), in place, so nine blocks of the real launch walk two tiles"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = (2 * cus // 8) * 8
    M = (grid + 9) * 128 - 3
    _resid_case(M, 128, 320, "inplace", grids=(0,))


# ================================================================================================ 128-row kernel: RESID_F32_LN
# Cc = 136 passes the shape check (N % 4 == 0, stats_sp = 4 x 2 column tiles) and runs the per-row path of its 128-column tiles
RESID_LN128 = wd.RESID_LN128


def _resid_ln_case(M, Cc, K, bf16=False):
    rd, fl = b16.rd(bf16), b16.fl(bf16)
    d = wd.operands(M, Cc, K)
    A0, W0, b, r = rd(to_dev(d["A"])), rd(to_dev(d["W"])), to_dev(d["b"]), to_dev(d["r"])
    A, W = poisoned_in(A0, ld=K + 8), poisoned_in(W0, ld=K + 8)
    ref = fl(A0).double() @ fl(W0).double().t() + b.double() + r.double()
    sp = 4 * hh.column_tiles(Cc)

    def run():
        x, cx = guarded_out((M, Cc), F32, init=r)
        x16, c16 = guarded_out((M, Cc), F16)
        st, cst = guarded_out((M, sp, 2), F32)
        with hh.switches(bf16=bf16, gemm256=False):
            hh.gemm(A, W, b, _lib.EPI_RESID_F32_LN, resid=x, out=x, out_f16=x16, stats_out=st)
        for c, what in ((cx, "x"), (c16, "x16"), (cst, "stats")):
            c(what)
        return x, x16, st

    outs = _per_grid(run)
    for blocks, (x, x16, st) in outs.items():
        _same(x, ref.float(), f"x, {blocks} blocks")
        _same(x16, rd(x), f"x16, {blocks} blocks")
        want = row_partials(x, sp)
        assert (st - want).abs().max() <= 2e-5 * float(want.abs().max()), (blocks, float((st - want).abs().max()))  # fp32 sums in another order
    _grid_invariant(outs, ("x", "x16", "stats"))


@pytest.mark.parametrize("M,Cc,K", RESID_LN128, ids=[f"M{c[0]}-C{c[1]}-K{c[2]}-{_tag(c[0], c[1], 128, wd.bn128(c[1], 'wide'))}" for c in RESID_LN128])
def test_gemm128_walk_resid_layernorm_producer(M, Cc, K):
    _resid_ln_case(M, Cc, K)


# ================================================================================================ 128-row kernel: LayerNorm-folded consumers
LN128 = wd.LN128


@pytest.mark.parametrize("M,Cc,N,epi", LN128, ids=[f"M{c[0]}-C{c[1]}-N{c[2]}-{c[3]}-{_tag(c[0], c[2], 128, wd.bn128(c[2], 'wide'))}" for c in LN128])
def test_gemm128_walk_layernorm_consumers(M, Cc, N, epi):
    """out = rstd (x16 W'^T - mu s) + c with (mu, rstd) from the producer's partial sums (ln_sp = 4 / 8 / 16 at Cc = 128 / 384 / 768); the rows'
    statistics differ from panel to panel (offsets -12 .. 12) and from row to row (scales 1 .. 3), so the stash of another tile is a large error.

    Reference: the same formula in fp64 from the same x16, W', s, c and the same partial sums (mu = S1 / K, rstd = (S2 / K - mu^2 + eps)^-1/2).
    Bound, per element, of the kernel's fp32 evaluation against it:
      * the MFMA sum of K products, accumulated in fp32 in some order: |d acc| <= K 2^-24 sum_k |x w'| (first-order bound of any summation order;
        exact products), scaled by rstd;
      * mu is an fp32 quotient and mu s one fp32 product inside an fma: 2 roundings of 2^-24 relative to |mu s|, scaled by rstd: |mu s| rstd 2^-23.
        It is the cancellation term: |mu s| may be far above |acc - mu s|;
      * one rounding of the 16-bit output: half an ulp, 2^-11 |ref| in fp16 (+ 2^-25: half the smallest subnormal step, outputs near zero).
    LN_GELU applies GELU (slope within [-0.13, 1.13]) to that value: 1.13 x the bound above + the activation's own error as test_hip_bounds
    bounds it (3e-4 + the fit's tail beyond |y| = 4.2) + half an ulp of the result.
    The true LayerNorm (fp64, then the projection) stays at the tolerance of test_gemm_layernorm_consumer_extents."""
    K = Cc
    x = wd.ln_rows(M, Cc, 128)
    Wp_, s_, c_ = wd.ln_weights(N, Cc)
    part_ = wd.row_partials128(x, wd.bn128(Cc, "wide")).astype(np.float32)  # integers: exact
    assert part_.shape[1] == 4 * hh.column_tiles(Cc) == {128: 4, 384: 8, 768: 16}[Cc]
    x16, Wp, s, c, part = to_dev(x).half(), to_dev(Wp_).half(), to_dev(s_), to_dev(c_), to_dev(part_)
    assert torch.equal(x16.float(), to_dev(x)) and torch.equal(Wp.float(), to_dev(Wp_))
    A, W = poisoned_in(x16, ld=Cc + 8), poisoned_in(Wp, ld=Cc + 8)
    e = _lib.EPI_LN_F16 if epi == "ln" else _lib.EPI_LN_GELU_F16
    eps = 1e-6

    def run():
        out, chk = guarded_out((M, N), F16, ld=N + 8)
        with hh.switches(bf16=False, gemm256=False):
            hh.gemm(A, W, c, e, out=out, ln_part=part, col_s=s, ln_eps=eps)
        chk("LN consumer out")
        return (out,)

    outs = _per_grid(run)
    pd = part.double()
    mu = pd[:, :, 0].sum(1) / K
    rstd = 1.0 / torch.sqrt(torch.clamp(pd[:, :, 1].sum(1) / K - mu * mu, min=0.0) + eps)
    acc = x16.double() @ Wp.double().t()
    pre = rstd[:, None] * (acc - mu[:, None] * s.double()[None, :]) + c.double()[None, :]
    sabs = x16.double().abs() @ Wp.double().abs().t()
    bound = K * 2.0 ** -24 * rstd[:, None] * sabs + (mu[:, None] * s.double()[None, :]).abs() * rstd[:, None] * 2.0 ** -23
    if epi == "ln":
        ref, tol = pre, bound + 2.0 ** -11 * pre.abs() + 2.0 ** -25
    else:
        ref = orc.gelu_erf(pre.float().cpu()).double().to(DEV)
        tail = torch.where(pre.abs() > 4.2, 1.3e-4 * pre.abs(), torch.zeros_like(pre))
        tol = 1.13 * bound + 3e-4 + tail + 2.0 ** -11 * ref.abs() + 2.0 ** -25
    true = torch.nn.functional.layer_norm(to_dev(x).double(), (Cc,), None, None, eps) @ Wp.double().t() + c.double()
    if epi != "ln":
        true = orc.gelu_erf(true.float().cpu()).double().to(DEV)
    for blocks, (out,) in outs.items():
        err = (out.double() - ref).abs()
        print(f"LN consumer {blocks} blocks: max err / bound = {float((err / tol).max()):.3f}")
        assert (err <= tol).all(), (blocks, float((err - tol).max()))
        err = (out.double() - true).abs()
        assert err.max() < 3e-2 and err.mean() < 1.2e-3, (blocks, float(err.max()), float(err.mean()))
    _grid_invariant(outs, ("out",))


# ================================================================================================ 128-row kernel: PATCH_F32
def _patch_case(pc, with_stats, bf16=False):
    """19 images of 63 patches (M = 1197: 10 row panels, image boundaries inside tiles); N = 384 (192-column tiles), K = 640, and N = 136
    (128 + 8 columns: ragged tiles followed by full ones), K = 128"""
    rd, fl = b16.rd(bf16), b16.fl(bf16)
    I, Np, Cc, K = (pc[k] for k in ("I", "Np", "Cc", "K"))
    M, T = I * Np, 1 + Np
    d = wd.operands(M, Cc, K)
    A0, W0, b, pos = rd(to_dev(d["A"])), rd(to_dev(d["W"])), to_dev(d["b"]), to_dev(wd.pos_rows(Np, Cc))
    A, W = poisoned_in(A0, ld=K + 8), poisoned_in(W0, ld=K + 8)
    ref = (fl(A0).double() @ fl(W0).double().t() + b.double()).reshape(I, Np, Cc) + pos[None, 1:].double()
    sp = 4 * hh.column_tiles(Cc)

    def run():
        g = guarded((I * T, Cc), F32)
        g16 = guarded((I * T, Cc), F16) if with_stats else None
        gst = guarded((I * T, sp, 2), F32) if with_stats else None
        with hh.switches(bf16=bf16, gemm256=False):
            hh.gemm(A, W, b, _lib.EPI_PATCH_F32, out=g.view, pos=pos, Np=Np, K=K, out_f16=g16.view if with_stats else None,
                    stats_out=gst.view if with_stats else None)
        g.check("patch out")
        o3 = g.view.unflatten(0, (I, T))
        assert (o3[:, 0].contiguous().view(torch.int32) == g.sentinel).all()  # CLS rows untouched
        if not with_stats:
            return (o3[:, 1:].contiguous(),)
        g16.check("patch x16")
        gst.check("patch stats")
        h3, s3 = g16.view.unflatten(0, (I, T)), gst.view.unflatten(0, (I, T))
        assert (h3[:, 0].contiguous().view(torch.int16) == g16.sentinel).all() and (s3[:, 0].contiguous().view(torch.int32) == gst.sentinel).all()
        return o3[:, 1:].contiguous(), h3[:, 1:].contiguous(), s3[:, 1:].contiguous()

    outs = _per_grid(run)
    for blocks, o in outs.items():
        _same(o[0], ref.float(), f"patch rows, {blocks} blocks")
        if with_stats:
            _same(o[1], rd(o[0]), f"patch x16, {blocks} blocks")
            want = row_partials(o[0].reshape(M, Cc), sp)
            got = o[2].reshape(M, sp, 2)
            assert (got - want).abs().max() <= 2e-5 * float(want.abs().max()), (blocks, float((got - want).abs().max()))
    _grid_invariant(outs, ("out", "x16", "stats"))


@pytest.mark.parametrize("with_stats", [False, True], ids=["plain", "x16+stats"])
@pytest.mark.parametrize("pc", wd.PATCH128, ids=[f"N{pc['Cc']}-K{pc['K']}-{_tag(pc['I'] * pc['Np'], pc['Cc'], 128, wd.bn128(pc['Cc'], 'wide'))}"
                                                 for pc in wd.PATCH128])
def test_gemm128_walk_patch_epilogue(pc, with_stats):
    _patch_case(pc, with_stats)


def test_gemm128_walk_patch_embed_centred():
    """cs_op_patch_embed(centred=1) runs this kernel's PATCH epilogue with the per-patch means (pmean / wsum): 19 images of 7 x 9 patches"""
    I, H, W, P, Cc = 19, 98, 126, 14, 384
    Np = (H // P) * (W // P)
    g = np.random.Generator(np.random.PCG64(19))
    x = to_dev(g.standard_normal((I, 3, H, W), dtype=np.float32) + 0.5)
    wconv = to_dev(g.standard_normal((Cc, 3, P, P), dtype=np.float32) / math.sqrt(588))
    b = to_dev(g.standard_normal((Cc,), dtype=np.float32))
    pos = to_dev(g.standard_normal((1 + Np, Cc), dtype=np.float32))
    ref = torch.nn.functional.conv2d(x.double(), wconv.double(), b.double(), stride=P).flatten(2).transpose(1, 2) + pos[None, 1:].double()

    def run():
        gg = guarded((I * (1 + Np), Cc), F32)
        with hh.switches(bf16=False, gemm256=False):
            hh.patch_embed(x, wconv, b, pos, P, 1, out=gg.view)
        gg.check("patch_embed centred")
        o3 = gg.view.reshape(I, 1 + Np, Cc)
        assert (o3[:, 0].contiguous().view(torch.int32) == gg.sentinel).all()
        return (o3[:, 1:].contiguous(),)

    outs = _per_grid(run)
    for blocks, (o,) in outs.items():
        assert (o.double() - ref).abs().mean() < 4e-4, blocks  # the bound of test_patch_embeddings_and_im2col_extents
    _grid_invariant(outs, ("patch rows",))


# ================================================================================================ 128-row kernel: HEAD_SCORE
def _head_case(P, act, powp, bf16=False):
    """19 images of 7 x 9 patch rows (M = 1197: images straddle the 128-row tiles, 10 panels); P = 14: column tiles 128 + 68, P = 8: one of 64"""
    rd, fl = b16.rd(bf16), b16.fl(bf16)
    gh, gw, B, Cc = (wd.HEAD128[k] for k in ("gh", "gw", "B", "Cc"))
    Np = gh * gw
    M = B * Np
    g = np.random.Generator(np.random.PCG64(P * 10 + act))
    A0 = rd(to_dev(g.standard_normal((M, Cc), dtype=np.float32)))
    W0 = rd(to_dev(g.standard_normal((P * P, Cc), dtype=np.float32) / math.sqrt(Cc)))
    b = to_dev(g.standard_normal((P * P,), dtype=np.float32))
    A, W = poisoned_in(A0, ld=Cc + 8), poisoned_in(W0, ld=Cc + 8)
    y = fl(A0).double() @ fl(W0).double().t() + b.double()
    y = torch.sigmoid(y) if act == 0 else torch.tanh(y)
    if powp != 1.0:
        y = y ** powp
    ref = orc.jigsaw_to_image(y.cpu().view(B, Np, P, P), gh, gw).to(DEV)

    def run():
        score, cs = guarded_out((B, gh * P, gw * P), F32)
        part, cp = guarded_out((M, hh.head_sp(P)), F32)
        cnt, cc = guarded_out((B,), torch.int32, init=torch.zeros(B, dtype=torch.int32, device=DEV))
        mean, cm = guarded_out((B,), F32)
        mean2, cm2 = guarded_out((B,), F32)
        with hh.switches(bf16=bf16, gemm256=False):
            hh.head_score(A, W, b, B, gh, gw, P, act=act, powp=powp, cnt=cnt, score=score, part=part, mean=mean)
            for chk, what in ((cs, "score"), (cp, "mean_part"), (cc, "counters"), (cm, "mean")):
                chk(what)
            assert int(cnt.abs().sum()) == 0  # the finishers put the arrival counters back
            hh.head_score(A, W, b, B, gh, gw, P, act=act, powp=powp, cnt=cnt, score=score, part=part, mean=mean2)  # the same counters again
            for chk, what in ((cs, "score"), (cp, "mean_part"), (cc, "counters"), (cm2, "mean")):
                chk(what)
        assert int(cnt.abs().sum()) == 0
        _same(mean2, mean, "second launch on the same counters")
        return score, mean

    outs = _per_grid(run)
    for blocks, (score, mean) in outs.items():
        assert (score.double() - ref).abs().max() < 1e-5, blocks  # the tolerance of test_gemm_head_score_jigsaw
        err = float((mean.double() - score.double().mean(dim=(-1, -2))).abs().max())
        assert err < 2e-7 * max(1.0, math.sqrt(Np * P * P) / 64), (blocks, err)
    _grid_invariant(outs, ("score", "mean"))


@pytest.mark.parametrize("powp", [1.0, 2.0])
@pytest.mark.parametrize("act", [0, 1], ids=["sigmoid", "tanh"])
@pytest.mark.parametrize("P", [14, 8])
def test_gemm128_walk_head_score(P, act, powp):
    _head_case(P, act, powp)


# ================================================================================================ 128-row kernel: bf16 operands
@pytest.mark.parametrize("what", ["bias", "relu", "resid", "resid-pipe", "resid-ln", "patch", "head"])
def test_gemm128_walk_bf16_operands(what):
    if what in ("bias", "relu"):
        _half_case(*wd.BF16_128[what], what, bf16=True)
    elif what == "resid":
        _resid_case(*wd.BF16_128[what], "inplace", bf16=True)
    elif what == "resid-pipe":
        _resid_case(*wd.BF16_128[what], "sep", bf16=True)
    elif what == "resid-ln":
        # the 128-row kernel builds RESID_F32_LN for fp16 operands only and says so (the bf16 producer is gemm256.hip's: test_gemm256_walk)
        with pytest.raises(ValueError, match="built for fp16 operands only"):
            _resid_ln_case(*wd.BF16_128[what], bf16=True)
    elif what == "patch":
        _patch_case(wd.PATCH128[0], True, bf16=True)
    else:
        _head_case(14, 0, 1.0, bf16=True)


# ================================================================================================ the 256-tile kernel
# M = 768: 3 panels (five XCDs idle); M = 2301 = 9 * 256 - 3: XCD 0 walks a full panel, then a ragged one.  N = 3328 > 3072: bias from memory.
# K = 384: six K tiles, the prologue meets the seam
G256 = wd.G256


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("M,N,K,epi", G256, ids=[f"M{c[0]}-N{c[1]}-K{c[2]}-{c[3]}-{_tag(c[0], c[1], 256, 256)}" for c in G256])
def test_gemm256_walk(M, N, K, epi, bf16):
    """bias / GELU / RESID_F32 (in place, separate) / RESID_F32_LN + cs_op_ln_finalize under 8 and 16 blocks: exact (GELU: the bound of
    test_hip_bounds), bit-equal to the default grid and, for the bias and residual epilogues, to the 128-row kernel"""
    rd, fl = b16.rd(bf16), b16.fl(bf16)
    d = wd.operands(M, N, K)
    A0, W0, b, r = rd(to_dev(d["A"])), rd(to_dev(d["W"])), to_dev(d["b"]), to_dev(d["r"])
    A, W = poisoned_in(A0, ld=K + 8), poisoned_in(W0, ld=K + 8)
    y = fl(A0).double() @ fl(W0).double().t() + b.double()
    rsep = poisoned_in(r, ld=N + 8)
    sp = N // 64

    def run(g256=True):
        with hh.switches(bf16=bf16, gemm256=g256):
            if epi in ("bias", "gelu"):
                out, chk = guarded_out((M, N), F16, ld=N + 8)
                hh.gemm(A, W, b, _lib.EPI_BIAS_F16 if epi == "bias" else _lib.EPI_BIAS_GELU_F16, out=out)
                chk(epi)
                return (out,)
            if epi.startswith("resid-") and epi != "resid-ln":
                inplace = epi == "resid-inplace"
                out, chk = guarded_out((M, N), F32, ld=N + 8, init=r if inplace else None)
                hh.gemm(A, W, b, _lib.EPI_RESID_F32, resid=out if inplace else rsep, out=out)
                chk(epi)
                return (out,)
            x, cx = guarded_out((M, N), F32, init=r)
            x16, c16 = guarded_out((M, N), F16)
            st, cst = guarded_out((M, sp, 2), F32)
            hh.gemm(A, W, b, _lib.EPI_RESID_F32_LN, resid=x, out=x, out_f16=x16, stats_out=st)
            stat, cstat = guarded_out(((M + 255) // 256 * 256, 1, 2), F32)
            hh.ln_finalize(st, N, stat=stat)
            for c, what in ((cx, "x"), (c16, "x16"), (cst, "stats"), (cstat, "ln_finalize stat")):
                c(what)
            return x, x16, st, stat

    outs = _per_grid(run)
    for blocks, o in outs.items():
        if epi == "bias":
            _exact_16bit(y, bf16)
            _same(o[0], rd(y.float()), f"bias, {blocks} blocks")
        elif epi == "gelu":
            ref = orc.gelu_erf(y.float().cpu()).double().to(DEV)
            tail = torch.where(y.abs() > 4.2, 1.3e-4 * y.abs(), torch.zeros_like(y))
            err = (fl(o[0]).double() - ref).abs()
            assert (err <= (4.2e-3 if bf16 else 6e-4) * ref.abs() + 3e-4 + tail).all(), (blocks, float(err.max()))
        else:
            _same(o[0], (y + r.double()).float(), f"{epi}, {blocks} blocks")
        if epi == "resid-ln":
            x, x16, st, stat = o
            _same(x16, rd(x), f"x16, {blocks} blocks")
            want = torch.stack([x.view(M, sp, 64).sum(2), (x * x).view(M, sp, 64).sum(2)], dim=2)
            assert (st - want).abs().max() <= 2e-5 * float(want.abs().max()), blocks
            mu, var = x.double().mean(1), x.double().var(1, unbiased=False)
            assert (stat[:M, 0, 0].double() - mu).abs().max() < 1e-4
            assert ((stat[:M, 0, 1].double() * torch.sqrt(var + 1e-6)) - 1).abs().max() < 2e-4
            assert (stat[M:] == 0).all()
    _grid_invariant(outs, ("out", "x16", "stats", "stat"))
    if epi in ("bias", "resid-inplace", "resid-sep"):
        small = run(g256=False)
        torch.cuda.synchronize()
        _same(small[0], outs[8][0], "the 128-row kernel against the 256-tile kernel")


LN256 = wd.LN256


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("M,Cc,N,epi", LN256, ids=[f"M{c[0]}-C{c[1]}-N{c[2]}-{c[3]}-{_tag(c[0], c[2], 256, 256)}" for c in LN256])
def test_gemm256_walk_layernorm_consumers(M, Cc, N, epi, bf16):
    """the two LayerNorm-folded consumers of the 256-tile kernel from finalised rows (cs_op_ln_finalize), checked as
    test_gemm256_layernorm_folded_chain checks them, on rows whose statistics differ from row panel to row panel and from row to row"""
    rd, fl = b16.rd(bf16), b16.fl(bf16)
    x = to_dev(wd.ln_rows(M, Cc, 256))
    Wp_, s_, c_ = wd.ln_weights(N, Cc)
    x16, Wp, s, c = rd(x), rd(to_dev(Wp_)), to_dev(s_), to_dev(c_)
    assert torch.equal(fl(x16), x) and torch.equal(fl(Wp), to_dev(Wp_))
    part = torch.stack([x.view(M, Cc // 64, 64).sum(2), (x * x).view(M, Cc // 64, 64).sum(2)], dim=2)
    A, W = poisoned_in(x16, ld=Cc + 8), poisoned_in(Wp, ld=Cc + 8)
    e = _lib.EPI_LN_F16 if epi == "ln" else _lib.EPI_LN_GELU_F16

    def run():
        with hh.switches(bf16=bf16, gemm256=True):
            stat, cstat = guarded_out(((M + 255) // 256 * 256, 1, 2), F32)
            hh.ln_finalize(part, Cc, stat=stat)
            out, chk = guarded_out((M, N), F16, ld=N + 8)
            hh.gemm(A, W, c, e, out=out, ln_part=stat, col_s=s, ln_eps=1e-6)
            cstat("ln_finalize stat")
            chk("LN consumer out")
        return out, stat

    outs = _per_grid(run)
    true = torch.nn.functional.layer_norm(x.double(), (Cc,), None, None, 1e-6) @ fl(Wp).double().t() + c.double()
    for blocks, (out, stat) in outs.items():
        xn = (fl(x16) - stat[:M, 0, 0:1]) * stat[:M, 0, 1:2]
        same = xn @ fl(Wp).t() + c
        tr = true
        if epi != "ln":
            same, tr = orc.gelu_erf(same.cpu()).to(DEV), orc.gelu_erf(true.float().cpu()).double().to(DEV)
        o = fl(out)
        rel = 4.2e-3 if bf16 else 6e-4
        err = (o - same).abs()
        assert (err <= rel * same.abs() + (4e-3 if bf16 else 1.5e-3)).all(), (blocks, float((err - rel * same.abs()).max()))
        err = (o.double() - tr).abs()
        assert err.mean() < (8e-3 if bf16 else 1.2e-3) and err.max() < (0.2 if bf16 else 3e-2), (blocks, float(err.mean()), float(err.max()))
    _grid_invariant(outs, ("out", "stat"))


# ================================================================================================ one whole forward
@pytest.mark.parametrize("back", ["synthetic/dinov2-tiny", "synthetic/dinov2-small-2l"], ids=["tiny", "vits-2l"])
def test_forward_is_bit_equal_under_the_grid_hook(back):
    """every production epilogue combination through a walk in context: 20 images of 63 patches (10 row panels of 128) with 8 blocks per GEMM
    launch against the default grid, on the same handle (launches are issued live and read the hook each time)"""
    from crossscore_amd import synth

    net = make_net(back, 3, device=DEV)[0]
    q, r = (torch.from_numpy(a).to(DEV) for a in synth.make_inputs(5, 3, 98, 126, 5))
    outs = {}
    for blocks in (0, 8):
        with hh.switches(grid=blocks):
            o = net(q, r, False, 0, False, return_mean=True)
            torch.cuda.synchronize()
            outs[blocks] = (o["score_map_ref_cross"].clone(), o["score_mean_ref_cross"].clone())
    assert torch.isfinite(outs[0][0]).all()
    _same(outs[8][0], outs[0][0], "score maps")
    _same(outs[8][1], outs[0][1], "means")
