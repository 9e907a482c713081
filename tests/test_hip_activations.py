"""Every activation function a kernel computes, evaluated by the kernel itself on every finite 16-bit input and compared with a float64 reference
of the same function (and, for the token-panel kernels' packed-half GELU, bit for bit with tools/gelu_pk16_fit.py's emulation of its
instructions).  The other GPU tests cover shapes; their values are Gaussian, so they never see a tail, a denormal or a rounding tie.

Each test drives one kernel so that its matrix product degenerates to a selection -- a one-hot operand, zero weights, a 0 / 1 selector -- and the
activation's input is known exactly and its output is read back unmixed.  Non-finite operand patterns are kept out of the matrices (0 x inf
inside an MFMA sum is NaN and would poison a whole row); NaN inputs are out of scope.

Which GEMM kernel runs is the documented routing rule (cs_gemm256_supported: M >= 256, N % 256 == 0, K >= 384 and K % 128 == 0 go to
csrc/gemm256.hip unless cs_debug_gemm256_enable(0)); the single-op entry points keep no routing counters."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from crossscore_amd import _lib  # noqa: E402
from oracle import crossscore_oracle as orc  # noqa: E402
import hip_helpers as hh  # noqa: E402
from bits16 import MODES, bits  # noqa: E402
from kernel_data import gelu_compiled, gelu_kernel_constants, gelu_tool  # noqa: E402

DEV = "cuda"
F16, BF16 = torch.float16, torch.bfloat16
EPIS = {"bias": _lib.EPI_BIAS_F16, "gelu": _lib.EPI_BIAS_GELU_F16, "relu": _lib.EPI_BIAS_RELU_F16, "leaky": _lib.EPI_BIAS_LEAKY_F16}


def _dt(bf16):
    return BF16 if bf16 else F16


def _patterns():
    """all 65 536 16-bit patterns in ascending order, as int16 bits (CPU)"""
    return torch.from_numpy(np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.int16).copy())


def _finite_sweep(bf16):
    """(65536,) tensor of the operand type: pattern i reinterpreted, the non-finite patterns replaced by +0"""
    v = _patterns().view(_dt(bf16))
    return torch.where(torch.isfinite(v), v, torch.zeros_like(v))


def _gelu64(x):
    """exact erf GELU in float64 (HF ACT2FN["gelu"]); -inf gives the limit -0"""
    x = x.double()
    g = 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))
    return torch.where(torch.isinf(x) & (x < 0), torch.zeros_like(x), g)


# ================================================================================================ a. GEMM epilogues
GM, GN, GK = 256, 256, 384  # the smallest shape the 256-tile kernel takes


def _gemm_operands(bf16):
    """A one-hot (A[m, m] = 1), W[n, k] = pattern n * 256 + k for k < 256 (non-finite -> 0), 0 beyond: out[m, n] = epi(W[n, m] + bias[n])"""
    dt = _dt(bf16)
    A = torch.zeros((GM, GK), dtype=dt)
    A[torch.arange(GM), torch.arange(GM)] = 1.0
    W = torch.zeros((GN, GK), dtype=dt)
    W[:, :256] = _finite_sweep(bf16).view(256, 256)
    return A.view(F16).to(DEV), W.view(F16).to(DEV), W[:, :256].clone()


def _gemm_run(A, W, bias, epi, bf16):
    """-> (256, 256) CPU tensor of the operand type, [n, k] = the epilogue's result for pattern n * 256 + k"""
    out = hh.gemm(A, W, bias, epi)
    torch.cuda.synchronize()
    return out.t().contiguous().cpu().view(_dt(bf16))


@pytest.fixture(scope="module")
def gemm_sweep():
    """every (operand type, kernel, epilogue) once, bias 0: {(bf16, g256, name): (256, 256) outputs}, and the inputs per operand type"""
    outs, xs = {}, {}
    for bf16 in (False, True):
        A, W, x = _gemm_operands(bf16)
        xs[bf16] = x
        zero = torch.zeros((GN,), device=DEV)
        for g256 in (True, False):
            with hh.switches(bf16=bf16, gemm256=g256):
                for name, epi in EPIS.items():
                    outs[(bf16, g256, name)] = _gemm_run(A, W, zero, epi, bf16)
    return outs, xs


@MODES
def test_gemm_bias_relu_leaky_are_exact_on_every_finite_input(gemm_sweep, bf16):
    """bias 0: BIAS returns its input, ReLU max(x, 0), LeakyReLU the operand-type rounding of the fp32 product 0.01f * x below 0 -- bit for bit,
    both kernels.  (-0 comes back as +0: it enters an fp32 sum that starts at the bias +0 and holds the +0 products of the padding columns.)"""
    outs, xs = gemm_sweep
    x = xs[bf16]
    x32 = x.float()
    want = {"bias": (x32 + 0.0).to(x.dtype),
            "relu": torch.where(x32 > 0, x32, torch.zeros_like(x32)).to(x.dtype),
            "leaky": torch.where(x32 >= 0, x32 + 0.0, x32 * torch.tensor(0.01, dtype=torch.float32)).to(x.dtype)}
    for g256 in (True, False):
        for name, w in want.items():
            got = outs[(bf16, g256, name)]
            bad = bits(got) != bits(w)
            n = int(bad.sum())
            first = [(hex(int(i)), float(got.flatten()[i]), float(w.flatten()[i])) for i in bad.flatten().nonzero().flatten()[:6]]
            print(f"gemm{'256' if g256 else '128'} {name} {'bf16' if bf16 else 'fp16'}: {n} of 65536 patterns differ {first}")
            assert n == 0, (g256, name, n, first)


@MODES
@pytest.mark.parametrize("g256", [True, False], ids=["gemm256", "gemm128"])
def test_gemm_gelu_on_every_finite_input(gemm_sweep, bf16, g256):
    """BIAS_GELU (cs_common.h gelu_erf4) against the float64 erf GELU of the exact input:
        |y - gelu(x)| <= 2.1e-4 + (h + 3.1e-5) |gelu(x)|,   h = 2^-11 (fp16) / 2^-8 (bf16)
    2.1e-4: the header's figure for the fit as evaluated in fp32; 3.1e-5 = 1 - Phi_fit(4.2), the relative slope above the clamp; h: half an ulp
    of the store.  No free parameter.  And a negative input never gives a positive output."""
    outs, xs = gemm_sweep
    x = xs[bf16].double().flatten()
    y = outs[(bf16, g256, "gelu")].double().flatten()
    g = _gelu64(x)
    h = 2.0 ** -8 if bf16 else 2.0 ** -11
    slack = (y - g).abs() - (2.1e-4 + (h + 3.1e-5) * g.abs())
    i = int(slack.argmax())
    nbad = int((slack > 0).sum())
    print(f"gemm{'256' if g256 else '128'} GELU {'bf16' if bf16 else 'fp16'}: worst |y - gelu| - bound {float(slack[i]):.3e} at x = {float(x[i]):.6g} "
          f"(y = {float(y[i]):.6g}); {nbad} inputs over the bound" + (f", the largest of them x = {float(x[slack > 0].max()):.6g}" if nbad else ""))
    assert torch.isfinite(y).all()
    assert nbad == 0, (nbad, float(x[i]), float(y[i]), float(g[i]))
    assert float(y[x < 0].max()) <= 0.0


@MODES
def test_gemm_kernels_agree_bit_for_bit_on_every_epilogue(gemm_sweep, bf16):
    """the two GEMM kernels share their epilogue functions and start their accumulators at the bias: the same bits (the header's standing claim)"""
    outs, _ = gemm_sweep
    for name in EPIS:
        assert torch.equal(bits(outs[(bf16, True, name)]), bits(outs[(bf16, False, name)])), name


# fractions of one ulp of the 16-bit type: exact ties, quarter / three-quarter points, near-ties one fp32-representable step to either side
_TIE_FRACTIONS = [0.5, -0.5, 0.25, -0.25, 0.75, -0.75, 0.375, -0.375, 0.5 + 2.0 ** -13, 0.5 - 2.0 ** -13, -0.5 - 2.0 ** -13, -0.5 + 2.0 ** -13,
                  1.5, -1.5, 0.5 + 2.0 ** -6, -0.5 - 2.0 ** -6]


def _row_ulp(n, bf16):
    """spacing of the operand type at pattern n * 256 (row n of the sweep; a bf16 row spans two binades: the lower one's)"""
    if bf16:
        e = (n & 0x7F) << 1
        return 2.0 ** (max(e, 1) - 127 - 7)
    e = (n >> 2) & 0x1F
    return 2.0 ** (max(e, 1) - 15 - 10)


@MODES
def test_gemm_bias_rounds_to_nearest_even_at_ties_and_near_ties(bf16):
    """BIAS with fp32 offsets that put W + bias on and next to the rounding ties of the output type: bias[n] = f * ulp(row n), f through
    +-1/2, +-1/4, +-3/4, +-3/8, +-(1/2 +- 2^-13), +-3/2, +-(1/2 + 2^-6); 16 launches rotate the fractions over the rows, so that every binade
    (values in [1, 2): +-2^-11, +-2^-12, +-3 2^-12, +-3 2^-13 .. in fp16) meets every fraction.  W + bias is exact in fp32 (an 11- or 8-bit value
    and an offset of at most 14 more bits), so the store's rounding is the only one: equal to torch's (W.float() + bias).to(dtype), bit for bit."""
    A, W, x = _gemm_operands(bf16)
    x32 = x.float()
    worst = 0
    for g256 in (True, False):
        with hh.switches(bf16=bf16, gemm256=g256):
            for t in range(16):
                b64 = torch.tensor([_TIE_FRACTIONS[(n + t) % 16] * _row_ulp(n, bf16) for n in range(GN)], dtype=torch.float64)
                bias = b64.float() + 0.0   # (an offset that underflows becomes +0, never -0: the sum of the padding columns holds +0)
                got = _gemm_run(A, W, bias.to(DEV), _lib.EPI_BIAS_F16, bf16)
                want = (x32 + bias[:, None]).to(x.dtype)
                bad = bits(got) != bits(want)
                worst = max(worst, int(bad.sum()))
                first = [(hex(int(i)), float(bias[int(i) // 256]), float(got.flatten()[i]), float(want.flatten()[i])) for i in bad.flatten().nonzero().flatten()[:6]]
                assert not bad.any(), (g256, t, int(bad.sum()), first)
    print(f"gemm bias ties {'bf16' if bf16 else 'fp16'}: 2 kernels x 16 rotations x 65536 sums, {worst} differ from torch")


@pytest.mark.parametrize("g256", [True, False], ids=["gemm256", "gemm128"])
def test_gemm_ln_gelu_is_the_same_function(gemm_sweep, g256):
    """LN_GELU calls the same gelu_erf4: zero accumulators, rows of mean 0 and rstd 1 through the statistics inputs, s = 0, and every 43rd half
    pattern in c[n] -- rstd * (0 - 0 * s) + c = c exactly -- must give the bits BIAS_GELU gave for that pattern."""
    outs, xs = gemm_sweep
    M, Cc, N = 257, 384, 1536
    idx = (torch.arange(N) * 43) % 65536
    c = xs[False].flatten()[idx].float()
    A = torch.zeros((M, Cc), dtype=F16, device=DEV)
    W = torch.zeros((N, Cc), dtype=F16, device=DEV)
    with hh.switches(bf16=False, gemm256=g256):
        if g256:   # finalised (mean, rstd) rows, padded to whole 256-row tiles
            ln = torch.zeros((512, 1, 2), device=DEV)
            ln[:, 0, 1] = 1.0
        else:      # partial (sum, sum of squares): variance 1 - eps
            sp = 4 * hh.column_tiles(Cc)
            ln = torch.zeros((M, sp, 2), device=DEV)
            ln[:, :, 1] = Cc * (1.0 - 1e-6) / sp
        out = hh.gemm(A, W, c.to(DEV), _lib.EPI_LN_GELU_F16, ln_part=ln, col_s=torch.zeros((N,), device=DEV), ln_eps=1e-6)
        torch.cuda.synchronize()
    want = outs[(False, g256, "gelu")].flatten()[idx]
    out = out.cpu()
    assert torch.equal(bits(out), bits(want[None, :].expand(M, N)))


# ================================================================================================ b. the token-panel kernels' packed-half GELU
PC, PF, PM = 384, 1536, 130  # one full 128-row panel and a ragged one

_f = np.float32


def _hi_lo(v, bf16):
    """What panel4.hip makes of an fc1 bias: it enters through the matrix pipe as hi + lo, two values of the operand type (hi = the rounded
    bias, lo = the rounded rest: 22 significant bits in fp16 mode, 16 in bf16 mode); panel.hip starts its accumulators at the fp32 bias itself."""
    v = np.asarray(v, dtype=_f)
    t = gelu_tool()
    rd = (lambda a: t.rbf16(a).astype(_f)) if bf16 else (lambda a: a.astype(np.float16).astype(_f))
    hi = rd(v)
    return (hi + rd((v - hi).astype(_f))).astype(_f)


# 32 edge values per operand mode (fp32 pre-activations): zeros, half denormals, the tie between 0 and the smallest one and a value just above
# it, the fit's worst point 2.3, GELU's minimum, both sides of the clamp of d at |x| = 4, the tail, the largest half, ties and near-ties of the
# half conversion (2^-21 to either side: the nearest that the hi + lo pair still carries), -65520 (-> -inf) and beyond, 65520 - 2^-5 (rounds
# down to 65504; 65520 itself would be +inf in the hidden row, and inf x 0 in fc2 poisons the whole row)
_E_FP16 = [0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -14, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23), 1.0, -1.0, 2.3, -2.3, 3.998, -3.998, 4.0, -4.0,
           4.004, -4.004, -8.375, 65504.0, -65504.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 3 * 2.0 ** -12, -(1 + 2.0 ** -11),
           1 + 2.0 ** -11 + 2.0 ** -21, 1 + 2.0 ** -11 - 2.0 ** -21, -65520.0, -7.0e4, 65520.0 - 2.0 ** -5, -0.7518, 3.0, -3.0]
# bf16 mode: the relu stays fp32, so values beyond the half range come in on both sides, and fp32 values that are ties and near-ties (2^-15 to
# either side) of the bf16 store and of the half conversion of the correction term's input
_E_BF16 = [0.0, -0.0, 2.0 ** -24, 2.0 ** -14, 1.0, -1.0, 2.3, -2.3, 3.998, -3.998, 4.0, -4.0, 4.004, -4.004, -8.375, 65504.0, -65504.0, -65520.0,
           -7.0e4, 1 + 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -15, 1.0e6, -1.0e6, 3.0e38, -3.0e38, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8,
           1 + 2.0 ** -8 + 2.0 ** -15, 1 + 2.0 ** -8 - 2.0 ** -15, 65520.0, 7.0e4, 3.0]
assert len(_E_FP16) == 32 and len(_E_BF16) == 32


def _edge_values(bf16):
    """The edge set as fp32 pre-activations both kernels see identically.  bf16 mode: the decimal entries are rounded to their hi + lo pair, so
    that the fp32 relu of both kernels gets the same number.  fp16 mode: the GELU's input is the half rounding of the pre-activation, which is
    the same for every entry and its pair (checked here, as is the exactness of the bf16 set)."""
    E = np.asarray(_E_BF16 if bf16 else _E_FP16, dtype=np.float64).astype(_f)
    if bf16:
        E = _hi_lo(E, True)
        assert np.array_equal(_hi_lo(E, True), E)
        return E
    inside = np.abs(E) <= 65504.0   # (beyond the half range the pair is -inf + inf: NaN, which the clamp of d turns into the same tail as -inf)
    assert np.array_equal(_hi_lo(E[inside], False).astype(np.float16), E[inside].astype(np.float16))
    return E


def _panel_values(bf16):
    """coverage (i): every finite value of the operand type and -inf (fp16 mode: and two finite fp32 values below the half range; its positive
    values beyond 65504 are left out -- the kernel documents that they become inf), padded with 0 to whole b1 vectors -> (vectors, 1536) fp32.
    The values below the half range (and -65520, -7e4 of the edge sets) reach the GELU as -inf in panel.hip only.  In panel4.hip their hi + lo
    pair is (-inf, +inf) or (-inf, NaN) and the accumulator holds NaN: there these inputs test that the clamp of d and the maxima swallow a NaN
    and return the same tail, not the -inf path."""
    v = _finite_sweep(bf16).float().numpy()
    v = v[np.isfinite(_patterns().view(_dt(bf16)).float().numpy())]
    extra = [-np.inf] if bf16 else [-7.0e4, -1.0e9, -np.inf]
    v = np.concatenate([v, np.asarray(extra, dtype=_f)])
    rows = -(-v.size // PF)
    out = np.zeros((rows * PF,), dtype=_f)
    out[:v.size] = v
    return out.reshape(rows, PF)


def _panel_edges(bf16):
    """coverage (ii): b1[j] = E[(j + t) % 32], t = 0..31 -> (32, 1536) fp32: every hidden position meets every edge value"""
    E = _edge_values(bf16)
    j = np.arange(PF)
    return np.stack([E[(j + t) % 32] for t in range(32)])


def _panel_run(b1_rows):
    """b1_rows (V, 1536) fp32 -> (V, 130, 1536) fp32: [v, m, j] = the kernel's GELU(b1_rows[v, j]) as row m saw it.  x = 0 and w1 = 0 make the
    hidden row b1 itself (panel4.hip: the hi + lo pair of b1, which is b1 for every value used here: _hi_lo, _edge_values); w2 selects hidden value 4 c + k for output column c (four weight images, k = 0..3), everything else is absent or 0, so
    x_out[m, c] is one non-zero term of an fp32 sum and a value of the 16-bit type already."""
    V = b1_rows.shape[0]
    b1 = torch.from_numpy(b1_rows).to(DEV)
    w1 = torch.zeros((PF, PC), device=DEV)
    b2 = torch.zeros((PC,), device=DEV)
    X = torch.zeros((4, V, PM, PC), device=DEV)
    for k in range(4):
        w2 = torch.zeros((PC, PF), device=DEV)
        w2[torch.arange(PC), 4 * torch.arange(PC) + k] = 1.0
        img = hh.panel_pack(None, None, w1, None, w2, None)
        for v in range(V):
            hh.encoder_panel(X[k, v], None, img, None, b1[v], b2, want_u=False)
    torch.cuda.synchronize()
    return X.permute(1, 2, 3, 0).reshape(V, PM, PF).cpu()   # [v, m, 4 c + k]


@pytest.fixture(scope="module", params=[(0, False), (0, True), (1, False), (1, True)], ids=["panel8-fp16", "panel8-bf16", "panel4-fp16", "panel4-bf16"])
def panel_gelu(request):
    """both coverage sets through one kernel and operand mode: (impl, bf16, b1 rows, kernel outputs of row 0, rows-all-equal flag, emulation)"""
    impl, bf16 = request.param
    rows = np.concatenate([_panel_values(bf16), _panel_edges(bf16)])
    with hh.switches(bf16=bf16, gemm256=True, panel_impl=impl):
        out = _panel_run(rows)
    t = gelu_tool()
    c = gelu_compiled(gelu_kernel_constants())
    with np.errstate(over="ignore"):
        emu = t.kernel_gelu_bf16(rows, c) if bf16 else t.kernel_gelu(rows.astype(np.float64), c)
    return impl, bf16, rows, out, emu


def test_panel_gelu_is_the_same_in_every_row(panel_gelu):
    """the hidden row does not depend on the token row: all 130 rows (every accumulator register and lane of the fc1 tile, both halves of every
    packed pair, the ragged second panel) carry row 0's bits"""
    _, _, _, out, _ = panel_gelu
    assert torch.equal(out.view(torch.int32), out[:, :1].expand_as(out).contiguous().view(torch.int32))


def test_panel_gelu_matches_the_emulation_bit_for_bit(panel_gelu):
    """tools/gelu_pk16_fit.py kernel_gelu / kernel_gelu_bf16 on the compiled constants is the project's model of the instructions: equal on every
    finite value of the operand type (and -inf, -7e4, -1e9: a NaN pre-activation in panel4.hip, see _panel_values) and on the 32 edge values at each of the 1536 hidden positions.  (The fp32 output
    cannot tell -0 from +0: it is 0 + the term.)"""
    impl, bf16, rows, out, emu = panel_gelu
    got = out[:, 0].double().numpy()
    assert np.isfinite(got).all()
    bad = got != emu
    where = np.argwhere(bad)
    first = [(float(rows[v, j]), float(got[v, j]), float(emu[v, j]), int(j)) for v, j in where[:8]]
    nv = _panel_values(bf16).shape[0]
    print(f"panel{4 if impl else 8} {'bf16' if bf16 else 'fp16'} GELU vs emulation: {int(bad[:nv].sum())} of {nv * PF} sweep slots and "
          f"{int(bad[nv:].sum())} of {32 * PF} edge slots differ {first}")
    assert not bad.any(), (int(bad.sum()), first)


def test_panel_gelu_against_the_exact_gelu_on_every_value(panel_gelu):
    """independently of the emulation, coverage (i) against the float64 erf GELU, with the figures tests/test_gelu_pk16.py asserts of the
    emulation: fp16 mode < 2.5e-3 on |x| <= 8, < 2e-4 for x <= -4 (the -1.2e-4 tail, also at -7e4, -1e9 and -inf -- panel4.hip gets there from a NaN, see _panel_values), relative < 2^-11 + 5e-5 for
    x >= 4; bf16 mode |y - gelu(a)| <= 2.5e-3 + 2^-8 |gelu(a)| (the same fit figure plus half a bf16 ulp)."""
    impl, bf16, rows, out, _ = panel_gelu
    nv = _panel_values(bf16).shape[0]
    x = torch.from_numpy(rows[:nv]).double().flatten()
    y = out[:nv, 0].double().flatten()
    g = _gelu64(x)
    e = (y - g).abs()
    tag = f"panel{4 if impl else 8} {'bf16' if bf16 else 'fp16'} GELU vs float64 erf GELU:"
    assert torch.isfinite(y).all()
    assert float(y[x < 0].max()) <= 0.0 and float(y[x < 0].min()) >= -0.16997 - 2.5e-3 - 2.0 ** -8 * 0.17
    if bf16:
        slack = e - (2.5e-3 + 2.0 ** -8 * g.abs())
        i = int(slack.argmax())
        print(f"{tag} worst |e| - bound {float(slack[i]):.3e} at a = {float(x[i]):.6g}; max |e| on |a| <= 8 {float(e[x.abs() <= 8].max()):.3e}")
        assert float(slack[i]) <= 0.0, (float(x[i]), float(y[i]))
        return
    mid, lo, hi = x.abs() <= 8.0, x <= -4.0, x >= 4.0
    rel = e[hi] / x[hi]
    print(f"{tag} max |e| {float(e[mid].max()):.3e} at x = {float(x[mid][e[mid].argmax()]):.6g} on |x| <= 8, {float(e[lo].max()):.3e} for x <= -4, "
          f"relative {float(rel.max()):.3e} for x >= 4")
    assert float(e[mid].max()) < 2.5e-3
    assert float(e[lo].max()) < 2e-4 and float(rel.max()) < 2.0 ** -11 + 5e-5
    tail = y[torch.isinf(x) | (x < -65504.0)]
    assert tail.numel() == 3 and bool((tail < -1.0e-4).all()) and bool((tail > -1.4e-4).all())   # -7e4, -1e9, -inf: P6(-1/2) = -1.2e-4


# ================================================================================================ c. the head's sigmoid / tanh / pow
@pytest.mark.parametrize("act,powp", [(0, 1.0), (0, 2.0), (0, 0.5), (1, 1.0), (1, 2.0)])
def test_head_activation_on_every_finite_half(act, powp):
    """sigmoid / tanh (+ pow) of the head epilogue on every finite half value: one-hot A (384 patches), W[n, k] = pattern (384 n + k) % 65536, so
    score pixel (patch k, column n) = act(W[n, k]); against float64 torch through the oracle's jigsaw at test_gemm_head_score_jigsaw's 1e-5, inside
    the function's range, exact at the ends of the half range, and the same launch's mean against the fp64 mean of the map it wrote.
    ((1, 0.5) is not run: the reference itself returns NaN for negative bases.)"""
    P, K, gh, gw = 14, 384, 16, 24
    Np, N = gh * gw, P * P
    sweep = _finite_sweep(False)
    W = sweep[(torch.arange(N * K) % 65536)].view(N, K)
    A = torch.zeros((Np, K), dtype=F16)
    A[torch.arange(Np), torch.arange(Np)] = 1.0
    with hh.switches(bf16=False, gemm256=True):
        score, mean, cnt = hh.head_score(A.to(DEV), W.to(DEV), torch.zeros((N,), device=DEV), 1, gh, gw, P, act=act, powp=powp)
        torch.cuda.synchronize()
    x = W.double().t().contiguous()                      # (patch m, column n)
    y = torch.sigmoid(x) if act == 0 else torch.tanh(x)
    if powp != 1.0:
        y = y ** powp
    ref = orc.jigsaw_to_image(y.view(1, Np, P, P), gh, gw)
    got = score.cpu().double()
    err = (got - ref).abs()
    i = int(err.argmax())
    back = got.view(gh, P, gw, P).permute(0, 2, 1, 3).reshape(Np, N)   # the jigsaw undone: (patch, column)
    print(f"head act={act} pow={powp}: max |score - float64| {float(err.max()):.2e} at x = {float(x.flatten()[int((back - y).abs().argmax())]):.6g}")
    assert torch.isfinite(got).all()
    assert float(err.flatten()[i]) < 1e-5
    assert float(got.min()) >= (0.0 if act == 0 or powp == 2.0 else -1.0) and float(got.max()) <= 1.0
    lo, hi = back[x == -65504.0], back[x == 65504.0]
    assert lo.numel() >= 1 and hi.numel() >= 1
    if act == 0:
        assert bool((lo == 0.0).all()) and bool((hi == 1.0).all())          # sigmoid(-65504) is exactly 0, also squared or under the root
    else:
        assert bool((lo == (-1.0 if powp == 1.0 else 1.0)).all()) and bool((hi == 1.0).all())   # tanh(+-65504) is exactly +-1
    merr = abs(float(mean[0].double().cpu()) - float(got.mean()))
    print(f"head act={act} pow={powp}: |mean - fp64 mean of the map| = {merr:.2e}")
    assert merr < 2e-7 * max(1.0, math.sqrt(Np * P * P) / 64)
    assert int(cnt.abs().sum()) == 0


# ================================================================================================ d. the SwiGLU gate
@MODES
def test_silu_mul_on_every_finite_input(bf16):
    """cs_op_silu_mul with x1 through every finite pattern of the operand type and x2 = 1, -1, 0.5: test_silu_mul's tolerance (one rounding of an
    fp32 evaluation + half an ulp of the 16-bit output), finite everywhere (the exp overflows for x1 < -88), exactly 0 from -100 downwards"""
    dt = _dt(bf16)
    F = 65536
    x = torch.empty((3, 2 * F), dtype=dt)
    x[:, :F] = _finite_sweep(bf16)[None, :]
    for m, v in enumerate((1.0, -1.0, 0.5)):
        x[m, F:] = v
    buf = x.view(F16).to(DEV)
    with hh.switches(bf16=bf16, gemm256=True):
        hh.silu_mul(buf)
        torch.cuda.synchronize()
    out = buf.cpu().view(dt)
    assert torch.equal(bits(out[:, F:]), bits(x[:, F:]))
    x1, x2 = x[:, :F].double(), x[:, F:].double()
    ref = x1 / (1.0 + torch.exp(-x1)) * x2
    o = out[:, :F].double()
    half = 2.0 ** -8 if bf16 else 2.0 ** -11
    slack = (o - ref).abs() - ((half + 2e-6) * ref.abs() + 2.0 ** -24)
    i = int(slack.argmax())
    print(f"silu_mul {'bf16' if bf16 else 'fp16'}: worst |o - ref| - bound {float(slack.flatten()[i]):.3e} at x1 = {float(x1.flatten()[i]):.6g}, "
          f"x2 = {float(x2.flatten()[i]):.3g}")
    assert torch.isfinite(o).all()
    assert float(slack.max()) <= 0.0, (float(x1.flatten()[i]), float(o.flatten()[i]), float(ref.flatten()[i]))
    assert bool((o[x1 <= -100.0] == 0.0).all())
