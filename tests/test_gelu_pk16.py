"""The panel kernel's packed-half GELU (csrc/panel.hip, round 5), checked on the CPU: the half constants compiled into the kernel are the ones
tools/gelu_pk16_fit.py derives, and the kernel's instruction sequence -- emulated with one half rounding per packed fma, exactly as the tool
does -- stays inside the error figures DESIGN.md / panel.hip quote against the exact erf-GELU of HF ACT2FN["gelu"] (modeling_dinov2.py:293-297).
The GPU side of the same claim is tests/test_hip_activations.py: the kernels' own instructions against this emulation, bit for bit, on every
finite 16-bit input and at every hidden position (tests/test_hip_panel.py and tests/test_hip_stages.py see the GELU only through fc2, on
Gaussian inputs).  The same file holds the expected-value side of the fp32 GELU of the GEMM epilogues (cs_common.h gelu_erf4), modelled here
in numpy and checked on every finite half and bfloat16 input."""
import os
import re

import numpy as np

from kernel_data import REPO, gelu_compiled, gelu_kernel_constants, gelu_tool


def test_kernel_constants_are_the_fitted_ones_and_the_error_figures_hold():
    t = gelu_tool()
    k = gelu_kernel_constants()
    assert set(k) == {"nk", "c5", "c4", "c3", "c2", "c1", "c0", "vc6"} and k["nk"] == -0.25  # -1 / R, R = 4
    c, fit_err = t.fit()
    assert fit_err < 1.0e-4  # 8.2e-5: minimax fit of -|x| Phi(-|x|) in z on |x| <= 4
    fitted = [float(np.float16(v)) for v in c]
    compiled = [k["c0"], k["c1"], k["c2"], k["c3"], k["c4"], k["c5"], k["vc6"]]
    assert compiled == fitted, (compiled, fitted)
    # the kernel's arithmetic on its own constants
    rng = np.random.default_rng(0)
    for sigma, rms_bound in ((0.5, 2.6e-4), (1.0, 3.2e-4), (2.0, 5.0e-4)):   # measured 2.1e-4 / 2.6e-4 / 4.0e-4
        x = (rng.standard_normal(200000) * sigma).astype(np.float32).astype(np.float64)
        e = t.kernel_gelu(x, np.asarray(compiled)) - t.gelu(x)
        assert float(np.sqrt((e ** 2).mean())) < rms_bound, sigma
        # never much worse than the reference's own 16-mixed arithmetic (GELU of the half-rounded input, rounded to half)
        ref16 = t.r16(t.gelu(t.r16(x))) - t.gelu(x)
        assert float(np.sqrt((e ** 2).mean())) < 2.4 * float(np.sqrt((ref16 ** 2).mean()))
    xl = np.linspace(-8.0, 8.0, 400001)
    e = np.abs(t.kernel_gelu(xl, np.asarray(compiled)) - t.gelu(xl))
    assert e.max() < 2.5e-3                      # 2.1e-3 at x = 2.30 (one half ulp is 9.8e-4 there)
    # beyond the fitted range the result is relu(x) + P6(-1/2) = relu(x) - 1.3e-4: exact to 2e-4 below -4, the output's half rounding above 4
    assert e[xl <= -4.0].max() < 2e-4 and (e[xl >= 4.0] / xl[xl >= 4.0]).max() < 2.0 ** -11 + 5e-5
    # values outside the half range behave as relu (what bf16 operand mode relies on for its correction term)
    big = np.array([7.0e4, -7.0e4, 1.0e9, -1.0e9, np.inf, -np.inf])
    with np.errstate(over="ignore"):  # (the half conversion of 7e4 / 1e9 overflows to inf by design: v_cvt_pk_f16_f32 does the same)
        y = t.kernel_gelu(big, np.asarray(compiled))
    assert np.all(y[[1, 3, 5]] <= 0) and np.all(np.abs(y[[1, 3, 5]]) < 2e-4) and np.all(np.isinf(y[[0, 2, 4]]))


def test_the_horner_form_of_phi_does_not_survive_half_precision():
    """Why the kernel does not evaluate Phi(x) = 0.5 + x Q(x^2) in halves (the form of the fp32 epilogues, cs_common.h gelu_erf4)."""
    t = gelu_tool()
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(100000) * 2.0).astype(np.float32).astype(np.float64)
    c, _ = t.fit()
    good = float(np.sqrt(((t.kernel_gelu(x, c) - t.gelu(x)) ** 2).mean()))
    naive = float(np.sqrt(((t.naive_gelu(x) - t.gelu(x)) ** 2).mean()))
    assert naive > 4 * good and naive > 1.5e-3, (naive, good)


def _all_finite_half():
    """the 63 488 finite IEEE half values, as float64"""
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    return h[np.isfinite(h)].astype(np.float64)


def _all_finite_bf16():
    """the 65 280 finite bfloat16 values, as float32"""
    b = (np.arange(65536, dtype=np.uint32) << 16).view(np.float32)
    return b[np.isfinite(b)]


def test_packed_half_gelu_on_every_finite_half_input():
    """fp16 operand mode: the eleven instructions on ALL finite half inputs (the linspace above never reaches the denormals, the values beyond
    8 or the largest ones).  Measured: max |e| 1.09e-3 on [-4, 4], 1.22e-4 for x <= -4, relative 3.2e-5 for x >= 4."""
    t = gelu_tool()
    x = _all_finite_half()
    assert x.size == 63488
    y = t.kernel_gelu(x, gelu_compiled(gelu_kernel_constants()))
    e = np.abs(y - t.gelu(x))
    print(f"packed-half GELU, every finite half: max |e| {e[np.abs(x) <= 8].max():.3e} on |x| <= 8, {e[x <= -4].max():.3e} for x <= -4, "
          f"relative {(e[x >= 4] / x[x >= 4]).max():.3e} for x >= 4")
    assert np.isfinite(y).all()
    assert e[np.abs(x) <= 8.0].max() < 2.5e-3
    assert e[x <= -4.0].max() < 2e-4 and (e[x >= 4.0] / x[x >= 4.0]).max() < 2.0 ** -11 + 5e-5
    # GELU's minimum is -0.16997 (at x = -0.7518); a negative input never gives a positive output
    assert y[x < 0].max() <= 0.0 and y[x < 0].min() >= -0.16997 - 2.5e-3


def test_packed_half_gelu_bf16_mode_on_every_finite_bf16_input():
    """bf16 operand mode (tools/gelu_pk16_fit.py kernel_gelu_bf16: correction term in halves on the half-rounded input, relu and the sum in fp32,
    one bf16 rounding): the fit figure of the fp16 form plus half a bf16 ulp of the result, on ALL finite bfloat16 inputs -- fp32's range is what
    that mode is for, so +-3.4e38 must behave as relu."""
    t = gelu_tool()
    a = _all_finite_bf16()
    assert a.size == 65280
    y = t.kernel_gelu_bf16(a, gelu_compiled(gelu_kernel_constants()))
    g = t.gelu(a.astype(np.float64))
    e = np.abs(y - g)
    slack = e - (2.5e-3 + 2.0 ** -8 * np.abs(g))
    print(f"packed-half GELU, bf16 mode, every finite bf16: worst |e| - bound {slack.max():.3e} at a = {float(a[slack.argmax()]):.6g}")
    assert np.isfinite(y).all()
    assert slack.max() <= 0.0
    assert y[a < 0].max() <= 0.0 and y[a < 0].min() >= -0.16997 - 2.5e-3 - 2.0 ** -8 * 0.17
    assert float(y[a == a.min()][0]) == float(y[a == np.float32(-8.0)][0])   # -3.4e38 gives the same tail as -8: the term of d = 0
    assert float(y[a.argmax()]) == float(a.max())  # relu(3.4e38) - 1.3e-4, rounded, is 3.4e38


def _gelu_erf4_constants():
    """The eight Horner coefficients of gelu_erf4 (cs_common.h), highest power of t = x^2 first, as the asm block consumes them."""
    src = open(os.path.join(REPO, "crossscore_amd", "csrc", "cs_common.h")).read()
    body = src[src.index("void gelu_erf4("):src.index("// ---- kernel parameter blocks")]
    num = r"(-?[0-9.]+e[+-][0-9]+)f"
    c0, rest = re.findall(r"gelu_c\(" + num + r"\)", body)[0], re.findall(r"gelu_c\(" + num + r"\)", body)[1:]
    c1 = re.search(r"f32x2_t c1 = \{" + num, body).group(1)
    k = [np.float32(v) for v in [c0, c1] + rest]
    assert len(k) == 8, k
    return k


def gelu_erf4_model(x, k):
    """gelu_erf4 per value in fp32, one rounding per instruction: c = med3(x, -4.2, 4.2), t = c c, seven fmas down the Horner chain,
    Phi = fma(c, q, 0.5), y = max(x, -4.2) Phi.  (Products of two fp32 values are exact in float64, so each fma below rounds its exact
    product-sum to float64 and then to fp32: one fp32 rounding but for double-rounding ties, which a bound -- not bit equality -- ignores.)"""
    f32, f64 = np.float32, np.float64
    fma = lambda a, b, c: (a.astype(f64) * b.astype(f64) + f64(c)).astype(f32)
    x = np.asarray(x, dtype=f32)
    c = np.clip(x, f32(-4.2), f32(4.2))
    t = (c * c).astype(f32)
    q = fma(t, np.full_like(t, k[0]), k[1])
    for kk in k[2:]:
        q = fma(q, t, kk)
    phi = fma(c, q, f32(0.5))
    return (np.maximum(x, f32(-4.2)) * phi).astype(f32)


def test_fp32_gelu_of_the_gemm_epilogues_on_every_finite_16_bit_input():
    """gelu_erf4 before the store's rounding, against the float64 erf GELU of the exact input:
        |y - gelu(x)| <= 2.1e-4 + 3.1e-5 |gelu(x)|
    2.1e-4 is the header's figure for the fit as evaluated in fp32, 3.1e-5 = 1 - Phi_fit(4.2) the relative slope above the clamp (3.01e-5).
    On all 63 488 finite half and all 65 280 finite bfloat16 inputs (the factor in front of Phi has to be max(x, -4.2), not x, for that)."""
    t = gelu_tool()
    k = _gelu_erf4_constants()
    for name, x in (("half", _all_finite_half().astype(np.float32)), ("bf16", _all_finite_bf16())):
        g = t.gelu(x.astype(np.float64))
        bound = 2.1e-4 + 3.1e-5 * np.abs(g)
        y = gelu_erf4_model(x, k).astype(np.float64)
        slack = np.abs(y - g) - bound
        print(f"gelu_erf4 model, every finite {name}: worst |e| - bound {slack.max():.3e} at x = {float(x[slack.argmax()]):.6g}; "
              f"max |e| for x <= 4.2: {np.abs(y - g)[x <= 4.2].max():.3e}")
        assert np.isfinite(y).all()
        assert slack.max() <= 0.0, (name, float(x[slack.argmax()]))
        assert y[x < 0].max() <= 0.0
        assert np.all(y[x < -4.2] == y[x < -4.2][0]) and -1.3e-4 < float(y[x < -4.2][0]) < -1.2e-4   # the constant tail -4.2 Phi_fit(-4.2)
