"""Operands and references of the encoder token-panel kernels (csrc/panel.hip, csrc/panel4.hip) at the ViT-S width: shared by
test_hip_panel.py, the two tile-level modules, test_hip_bounds.py and the panel tools under tools/."""
import torch

from bits16 import r16

C, F = 384, 1536

# fp16: the bounds of test_hip_panel.py::test_panel_vs_torch.  bf16: max / mean of its concurrent-streams test (8 significant bits); u is a
# bf16 value of magnitude up to 4 (half an ulp 7.8e-3) of rows whose x carries up to 3.2e-2 of error at rstd ~ 0.45: 7.8e-3 + 1.5e-2, rounded up.
BOUNDS = {False: (4e-3, 4e-4, 6e-3), True: (3.2e-2, 2.4e-3, 3e-2)}


def bf(t):
    return t.to(torch.float16).to(torch.float32)


def norm(x, eps=1e-6):
    """LayerNorm without gamma / beta, in the input's dtype (fp32 and fp64 references alike)"""
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps)


def make(M, seed, dev):
    """-> (x (M, C) fp32 residual stream, o (M, C) fp16 attention output, the layer tail's fp32 weights)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dev)
    x = rn(M, C, sc=2.0)
    x[:, 7] += 3.0  # a feature with a large mean, as DINOv2 residual streams have
    o = rn(M, C).to(torch.float16)
    w = dict(wo=rn(C, C, sc=C ** -0.5), ls1=rn(C, sc=0.3) + 1.0, bo=rn(C, sc=0.1), w1=rn(F, C, sc=C ** -0.5), g2=rn(C, sc=0.2) + 1.0,
             b1=rn(F, sc=0.5), w2=rn(C, F, sc=F ** -0.5), ls2=rn(C, sc=0.3) + 1.0, b2=rn(C, sc=0.1))
    return x, o, w


def reference(x, o, w, outproj, emulate):
    """the layer tail in fp32 torch; emulate: with the kernel's fp16 operand roundings"""
    r = bf if emulate else (lambda t: t)
    x1 = x.clone()
    if outproj:
        x1 = x1 + o.float() @ r(w["wo"] * w["ls1"][:, None]).T + w["bo"]
    h = torch.nn.functional.gelu(r(norm(x1)) @ r(w["w1"] * w["g2"][None, :]).T + w["b1"])
    x2 = x1 + r(h) @ r(w["w2"] * w["ls2"][:, None]).T + w["b2"]
    return x2, norm(x2)


def reference64(x, o16, w, outproj, bf16):
    """the layer tail in fp64 on the same 16-bit-rounded operands (weights with LayerScale / gamma folded, norm2(x), the hidden slice), exact GELU"""
    d = torch.float64
    r = lambda t: r16(t.float(), bf16).to(d)
    x1 = x.to(d)
    if outproj:
        x1 = x1 + o16.to(d) @ r(w["wo"] * w["ls1"][:, None]).T + w["bo"].to(d)
    h = torch.nn.functional.gelu(r(norm(x1)) @ r(w["w1"] * w["g2"][None, :]).T + w["b1"].to(d))
    x2 = x1 + r(h) @ r(w["w2"] * w["ls2"][:, None]).T + w["b2"].to(d)
    return x2, norm(x2)


def zero_weights(dev):
    z = lambda *s: torch.zeros(*s, device=dev)
    one = lambda *s: torch.ones(*s, device=dev)
    return dict(wo=z(C, C), ls1=one(C), bo=z(C), w1=z(F, C), g2=one(C), b1=z(F), w2=z(C, F), ls2=one(C), b2=z(C))
