"""16-bit operand helpers of the kernel tests.  The ops take fp16 or bfloat16 operands as raw bits in a float16 tensor (the operand type is a
process-wide switch: hip_helpers.switches(bf16=...)); these helpers round to that type, read its values back and compare bit patterns."""
import time

import numpy as np
import pytest
import torch

F16, BF16 = torch.float16, torch.bfloat16
MODES = pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def to_dev(a, dtype=None, device="cuda"):
    """numpy array -> device tensor (of `dtype`, converted on the device, if given)"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return t if dtype is None else t.to(dtype)


def bits16(t, bf16):
    """values as the 16-bit operand tensor the ops take (raw bits in a float16 tensor in both modes), rounded to nearest even once"""
    return t.to(BF16).view(F16) if bf16 else t.to(F16)


def vals16(t, bf16, dtype=torch.float32):
    """the values of a 16-bit operand tensor, in `dtype`"""
    return (t.view(BF16) if bf16 else t).to(dtype)


def r16(t, bf16):
    """round to the operand type, back in the input's dtype"""
    return t.to(BF16 if bf16 else F16).to(t.dtype)


def rd(bf16):
    """bits16 for one operand type, as a function of the tensor"""
    return lambda t: bits16(t, bf16)


def fl(bf16):
    """vals16 (fp32) for one operand type, as a function of the tensor"""
    return lambda t: vals16(t, bf16)


def bits(t):
    """a 2- or 4-byte tensor as the integers of its bit patterns"""
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(got, want, what="", by_value=False):
    """bit for bit; 16-bit tensors always through their integer view (they may carry bfloat16 bits under a half dtype).  by_value: 4-byte tensors
    as torch.equal compares them (+0 equals -0, NaN nothing)."""
    if by_value and got.element_size() != 2:
        bad = got != want if got.shape == want.shape else None
        ok = torch.equal(got, want)
    else:
        g, w = bits(got), bits(want)
        bad = g != w if g.shape == w.shape else None
        ok = torch.equal(g, w)
    if ok:
        return
    if bad is None:
        raise AssertionError(f"{what}: shapes {tuple(got.shape)} against {tuple(want.shape)}")
    first = tuple(torch.nonzero(bad)[0].tolist())
    show = (lambda t: hex(int(bits(t)[first]) & 0xFFFF)) if got.element_size() == 2 else (lambda t: repr(float(t[first])))
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ{'' if by_value else ' in their bits'}; the first at "
                         f"{list(first)}: {show(got)} against {show(want)}")


def ordered16(t):
    """16-bit patterns as integers in the order of their values: neighbours differ by 1 (+0 and -0 by 0)"""
    b = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(b >= 0x8000, -(b & 0x7FFF), b & 0x7FFF)


def spacing16(x, bf16):
    """the spacing of the operand type's values around |x| (fp64 tensor): 2^(floor(log2 |x|) - 10) in fp16 from its smallest normal 2^-14 up,
    2^(floor(log2 |x|) - 7) in bf16 from 2^-126"""
    e = torch.frexp(x.abs())[1].double() - 1.0
    e = torch.where(x == 0, torch.full_like(e, -1000.0), e)
    return torch.exp2(torch.clamp(e, min=-126.0 if bf16 else -14.0) - (7.0 if bf16 else 10.0))


class Worst:
    """The worst figure per (test, operand type) of a module and the module's wall time, printed at teardown: a module's setup_module /
    teardown_module call start() / report().  A module that only wants its wall time notes nothing."""

    def __init__(self, module, label=None):
        self.label, self.module, self.worst, self.t0 = label, module, {}, None

    def start(self):
        self.t0 = time.time()

    def note(self, name, bf16, **figs):
        w = self.worst.setdefault((name, bf16), {})
        for k, v in figs.items():
            w[k] = max(w.get(k, 0.0), float(v))

    def report(self):
        print()
        for (name, bf16), figs in sorted(self.worst.items()):
            print(f"{self.label} worst, {name}, {'bf16' if bf16 else 'fp16'}: " + ", ".join(f"{k} {v:.3e}" for k, v in figs.items()))
        print(f"{self.module} wall time: {time.time() - self.t0:.1f} s")
