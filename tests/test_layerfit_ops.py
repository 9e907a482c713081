"""cs_op_layer_backward (csrc/layerfit.hip) against tests/layerfit_oracle.py, in both operand types.  Os, lse_s, O and lse are
cs_op_attention's on the same operands, never the oracle's.  Every bound is assembled from the number formats and the case's own tensors
(layerfit_helpers.layer_fro_bounds; tests/test_layerfit_host.py checks on the CPU that the rounded oracle stays inside them and that every planted
defect leaves them); outputs sit inside tests/guard.py bands, the 16-bit operands are strided views of poisoned buffers (Qs' | Ks | Vs side by side
in one packed buffer, as the forward leaves them)."""
import ctypes as C
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import headfit_helpers as hh  # noqa: E402
import layerfit_helpers as lh  # noqa: E402
import layerfit_oracle as lo  # noqa: E402
from bits16 import MODES  # noqa: E402
from guard import guarded_out  # noqa: E402
from hip_helpers import switches  # noqa: E402
from crossscore_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
P = 14


def _run_layer(lib, c, d, Cc, accumulate=0, init=None):
    """one call on fresh guarded outputs (init: their starting content) -> (the twenty-two gradients, the loss)"""
    outs = [guarded_out(s, torch.float32, init=None if init is None else init[i]) for i, s in enumerate(lh.layer_shapes(Cc))]
    loss = torch.full((), 7.0, dtype=F64, device="cuda") if init is None else init[22].clone()
    ws = hh.workspace(lib.cs_layer_backward_workspace_bytes(c["B"], c["gh"] * c["gw"], c["N"], Cc, P, c["h"]))
    _lib.check(lib.cs_op_layer_backward(*lh.layer_backward_args(d, c, P, accumulate, [o[0] for o in outs] + [loss], ws)))
    torch.cuda.synchronize()
    for (_, chk), name in zip(outs, lo.KEYS):
        chk(name)
    return [o[0].contiguous().clone() for o in outs], loss


@MODES
@pytest.mark.parametrize("Cc,h", lh.WIDTHS)
@pytest.mark.parametrize("B,N,gh,gw,short_cut", lh.LAYER_OP_CASES)
def test_layer_backward(B, N, gh, gw, short_cut, Cc, h, bf16):
    lib = _lib.load()
    c = lh.layer_case(B, N, gh, gw, Cc, h, 0, 1.0, bf16, seed=lh.case_seed(B, gh, gw, Cc), attn=lh.gpu_attention(bf16), short_cut=short_cut)
    ref = lh.layer_oracle(c, bf16)
    bounds = lh.layer_fro_bounds(ref, c, bf16)
    d = lh.layer_device(c, bf16)
    M = B * gh * gw
    with switches(bf16=bf16):
        got, loss = _run_layer(lib, c, d, Cc)
        # the sixteen inner gradients and the loss: cs_op_cross_backward's on the same tensors, bit for bit
        xouts = [torch.full(s, 7.0, device="cuda") for s in lh.layer_shapes(Cc)[6:]]
        xloss = torch.full((), 7.0, dtype=F64, device="cuda")
        xws = hh.workspace(lib.cs_cross_backward_workspace_bytes(B, gh * gw, N, Cc, P, h))
        _lib.check(lib.cs_op_cross_backward(*lh.cross_args_device(d, c, P, 0, xouts + [xloss], xws)))
        torch.cuda.synchronize()
        again, loss2 = _run_layer(lib, c, d, Cc)
        # accumulate = 1 on top of known contents: (old + new) in fp32, the kernels' own rule
        base = [torch.full(s, 0.25, device="cuda") for s in lh.layer_shapes(Cc)] + [torch.full((), 0.5, dtype=F64, device="cuda")]
        added, loss3 = _run_layer(lib, c, d, Cc, accumulate=1, init=base)
    for o, t, name in zip(got[6:], xouts, lo.KEYS[6:]):
        assert torch.equal(o, t), f"{name}: the sixteen inner gradients are cs_op_cross_backward's bit for bit"
    assert float(loss) == float(xloss) == float(loss2)
    for a, b, name in zip(got, again, lo.KEYS):
        assert torch.equal(a, b), f"{name}: two identical calls give identical bits"
    for a, g, name in zip(added, got, lo.KEYS):
        assert torch.allclose(a, g + 0.25, rtol=0, atol=2.0 ** -22 * (0.25 + float(g.abs().max()))), f"{name}: accumulate = 1 adds to what is there"
    assert abs(float(loss3) - (0.5 + float(loss))) <= 1e-12
    have = lh.split_layer([t.double().cpu() for t in got[:6]], Cc)
    want = lh.split_layer(ref, Cc)
    tag = f"M {M} Np {gh * gw} C {Cc} {'bf16' if bf16 else 'fp16'}{'' if short_cut else ' no short cut'}"
    for name in lh.LAYER_PARTS:
        err, nrm = float((have[name] - want[name]).norm()), float(want[name].norm())
        print(f"layer_backward {tag} {name}: rel Frobenius {err / max(nrm, 1e-300):.3e}, err/bound {err / bounds[name]:.4f}, bound/|ref| {bounds[name] / max(nrm, 1e-300):.2e}")
        if name == "dbk_s":
            continue
        assert err <= bounds[name], name  # (that these bounds discriminate: test_layerfit_host.test_defects_exceed_the_op_bounds, same cases)
    # the K bias gradient: zero in exact arithmetic; the op returns no more than the residue the oracle with roundings on predicts, plus its bound
    assert float(have["dbk_s"].norm()) <= float(want["dbk_s"].norm()) + bounds["dbk_s"]


def test_layer_backward_rejections():
    """every rejection returns before any launch, with the specified code: the poisoned outputs keep their bits"""
    B, N, gh, gw, Cc, h = 1, 2, 2, 3, 128, 8
    c = lh.layer_case(B, N, gh, gw, Cc, h, 0, 1.0, False, seed=3)
    lib = _lib.load()
    d = lh.layer_device(c, False)
    outs = [torch.full(s, 7.0, device="cuda") for s in lh.layer_shapes(Cc)] + [torch.full((), 7.0, dtype=F64, device="cuda")]
    ws = hh.workspace(lib.cs_layer_backward_workspace_bytes(B, gh * gw, N, Cc, P, h))
    good = lh.layer_backward_args(d, c, P, 0, outs, ws)
    assert len(good) == len(_lib.SYMBOLS["cs_op_layer_backward"][1])
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)  # noqa: E731
    BAD, UNS = _lib.CS_ERR_BAD_ARG, _lib.CS_ERR_UNSUPPORTED
    # indices: the fourteen leading arguments of the block, then cs_op_cross_backward's list shifted by 14 (its 47 inputs, 6 + 16 gradients, loss, ws)
    edits = {"null x0": (0, None, BAD), "null Qs": (1, None, BAD), "null Ks": (2, None, BAD), "null Vs": (3, None, BAD), "null Os": (5, None, BAD),
             "null lse_s": (7, None, BAD), "null Wq": (8, None, BAD), "null Wo_s": (10, None, BAD), "null bo_s": (12, None, BAD),
             "null gamma1": (13, None, BAD), "null dWin_s": (61, None, BAD), "null dbeta1": (66, None, BAD), "null dWin": (67, None, BAD),
             "null x1": (14, None, BAD), "null loss": (83, None, BAD), "null workspace": (84, None, BAD),
             "short Q|K|V pitch": (4, Cc - 8, BAD), "odd Q|K|V pitch": (4, 3 * Cc + 4, BAD), "odd Os pitch": (6, Cc + 4, BAD),
             "short Wq pitch": (9, Cc - 8, BAD), "odd Wo_s pitch": (11, Cc + 4, BAD), "misaligned x0": (0, off(d["x0"], 4), BAD),
             "misaligned Qs": (1, off(d["Qs"], 8), BAD), "misaligned Os": (5, off(d["Os"], 2), BAD), "misaligned lse_s": (7, off(d["lse_s"], 2), BAD),
             "misaligned dWo_s": (63, off(outs[2], 2), BAD), "misaligned workspace": (84, off(ws, 16), BAD), "N 0": (31, 0, BAD),
             "empty batch": (52, 0, BAD), "inv_count 0": (59, 0.0, BAD), "heads 7": (32, 7, UNS), "heads 2 (head dim 64)": (32, 2, UNS),
             "heads 1 (head dim 128)": (32, 1, UNS), "patch 16": (55, 16, UNS), "hidden 96": (56, 96, UNS)}
    for what, (i, v, code) in edits.items():
        args = list(good)
        args[i] = v
        assert lib.cs_op_layer_backward(*args) == code, what
        assert _lib.last_error(), what
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 7.0).all())
    assert lib.cs_layer_backward_workspace_bytes(B, gh * gw, N, Cc, P, 2) == 0 and lib.cs_layer_backward_workspace_bytes(B, gh * gw, N, Cc, 16, h) == 0
    assert lib.cs_layer_backward_workspace_bytes(B, gh * gw, N, Cc, P, h) > lib.cs_cross_backward_workspace_bytes(B, gh * gw, N, Cc, P, h) > 0
    assert lib.cs_op_layer_backward(*good) == 0
    torch.cuda.synchronize()
