"""Host-side checks of the tail fit: the fp64 oracle's ten gradients against torch.autograd of the tail the reference's
modules execute, its AdamW trajectory against torch.optim.AdamW, the properties of the LayerNorm and ReLU backward, the driver's fit_scope
option, and that the kernel file is listed, declared and bound."""
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import headfit_oracle as ho  # noqa: E402
import tailfit_helpers as th  # noqa: E402
import tailfit_oracle as to  # noqa: E402
from crossscore_amd import _lib, build  # noqa: E402
from crossscore_amd.config import load_config, model_config  # noqa: E402
from crossscore_amd.model import CrossScoreNet, HeadFitState  # noqa: E402

F64 = torch.float64
P, PP = 14, 196
CONFIGS = [(0, 1.0), (0, 2.5), (1, 1.0)]  # (act, p)


def _case(B, gh, gw, Cc, act, p, seed, dtype=F64):
    """x2, the ten parameters and a gt at least 0.05 away from the tail's own score everywhere"""
    g = torch.Generator().manual_seed(seed)
    M = B * gh * gw
    rn = lambda *s: torch.randn(s, generator=g, dtype=F64)  # noqa: E731
    x2 = rn(M, Cc)
    params = [rn(Cc, Cc) / Cc ** 0.5, rn(Cc) * 0.1, rn(Cc, Cc) / Cc ** 0.5, rn(Cc) * 0.1, 1.0 + 0.2 * rn(Cc), 0.1 * rn(Cc),
              rn(Cc, Cc) / Cc ** 0.5, rn(Cc) * 0.1, rn(PP, Cc) * (1.5 / Cc ** 0.5), rn(PP) * 0.3]
    H, _, X, A = to.tail_forward(x2, *params[:8])
    s, _ = ho.scores(A, params[8], params[9], act, p)
    off = (0.05 + 0.25 * torch.rand(s.shape, generator=g, dtype=F64)) * torch.where(torch.rand(s.shape, generator=g) < 0.5, -1.0, 1.0)
    gt_rows = s + off
    return x2.to(dtype), [t.to(dtype) for t in params], gt_rows.to(dtype)


def _oracle(x2, params, gt_rows, act, p):
    W1, b1, W2, b2, g3, b3, Wa, ba, Wb, bb = params
    H, _, X, A = to.tail_forward(x2, W1, b1, W2, b2, g3, b3, Wa, ba)
    return to.backward(x2, H, X, A, W2, b2, g3, Wa, Wb, bb, gt_rows, act, p, 1.0 / gt_rows.numel())


@pytest.mark.parametrize("act,p", CONFIGS)
@pytest.mark.parametrize("B,gh,gw,Cc", [(2, 5, 13, 128), (1, 1, 1, 64)])
def test_oracle_equals_autograd(B, gh, gw, Cc, act, p):
    """operand roundings off: the written-out formulas against fp64 autograd, 1e-12 relative Frobenius error per tensor"""
    x2, params, gt_rows = _case(B, gh, gw, Cc, act, p, seed=17 + Cc + act)
    r = _oracle(x2, params, gt_rows, act, p)
    loss, grads = th.autograd_tail(x2, params, ho.to_image(gt_rows, B, gh, gw, P), act, p, gh, gw, P)
    assert abs(float(r["loss"]) - float(loss)) <= 1e-12 * float(loss)
    for name, want in zip(to.KEYS, grads):
        assert th.rel_fro(r[name], want) <= 1e-12, name


@pytest.mark.parametrize("act,p", CONFIGS)
def test_oracle_adamw_equals_torch(act, p):
    """three steps of AdamW(lr 5e-4) + StepLR(2, 0.5) over the ten tensors: tailfit_oracle.fit against torch.optim.AdamW on autograd of the same
    tail in fp64.  The bound is test_headfit_host's: twice what torch's own fp32 run differs from its fp64 run by (per parameter), plus the
    fp32 storage of the change."""
    B, gh, gw, Cc = 2, 3, 5, 64
    x2, params, gt_rows = _case(B, gh, gw, Cc, act, p, seed=5)
    gt = ho.to_image(gt_rows, B, gh, gw, P)

    def torch_run(dtype):
        prm = [t.to(dtype).clone().requires_grad_(True) for t in params]
        opt = torch.optim.AdamW(prm, lr=5e-4)
        sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
        for _ in range(3):
            _, grads = th.autograd_tail(x2.to(dtype), [t.detach() for t in prm], gt.to(dtype), act, p, gh, gw, P)
            for t, g in zip(prm, grads):
                t.grad = g
            opt.step()
            sched.step()
        return [t.detach().double() - t0 for t, t0 in zip(prm, params)]

    d64, d32 = torch_run(F64), torch_run(torch.float32)
    _, got = to.fit(x2, params, gt_rows, act, p, steps=3, lr=5e-4, step_size=2, gamma=0.5)
    for k, name in enumerate(to.KEYS):
        dev = float((d32[k] - d64[k]).abs().max())
        err = (got[k] - params[k] - d64[k]).abs()
        assert float((err - (2.0 * dev + 2.0 ** -24 * d64[k].abs())).max()) <= 0, name


def test_ln_backward_properties():
    g = torch.Generator().manual_seed(3)
    M, Cc = 9, 64
    y = torch.randn((M, Cc), generator=g, dtype=F64) * 3 + 1
    dX = torch.randn((M, Cc), generator=g, dtype=F64)
    gamma = 1 + 0.3 * torch.randn((Cc,), generator=g, dtype=F64)
    y[4] = 2.5  # a constant row: zero variance, rstd = 1 / sqrt(eps)
    gamma[7] = 0.0
    r = to.ln_backward(y, dX, gamma, 1.0)
    dy, xhat = r["dy"], r["xhat"]
    scale = (r["rstd"] * (gamma * dX).abs().sum(1, keepdim=True)).squeeze(1)
    assert float((dy.sum(1).abs() / scale).max()) <= 64 * 2.0 ** -52          # sum_c dy = 0
    # sum_c dy xhat = 0 holds for eps = 0 (sum_c xhat^2 = C); with eps it is rstd^3 eps sum_c gamma dX xhat, since sum_c xhat^2 = C var rstd^2
    rest = (r["rstd"].squeeze(1) ** 3) * to.EPS * (gamma * dX * xhat).sum(1)
    assert float((((dy * xhat).sum(1) - rest).abs() / scale).max()) <= 64 * 2.0 ** -52
    keep = [m for m in range(M) if m != 4]
    r0 = to.ln_backward(y[keep], dX[keep], gamma, 1.0, eps=0.0)
    assert float(((r0["dy"] * r0["xhat"]).sum(1).abs() / scale[keep]).max()) <= 64 * 2.0 ** -52
    assert bool(torch.isfinite(dy).all()) and bool(torch.isfinite(r["dgamma"]).all())
    assert float(xhat[4].abs().max()) == 0.0
    # gamma_c = 0 takes column c out of dy: dX there changes nothing anywhere
    dX2 = dX.clone()
    dX2[:, 7] += 5.0
    assert torch.equal(to.ln_backward(y, dX2, gamma, 1.0)["dy"], dy)


def test_relu_zero_entries_get_no_gradient():
    act, p, B, gh, gw, Cc = 0, 1.0, 1, 2, 3, 64
    x2, params, gt_rows = _case(B, gh, gw, Cc, act, p, seed=9)
    W1, b1, W2, b2, g3, b3, Wa, ba, Wb, bb = params
    H, _, X, A = to.tail_forward(x2, *params[:8])
    assert int((H == 0).sum()) > 0 and int((H > 0).sum()) > 0
    r = to.backward(x2, H, X, A, W2, b2, g3, Wa, Wb, bb, gt_rows, act, p, 1.0)
    assert float(r["dHh"][H == 0].abs().max()) == 0.0 and float(r["dH"][H > 0].abs().min()) > 0.0
    # a unit whose activation is zero in every row gets no weight or bias gradient
    Hz = H.clone()
    Hz[:, 5] = 0.0
    rz = to.backward(x2, Hz, X, A, W2, b2, g3, Wa, Wb, bb, gt_rows, act, p, 1.0)
    assert float(rz["dW1"][5].abs().max()) == 0.0 and float(rz["db1"][5]) == 0.0 and float(rz["dW2"][:, 5].abs().max()) == 0.0


def test_fit_scope_option():
    from crossscore_amd.fit_head import check_config, fit_scope

    cfg = load_config("default_fit_head", [])
    check_config(cfg)
    assert fit_scope(cfg) == "head"
    del cfg["this_main"]["fit_scope"]  # no key at all: the head, as before
    check_config(cfg)
    assert fit_scope(cfg) == "head"
    for scope in ("head", "tail"):
        cfg = load_config("default_fit_head", [f"this_main.fit_scope={scope}"])
        check_config(cfg)
        assert fit_scope(cfg) == scope
    for bad in ("decoder", "Tail", ""):
        with pytest.raises(ValueError):
            check_config(load_config("default_fit_head", [f"this_main.fit_scope={bad}"]))


def test_tail_keys_and_options():
    net = CrossScoreNet(model_config(**{"backbone.from_pretrained": "synthetic/dinov2-tiny"}))
    keys = net.TAIL_KEYS
    last = f"ref_cross.attn.layers.{net.arch.dec_layers - 1}."
    assert len(keys) == 10 and keys[6:] == CrossScoreNet.HEAD_KEYS
    assert keys[:6] == tuple(last + k for k in ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm3.weight", "norm3.bias"))
    sd = net.state_dict()
    assert [tuple(p.shape) for p in net.tail_parameters()] == [tuple(sd[k].shape) for k in keys]
    st, gt = HeadFitState(), torch.zeros((1, 42, 42))
    with pytest.raises(ValueError):
        net.fit_tail_step(torch.zeros((1, 3, 42, 42)), None, gt, st)  # neither images nor tokens
    with pytest.raises(ValueError):
        net.fit_tail_step(torch.zeros((1, 3, 42, 42)), torch.zeros((1, 1, 3, 42, 42)), gt, st)  # parameters not on a device
    with pytest.raises(ValueError):
        CrossScoreNet(model_config(**{"backbone.from_pretrained": "synthetic/dinov2-tiny", "do_reference_cross": False})).tail_parameters()


TAILFIT_SYMBOLS = ("cs_tail_fit_supported", "cs_tail_fit_ln_row_tile", "cs_ln_backward_workspace_bytes", "cs_tail_backward_workspace_bytes",
                   "cs_op_ln_backward", "cs_op_tail_backward", "cs_fit_tail_keep", "cs_tail_backward", "cs_debug_tail_inputs", "cs_set_tail_weights")


def test_tailfit_listed_declared_and_bound():
    assert "tailfit.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "tailfit.hip"))
    header = open(os.path.join(REPO, "include", "crossscore_hip.h")).read()
    common = open(os.path.join(build.CSRC, "cs_common.h")).read()
    for name in TAILFIT_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SYMBOLS, name
    for launch in ("cs_ln_backward_launch", "cs_tail_backward_launch", "cs_transpose16_launch"):
        assert launch in common, launch
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.cs_tail_fit_supported(384, 14) == 1 and lib.cs_tail_fit_supported(1536, 14) == 1
        assert lib.cs_tail_fit_supported(96, 14) == 0 and lib.cs_tail_fit_supported(384, 16) == 0 and lib.cs_tail_fit_supported(4096, 14) == 0
        assert lib.cs_tail_fit_ln_row_tile() > 0
