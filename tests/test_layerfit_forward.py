"""The whole-layer fit at the level of a whole module: cs_fit_layer_keep leaves every output bit of the forward alone and adds
only its copies to the census; what layer_inputs hands out is the self-attention's own output and lse (not the cross-attention's, which
overwrite them in the workspace); layer_backward agrees with cross_backward on the inner scopes bit for bit and writes no kept input; the
CS_ERR_STATE case; the six new gradients against fp64 autograd of the layer on the x0 the forward left, beside torch.autocast's own error;
fit_layer_step against the fp64 trajectory, beside eager autocast's own deviation; and the weight hand-back."""
import ctypes as C
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import headfit_oracle as ho  # noqa: E402
import layerfit_helpers as lh  # noqa: E402
import layerfit_oracle as lo  # noqa: E402
import tailfit_helpers as th  # noqa: E402
from bits16 import same_bits, vals16  # noqa: E402
from hip_helpers import attention, switches  # noqa: E402
from nets import SMALL, TINY, make_net  # noqa: E402
from crossscore_amd import _lib, synth  # noqa: E402
from crossscore_amd.model import HeadFitState  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
P = 14
DTYPES = pytest.mark.parametrize("dtype", ["fp16", "bf16"])
NETS = {"tiny": (TINY, 2), "small": (SMALL, 1)}  # backbone, reference views
B, H, W = 2, 42, 70  # M = 30
GH, GW = H // P, W // P
M = B * GH * GW


def _inputs(N, seed=5):
    q, r = synth.make_inputs(B, N, H, W, seed)
    return torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()


def _tokens(net, r):
    Bn, N = r.shape[:2]
    return net.encode_references(r.reshape(Bn * N, 3, H, W)).reshape(Bn, N, -1, net.arch.hidden)


def _gt_near(score, seed):
    g = torch.Generator().manual_seed(seed)
    off = (0.05 + 0.25 * torch.rand(score.shape, generator=g)) * torch.where(torch.rand(score.shape, generator=g) < 0.5, -1.0, 1.0)
    return (score.cpu() + off).cuda().contiguous()


@pytest.mark.parametrize("rowln", [1, 0])
@pytest.mark.parametrize("how", ["forward", "cached"])
@pytest.mark.parametrize("tag", sorted(NETS))
def test_keep_switch_leaves_the_forward_alone(tag, how, rowln):
    backbone, N = NETS[tag]
    net = make_net(backbone, 3, "fp16")[0]
    q, r = _inputs(N)

    def run():
        if how == "forward":
            res = net.forward(q, r, need_attn_weights=True, return_mean=True)
        else:
            res = net.forward_cached(q, _tokens(net, r), need_attn_weights=True, return_mean=True)
        return (res["score_map_ref_cross"].clone(), res["score_mean_ref_cross"].clone(), res["attn_weights_map_ref_cross"].clone(),
                net.forward_stats()["kernels"])

    with switches(rowln=rowln):
        s0, m0, a0, c0 = run()
        assert not any(k.endswith("_keep") for k in c0)
        net.fit_layer_keep(True)
        s1, m1, a1, c1 = run()
        x0 = net.layer_inputs(M)[0]
        net.fit_layer_keep(False)
        s2, m2, a2, c2 = run()
    assert torch.equal(s1, s0) and torch.equal(m1, m0) and torch.equal(a1, a0) and torch.equal(s2, s0) and torch.equal(m2, m0) and torch.equal(a2, a0)
    assert c1 == {**c0, "tail_keep": 2, "cross_keep": 1, "layer_keep": 2} and c2 == c0
    assert bool(torch.isfinite(x0).all())


@DTYPES
@pytest.mark.parametrize("rowln", [1, 0])
@pytest.mark.parametrize("tag", sorted(NETS))
def test_layer_inputs_are_the_self_attentions(tag, rowln, dtype):
    """Os and lse_s are what cs_op_attention gives on the returned Qs', Ks, Vs bit for bit -- the cross-attention's output and lse, which sit in
    the same workspace buffers by the end of the forward, are not (they are compared too: they differ) -- and x1 = norm1(x0 + Os Wo_s^T + bo_s)"""
    backbone, N = NETS[tag]
    bf16 = dtype == "bf16"
    net = make_net(backbone, 3, dtype)[0]
    Cc, h = net.arch.hidden, net.arch.dec_heads
    q, r = _inputs(N)
    tok = _tokens(net, r)
    net.fit_layer_keep(True)
    with switches(rowln=rowln):
        net.forward_cached(q, tok)
    x0, Qs, Ks, Vs, Os, lse_s = net.layer_inputs(M)
    x1, _, O, lse = net.cross_inputs(M, N)[:4]
    f16 = lambda t: t.view(torch.float16).reshape(B, -1, Cc)  # noqa: E731
    with switches(bf16=bf16):
        O2, lse2 = attention(f16(Qs), f16(Ks), f16(Vs), h, Cc // h, lse=True, q_scale=1.0)
    same_bits(O2.reshape(M, Cc), Os.view(torch.float16), "Os")
    same_bits(lse2.reshape(-1), lse_s, "lse_s")
    assert not torch.equal(Os.view(torch.int16), O.view(torch.int16)) and not torch.equal(lse_s, lse)
    v16 = lambda t: vals16(t.view(torch.float16), bf16, F64).cpu()  # noqa: E731
    Wo_s, bo_s, g1, be1 = (t.double().cpu() for t in net.layer_parameters()[2:6])
    from bits16 import r16
    import tailfit_oracle as to
    y1 = x0.double().cpu() + v16(Os) @ r16(Wo_s, bf16).T + bo_s
    _, rstd, xhat = to.ln_stats(y1)
    want = xhat * g1 + be1
    # the forward's own fp32 evaluation, as test_crossfit_forward prices it for x2
    dy = (Cc + 2) * 2.0 ** -24 * float((x0.double().cpu().abs() + v16(Os).abs() @ r16(Wo_s, bf16).abs().T + bo_s.abs()).max())
    assert float((x1.double().cpu() - want).abs().max()) <= 3 * dy * float(rstd.max()) * float(g1.abs().max()) + 8 * 2.0 ** -24 * float(want.abs().max())


@DTYPES
@pytest.mark.parametrize("tag", sorted(NETS))
def test_nested_agreement_and_kept_inputs_untouched(tag, dtype):
    """on one forward: layer_backward's last seventeen outputs are cross_backward's bit for bit, two calls agree, and no kept input changes"""
    backbone, N = NETS[tag]
    net = make_net(backbone, 3, dtype)[0]
    q, r = _inputs(N)
    tok = _tokens(net, r)
    net.fit_layer_keep(True)
    gt = _gt_near(net.forward_cached(q, tok)["score_map_ref_cross"], 9)
    kept = [t.clone() for t in net.layer_inputs(M) + net.cross_inputs(M, N) + net.tail_inputs(M) + net.head_inputs(M)]
    layer = [t.clone() for t in net.layer_backward(gt)]
    cross = [t.clone() for t in net.cross_backward(gt)]
    again = net.layer_backward(gt)
    after = net.layer_inputs(M) + net.cross_inputs(M, N) + net.tail_inputs(M) + net.head_inputs(M)
    assert len(layer) == 23 and len(cross) == 17
    for a, b, name in zip(layer[6:], cross, lo.KEYS[6:] + ("loss",)):
        assert torch.equal(a, b), name
    for a, b, name in zip(layer, again, lo.KEYS + ("loss",)):
        assert torch.equal(a, b), name
    for a, b in zip(kept, after):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for t in layer[:6]:
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0


def test_state_errors():
    net = make_net(TINY, 3, "fp16")[0]
    lib = _lib.load()
    q, r = _inputs(1)
    h = net._ensure_handle(q.device)
    outs = [torch.full(s, 7.0, device="cuda") for s in lh.layer_shapes(net.arch.hidden)] + [torch.full((), 7.0, dtype=F64, device="cuda")]
    gt = torch.zeros((B, H, W), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(Bn=B):
        return lib.cs_layer_backward(h, C.c_void_p(gt.data_ptr()), Bn, H, W, 1e-3, 0, *(C.c_void_p(t.data_ptr()) for t in outs), st)

    assert call() == _lib.CS_ERR_STATE  # no forward yet
    net.fit_cross_keep(True)
    net(q, r)
    assert net._handle == h
    assert call() == _lib.CS_ERR_STATE  # the cross switch alone is not enough
    assert lib.cs_debug_layer_inputs(h, None, None, None, None, None, None, M, st) == _lib.CS_ERR_STATE
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs)
    net.fit_cross_keep(False)
    net.fit_layer_keep(True)
    net(q, r)
    assert call(B + 1) == _lib.CS_ERR_STATE  # another shape
    assert call() == 0
    assert len(net.cross_backward(gt)) == 17  # the layer switch implies the cross switch's copies
    net.fit_layer_keep(False)
    net(q, r)
    assert call() == _lib.CS_ERR_STATE
    torch.cuda.synchronize()


def _layer_case(net, x0, mem, gt, dtype=F64):
    """the dict layerfit_helpers.autograd_layer takes, from a module's own twenty-two tensors"""
    c = {k: t.detach().to(dtype).cpu() for k, t in zip(lo.PARAMS, net.layer_parameters())}
    c.update(x0=x0.to(dtype).cpu(), mem=mem.to(dtype).cpu(), gt_rows=ho.to_rows(gt.to(dtype).cpu(), GH, GW, P), B=B, C=net.arch.hidden,
             h=net.arch.dec_heads, gh=GH, gw=GW, act=net._act, p=net._pow, short_cut=True)
    return c


@DTYPES
@pytest.mark.parametrize("tag", sorted(NETS))
def test_gradients_against_fp64_autograd(tag, dtype):
    """cs_layer_backward on a forward of this net against fp64 autograd of the last layer (self-attention, residual, norm1, the cross-attention
    block, the tail and the head) on the x0 that forward left and the reference tokens it read: for each of the six new tensors, relative
    Frobenius error at most twice torch.autocast's own on the same x0, tokens, weights and gt (fp16 with the loss scaled by 1024, as a
    GradScaler does) -- the bound test_crossfit_forward.py uses for the same comparison.  Measured values: DESIGN.md 6, f18."""
    backbone, N = NETS[tag]
    bf16 = dtype == "bf16"
    net = make_net(backbone, 3, dtype)[0]
    Cc = net.arch.hidden
    q, r = _inputs(N)
    tok = _tokens(net, r)
    net.fit_layer_keep(True)
    score = net.forward_cached(q, tok)["score_map_ref_cross"]
    gt = _gt_near(score, 9)
    got = net.layer_backward(gt)
    x0 = net.layer_inputs(M)[0]
    mem = vals16(tok.reshape(-1, Cc).view(torch.float16), bf16, F64)
    loss64, want = lh.autograd_layer(_layer_case(net, x0.double(), mem, gt))
    half = torch.bfloat16 if bf16 else torch.float16
    _, cast = lh.autograd_layer(_layer_case(net, x0, mem, gt, torch.float32), autocast=half, loss_scale=1.0 if bf16 else 1024.0)
    ratios = []
    for o, name, w, a in zip(got[:6], lo.KEYS, want, cast):
        rel, yard = th.rel_fro(o.cpu(), w), th.rel_fro(a, w)
        ratios.append((name, rel, yard))
        print(f"layer gradients {tag} {dtype} {name}: rel Frobenius {rel:.3e}, autocast's own {yard:.3e}, ratio {rel / yard:.3f}")
    for name, rel, yard in ratios:
        assert rel <= 2.0 * yard, name
    assert abs(float(got[22]) - float(loss64)) <= 0.1 * float(loss64)


def _autocast_trajectory(case32, half, loss_scale, steps, lr):
    """the same AdamW steps in eager PyTorch: fp32 master tensors, every forward and backward under torch.autocast -> losses before each step"""
    params = [case32[k].clone() for k in lo.PARAMS]
    m = [torch.zeros_like(t) for t in params]
    v = [torch.zeros_like(t) for t in params]
    losses = []
    for t in range(1, steps + 1):
        c = dict(case32, **dict(zip(lo.PARAMS, params)))
        loss, grads = lh.autograd_layer(c, autocast=half, loss_scale=loss_scale)
        losses.append(float(loss))
        for k in range(len(params)):
            params[k], m[k], v[k] = ho.adamw_step(params[k], m[k], v[k], grads[k].float(), t, lr=lr)
    return losses


@DTYPES
def test_fit_layer_step(dtype):
    """ten fit_layer_steps on one batch follow the fp64 trajectory of the loss at most twice as far off as eager autocast's own ten steps do;
    the loss falls; exactly the twenty-two tensors change; a fresh module built from them scores the batch with the same bits"""
    bf16 = dtype == "bf16"
    N = 2
    net = make_net(TINY, 3, dtype)[0]
    Cc = net.arch.hidden
    q, r = _inputs(N)
    tok = _tokens(net, r)
    before = net.forward_cached(q, tok)["score_map_ref_cross"].clone()
    census = net.forward_stats()["kernels"]
    handle = net._handle
    gt = _gt_near(before, 11)
    start = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net.fit_layer_keep(True)
    net.forward_cached(q, tok)
    x0 = net.layer_inputs(M)[0]
    net.fit_layer_keep(False)
    mem = vals16(tok.reshape(-1, Cc).view(torch.float16), bf16, F64).cpu()
    gt_rows = ho.to_rows(gt.double().cpu(), GH, GW, P)
    want, _ = lo.fit(x0.double().cpu(), mem, [t.detach().double().cpu() for t in net.layer_parameters()], gt_rows, net._act, net._pow, B,
                     net.arch.dec_heads, steps=10, lr=5e-4)
    eager = _autocast_trajectory(_layer_case(net, x0, mem, gt, torch.float32), torch.bfloat16 if bf16 else torch.float16, 1.0 if bf16 else 1024.0, 10, 5e-4)
    state = HeadFitState(lr=5e-4)
    got = [net.fit_layer_step(q, None, gt, state, ref_tokens=tok) for _ in range(10)]
    assert all(t.dtype == F64 and t.is_cuda and t.dim() == 0 for t in got)
    got = [float(t) for t in got]
    worst = max(abs(a - b) / b for a, b in zip(got, want))
    yard = max(abs(a - b) / b for a, b in zip(eager, want))
    for i, (a, e, b) in enumerate(zip(got, eager, want)):
        print(f"layer fit step {i + 1} {dtype}: loss {a:.9f}, eager autocast {e:.9f}, fp64 {b:.9f}")
    print(f"layer fit {dtype}: worst relative deviation {worst:.3e}, eager autocast's own {yard:.3e}, ratio {worst / yard:.3f}")
    assert worst <= 2.0 * yard
    assert got[-1] == got[-1] and abs(got[-1]) < float("inf") and got[-1] < got[0]
    assert state.step == 10 and len(state.grads) == 22
    assert net._handle == handle and not net._dirty and not net._layer_keep and not net._cross_keep and not net._tail_keep
    after = net.forward_cached(q, tok)["score_map_ref_cross"].clone()
    assert net.forward_stats()["kernels"] == census
    assert not torch.equal(after, before)
    sd = net.state_dict()
    assert {k for k in sd if not torch.equal(sd[k], start[k])} == set(net.LAYER_KEYS)
    # hand-back: a fresh module built from the same fp32 tensors scores the batch with the same bits
    fresh = make_net(TINY, 4, dtype)[0]
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in sd.items()}, strict=True)
    again = fresh.to("cuda").forward_cached(q, tok)["score_map_ref_cross"]
    assert torch.equal(again, after)
