"""The cross-attention fit at the level of a whole module: cs_fit_cross_keep leaves every output bit of the forward alone
and adds one copy to the census; what cross_inputs hands out belongs to one forward and is what a separate cs_op_attention gives; the
CS_ERR_STATE cases; the sixteen gradients against fp64 autograd of the block on the x1 the forward left, shown beside torch.autocast's own
error on the same inputs; fit_cross_step against the fp64 oracle's trajectory and against the tail's fit, and the weight hand-back."""
import ctypes as C
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import crossfit_helpers as ch  # noqa: E402
import crossfit_oracle as co  # noqa: E402
import headfit_oracle as ho  # noqa: E402
import tailfit_helpers as th  # noqa: E402
from bits16 import r16, same_bits, vals16  # noqa: E402
from hip_helpers import attention, switches  # noqa: E402
from nets import SMALL, TINY, make_net  # noqa: E402
from crossscore_amd import _lib, synth  # noqa: E402
from crossscore_amd.model import HeadFitState  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
P = 14
DTYPES = pytest.mark.parametrize("dtype", ["fp16", "bf16"])
NETS = {"tiny": (TINY, 2), "small": (SMALL, 1)}  # backbone, reference views
# test_fit_cross_step: 3 x the largest relative deviation |loss - oracle| / oracle measured over the ten steps on the MI355X
# (8.1e-5 in fp16, 1.4e-4 in bf16), as f15 and f16 set theirs
TRAJECTORY_BOUND = {"fp16": 3 * 8.1e-5, "bf16": 3 * 1.4e-4}


def _inputs(B, N, H, W, seed):
    q, r = synth.make_inputs(B, N, H, W, seed)
    return torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()


def _tokens(net, r):
    B, N, _, H, W = r.shape
    return net.encode_references(r.reshape(B * N, 3, H, W)).reshape(B, N, -1, net.arch.hidden)


def _gt_near(score, seed):
    g = torch.Generator().manual_seed(seed)
    off = (0.05 + 0.25 * torch.rand(score.shape, generator=g)) * torch.where(torch.rand(score.shape, generator=g) < 0.5, -1.0, 1.0)
    return (score.cpu() + off).cuda().contiguous()


@pytest.mark.parametrize("rowln", [1, 0])
@pytest.mark.parametrize("backbone,B,N,H,W,how", [(TINY, 2, 2, 42, 70, "forward"), (TINY, 2, 2, 28, 42, "cached"), (SMALL, 2, 1, 42, 70, "forward"),
                                                  (SMALL, 2, 1, 42, 70, "cached")])
def test_keep_switch_leaves_the_forward_alone(backbone, B, N, H, W, how, rowln):
    net = make_net(backbone, 3, "fp16")[0]
    q, r = _inputs(B, N, H, W, 5)

    def run():
        if how == "forward":
            res = net.forward(q, r, need_attn_weights=True, return_mean=True)
        else:
            res = net.forward_cached(q, _tokens(net, r), need_attn_weights=True, return_mean=True)
        return (res["score_map_ref_cross"].clone(), res["score_mean_ref_cross"].clone(), res["attn_weights_map_ref_cross"].clone(),
                net.forward_stats()["kernels"])

    with switches(rowln=rowln):
        s0, m0, a0, c0 = run()
        assert "cross_keep" not in c0 and "tail_keep" not in c0
        net.fit_cross_keep(True)
        s1, m1, a1, c1 = run()
        x1 = net.cross_inputs(B * (H // P) * (W // P), N)[0]
        net.fit_cross_keep(False)
        s2, m2, a2, c2 = run()
    assert torch.equal(s1, s0) and torch.equal(m1, m0) and torch.equal(a1, a0) and torch.equal(s2, s0) and torch.equal(a2, a0)
    assert c1 == {**c0, "tail_keep": 2, "cross_keep": 1} and c2 == c0
    assert bool(torch.isfinite(x1).all())


@DTYPES
@pytest.mark.parametrize("rowln", [1, 0])
@pytest.mark.parametrize("tag", sorted(NETS))
def test_cross_inputs_belong_to_one_forward(tag, rowln, dtype):
    """Q' is the folded projection of the kept x1, K and V are the projections of the reference tokens (one 16-bit rounding each on top of the
    fp32 accumulation), O and lse are what cs_op_attention gives on those Q', K, V bit for bit, and x2 = norm2(x1 + O Wo^T + bo)"""
    backbone, N = NETS[tag]
    bf16 = dtype == "bf16"
    B, H, W = 2, 42, 70
    M = B * (H // P) * (W // P)
    net = make_net(backbone, 3, dtype)[0]
    Cc, h = net.arch.hidden, net.arch.dec_heads
    q, r = _inputs(B, N, H, W, 5)
    tok = _tokens(net, r)
    net.fit_cross_keep(True)
    with switches(rowln=rowln):
        net.forward_cached(q, tok)
    x1, Qp, O, lse, K, V = net.cross_inputs(M, N)
    x2 = net.tail_inputs(M)[0]
    e16 = 2.0 ** (-7 if bf16 else -10)
    v16 = lambda t: vals16(t.view(torch.float16), bf16, F64).cpu()  # noqa: E731
    Win, bin_, Wo, bo, g2, be2 = (t.double().cpu() for t in net.cross_parameters()[:6])
    c = co.LOG2E / (Cc // h) ** 0.5
    mem = v16(tok.reshape(-1, Cc))
    pre_q = r16(x1.double().cpu(), bf16) @ r16(c * Win[:Cc], bf16).T + c * bin_[:Cc]
    assert float((v16(Qp) - pre_q).abs().max()) <= e16 * float(pre_q.abs().max())
    for got, rows in ((K, slice(Cc, 2 * Cc)), (V, slice(2 * Cc, 3 * Cc))):
        pre = mem @ r16(Win[rows], bf16).T + bin_[rows]
        assert float((v16(got) - pre).abs().max()) <= e16 * float(pre.abs().max())
    with switches(bf16=bf16):
        O2, lse2 = attention(Qp.view(torch.float16).reshape(B, -1, Cc), K.view(torch.float16).reshape(B, -1, Cc), V.view(torch.float16).reshape(B, -1, Cc),
                             h, Cc // h, lse=True, q_scale=1.0)
    same_bits(O2.reshape(M, Cc), O.view(torch.float16), "O")
    same_bits(lse2.reshape(-1), lse, "lse")
    y2 = x1.double().cpu() + v16(O) @ r16(Wo, bf16).T + bo
    import tailfit_oracle as to
    _, rstd, xhat = to.ln_stats(y2)
    want = xhat * g2 + be2
    # the forward's own fp32 evaluation: (C + 2) 2^-24 of the sum of magnitudes in y2, three times that through the LayerNorm (the row's mean and
    # variance move with it), and a few roundings of the normalised row
    dy = (Cc + 2) * 2.0 ** -24 * float((x1.double().cpu().abs() + v16(O).abs() @ r16(Wo, bf16).abs().T + bo.abs()).max())
    assert float((x2.double().cpu() - want).abs().max()) <= 3 * dy * float(rstd.max()) * float(g2.abs().max()) + 8 * 2.0 ** -24 * float(want.abs().max())


def test_state_errors():
    net = make_net(TINY, 3, "fp16")[0]
    lib = _lib.load()
    q, r = _inputs(2, 1, 42, 42, 5)
    h = net._ensure_handle(q.device)
    outs = ch.cross_outs(net.arch.hidden)
    gt = torch.zeros((3, 42, 42), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(B, H, W):
        return lib.cs_cross_backward(h, C.c_void_p(gt.data_ptr()), B, H, W, 1e-3, 0, *(C.c_void_p(t.data_ptr()) for t in outs), st)

    assert call(2, 42, 42) == _lib.CS_ERR_STATE  # no forward yet
    net(q, r)
    assert net._handle == h
    assert call(2, 42, 42) == _lib.CS_ERR_STATE  # a forward with the switch off
    assert lib.cs_debug_cross_inputs(h, None, None, None, None, None, None, 18, st) == _lib.CS_ERR_STATE
    net.fit_tail_keep(True)
    net(q, r)
    assert call(2, 42, 42) == _lib.CS_ERR_STATE  # the tail's switch alone is not enough
    net.fit_tail_keep(False)
    net.fit_cross_keep(True)
    net(q, r)
    assert call(3, 42, 42) == _lib.CS_ERR_STATE and call(2, 42, 56) == _lib.CS_ERR_STATE  # another shape
    assert call(2, 42, 42) == 0
    tail_outs = th.fresh_outs(net.arch.hidden)  # the cross switch implies the tail's
    assert lib.cs_tail_backward(h, C.c_void_p(gt.data_ptr()), 2, 42, 42, 1e-3, 0, *(C.c_void_p(t.data_ptr()) for t in tail_outs), st) == 0
    net.encode_references(r.reshape(2, 3, 42, 42))
    assert call(2, 42, 42) == _lib.CS_ERR_STATE  # the last call only encoded
    net(q, r)
    net.fit_cross_keep(False)
    assert call(2, 42, 42) == 0  # the switch counts when the forward runs, not afterwards
    net(q, r)
    assert call(2, 42, 42) == _lib.CS_ERR_STATE
    torch.cuda.synchronize()
    for t in outs[:16]:
        assert bool(torch.isfinite(t).all())
    for a, b in zip(outs[6:16], tail_outs[:10]):
        assert torch.equal(a, b)


def _block_case(net, x1, mem, gt, B, gh, gw, dtype=F64):
    """the dict crossfit_helpers.autograd_block takes, from a module's own sixteen tensors"""
    c = {k: t.detach().to(dtype).cpu() for k, t in zip(co.PARAMS, net.cross_parameters())}
    c.update(x1=x1.to(dtype).cpu(), mem=mem.to(dtype).cpu(), gt_rows=ho.to_rows(gt.to(dtype).cpu(), gh, gw, P), B=B, C=net.arch.hidden, h=net.arch.dec_heads,
             gh=gh, gw=gw, act=net._act, p=net._pow, short_cut=True)
    return c


@DTYPES
@pytest.mark.parametrize("tag", sorted(NETS))
def test_gradients_against_fp64_autograd(tag, dtype):
    """cs_cross_backward on a forward of this net against fp64 autograd of the block (F.multi_head_attention_forward, the residual, norm2, the tail
    and the head) on the x1 that forward left and the reference tokens it read: per tensor, relative Frobenius error at most twice
    torch.autocast's own on the same x1, tokens, weights and gt (fp16 with the loss scaled by 1024, as a GradScaler does).  Both sides are
    dominated by the few ReLU and LeakyReLU masks the 16-bit forward decides differently from fp64.  Measured values: DESIGN.md 6, f17."""
    backbone, N = NETS[tag]
    bf16 = dtype == "bf16"
    B, H, W = 2, 42, 70
    gh, gw = H // P, W // P
    M = B * gh * gw
    net = make_net(backbone, 3, dtype)[0]
    Cc = net.arch.hidden
    q, r = _inputs(B, N, H, W, 5)
    tok = _tokens(net, r)
    net.fit_cross_keep(True)
    score = net.forward_cached(q, tok)["score_map_ref_cross"]
    gt = _gt_near(score, 9)
    got = net.cross_backward(gt)
    x1 = net.cross_inputs(M, N)[0]
    mem = vals16(tok.reshape(-1, Cc).view(torch.float16), bf16, F64)
    loss64, want = ch.autograd_block(_block_case(net, x1.double(), mem, gt, B, gh, gw))
    half = torch.bfloat16 if bf16 else torch.float16
    _, cast = ch.autograd_block(_block_case(net, x1, mem, gt, B, gh, gw, torch.float32), autocast=half, loss_scale=1.0 if bf16 else 1024.0)
    for o, name, w, a in zip(got[:16], co.KEYS, want, cast):
        rel, yard = th.rel_fro(o.cpu(), w), th.rel_fro(a, w)
        print(f"cross gradients {tag} {dtype} {name}: rel Frobenius {rel:.3e}, autocast's own {yard:.3e}")
        assert rel <= 2.0 * yard, name
    assert abs(float(got[16]) - float(loss64)) <= 0.1 * float(loss64)


@DTYPES
def test_fit_cross_step(dtype):
    bf16 = dtype == "bf16"
    B, N, H, W = 2, 2, 42, 70
    gh, gw = H // P, W // P
    M = B * gh * gw
    net = make_net(TINY, 3, dtype)[0]
    Cc = net.arch.hidden
    q, r = _inputs(B, N, H, W, 5)
    tok = _tokens(net, r)
    before = net.forward_cached(q, tok)["score_map_ref_cross"].clone()
    census = net.forward_stats()["kernels"]
    handle = net._handle
    gt = _gt_near(before, 11)
    start = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net.fit_cross_keep(True)
    net.forward_cached(q, tok)
    x1 = net.cross_inputs(M, N)[0].double().cpu()
    net.fit_cross_keep(False)
    mem = vals16(tok.reshape(-1, Cc).view(torch.float16), bf16, F64).cpu()
    want, _ = co.fit(x1, mem, [t.detach().double().cpu() for t in net.cross_parameters()], ho.to_rows(gt.double().cpu(), gh, gw, P), net._act, net._pow,
                     B, net.arch.dec_heads, steps=10, lr=5e-4)
    state = HeadFitState(lr=5e-4)
    got = [net.fit_cross_step(q, None, gt, state, ref_tokens=tok) for _ in range(10)]
    assert all(t.dtype == F64 and t.is_cuda and t.dim() == 0 for t in got)
    got = [float(t) for t in got]
    worst = 0.0
    for i, (a, b) in enumerate(zip(got, want)):
        worst = max(worst, abs(a - b) / b)
        print(f"cross fit step {i + 1} {dtype}: loss {a:.9f}, fp64 oracle {b:.9f}, relative deviation {abs(a - b) / b:.3e}")
    print(f"cross fit {dtype}: worst relative deviation {worst:.3e}, bound {TRAJECTORY_BOUND[dtype]:.3e}")
    assert worst <= TRAJECTORY_BOUND[dtype]
    assert got[-1] < got[0] and state.step == 10 and len(state.grads) == 16
    assert net._handle == handle and not net._dirty and not net._cross_keep and not net._tail_keep  # the handle was kept; the switches are back off
    after = net.forward_cached(q, tok)["score_map_ref_cross"].clone()
    assert net.forward_stats()["kernels"] == census
    assert not torch.equal(after, before)
    sd = net.state_dict()
    assert {k for k in sd if not torch.equal(sd[k], start[k])} == set(net.CROSS_KEYS)
    # hand-back: a fresh module built from the state dict scores the batch with the same bits
    fresh = make_net(TINY, 4, dtype)[0]
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in sd.items()}, strict=True)
    again = fresh.to("cuda").forward_cached(q, tok)["score_map_ref_cross"]
    assert torch.equal(again, after)
    # the same ten steps over the tail alone, from the same start on the same batch, end above the sixteen tensors' loss
    tail_net = make_net(TINY, 3, dtype)[0]
    tail_state = HeadFitState(lr=5e-4)
    tail = [float(tail_net.fit_tail_step(q, None, gt, tail_state, ref_tokens=tok)) for _ in range(10)]
    print(f"cross fit {dtype}: loss before the tenth step {got[-1]:.9f}, the tail's {tail[-1]:.9f}")
    assert tail[0] == got[0] and got[-1] < tail[-1]


@DTYPES
def test_fit_cross_step_with_images_and_sub_batches(dtype):
    """the references as images, and the batch in two sub-batches (accumulate): the loss of the step is the unsplit one to fp64 rounding, the
    gradients differ by the order of fp32 row sums only"""
    B, N, H, W = 3, 1, 42, 70
    q, r = _inputs(B, N, H, W, 5)
    grads, losses = [], []
    for split in (False, True):
        net = make_net(TINY, 3, dtype)[0]
        gt = _gt_near(net(q, r)["score_map_ref_cross"], 9)
        if split:
            net._sub_batches = lambda B_, N_, Np_: [(0, 1), (1, B_)]
        st = HeadFitState()
        losses.append(float(net.fit_cross_step(q, r, gt, st)))
        grads.append([t.double().cpu() for t in st.grads])
    assert abs(losses[0] - losses[1]) <= 2.0 ** -50 * losses[0]
    # (the two runs add the same fp32 row terms in another order: 2 M 2^-24 = 6e-6 of the sums of magnitudes, which the op tests bound rigorously;
    #  here 1e-3 of each tensor's norm is granted for the cancellation inside the sums)
    for a, b, name in zip(grads[0], grads[1], co.KEYS):
        assert float((a - b).norm()) <= 1e-3 * float(a.norm()), name
