"""The tail fit at the level of a whole module: cs_fit_tail_keep leaves every output bit of the forward alone; the two kept
tensors belong to one forward; cs_tail_backward is the single-op entry point on them bit for bit; the ten gradients against fp64 autograd of
the tail, measured with torch.autocast's own error on the same case (tests/golden/t0_tail_fit.npz, made by tests/golden/make_tail_fit.py);
fit_tail_step against the fp64 oracle's trajectory, the weight hand-back and sub-batches."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import headfit_oracle as ho  # noqa: E402
import tailfit_helpers as th  # noqa: E402
import tailfit_oracle as to  # noqa: E402
from bits16 import bits16, r16, same_bits, vals16  # noqa: E402
from hip_helpers import switches  # noqa: E402
from nets import SMALL, TINY, make_net  # noqa: E402
from crossscore_amd import _lib, synth  # noqa: E402
from crossscore_amd.model import HeadFitState, U8Batch, U8Image  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
U32 = 2.0 ** -24
P = 14
DTYPES = pytest.mark.parametrize("dtype", ["fp16", "bf16"])
NETS = {"tiny": (TINY, 2), "small": (SMALL, 1)}  # the golden's cases: backbone, reference views
# test_fit_tail_step: 3 x the largest relative deviation |loss - oracle| / oracle measured over the ten steps on the MI355X (3.6e-5 in fp16,
# 9.6e-5 in bf16), as the stage tests set theirs
TRAJECTORY_BOUND = {"fp16": 3 * 3.6e-5, "bf16": 3 * 9.6e-5}


def _inputs(B, N, H, W, seed):
    q, r = synth.make_inputs(B, N, H, W, seed)
    return torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()


def _gt_near(score, seed):
    g = torch.Generator().manual_seed(seed)
    off = (0.05 + 0.25 * torch.rand(score.shape, generator=g)) * torch.where(torch.rand(score.shape, generator=g) < 0.5, -1.0, 1.0)
    return (score.cpu() + off).cuda().contiguous()


def _u8_batch(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return U8Batch([U8Image(torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda(), H, W, (H, W)) for _ in range(n)], (H, W))


def _golden():
    return np.load(os.path.join(HERE, "golden", "t0_tail_fit.npz"))


@pytest.mark.parametrize("rowln", [1, 0])
@pytest.mark.parametrize("backbone,B,N,H,W,how", [(TINY, 2, 2, 42, 70, "forward"), (TINY, 2, 2, 28, 42, "cached"), (SMALL, 2, 1, 42, 70, "forward"),
                                                  (SMALL, 2, 1, 28, 42, "u8"), (SMALL, 2, 1, 42, 70, "cached")])
def test_keep_switch_leaves_the_forward_alone(backbone, B, N, H, W, how, rowln):
    net = make_net(backbone, 3, "fp16")[0]
    q, r = _inputs(B, N, H, W, 5)
    u8 = (_u8_batch(B, H, W, 1), _u8_batch(B * N, H, W, 2))

    def run():
        if how == "forward":
            res = net.forward(q, r, return_mean=True)
        elif how == "cached":
            tok = net.encode_references(r.reshape(B * N, 3, H, W)).reshape(B, N, -1, net.arch.hidden)
            res = net.forward_cached(q, tok, return_mean=True)
        else:
            res = net.forward(*u8, return_mean=True)
        return res["score_map_ref_cross"].clone(), res["score_mean_ref_cross"].clone(), net.forward_stats()["kernels"]

    with switches(rowln=rowln):
        s0, m0, c0 = run()
        assert "tail_keep" not in c0
        net.fit_tail_keep(True)
        s1, m1, c1 = run()
        x2, Hk = net.tail_inputs(B * (H // P) * (W // P))
        net.fit_tail_keep(False)
        s2, m2, c2 = run()
    assert torch.equal(s1, s0) and torch.equal(m1, m0) and torch.equal(s2, s0)
    assert c1 == {**c0, "tail_keep": 2} and c2 == c0
    assert bool(torch.isfinite(x2).all()) and int((Hk.view(torch.int16) == 0).sum()) > 0  # (ReLU rows: exact zeros)


@DTYPES
@pytest.mark.parametrize("rowln", [1, 0])
@pytest.mark.parametrize("tag", sorted(NETS))
def test_tail_inputs_belong_to_one_forward_and_backward_equals_op(tag, rowln, dtype):
    backbone, N = NETS[tag]
    bf16 = dtype == "bf16"
    B, H, W = 2, 42, 70
    gh, gw = H // P, W // P
    M = B * gh * gw
    net = make_net(backbone, 3, dtype)[0]
    q, r = _inputs(B, N, H, W, 5)
    net.fit_tail_keep(True)
    with switches(rowln=rowln):
        score = net(q, r)["score_map_ref_cross"]
    gt = _gt_near(score, 9)
    got = net.tail_backward(gt)
    x2, Hk = net.tail_inputs(M)
    X, A = net.head_inputs(M)
    W1, b1, W2, b2, g3, b3, Wa, ba, Wb, bb = th.tail_params(net)
    # H = relu(x2h W1^T + b1) of THIS forward: one 16-bit rounding of the output (2^-10 / 2^-7 of the largest pre-activation) on top of the
    # fp32 accumulation, the bound test_headfit_forward uses for the head's hidden rows
    pre = r16(x2.double().cpu(), bf16) @ r16(W1.double().cpu(), bf16).T + b1.double().cpu()
    H64 = vals16(Hk.view(torch.float16), bf16, F64).cpu()
    assert float((H64 - torch.relu(pre)).abs().max()) <= 2.0 ** (-7 if bf16 else -10) * float(pre.abs().max())
    # ... and X = norm3(x2 + H W2^T + b2) of the same forward, by the same bound on the normalised rows
    X64 = vals16(X.view(torch.float16), bf16, F64).cpu()
    y = x2.double().cpu() + H64 @ r16(W2.double().cpu(), bf16).T + b2.double().cpu()
    Xref = to.ln_stats(y)[2] * g3.double().cpu() + b3.double().cpu()
    assert float((X64 - Xref).abs().max()) <= 2.0 ** (-7 if bf16 else -10) * float(Xref.abs().max())
    with switches(bf16=bf16):
        want = th.tail_backward(x2, Hk.view(torch.float16), X.view(torch.float16), A.view(torch.float16), bits16(W2, bf16), b2, g3, bits16(Wa, bf16),
                                bits16(Wb, bf16), bb, gt, B, gh, gw, P, net._act, net._pow, 1.0 / gt.numel())
    torch.cuda.synchronize()
    for a, b, name in zip(got[:10], want[:10], to.KEYS):
        same_bits(a, b, name)
    assert float(got[10]) == float(want[10])
    head = net.head_backward(gt)  # the head's own entry on the same forward
    for a, b, name in zip(got[6:10], head[:4], to.KEYS[6:]):
        same_bits(a, b, name)


def test_state_errors():
    net = make_net(TINY, 3, "fp16")[0]
    lib = _lib.load()
    q, r = _inputs(2, 1, 42, 42, 5)
    h = net._ensure_handle(q.device)
    outs = th.fresh_outs(net.arch.hidden)
    gt = torch.zeros((3, 42, 42), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(B, H, W):
        return lib.cs_tail_backward(h, C.c_void_p(gt.data_ptr()), B, H, W, 1e-3, 0, *(C.c_void_p(t.data_ptr()) for t in outs), st)

    assert call(2, 42, 42) == _lib.CS_ERR_STATE  # no forward yet
    net(q, r)
    assert net._handle == h
    assert call(2, 42, 42) == _lib.CS_ERR_STATE  # a forward with the switch off
    assert lib.cs_debug_tail_inputs(h, None, None, 18, st) == _lib.CS_ERR_STATE
    net.fit_tail_keep(True)
    net(q, r)
    assert call(3, 42, 42) == _lib.CS_ERR_STATE and call(2, 42, 56) == _lib.CS_ERR_STATE  # another shape
    assert call(2, 42, 42) == 0
    net.encode_references(r.reshape(2, 3, 42, 42))
    assert call(2, 42, 42) == _lib.CS_ERR_STATE  # the last call only encoded
    net(q, r)
    net.fit_tail_keep(False)
    assert call(2, 42, 42) == 0  # the switch counts when the forward runs, not afterwards
    net(q, r)
    assert call(2, 42, 42) == _lib.CS_ERR_STATE
    torch.cuda.synchronize()
    for t in outs[:10]:
        assert bool(torch.isfinite(t).all())


@DTYPES
@pytest.mark.parametrize("tag", sorted(NETS))
def test_gradients_against_fp64_autograd(tag, dtype):
    """The golden's case: x2, H, X and A as a forward of this net left them on the device (tapped by tests/golden/make_tail_fit.py), through
    cs_op_tail_backward -- which cs_tail_backward equals bit for bit, see above -- against fp64 autograd of the tail on that x2: per tensor,
    relative Frobenius error at most twice torch.autocast's own on the same x2, weights and gt.  Both sides are dominated by the few ReLU and
    LeakyReLU masks that the 16-bit forward decides differently from fp64 (one such row moves a gradient by percents at M = 30).  Measured
    values: DESIGN.md 6, f16."""
    backbone, N = NETS[tag]
    bf16 = dtype == "bf16"
    g = _golden()
    B, gh, gw, P_ = (int(v) for v in g["shape"])
    net = make_net(backbone, 3, dtype)[0]
    x2 = torch.from_numpy(g[f"{tag}_{dtype}_x2"]).cuda()
    Hk, X, A = (torch.from_numpy(g[f"{tag}_{dtype}_{k}"]).cuda().view(torch.float16) for k in ("H", "X", "A"))
    gt = torch.from_numpy(g[f"{tag}_gt"]).cuda()
    W1, b1, W2, b2, g3, b3, Wa, ba, Wb, bb = th.tail_params(net)
    with switches(bf16=bf16):
        got = th.tail_backward(x2, Hk, X, A, bits16(W2, bf16), b2, g3, bits16(Wa, bf16), bits16(Wb, bf16), bb, gt, B, gh, gw, P_, net._act, net._pow,
                               1.0 / gt.numel())
    # the golden's taps are this net's: a forward now leaves the same rows (bit for bit when the taps were made) up to four unit roundoffs of
    # the operand type in relative Frobenius norm; a forward that drifts further needs new taps and a new yardstick (make_tail_fit.py)
    net.fit_tail_keep(True)
    q, r = _inputs(B, N, gh * P_, gw * P_, 5)
    net(q, r)
    assert th.rel_fro(net.tail_inputs(B * gh * gw)[0].cpu(), x2.cpu()) <= 4 * 2.0 ** (-8 if bf16 else -11)
    params = [t.double().cpu() for t in th.tail_params(net)]
    loss64, want = th.autograd_tail(x2.double().cpu(), params, gt.double().cpu(), net._act, net._pow, gh, gw, P_)
    assert abs(float(loss64) - float(g[f"{tag}_{dtype}_loss"])) <= 1e-12 * float(loss64)  # the case the yardstick was made on
    yard = g[f"{tag}_{dtype}_acerr"]
    for o, name, w, y in zip(got[:10], to.KEYS, want, yard):
        rel = th.rel_fro(o.cpu(), w)
        print(f"tail gradients {tag} {dtype} {name}: rel Frobenius {rel:.3e}, autocast's own {float(y):.3e}")
        assert rel <= 2.0 * float(y), name
    assert abs(float(got[10]) - float(loss64)) <= 2.0 * float(yard.max()) * float(loss64)


@DTYPES
def test_fit_tail_step(dtype):
    B, N, H, W = 2, 2, 42, 70
    gh, gw = H // P, W // P
    net = make_net(TINY, 3, dtype)[0]
    q, r = _inputs(B, N, H, W, 5)
    before = net(q, r)["score_map_ref_cross"].clone()
    census = net.forward_stats()["kernels"]
    handle = net._handle
    gt = _gt_near(before, 11)
    start = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net.fit_tail_keep(True)
    net(q, r)
    x2 = net.tail_inputs(B * gh * gw)[0].double().cpu()
    net.fit_tail_keep(False)
    want, _ = to.fit(x2, [t.double().cpu() for t in th.tail_params(net)], ho.to_rows(gt.double().cpu(), gh, gw, P), net._act, net._pow, steps=10, lr=5e-4)
    state = HeadFitState(lr=5e-4)
    got = [net.fit_tail_step(q, r, gt, state) for _ in range(10)]
    assert all(t.dtype == F64 and t.is_cuda and t.dim() == 0 for t in got)
    got = [float(t) for t in got]
    worst = 0.0
    for i, (a, b) in enumerate(zip(got, want)):
        worst = max(worst, abs(a - b) / b)
        print(f"tail fit step {i + 1} {dtype}: loss {a:.9f}, fp64 oracle {b:.9f}, relative deviation {abs(a - b) / b:.3e}")
    print(f"tail fit {dtype}: worst relative deviation {worst:.3e}, bound {TRAJECTORY_BOUND[dtype]:.3e}")
    assert worst <= TRAJECTORY_BOUND[dtype]
    assert got[-1] < got[0] and state.step == 10 and len(state.grads) == 10
    assert net._handle == handle and not net._dirty and not net._tail_keep  # the handle was kept; the switch is back off
    after = net(q, r)["score_map_ref_cross"].clone()
    assert net.forward_stats()["kernels"] == census
    assert not torch.equal(after, before)
    sd = net.state_dict()
    assert {k for k in sd if not torch.equal(sd[k], start[k])} == set(net.TAIL_KEYS)
    # hand-back: a fresh module built from the state dict scores the batch with the same bits
    fresh = make_net(TINY, 4, dtype)[0]
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in sd.items()}, strict=True)
    again = fresh.to("cuda")(q, r)["score_map_ref_cross"]
    assert torch.equal(again, after)


@DTYPES
def test_sub_batched_equals_unsplit(dtype):
    """fit_tail_step over two sub-batches (accumulate) against the unsplit batch: the gradients differ by the order of the fp32 row sums"""
    bf16 = dtype == "bf16"
    B, N, H, W = 3, 1, 42, 70
    gh, gw = H // P, W // P
    M = B * gh * gw
    q, r = _inputs(B, N, H, W, 5)
    grads, losses = [], []
    for split in (False, True):
        net = make_net(TINY, 3, dtype)[0]
        gt = _gt_near(net(q, r)["score_map_ref_cross"], 9)
        if split:
            net._sub_batches = lambda B_, N_, Np_: [(0, 1), (1, B_)]
        st = HeadFitState()
        if not split:
            net.fit_tail_keep(True)
            net(q, r)
            x2, Hk = net.tail_inputs(M)
            X, A = net.head_inputs(M)
            prm = [t.double().cpu() for t in th.tail_params(net)]
            net.fit_tail_keep(False)
        losses.append(float(net.fit_tail_step(q, r, gt, st)))
        grads.append([t.double().cpu() for t in st.grads])
    v16 = lambda t: vals16(t.view(torch.float16), bf16, F64).cpu()  # noqa: E731
    W1, b1, W2, b2, g3, b3, Wa, ba, Wb, bb = prm
    inv = 1.0 / gt.numel()
    ref = to.backward(x2.double().cpu(), v16(Hk), v16(X), v16(A), r16(W2, bf16), b2, g3, r16(Wa, bf16), r16(Wb, bf16), bb,
                      ho.to_rows(gt.double().cpu(), gh, gw, P), net._act, net._pow, inv, rnd=lambda t: r16(t, bf16))
    a_ = {k: ref[k].abs() for k in ("g", "dpre", "dyh", "dHh", "dX", "x2h")}
    sums = [a_["dHh"].T @ a_["x2h"], a_["dHh"].sum(0), a_["dyh"].T @ v16(Hk).abs(), a_["dyh"].sum(0), (ref["dX"] * ref["xhat"]).abs().sum(0),
            a_["dX"].sum(0), a_["dpre"].T @ v16(X).abs(), a_["dpre"].sum(0), a_["g"].T @ v16(A).abs(), a_["g"].sum(0)]
    for a, b, s, name in zip(grads[0], grads[1], sums, to.KEYS):
        assert float(((a - b).abs() - (2 * M * U32 * inv * s + 2 * U32 * a.abs())).max()) <= 0, name
    assert abs(losses[0] - losses[1]) <= 2.0 ** -50 * losses[0]
