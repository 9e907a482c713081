"""The head fit at the level of a whole module: cs_head_backward over what a forward left behind, against the single-op
entry point on the same tokens bit for bit; its loss against the forward's own score map; gradients against the goldens made from the reference's
head, measured with the reference's own mixed-precision error; fit_head_step against the fp64 oracle's trajectory, and the weight hand-back."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import headfit_helpers as hh  # noqa: E402
import headfit_oracle as ho  # noqa: E402
from bits16 import bits16, r16, same_bits, vals16  # noqa: E402
from hip_helpers import switches  # noqa: E402
from nets import SMALL, TINY, make_net  # noqa: E402
from crossscore_amd import _lib, synth  # noqa: E402
from crossscore_amd.model import HeadFitState, U8Batch, U8Image, load_lightning_checkpoint, save_lightning_checkpoint  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
U32 = 2.0 ** -24
P = 14
DTYPES = pytest.mark.parametrize("dtype", ["fp16", "bf16"])
GOLDEN_CONFIGS = {"c0": (0, 1.0), "c1": (0, 2.0), "c2": (1, 1.0)}
KEYS = ("Wa", "ba", "Wb", "bb")


def _inputs(B, N, H, W, seed):
    q, r = synth.make_inputs(B, N, H, W, seed)
    return torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()


def _gt_near(score, seed):
    """a ground truth 0.05 .. 0.3 away from the score map everywhere: no sign of s - gt is in doubt"""
    g = torch.Generator().manual_seed(seed)
    off = (0.05 + 0.25 * torch.rand(score.shape, generator=g)) * torch.where(torch.rand(score.shape, generator=g) < 0.5, -1.0, 1.0)
    return (score.cpu() + off).cuda().contiguous()


def _head(net):
    return [p.detach() for p in net.head_parameters()]


def _u8_batch(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return U8Batch([U8Image(torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda(), H, W, (H, W)) for _ in range(n)], (H, W))


@DTYPES
@pytest.mark.parametrize("backbone,B,N,how", [(TINY, 2, 2, "forward"), (TINY, 2, 2, "cached"), (SMALL, 2, 1, "forward"), (SMALL, 2, 1, "u8")])
def test_backward_equals_op_on_the_forwards_tokens(backbone, B, N, how, dtype):
    H, W = 42, 70  # a 3 x 5 grid
    bf16 = dtype == "bf16"
    net = make_net(backbone, 3, dtype)[0]
    q, r = _inputs(B, N, H, W, 5)
    if how == "forward":
        score = net(q, r)["score_map_ref_cross"]
    elif how == "cached":
        tok = net.encode_references(r.reshape(B * N, 3, H, W)).reshape(B, N, -1, net.arch.hidden)
        score = net.forward_cached(q, tok)["score_map_ref_cross"]
    else:
        score = net.forward(_u8_batch(B, H, W, 1), _u8_batch(B * N, H, W, 2))["score_map_ref_cross"]
    gh, gw, Cc = H // P, W // P, net.arch.hidden
    M = B * gh * gw
    gt = _gt_near(score, 9)
    got = net.head_backward(gt)
    X, A = net.head_inputs(M)
    Wa, ba, Wb, bb = _head(net)
    with switches(bf16=bf16):
        want = hh.head_backward(X.view(torch.float16), A.view(torch.float16), bits16(Wb, bf16), bb, gt, B, gh, gw, P, net._act, net._pow,
                                1.0 / gt.numel())
    torch.cuda.synchronize()
    for a, b, name in zip(got[:4], want[:4], ("dWa", "dba", "dWb", "dbb")):
        same_bits(a, b, name)
    assert float(got[4]) == float(want[4])
    # the loss against mean |score - gt| from the forward's own map: the two kernels add the same products in different orders, so each pixel's z
    # differs by at most twice the case's |dz|, s by ds/dz times that plus the fp32 evaluation of the activation in each (2^-19, see
    # test_headfit_ops.test_head_grad_z)
    A64, Wb64 = vals16(A.view(torch.float16), bf16, F64).cpu(), r16(Wb.double().cpu(), bf16)
    dz = hh.dz_bound(A64, Wb64, bb.double().cpu())
    z = A64 @ Wb64.T + bb.double().cpu()
    d1 = ho.activation(z, net._act, net._pow)[2]
    host = float((score.double() - gt.double()).abs().mean())
    print(f"{how} {backbone} {dtype}: loss {float(got[4]):.9f} host {host:.9f} dz {dz:.2e}")
    assert abs(float(got[4]) - host) <= 2 * float(d1.abs().max()) * dz + 2 * 2.0 ** -19
    # the forward's hidden rows are the leaky-ReLU of the tokens through the head's first linear (what the backward's mask relies on)
    pre = vals16(X.view(torch.float16), bf16, F64).cpu() @ r16(Wa.double().cpu(), bf16).T + ba.double().cpu()
    assert float((A64 - ho.leaky(pre)).abs().max()) <= 2.0 ** (-7 if bf16 else -10) * float(pre.abs().max())


def test_state_errors():
    net = make_net(TINY, 3, "fp16")[0]
    lib = _lib.load()
    q, r = _inputs(2, 1, 42, 42, 5)
    h = net._ensure_handle(q.device)
    Cc = net.arch.hidden
    outs = [torch.full(s, 7.0, device="cuda") for s in ((Cc, Cc), (Cc,), (196, Cc), (196,))] + [torch.full((), 7.0, dtype=F64, device="cuda")]
    gt = torch.zeros((3, 42, 42), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(B, H, W):
        return lib.cs_head_backward(h, C.c_void_p(gt.data_ptr()), B, H, W, 1e-3, 0, *(C.c_void_p(t.data_ptr()) for t in outs), st)

    assert call(2, 42, 42) == _lib.CS_ERR_STATE  # no forward yet
    net(q, r)
    assert net._handle == h
    assert call(3, 42, 42) == _lib.CS_ERR_STATE and call(2, 42, 56) == _lib.CS_ERR_STATE  # another shape
    assert call(2, 42, 42) == 0
    net.encode_references(r.reshape(2, 3, 42, 42))
    assert call(2, 42, 42) == _lib.CS_ERR_STATE  # the last call only encoded
    torch.cuda.synchronize()


@DTYPES
@pytest.mark.parametrize("tag", ["h0", "h1"])
@pytest.mark.parametrize("cname", sorted(GOLDEN_CONFIGS))
def test_gradients_against_the_golden(cname, tag, dtype):
    """cs_op_head_backward on the golden's tokens and weights as the forward would hold them (16-bit tokens, weights and hidden rows) against the
    fp64 autograd gradients of the reference's head: relative Frobenius error at most twice the reference's own autocast error on the same case
    (this path rounds g and dpre where autocast rounds the matching activations; nothing else differs)."""
    bf16 = dtype == "bf16"
    g = np.load(os.path.join(HERE, "golden", f"{tag}_head_fit.npz"))
    B, gh, gw, Cc, P_ = (int(v) for v in g["shape"])
    act, p = GOLDEN_CONFIGS[cname]
    X = torch.from_numpy(g["X"]).double()
    Wa, ba, Wb, bb = (torch.from_numpy(g[k]).double() for k in KEYS)
    A = r16(ho.leaky(X @ r16(Wa, bf16).T + ba), bf16)
    gt = torch.from_numpy(g[f"{cname}_gt"]).cuda()
    with switches(bf16=bf16):
        outs = hh.head_backward(bits16(X.float().cuda(), bf16), bits16(A.float().cuda(), bf16), bits16(Wb.float().cuda(), bf16), bb.float().cuda(), gt,
                                B, gh, gw, P_, act, p, 1.0 / gt.numel())
    yard = g[f"{cname}_acerr_{dtype}"]
    for o, k, y in zip(outs[:4], KEYS, yard):
        want = torch.from_numpy(g[f"{cname}_d{k}"])
        rel = float((o.double().cpu() - want).norm() / want.norm())
        print(f"golden {tag} {cname} {dtype} d{k}: rel Frobenius {rel:.3e}, the reference's autocast {float(y):.3e}")
        assert rel <= 2.0 * float(y), k
    assert abs(float(outs[4]) - float(g[f"{cname}_loss"])) <= 2.0 * float(yard.max()) * float(g[f"{cname}_loss"])


@DTYPES
def test_sub_batched_equals_unsplit(dtype):
    """fit_head_step over two sub-batches (accumulate) against the unsplit batch: the gradients differ by the order of the fp32 row sums"""
    bf16 = dtype == "bf16"
    B, N, H, W = 3, 1, 42, 70
    q, r = _inputs(B, N, H, W, 5)
    grads, losses = [], []
    for split in (False, True):
        net = make_net(TINY, 3, dtype)[0]
        gt = _gt_near(net(q, r)["score_map_ref_cross"], 9)
        if split:
            net._sub_batches = lambda B_, N_, Np_: [(0, 1), (1, B_)]
        st = HeadFitState()
        losses.append(float(net.fit_head_step(q, r, gt, st)))
        grads.append([t.double().cpu() for t in st.grads])
        if not split:
            M = B * (H // P) * (W // P)
            X, A = (vals16(t.view(torch.float16), bf16, F64).cpu() for t in net.head_inputs(M))
    Wa, ba, Wb, bb = (t.double().cpu() for t in _head(make_net(TINY, 3, dtype)[0]))
    inv = 1.0 / gt.numel()
    ref = ho.backward(X, A, r16(Wb, bf16), bb, ho.to_rows(gt.double().cpu(), H // P, W // P, P), net._act, net._pow, inv, rnd=lambda t: r16(t, bf16))
    g_, d_ = ref["g"].abs(), ref["dpre"].abs()
    sums = [d_.T @ X.abs(), d_.sum(0), g_.T @ A.abs(), g_.sum(0)]
    for a, b, s in zip(grads[0], grads[1], sums):
        assert float(((a - b).abs() - (2 * X.shape[0] * U32 * inv * s + 2 * U32 * a.abs())).max()) <= 0
    assert abs(losses[0] - losses[1]) <= 2.0 ** -50 * losses[0]


@DTYPES
def test_fit_head_step(dtype, tmp_path):
    bf16 = dtype == "bf16"
    B, N, H, W = 2, 2, 42, 70
    gh, gw = H // P, W // P
    net = make_net(TINY, 3, dtype)[0]
    q, r = _inputs(B, N, H, W, 5)
    before = net(q, r)["score_map_ref_cross"].clone()
    census = net.forward_stats()["kernels"]
    handle = net._handle
    gt = _gt_near(before, 11)
    X = vals16(net.head_inputs(B * gh * gw)[0].view(torch.float16), bf16, F64).cpu()
    want, _ = ho.fit(X, [t.double().cpu() for t in _head(net)], ho.to_rows(gt.double().cpu(), gh, gw, P), net._act, net._pow, steps=10, lr=5e-4)
    state = HeadFitState(lr=5e-4)
    got = [net.fit_head_step(q, r, gt, state) for _ in range(10)]
    assert all(t.dtype == F64 and t.is_cuda and t.dim() == 0 for t in got)
    got = [float(t) for t in got]
    yard = float(np.load(os.path.join(HERE, "golden", "h0_head_fit.npz"))[f"c0_acerr_{dtype}"].max())
    for i, (a, b) in enumerate(zip(got, want)):
        print(f"fit step {i + 1} {dtype}: loss {a:.9f}, fp64 oracle {b:.9f}")
        assert abs(a - b) <= 2.0 * yard * b, i
    assert got[-1] < got[0] and state.step == 10
    assert net._handle == handle and not net._dirty  # the handle was kept: only the head's buffers were re-packed
    after = net(q, r)["score_map_ref_cross"].clone()
    assert net.forward_stats()["kernels"] == census
    assert not torch.equal(after, before)
    path = str(tmp_path / "last.ckpt")
    save_lightning_checkpoint(path, net)
    fresh = make_net(TINY, 4, dtype)[0]
    fresh.load_state_dict(load_lightning_checkpoint(path), strict=True)
    again = fresh.to("cuda")(q, r)["score_map_ref_cross"]
    same_bits(again, after, "a fresh module from the checkpoint")
