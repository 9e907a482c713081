#!/usr/bin/env python3
"""What one tail-fit step costs beside its forward and beside the head-only step -> profiles/tail_fit.txt.

At cfg-2's shape (ViT-S, 8 queries of 518 x 518 with 5 reference views: M = 10 952 token rows, C = 384), per operand type, medians of RUNS
runs timed with device events around the calls on one stream, all in one process: forward_cached with cs_fit_tail_keep off and on (the two
copies), cs_head_backward and the head's update (4 x cs_op_adamw + cs_set_head_weights) as tools/head_fit_cost.py measures them,
cs_tail_backward and the tail's update (10 x cs_op_adamw + both hand-backs), cs_op_ln_backward alone on rows of the same shape (its share of
the backward), and the same tail's forward + backward under PyTorch eager autograd (autocast to the operand type) on the kept x2.

    python tools/tail_fit_cost.py [--runs 7] [--out profiles/tail_fit.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from crossscore_amd import _lib, synth  # noqa: E402
from crossscore_amd.config import model_config  # noqa: E402
from crossscore_amd.model import CrossScoreNet, HeadFitState  # noqa: E402


def timed(fn, runs):
    out = []
    for _ in range(runs + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out[2:])  # (two warm-up runs)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def measure(dtype, runs):
    B, N, H, W = 8, 5, 518, 518
    net = CrossScoreNet(model_config(**{"backbone.from_pretrained": "facebook/dinov2-small"}))
    net.load_numpy_state_dict(synth.make_state_dict(net.arch, 3))
    net.operand_dtype = dtype
    net = net.cuda()
    q, r = synth.make_inputs(B, N, H, W, 5)
    q, r = torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()
    tok = net.encode_references(r.reshape(B * N, 3, H, W)).reshape(B, N, -1, net.arch.hidden)
    score = net.forward_cached(q, tok)["score_map_ref_cross"]
    gt = (score + 0.1).contiguous()
    gh, gw, Cc = H // 14, W // 14, net.arch.hidden
    M = B * gh * gw
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fwd_off = timed(lambda: net.forward_cached(q, tok), runs)
    net.fit_tail_keep(True)
    fwd_on = timed(lambda: net.forward_cached(q, tok), runs)
    houts = net.head_backward(gt)
    hbwd = timed(lambda: net.head_backward(gt, out=houts), runs)
    touts = net.tail_backward(gt)
    tbwd = timed(lambda: net.tail_backward(gt, out=touts), runs)

    def update(params, grads, state, tail):
        def go():
            for p, m, v, g in zip(params, state.m, state.v, grads):
                _lib.check(lib.cs_op_adamw(_ptr(p), _ptr(m), _ptr(v), _ptr(g), p.numel(), state.lr, 0.9, 0.999, 1e-8, 1e-2, 1, None, st))
            if tail:
                _lib.check(lib.cs_set_tail_weights(net._handle, *(_ptr(p) for p in params[:6]), st))
            _lib.check(lib.cs_set_head_weights(net._handle, *(_ptr(p) for p in params[-4:]), st))
        return go

    hstate, tstate = HeadFitState(lr=0.0), HeadFitState(lr=0.0)  # (rate 0, no decay below: the weights stay what they are between the runs)
    hstate.weight_decay = tstate.weight_decay = 0.0
    hstate.prepare(net.head_parameters())
    tstate.prepare(net.tail_parameters())
    hupd = timed(update(net.head_parameters(), houts[:4], hstate, False), runs)
    tupd = timed(update(net.tail_parameters(), touts[:10], tstate, True), runs)
    # ln_backward alone, on rows of the backward's shape
    y, dX = torch.randn((M, Cc), device="cuda"), torch.randn((M, Cc), device="cuda") * 1e-4
    gamma, dyh = torch.ones((Cc,), device="cuda"), torch.empty((M, Cc), dtype=torch.float16, device="cuda")
    dg, db = torch.zeros((Cc,), device="cuda"), torch.zeros((Cc,), device="cuda")
    ws = torch.empty((lib.cs_ln_backward_workspace_bytes(M, Cc),), dtype=torch.uint8, device="cuda")
    bf = int(dtype == "bf16")
    ln = timed(lambda: _lib.check(lib.cs_op_ln_backward(_ptr(y), Cc, _ptr(dX), Cc, _ptr(gamma), M, Cc, 1e-5, bf, 1.0 / gt.numel(), 0, _ptr(dyh), Cc,
                                                        _ptr(dg), _ptr(db), _ptr(ws), st)), runs)
    # the same tail under eager autograd
    x2 = net.tail_inputs(M)[0]
    prm = [p.detach().clone().requires_grad_(True) for p in net.tail_parameters()]
    W1, b1, W2, b2, g3, b3, Wa, ba, Wb, bb = prm

    def eager():
        for t in prm:
            t.grad = None
        with torch.autocast("cuda", dtype=net.token_dtype):
            X = F.layer_norm(x2 + F.linear(F.relu(F.linear(x2, W1, b1)), W2, b2), (Cc,), g3, b3, 1e-5)
            z = F.linear(F.leaky_relu(F.linear(X, Wa, ba), 0.01), Wb, bb)
            s = torch.sigmoid(z) if net._act == 0 else torch.tanh(z)
        s = s.float() ** net._pow if net._pow != 1.0 else s.float()
        img = s.reshape(B, gh, gw, 14, 14).permute(0, 1, 3, 2, 4).reshape(B, gh * 14, gw * 14)
        (img - gt).abs().mean().backward()

    eag = timed(eager, runs)
    return (f"{dtype}: forward_cached {fwd_off:8.1f} us, with cs_fit_tail_keep {fwd_on:8.1f} us ({fwd_on - fwd_off:+.1f}) | head backward {hbwd:7.1f} us, "
            f"head update {hupd:6.1f} us | tail backward {tbwd:7.1f} us (ln_backward + its reduce alone {ln:6.1f} us = {100 * ln / tbwd:.1f} %), "
            f"tail update (10 adamw + 2 hand-backs) {tupd:6.1f} us | step / forward: head {(fwd_off + hbwd + hupd) / fwd_off:.3f}, tail "
            f"{(fwd_on + tbwd + tupd) / fwd_off:.3f} | the tail under eager autograd (forward + backward) {eag:7.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tail_fit.txt"))
    a = ap.parse_args()
    assert a.runs >= 5
    lines = [f"tail fit at cfg-2's shape (M = 10 952, C = 384), medians of {a.runs} runs, device events around the calls ({torch.cuda.get_device_name(0)})"]
    lines += [measure(d, a.runs) for d in ("fp16", "bf16")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
