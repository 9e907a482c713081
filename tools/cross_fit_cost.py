#!/usr/bin/env python3
"""What one cross-attention-fit step costs beside its forward and beside the tail's step -> profiles/cross_fit.txt.

At cfg-2's shape (ViT-S, 8 queries of 518 x 518 with 5 reference views: M = 10 952 query rows, Mk = 54 760 memory rows, C = 384, 8 heads of 48),
per operand type, medians of RUNS runs timed with device events around the calls on one stream, all in one process: forward_cached with
cs_fit_cross_keep off and on (three copies and the lse store), cs_tail_backward for context, cs_cross_backward and its update (16 x cs_op_adamw
+ the three hand-backs), cs_op_attention_backward alone on the kept Q', K, V, O and lse -- as time and as TFLOP/s over 14 B h Lq Lk dh flops
(seven products of 2 Lq Lk dh each in the two-kernel form) -- beside cs_op_attention on the same operands (the forward's cross-attention launch,
4 B h Lq Lk dh flops), and the same block's forward + backward under PyTorch eager autograd (autocast to the operand type) on the kept x1.

    python tools/cross_fit_cost.py [--runs 7] [--out profiles/cross_fit.txt]"""
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
    gh, gw, Cc, heads = H // 14, W // 14, net.arch.hidden, net.arch.dec_heads
    Np, dh = gh * gw, Cc // heads
    M = B * Np
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fwd_off = timed(lambda: net.forward_cached(q, tok), runs)
    net.fit_tail_keep(True)
    net.forward_cached(q, tok)
    touts = net.tail_backward(gt)
    tbwd = timed(lambda: net.tail_backward(gt, out=touts), runs)
    net.fit_tail_keep(False)
    net.fit_cross_keep(True)
    fwd_on = timed(lambda: net.forward_cached(q, tok), runs)
    couts = net.cross_backward(gt)
    cbwd = timed(lambda: net.cross_backward(gt, out=couts), runs)
    params = net.cross_parameters()
    state = HeadFitState(lr=0.0)  # (rate 0, no decay: the weights stay what they are between the runs)
    state.weight_decay = 0.0
    state.prepare(params)

    def update():
        for p, m, v, g in zip(params, state.m, state.v, couts[:16]):
            _lib.check(lib.cs_op_adamw(_ptr(p), _ptr(m), _ptr(v), _ptr(g), p.numel(), state.lr, 0.9, 0.999, 1e-8, 0.0, 1, None, st))
        _lib.check(lib.cs_set_cross_weights(net._handle, *(_ptr(p) for p in params[:6]), st))
        _lib.check(lib.cs_set_tail_weights(net._handle, *(_ptr(p) for p in params[6:12]), st))
        _lib.check(lib.cs_set_head_weights(net._handle, *(_ptr(p) for p in params[12:]), st))

    cupd = timed(update, runs)
    # the attention backward alone, and the forward's launch on the same operands
    x1, Qp, O, lse, K, V = net.cross_inputs(M, N)
    dO = (torch.randn((M, Cc), device="cuda") * 1e-3).to(net.token_dtype)
    dQ, dKV = torch.empty_like(Qp), torch.empty((M * N, 2 * Cc), dtype=net.token_dtype, device="cuda")
    ws = torch.empty((lib.cs_attention_backward_workspace_bytes(B, heads, Np, N * Np, dh),), dtype=torch.uint8, device="cuda")
    O2, lse2 = torch.empty_like(O), torch.empty_like(lse)
    _lib.check(lib.cs_debug_set_op_operand_dtype(int(dtype == "bf16")))
    try:
        abwd = timed(lambda: _lib.check(lib.cs_op_attention_backward(
            _ptr(Qp), _ptr(K), _ptr(V), _ptr(O), _ptr(dO), _ptr(lse), Cc, Cc, Cc, Cc, Cc, Np * Cc, N * Np * Cc, N * Np * Cc, Np * Cc, Np * Cc, B, heads,
            Np, N * Np, dh, 1.0, _ptr(dQ), Cc, Np * Cc, _ptr(dKV), 2 * Cc, N * Np * 2 * Cc, C.c_void_p(dKV.data_ptr() + 2 * Cc), 2 * Cc, N * Np * 2 * Cc,
            _ptr(ws), st)), runs)
        afwd = timed(lambda: _lib.check(lib.cs_op_attention(_ptr(Qp), _ptr(K), _ptr(V), _ptr(O2), Cc, Cc, Cc, Cc, Np * Cc, N * Np * Cc, N * Np * Cc, Np * Cc,
                                                            B, heads, Np, N * Np, dh, 1.0, _ptr(lse2), st)), runs)
    finally:
        lib.cs_debug_set_op_operand_dtype(0)
    pair = float(B) * heads * Np * N * Np * dh
    # the same block under eager autograd
    mem = tok.reshape(B, N * Np, Cc).transpose(0, 1)
    prm = [p.detach().clone().requires_grad_(True) for p in params]
    Win, bin_, Wo, bo, g2, be2, W1, b1, W2, b2, g3, b3, Wa, ba, Wb, bb = prm
    xq = x1.reshape(B, Np, Cc).transpose(0, 1)

    def eager():
        for t in prm:
            t.grad = None
        with torch.autocast("cuda", dtype=net.token_dtype):
            a, _ = F.multi_head_attention_forward(xq, mem, mem, Cc, heads, Win, bin_, None, None, False, 0.0, Wo, bo, training=False, need_weights=False)
            x2 = F.layer_norm(x1 + a.transpose(0, 1).reshape(M, Cc), (Cc,), g2, be2, 1e-5)
            X = F.layer_norm(x2 + F.linear(F.relu(F.linear(x2, W1, b1)), W2, b2), (Cc,), g3, b3, 1e-5)
            z = F.linear(F.leaky_relu(F.linear(X, Wa, ba), 0.01), Wb, bb)
            s = torch.sigmoid(z) if net._act == 0 else torch.tanh(z)
        s = s.float() ** net._pow if net._pow != 1.0 else s.float()
        img = s.reshape(B, gh, gw, 14, 14).permute(0, 1, 3, 2, 4).reshape(B, gh * 14, gw * 14)
        (img - gt).abs().mean().backward()

    eag = timed(eager, runs)
    return (f"{dtype}: forward_cached {fwd_off:8.1f} us, with cs_fit_cross_keep {fwd_on:8.1f} us ({fwd_on - fwd_off:+.1f}) | tail backward {tbwd:7.1f} us | "
            f"cross backward {cbwd:8.1f} us, cross update (16 adamw + 3 hand-backs) {cupd:6.1f} us | cs_op_attention_backward alone {abwd:8.1f} us = "
            f"{14 * pair / abwd * 1e-6:6.1f} TFLOP/s ({100 * abwd / cbwd:.1f} % of the backward), cs_op_attention on the same operands {afwd:7.1f} us = "
            f"{4 * pair / afwd * 1e-6:6.1f} TFLOP/s | step / forward: tail {(fwd_off + tbwd) / fwd_off:.3f} (without its update), cross "
            f"{(fwd_on + cbwd + cupd) / fwd_off:.3f} | the block under eager autograd (forward + backward) {eag:8.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cross_fit.txt"))
    a = ap.parse_args()
    assert a.runs >= 5
    lines = [f"cross-attention fit at cfg-2's shape (M = 10 952, Mk = 54 760, C = 384, 8 heads of 48), medians of {a.runs} runs, device events around "
             f"the calls ({torch.cuda.get_device_name(0)})"]
    lines += [measure(d, a.runs) for d in ("fp16", "bf16")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
