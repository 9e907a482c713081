#!/usr/bin/env python3
"""What one head-fit step costs beside its forward -> profiles/head_fit.txt.

At cfg-2's shape (ViT-S, 8 queries of 518 x 518 with 5 reference views: M = 10 952 token rows, C = 384), per operand type, medians of RUNS
runs timed with device events around the calls on one stream: forward_cached, cs_head_backward behind it (9 launches: the 16-bit rounding of the
tokens, grad_z, the loss finish, the transpose of Wb, dA, and gemm_tn + reduce for each of dWb and dWa), the update (4 x cs_op_adamw +
cs_set_head_weights), and the same head's forward + backward under PyTorch eager autograd (autocast to the operand type) on the same tokens.

    python tools/head_fit_cost.py [--runs 7] [--out profiles/head_fit.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

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
    M = B * (H // 14) * (W // 14)
    fwd = timed(lambda: net.forward_cached(q, tok), runs)
    outs = net.head_backward(gt)
    bwd = timed(lambda: net.head_backward(gt, out=outs), runs)
    state, params, lib = HeadFitState(), net.head_parameters(), _lib.load()
    state.prepare(params)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def update():
        for p, m, v, g in zip(params, state.m, state.v, outs[:4]):
            _lib.check(lib.cs_op_adamw(C.c_void_p(p.data_ptr()), C.c_void_p(m.data_ptr()), C.c_void_p(v.data_ptr()), C.c_void_p(g.data_ptr()), p.numel(),
                                       state.lr, 0.9, 0.999, 1e-8, 1e-2, 1, None, st))
        _lib.check(lib.cs_set_head_weights(net._handle, *(C.c_void_p(p.data_ptr()) for p in params), st))

    upd = timed(update, runs)
    X = net.head_inputs(M)[0]
    Wa, ba, Wb, bb = (p.detach().clone().requires_grad_(True) for p in params)
    gh, gw = H // 14, W // 14

    def eager():
        for t in (Wa, ba, Wb, bb):
            t.grad = None
        with torch.autocast("cuda", dtype=X.dtype):
            a = torch.nn.functional.leaky_relu(torch.nn.functional.linear(X, Wa, ba), 0.01)
            s = torch.sigmoid(torch.nn.functional.linear(a, Wb, bb)) if net._act == 0 else torch.tanh(torch.nn.functional.linear(a, Wb, bb))
        s = s.float() ** net._pow if net._pow != 1.0 else s.float()
        img = s.reshape(B, gh, gw, 14, 14).permute(0, 1, 3, 2, 4).reshape(B, gh * 14, gw * 14)
        (img - gt).abs().mean().backward()

    eag = timed(eager, runs)
    return (f"{dtype}: forward_cached {fwd:8.1f} us | head backward (9 launches) {bwd:7.1f} us | update (4 adamw + hand-back) {upd:6.1f} us | "
            f"step / forward {(fwd + bwd + upd) / fwd:.3f} | the head alone under eager autograd (forward + backward) {eag:7.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "head_fit.txt"))
    a = ap.parse_args()
    assert a.runs >= 5
    lines = [f"head fit at cfg-2's shape (M = 10 952, C = 384), medians of {a.runs} runs, device events around the calls ({torch.cuda.get_device_name(0)})"]
    lines += [measure(d, a.runs) for d in ("fp16", "bf16")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
