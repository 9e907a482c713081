#!/usr/bin/env python3
"""What one whole-layer-fit step costs beside its forward and beside the cross-attention fit's step -> profiles/layer_fit.txt.

At cfg-2's shape (ViT-S, 8 queries of 518 x 518 with 5 cached reference views: M = 10 952 query rows, Mk = 54 760 memory rows, C = 384, 8 heads
of 48), per operand type, medians of RUNS runs timed with device events around the calls on one stream, all in one process: forward_cached with
the keep switches off, with cs_fit_cross_keep and with cs_fit_layer_keep on (two more copies and one more lse store), cs_cross_backward and
cs_layer_backward in the same run, the two updates (16 / 22 x cs_op_adamw + the hand-backs), and the step / forward ratio of both scopes.

    python tools/layer_fit_cost.py [--runs 7] [--out profiles/layer_fit.txt]"""
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
from crossscore_amd.model import FIT_CROSS, FIT_LAYER, CrossScoreNet, HeadFitState  # noqa: E402


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
    gt = (net.forward_cached(q, tok)["score_map_ref_cross"] + 0.1).contiguous()
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fwd_off = timed(lambda: net.forward_cached(q, tok), runs)

    def scope_cost(scope, keep, backward, params):
        keep(True)
        fwd = timed(lambda: net.forward_cached(q, tok), runs)
        outs = backward(gt)
        bwd = timed(lambda: backward(gt, out=outs), runs)
        state = HeadFitState(lr=0.0)  # (rate 0, no decay: the weights stay what they are between the runs)
        state.weight_decay = 0.0
        state.prepare(params)

        def update():
            for p, m, v, g in zip(params, state.m, state.v, outs[:len(params)]):
                _lib.check(lib.cs_op_adamw(_ptr(p), _ptr(m), _ptr(v), _ptr(g), p.numel(), state.lr, 0.9, 0.999, 1e-8, 0.0, 1, None, st))
            at = 0
            for s in scope.chain():
                own = params[at:at + len(s.own)]
                _lib.check(getattr(lib, s.set_weights)(net._handle, *(_ptr(p) for p in own), st))
                at += len(own)

        upd = timed(update, runs)
        keep(False)
        return fwd, bwd, upd

    cf, cb, cu = scope_cost(FIT_CROSS, net.fit_cross_keep, net.cross_backward, net.cross_parameters())
    lf, lb, lu = scope_cost(FIT_LAYER, net.fit_layer_keep, net.layer_backward, net.layer_parameters())
    return (f"{dtype}: forward_cached {fwd_off:8.1f} us, with cs_fit_cross_keep {cf:8.1f} us ({cf - fwd_off:+.1f}), with cs_fit_layer_keep {lf:8.1f} us "
            f"({lf - fwd_off:+.1f}) | cross backward {cb:8.1f} us, layer backward {lb:8.1f} us ({lb - cb:+.1f}) | update: cross (16 adamw + 3 hand-backs) "
            f"{cu:6.1f} us, layer (22 adamw + 4 hand-backs) {lu:6.1f} us | step / forward: cross {(cf + cb + cu) / fwd_off:.3f}, layer "
            f"{(lf + lb + lu) / fwd_off:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "layer_fit.txt"))
    a = ap.parse_args()
    assert a.runs >= 5
    lines = [f"whole-layer fit at cfg-2's shape (M = 10 952, Mk = 54 760, C = 384, 8 heads of 48), medians of {a.runs} runs, device events around "
             f"the calls, one process ({torch.cuda.get_device_name(0)})"]
    lines += [measure(d, a.runs) for d in ("fp16", "bf16")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
