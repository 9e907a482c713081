#!/usr/bin/env python3
"""Writes tests/golden/t0_tail_fit.npz: the cases and the yardstick of the tail fit's gradient test.  Two steps:

    python tests/golden/make_tail_fit.py tap TAPS.npz      (on the GPU)
    python tests/golden/make_tail_fit.py golden TAPS.npz   (CPU only)

`tap` runs the two nets of tests/test_tailfit_forward.py (synthetic tiny and the ViT-S width, seed 3, the inputs of synth.make_inputs(2, N, 42,
70, 5)) in both operand types with fit_tail_keep on and saves what the forward left: x2 (fp32), H, X and A (16-bit patterns) and the score map.
`golden` builds, per net, a gt 0.05 .. 0.3 away from both operand types' score maps, and per net and operand type differentiates the tail
(tests/tailfit_helpers.autograd_tail: the modules the reference executes) on the tapped x2 in fp64 and under torch.autocast on the CPU in that
type, the loss scaled by 2^16 and the gradients unscaled as a GradScaler does (without it 1 / n puts the fp16 gradients into the subnormal
range).  Stored: the taps, gt, the fp64 loss, and the relative Frobenius error of each of the ten autocast gradients against fp64.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

import tailfit_helpers as th  # noqa: E402
from crossscore_amd import synth  # noqa: E402
from nets import SMALL, TINY, make_net  # noqa: E402

P = 14
LOSS_SCALE = 2.0 ** 16
CASES = {"tiny": (TINY, 2), "small": (SMALL, 1)}  # tag -> (backbone, reference views)
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
B, H, W = 2, 42, 70


def tap(path):
    out = {}
    M = B * (H // P) * (W // P)
    for tag, (backbone, N) in CASES.items():
        q, r = synth.make_inputs(B, N, H, W, 5)
        q, r = torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()
        for dtype in DTYPES:
            net = make_net(backbone, 3, dtype)[0]
            net.fit_tail_keep(True)
            out[f"{tag}_{dtype}_score"] = net(q, r)["score_map_ref_cross"].cpu().numpy()
            x2, Hk = net.tail_inputs(M)
            X, A = net.head_inputs(M)
            out[f"{tag}_{dtype}_x2"] = x2.cpu().numpy()
            for name, t in (("H", Hk), ("X", X), ("A", A)):
                out[f"{tag}_{dtype}_{name}"] = t.view(torch.int16).cpu().numpy()
    np.savez_compressed(path, **out)


def golden(path):
    taps = np.load(path)
    out = {k: taps[k] for k in taps.files if not k.endswith("_score")}
    gh, gw = H // P, W // P
    for tag, (backbone, N) in CASES.items():
        net = make_net(backbone, 3, device="cpu")[0]
        params = [p.detach().float() for p in net.tail_parameters()]
        s16, sbf = (torch.from_numpy(taps[f"{tag}_{d}_score"]).double() for d in DTYPES)
        g = torch.Generator().manual_seed(11)
        off = (0.06 + 0.24 * torch.rand(s16.shape, generator=g)) * torch.where(torch.rand(s16.shape, generator=g) < 0.5, -1.0, 1.0)
        gt = (s16 + off).float()
        assert float((s16 - gt).abs().min()) >= 0.05 and float((sbf - gt).abs().min()) >= 0.05  # no sign of s - gt is in doubt in either type
        out[f"{tag}_gt"] = gt.numpy()
        for dtype, dt in DTYPES.items():
            x2 = torch.from_numpy(taps[f"{tag}_{dtype}_x2"])
            loss64, want = th.autograd_tail(x2.double(), [t.double() for t in params], gt.double(), net._act, net._pow, gh, gw, P)
            _, got = th.autograd_tail(x2, params, gt, net._act, net._pow, gh, gw, P, autocast=dt, loss_scale=LOSS_SCALE)
            err = np.array([th.rel_fro(a, b) for a, b in zip(got, want)])
            out[f"{tag}_{dtype}_acerr"], out[f"{tag}_{dtype}_loss"] = err, np.float64(loss64)
            print(tag, dtype, " ".join(f"{e:.2e}" for e in err))
    out["shape"] = np.array([B, gh, gw, P], dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "t0_tail_fit.npz"), **out)


if __name__ == "__main__":
    {"tap": tap, "golden": golden}[sys.argv[1]](sys.argv[2])
