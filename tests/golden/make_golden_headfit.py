#!/usr/bin/env python3
"""Golden vectors of the head fit, made by running the REFERENCE's own pieces on the CPU (build container only).

Imports the reference's RegressionLayer (model/regression_layer.py) and jigsaw_to_image (utils/misc/image.py) by the recipe of make_golden.py
(stubs for the packages that are absent offline) and composes the head exactly as CrossReferenceNet.__init__ does (cross_reference.py:45-50):
Linear(C, C) -> LeakyReLU() -> Linear(C, P P) -> RegressionLayer, then view + jigsaw (:85-87) and the L1 loss of task/core.py:283-285.  Gradients
come from torch autograd in fp64; the optimiser is torch.optim.AdamW(lr = 5e-4) with StepLR(step_size = 2, gamma = 0.5), three steps.
The Sequential is restated here from torch.nn pieces, not taken from a constructed CrossReferenceNet (which needs the whole configuration and a
DINOv2 config to build): RegressionLayer and jigsaw_to_image are the reference's own objects, the two Linears and LeakyReLU() (default slope
0.01) are the same torch classes with the same arguments as cross_reference.py:45-50 names.
Neither reference source nor bytecode is written to the repository: only seeds' inputs and the numbers that come out.

One file per shape (each stays well below the size limit of a committed file):
    h0_head_fit.npz   B = 2 on a 3 x 5 grid, with the three AdamW steps
    h1_head_fit.npz   B = 1 on a 2 x 3 grid
C = 64, P = 14; three configurations: c0 sigmoid p = 1 (ssim, min 0), c1 sigmoid p = 2 (mae, min 0), c2 tanh p = 1 (ssim, min -1).  The weights
are shared (fp32); X holds values both 16-bit types represent.  Per configuration: gt (the fp64 score map moved by 0.05 .. 0.3), loss, the four fp64 gradients; in h0 the parameters'
change after the three steps (fp64 run, stored as fp32 differences: 1e-10 absolute) and adam32_dev, the largest |fp32 run - fp64 run| per
parameter (torch against itself: the yardstick of the AdamW test); acerr_fp16 / acerr_bf16: the relative Frobenius error of the same head's
gradients under torch.autocast on the CPU (fp32 master weights, as the reference trains with precision 16-mixed; the fp16 run scales its loss
by 65536 and unscales the gradients, as its GradScaler does) against the fp64 gradients -- the yardstick of the gradient tests.

    python tests/golden/make_golden_headfit.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
C_, P = 64, 14
CONFIGS = {"c0": ("ssim", 0, "default"), "c1": ("mae", 0, "default"), "c2": ("ssim", -1, "default")}
SHAPES = {"h0": (2, 3, 5), "h1": (1, 2, 3)}
KEYS = ("Wa", "ba", "Wb", "bb")


def _import_reference():
    for name in ("imageio", "imageio.v2"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path[:0] = [REF]
    from model.regression_layer import RegressionLayer
    from utils.misc.image import jigsaw_to_image
    return RegressionLayer, jigsaw_to_image


def build_head(RegressionLayer, cfg, weights, dtype):
    mtype, mmin, powf = cfg
    head = torch.nn.Sequential(torch.nn.Linear(C_, C_), torch.nn.LeakyReLU(), torch.nn.Linear(C_, P * P), RegressionLayer(mtype, mmin, 1, powf))
    with torch.no_grad():
        for prm, k in zip((head[0].weight, head[0].bias, head[2].weight, head[2].bias), KEYS):
            prm.copy_(torch.from_numpy(weights[k]))
    return head.to(dtype)


def loss_of(head, jigsaw, X, gt, B, gh, gw):
    s = head(X.view(B, gh * gw, C_)).view(B, -1, P, P)
    return torch.abs(jigsaw(s, grid_size=(gh, gw)) - gt).mean()


def grads_of(head):
    return [p.grad.detach().double().clone() for p in (head[0].weight, head[0].bias, head[2].weight, head[2].bias)]


def main():
    RegressionLayer, jigsaw = _import_reference()
    rng = np.random.Generator(np.random.PCG64(2024))
    weights = {"Wa": (rng.normal(size=(C_, C_)) / np.sqrt(C_)).astype(np.float32), "ba": (rng.normal(size=(C_,)) * 0.1).astype(np.float32),
               "Wb": (rng.normal(size=(P * P, C_)) * 1.5 / np.sqrt(C_)).astype(np.float32), "bb": (rng.normal(size=(P * P,)) * 0.3).astype(np.float32)}
    for tag, (B, gh, gw) in SHAPES.items():
        out = dict(weights)
        out["shape"] = np.array([B, gh, gw, C_, P])
        X32 = torch.from_numpy(rng.normal(size=(B * gh * gw, C_)).astype(np.float32)).to(torch.bfloat16).float()  # 8 significant bits: both types hold it
        out["X"] = X32.numpy()
        for cname, cfg in CONFIGS.items():
            head = build_head(RegressionLayer, cfg, weights, torch.float64)
            # gt = the fp64 head's own score map moved by 0.05 .. 0.3 either way (not clipped): no sign of s - gt is in doubt in any precision, so
            # the errors recorded below are rounding, not the luck of a pixel that sits on its ground truth
            with torch.no_grad():
                s64 = jigsaw(head(X32.double().view(B, gh * gw, C_)).view(B, -1, P, P), grid_size=(gh, gw))
            off = rng.uniform(0.05, 0.3, size=tuple(s64.shape)) * rng.choice([-1.0, 1.0], size=tuple(s64.shape))
            gt32 = (s64 + torch.from_numpy(off)).float()
            assert float((s64 - gt32.double()).abs().min()) >= 0.049
            out[f"{cname}_gt"] = gt32.numpy()
            loss = loss_of(head, jigsaw, X32.double(), gt32.double(), B, gh, gw)
            loss.backward()
            ref = grads_of(head)
            out[f"{cname}_loss"] = np.float64(loss.item())
            for k, g in zip(KEYS, ref):
                out[f"{cname}_d{k}"] = g.numpy()
            # the reference's own mixed precision on the same head: fp32 master weights under autocast
            for name, dt, scale in (("fp16", torch.float16, 65536.0), ("bf16", torch.bfloat16, 1.0)):
                h32 = build_head(RegressionLayer, cfg, weights, torch.float32)
                with torch.autocast("cpu", dtype=dt):
                    l16 = loss_of(h32, jigsaw, X32, gt32, B, gh, gw)
                (l16.float() * scale).backward()
                out[f"{cname}_acerr_{name}"] = np.array([float((g / scale - r).norm() / r.norm()) for g, r in zip(grads_of(h32), ref)])
            if tag != "h0":
                continue
            runs = {}
            for dt in (torch.float64, torch.float32):
                h = build_head(RegressionLayer, cfg, weights, dt)
                opt = torch.optim.AdamW(h.parameters(), lr=5e-4)
                sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
                for _ in range(3):
                    opt.zero_grad()
                    loss_of(h, jigsaw, X32.to(dt), gt32.to(dt), B, gh, gw).backward()
                    opt.step()
                    sched.step()
                runs[dt] = [p.detach().double().clone() for p in (h[0].weight, h[0].bias, h[2].weight, h[2].bias)]
            for k, a in zip(KEYS, runs[torch.float64]):
                out[f"{cname}_step3_delta_{k}"] = (a - torch.from_numpy(weights[k]).double()).float().numpy()
            out[f"{cname}_adam32_dev"] = np.array([float((a - b).abs().max()) for a, b in zip(runs[torch.float32], runs[torch.float64])])
        path = os.path.join(HERE, f"{tag}_head_fit.npz")
        np.savez(path, **out)
        print(path, os.path.getsize(path), "bytes")
        for cname in CONFIGS:
            print(" ", cname, "loss", out[f"{cname}_loss"], "autocast fp16", out[f"{cname}_acerr_fp16"], "bf16", out[f"{cname}_acerr_bf16"],
                  "adam32", out.get(f"{cname}_adam32_dev"))


if __name__ == "__main__":
    main()
