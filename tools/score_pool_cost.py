"""What this_main.score_pool costs, in one run on one GPU:
  * device events, after warm-up, at cfg-2's geometry (a batch of 8 at 518 x 518, ViT-S, 5 references): the pool of the batch's score maps
    (cs_op_score_pool_f32, S = 56, five permilles) whole, without its window, and the 16-bit entry, beside that batch's uncached and cached
    forward; the pool's launches per batch are what scorepool.hip queues: 2 fills and 6 kernels, 2 + 4 without the window;
  * the predict loop's rate on 32 queries / 20 references of 540 x 720 (score maps written, batch 8) with the key off and on, alternating, three
    times each after one warm-up pair.  The off leg is the loop as it was.
usage: score_pool_cost.py [--out FILE] [--iters N, default 50]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from crossscore_amd import _lib, pooling, synth  # noqa: E402
from crossscore_amd.config import load_config, model_config  # noqa: E402
from crossscore_amd.model import CrossScoreNet  # noqa: E402

B, N, H, W, S = 8, 5, 518, 518, 56


def timed(fn, iters, repeats=5):
    """per-call device time in microseconds: `repeats` regions of `iters` calls between two events, after three calls of warm-up"""
    for _ in range(3):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(1e3 * a.elapsed_time(b) / iters)
    return out


def spread(v, unit="us"):
    return "median %.1f %s (min %.1f, max %.1f, n %d)" % (statistics.median(v), unit, min(v), max(v), len(v))


def device_times(iters, say):
    dev = torch.device("cuda", 0)
    net = CrossScoreNet(model_config())
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(net.arch, 1).items()}, strict=True)
    net = net.to(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    q = torch.randn((B, 3, H, W), generator=g).to(dev)
    r = torch.randn((B, N, 3, H, W), generator=g).to(dev)
    with torch.no_grad():
        tokens = net.encode_references(r.reshape(B * N, 3, H, W)).reshape(B, N, -1, net.arch.hidden)
        score = net.forward_cached(q, tokens)["score_map_ref_cross"].contiguous()
        t_full = timed(lambda: net.forward(q, r), max(3, iters // 10))
        t_cached = timed(lambda: net.forward_cached(q, tokens), max(3, iters // 5))
    lib = _lib.load()
    Q = len(pooling.PERMILLE)
    per = (C.c_int32 * Q)(*pooling.PERMILLE)
    out = torch.empty((B * (1 + Q + 3) + B * Q,), dtype=torch.int64, device=dev)
    base = out.data_ptr()
    p_sum, p_tail, p_win, p_quant = base, base + 8 * B, base + 8 * (B + B * Q), base + 8 * (B + B * Q + 3 * B)
    scratch = torch.empty((int(lib.cs_score_pool_workspace_bytes(B, H, W, Q)),), dtype=torch.uint8, device=dev)
    codes = torch.empty((B, H, W), dtype=torch.int16, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    signed = 1 if pooling.signed_range_of("ssim") else 0
    _lib.check(lib.cs_op_score_to_gray16(C.c_void_p(score.data_ptr()), score.numel(), signed, C.c_void_p(codes.data_ptr()), st))

    def pool_f32(window):
        _lib.check(lib.cs_op_score_pool_f32(C.c_void_p(score.data_ptr()), B, H, W, signed, per, Q, S if window else 0, C.c_void_p(p_sum),
                                            C.c_void_p(p_quant), C.c_void_p(p_tail), C.c_void_p(p_win) if window else None,
                                            C.c_void_p(scratch.data_ptr()), st))

    def pool_u16():
        _lib.check(lib.cs_op_score_pool_u16(C.c_void_p(codes.data_ptr()), B, H, W, W, H * W, per, Q, S, C.c_void_p(p_sum), C.c_void_p(p_quant),
                                            C.c_void_p(p_tail), C.c_void_p(p_win), C.c_void_p(scratch.data_ptr()), st))

    t_pool = timed(lambda: pool_f32(True), iters)
    t_nowin = timed(lambda: pool_f32(False), iters)
    t_u16 = timed(pool_u16, iters)
    say(f"device events, batch {B} x {H} x {W}, {N} references, ViT-S, S = {S}, permille {pooling.PERMILLE}; per batch:")
    say("  forward, uncached (cs_forward)            " + spread(t_full))
    say("  forward, cached tokens (cs_forward_cached)  " + spread(t_cached))
    say("  score pool, fp32 entry, 2 fills + 6 kernels " + spread(t_pool))
    say("  ... without the window, 1 fill + 4 kernels  " + spread(t_nowin))
    say("  score pool, 16-bit entry, 2 fills + 6 kernels " + spread(t_u16))
    mp, mc, mf = statistics.median(t_pool), statistics.median(t_cached), statistics.median(t_full)
    say("  the pool is %.2f %% of the cached forward and %.2f %% of the uncached one; its window launches are %.1f us of its %.1f us"
        % (100 * mp / mc, 100 * mp / mf, mp - statistics.median(t_nowin), mp))


def predict_rates(say):
    from PIL import Image

    from crossscore_amd.predict import predict

    root = tempfile.mkdtemp(prefix="score_pool_cost_")
    base = os.path.join(root, "data", "gaussian", "mfr", "res_540", "s00000", "test", "ours_1000")
    qd, rd = os.path.join(base, "renders"), os.path.join(base, "gt")
    os.makedirs(qd)
    os.makedirs(rd)
    rng = np.random.Generator(np.random.PCG64(1))
    yy, xx = np.mgrid[0:540, 0:720]

    def img(i):
        a = np.stack([127 + 100 * np.sin(xx / (17.0 + i) + i), 127 + 100 * np.cos(yy / (23.0 + i)), (xx + yy + 31 * i) % 256], axis=2)
        return (a + rng.normal(0, 8, a.shape)).clip(0, 255).astype(np.uint8)

    for i in range(32):
        Image.fromarray(img(i)).save(os.path.join(qd, f"frame_{i:05}.png"))
    for i in range(20):
        Image.fromarray(img(100 + i)).save(os.path.join(rd, f"frame_{i:05}.png"))
    arch = CrossScoreNet(model_config()).arch
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(arch, 1).items()}
    rates = {False: [], True: []}
    for rnd in range(4):  # (the first pair pays table builds, stream probes and page-ins: not reported)
        for on in (False, True):
            over = [f"data.dataset.query_dir={qd}", f"data.dataset.reference_dir={rd}", f"logger.predict.out_dir={root}/out_{rnd}_{on}",
                    "logger.predict.write.flag.image_query=False", "logger.predict.write.flag.image_reference=False"]
            if on:
                over.append("this_main.score_pool=True")
            with torch.no_grad():
                res = predict(load_config("default_predict", over), state_dict=sd, now="T")
            if rnd:
                rates[on].append(res["query_images_per_sec"])
    say("predict loop, 32 queries / 20 references of 540 x 720, batch 8, score maps written (host PNG encoder), query-images/s through the loop:")
    say("  score_pool off  " + " | ".join("%.1f" % v for v in rates[False]) + "   " + spread(rates[False], "q/s"))
    say("  score_pool on   " + " | ".join("%.1f" % v for v in rates[True]) + "   " + spread(rates[True], "q/s"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from crossscore_amd import configure_runtime
    configure_runtime()
    say("score pool cost (tools/score_pool_cost.py), %s" % torch.cuda.get_device_name(0))
    device_times(a.iters, say)
    predict_rates(say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
