"""What this_main.vis_sheet costs, in one run on one GPU:
  * device events, after warm-up, for one sheet at cfg-2's geometry (a 518 x 518 query with 5 references, predict's panels): the compose launch
    alone (cs_op_sheet_compose) and the whole sheet as vis.SheetWriter queues it (de-normalising the query and the references, colouring the
    score map, the compose launch, the device PNG encode with its copy to pinned memory), beside the cached forward of a batch of 8 at that size;
    median of 5 regions with their range;
  * the predict loop's rate on 32 queries / 20 references of 540 x 720 (score maps written, batch 8) with the key off and on, alternating, three
    times each after one warm-up pair.  The off leg is the loop as it was; each leg's input stage is printed, since the sheet reads the processed
    images and so keeps fused_input_stage=auto on the two-launch stage.
usage: vis_sheet_cost.py [--out FILE] [--iters N, default 20]"""
import argparse
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from crossscore_amd import synth, vis  # noqa: E402
from crossscore_amd.config import load_config, model_config  # noqa: E402
from crossscore_amd.model import CrossScoreNet  # noqa: E402
from crossscore_amd.writers import PngEncoder, ScoreMapEncoder, colormap_table, denorm_to_rgb8  # noqa: E402

B, N, H, W = 8, 5, 518, 518


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
        t_cached = timed(lambda: net.forward_cached(q, tokens), max(3, iters // 2))
    colour = ScoreMapEncoder("ssim", 0.0, 1.0, "rgb", dev)
    turbo = torch.from_numpy(colormap_table("turbo").reshape(-1)).to(dev)
    png = PngEncoder("fast")
    canvas_h, canvas_w, panels = vis.sheet_layout(H, W, N, False, False)
    canvas = torch.empty((canvas_h, canvas_w, 3), dtype=torch.uint8, device=dev)

    def images():
        query = denorm_to_rgb8(q[:1], net.img_mean_std)[0]
        thumbs = denorm_to_rgb8(r[0], net.img_mean_std)
        out = {"turbo": turbo, "query": query, "query_on_map": query[:score.shape[1], :score.shape[2]], "score": colour.device_image(score[:1])[0]}
        out.update({f"ref{k}": thumbs[k] for k in range(N)})
        return out

    bound = vis.bind(panels, images(), {"score_mean": 0.5}, tuple(score.shape[1:]))

    def sheet():
        c = vis.compose(vis.bind(panels, images(), {"score_mean": 0.5}, tuple(score.shape[1:])), canvas_h, canvas_w, out=canvas)
        png.encode_async(c[None])

    t_compose = timed(lambda: vis.compose(bound, canvas_h, canvas_w, out=canvas), iters)
    t_sheet = timed(sheet, iters)
    say(f"device events, one sheet of a {H} x {W} query with {N} references ({canvas_h} x {canvas_w} canvas, {len(bound)} panels), ViT-S; per sheet:")
    say("  compose launch alone (cs_op_sheet_compose)                    " + spread(t_compose))
    say("  whole sheet: 2 x denorm, colouring, compose, PNG encode + copy  " + spread(t_sheet))
    say(f"  forward of a batch of {B}, cached tokens (cs_forward_cached)      " + spread(t_cached))
    mc, ms, mf = statistics.median(t_compose), statistics.median(t_sheet), statistics.median(t_cached)
    say("  the compose launch is %.2f %% and the whole sheet %.2f %% of that batch's cached forward" % (100 * mc / mf, 100 * ms / mf))


def predict_rates(say):
    from PIL import Image

    from crossscore_amd.predict import predict

    root = tempfile.mkdtemp(prefix="vis_sheet_cost_")
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
    rates, stages = {False: [], True: []}, {}
    for rnd in range(4):  # (the first pair pays table builds, stream probes and page-ins: not reported)
        for on in (False, True):
            over = [f"data.dataset.query_dir={qd}", f"data.dataset.reference_dir={rd}", f"logger.predict.out_dir={root}/out_{rnd}_{on}",
                    "logger.predict.write.flag.image_query=False", "logger.predict.write.flag.image_reference=False"]
            if on:
                over.append("this_main.vis_sheet=True")
            with torch.no_grad():
                res = predict(load_config("default_predict", over), state_dict=sd, now="T")
            stages[on] = res["input_stage"]
            if rnd:
                rates[on].append(res["query_images_per_sec"])
    say("predict loop, 32 queries / 20 references of 540 x 720, batch 8, score maps written (host PNG encoder), a sheet per batch with the key on; "
        "query-images/s through the loop:")
    say("  vis_sheet off  " + " | ".join("%.1f" % v for v in rates[False]) + "   " + spread(rates[False], "q/s") + "   input stage: " + stages[False])
    say("  vis_sheet on   " + " | ".join("%.1f" % v for v in rates[True]) + "   " + spread(rates[True], "q/s") + "   input stage: " + stages[True])
    inside = min(rates[False]) <= statistics.median(rates[True]) <= max(rates[False])
    say("  the median with the key on lies %s the spread of the runs with it off" % ("inside" if inside else "OUTSIDE"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from crossscore_amd import configure_runtime
    configure_runtime()
    say("preview sheet cost (tools/vis_sheet_cost.py), %s" % torch.cuda.get_device_name(0))
    device_times(a.iters, say)
    predict_rates(say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
