"""Test phase against predict on the same generated tree: 540x720 renders (16 per split of one scene, as many captured images per split: the
cross references of the other split's renders), ViT-S, 5 references per query, batch 8, score maps only.  evaluate scores the renders of both splits against their GT maps (the GT
stage and the score-vs-GT sums on top of predict's work); predict scores the same 32 renders, split by split.  Prints one JSON line per run:
query-images/s through the scoring loop and over the wall, and the GPU-busy fraction of the loop (HIP events around every forward, from
ForwardPipeline.record_timeline, which the evaluate loop's extra launches sit behind on the same streams), and for evaluate the host time
spent queueing each batch's GT stage (it waits for nothing: a fraction of a millisecond against the forward's ~6 ms).
--png-decoders host,gpu runs every phase once per this_main.png_decoder value, alternating inside the round.
usage: python tools/evaluate_e2e.py [--images-per-split 16] [--rounds 2] [--size 540x720] [--png-decoders host,gpu]"""
import argparse, json, os, sys, tempfile, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
from PIL import Image
from crossscore_amd import pipeline, synth
from crossscore_amd.config import load_config, model_config
from crossscore_amd.evaluate import evaluate
from crossscore_amd.model import CrossScoreNet
from crossscore_amd.predict import predict

ap = argparse.ArgumentParser()
ap.add_argument("--images-per-split", type=int, default=16)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--size", default="540x720", help="render size HxW (518x518: cfg-2's geometry, no resize)")
ap.add_argument("--png-decoders", default="host", help="comma-separated this_main.png_decoder values, one leg each per phase")
ap.add_argument("--reference-use", action="store_true", help="predict legs only, without and with this_main.reference_use=True (DESIGN.md 6, f12), alternating")
args = ap.parse_args()
root = tempfile.mkdtemp(prefix="eval_e2e_")
base = os.path.join(root, "tree", "res_540")
H, W = (int(v) for v in args.size.split("x"))
rng = np.random.Generator(np.random.PCG64(1)); yy, xx = np.mgrid[0:H, 0:W]
def img(i):
    a = np.stack([127 + 100 * np.sin(xx / (17.0 + i) + i), 127 + 100 * np.cos(yy / (23.0 + i)), (xx + yy + 31 * i) % 256], axis=2)
    return (a + rng.normal(0, 8, a.shape)).clip(0, 255).astype(np.uint8)
for si, split in enumerate(("train", "test")):
    d = os.path.join(base, "s00000", split, "ours_1000")
    for k in ("renders", "gt", "metric_map/ssim"):
        os.makedirs(os.path.join(d, k))
    for i in range(args.images_per_split):
        Image.fromarray(img(100 * si + 50 + i)).save(os.path.join(d, "gt", f"frame_{i:05}.png"))
        Image.fromarray(img(100 * si + i)).save(os.path.join(d, "renders", f"frame_{i:05}.png"))
        m = (np.clip(0.5 + 0.4 * np.sin(xx / 40.0 + i) * np.cos(yy / 30.0), 0, 1) * 65534).astype(np.uint16)
        Image.fromarray(m).save(os.path.join(d, "metric_map/ssim", f"frame_{i:05}.png"))
with open(os.path.join(base, "split.json"), "w") as f:
    json.dump({"test": ["s00000"]}, f)
arch = CrossScoreNet(model_config()).arch
sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(arch, 1).items()}
n = 2 * args.images_per_split
common = ["data.loader.validation.batch_size=8", "data.loader.validation.num_workers=8", "logger.{}.write.flag.image_query=False",
          "logger.{}.write.flag.image_reference=False", "logger.{}.write.flag.item_path_json=False"]

spans = []  # (phase, ms busy, ms window) of each run: ForwardPipeline.in_flight_fractions of every pipeline the run built
_init = pipeline.ForwardPipeline.__init__
def _init_timed(self, *a, **k):
    _init(self, *a, **k)
    self.record_timeline(True)
    spans.append(self)
pipeline.ForwardPipeline.__init__ = _init_timed

# host time spent queueing the GT stage (InputStage.metric_maps): it must not wait for the forward ahead of it on the same stream
from crossscore_amd import data as data_mod
gt_host = []
_maps = data_mod.InputStage.metric_maps
def _maps_timed(self, *a, **k):
    t = time.perf_counter()
    _maps(self, *a, **k)
    gt_host.append(time.perf_counter() - t)
data_mod.InputStage.metric_maps = _maps_timed

for rnd in range(args.rounds):  # (the first round pays table builds, stream probes and page-ins)
    legs = [(ph, d, False) for ph in ("evaluate", "predict") for d in args.png_decoders.split(",")]
    if args.reference_use:
        legs = [("predict", d, use) for d in args.png_decoders.split(",") for use in (False, True)]
    for phase, dec, use in legs:
        spans.clear()
        gt_host.clear()
        t0 = time.perf_counter()
        if phase == "evaluate":
            over = [f"data.dataset.path={root}/tree", "data.loader.validation.shuffle=False", f"logger.test.out_dir={root}/out_{rnd}_eval_{dec}",
                    f"this_main.png_decoder={dec}"]
            res = evaluate(load_config("default_test", over + [c.format("test") for c in common]), state_dict=sd, now="T")
            loop = res["query_images_per_sec"]
        else:
            rates = []
            for split, other in (("train", "test"), ("test", "train")):
                d = os.path.join(base, "s00000")
                over = [f"data.dataset.query_dir={d}/{split}/ours_1000/renders", f"data.dataset.reference_dir={d}/{other}/ours_1000/gt",
                        f"logger.predict.out_dir={root}/out_{rnd}_{split}_pred_{dec}_{use}", "logger.predict.write.config.score_map_colour_mode=gray",
                        f"this_main.png_decoder={dec}", f"this_main.reference_use={use}"]
                r = predict(load_config("default_predict", over + [c.format("predict") for c in common]), state_dict=sd, now="T")
                rates.append(r["query_images_per_sec"])
            loop = n / sum(args.images_per_split / x for x in rates)
        dt = time.perf_counter() - t0
        fr = [p.in_flight_fractions() for p in spans]
        busy = sum(f["window_ms"] * (1 - f["fraction_idle"]) for f in fr if f) / max(sum(f["window_ms"] for f in fr if f), 1e-9)
        print(json.dumps({"round": rnd, "phase": phase, "png_decoder": dec, **({"reference_use": use} if args.reference_use else {}), "size": args.size, "query_images": n, "query_images_per_sec_loop": round(loop, 1),
                          "query_images_per_sec_wall": round(n / dt, 1), "gpu_busy_fraction_of_forward_window": round(busy, 3),
                          **({"gt_stage_host_ms_per_batch_median": round(1e3 * sorted(gt_host)[len(gt_host) // 2], 3),
                              "gt_stage_host_ms_per_batch_max": round(1e3 * max(gt_host), 3)} if gt_host else {})}), flush=True)
