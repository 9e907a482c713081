"""Ground-truth metric maps on the device (cs_op_gt_metric_map_u8): kernel time, the generator and the test loop.

(1) HIP-event time of the kernel for a batch of 8 pairs at 518 x 518 and 540 x 720, both kinds (median over --launches after a warm-up), beside
    its algorithmic traffic (2 * 3 + 2) * H * W * B bytes over the HBM rate a float4 copy reaches (6.29 TB/s), the existing GT stage it feeds
    (cs_op_metric_map_u16 + cs_op_score_gt_stats, timed here the same way) and the batch's forward (--forward-ms, 5.98 by default).
(2) python -m crossscore_amd.metric_maps on the tree of tools/evaluate_e2e.py without its metric_map/ (540 x 720, --images-per-split renders per
    split): files per second and PNG size against PIL's for the same arrays.
(3) crossscore_amd.evaluate on that tree, files mode (the generated maps) against compute mode, --rounds rounds alternating: loop and wall rates.
One JSON line per figure.  usage: python tools/gt_metric_maps_time.py [--images-per-split 48] [--rounds 2] [--launches 30]"""
import argparse, ctypes as C, io, json, os, shutil, sys, tempfile, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
from PIL import Image
from crossscore_amd import _lib, synth
from crossscore_amd.config import load_config, model_config
from crossscore_amd.data import InputStage
from crossscore_amd.decode import read_metric_map_u16
from crossscore_amd.evaluate import evaluate
from crossscore_amd.metric_maps import generate
from crossscore_amd.model import CrossScoreNet

ap = argparse.ArgumentParser()
ap.add_argument("--images-per-split", type=int, default=48)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--launches", type=int, default=30)
ap.add_argument("--forward-ms", type=float, default=5.98)
args = ap.parse_args()
lib = _lib.load()
dev = torch.device("cuda", 0)
HBM_TBS = 6.29
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731


def event_median_us(fn, n):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


# (1) the kernel
rng = np.random.default_rng(0)
for H, W in ((518, 518), (540, 720)):
    B = 8
    a = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    b = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    out = torch.empty((B, H, W), dtype=torch.int16, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for kind, name in ((_lib.GTMAP_SSIM, "ssim"), (_lib.GTMAP_MAE, "mae")):
        med, lo, hi = event_median_us(lambda: _lib.check(lib.cs_op_gt_metric_map_u8(p(a), p(b), B, H, W, H * W * 3, kind, p(out), W, st)), args.launches)
        traffic = (2 * 3 + 2) * H * W * B
        print(json.dumps({"kernel": f"gt_{name}", "B": B, "H": H, "W": W, "us_median": round(med, 1), "us_min": round(lo, 1), "us_max": round(hi, 1),
                          "algorithmic_bytes": traffic, "hbm_bound_us": round(traffic / (HBM_TBS * 1e6), 2),
                          "achieved_GBps_algorithmic": round(traffic / med / 1e3, 1), "share_of_forward": round(med / (args.forward_ms * 1e3), 4)}), flush=True)
    # the stage it feeds, the same way: cs_op_metric_map_u16 (resize to short side 518, integer-patch crop) + cs_op_score_gt_stats
    stage = InputStage(dev, resize_short_side=518, integer_patches=True)
    oh, ow = stage.geometry(H, W)[1][2:]
    gt = torch.empty((B, oh, ow), device=dev)
    score = torch.rand((B, oh, ow), device=dev)
    stats = torch.empty((B, 6), dtype=torch.float64, device=dev)
    scratch = torch.empty((lib.cs_score_gt_workspace_bytes(B, oh, ow),), dtype=torch.uint8, device=dev)
    maps = list(out)

    def fed():
        stage.metric_maps(maps, [(H, W)] * B, _lib.METRIC_SSIM_0_1, gt)
        _lib.check(lib.cs_op_score_gt_stats(p(score), p(gt), B, oh, ow, p(stats), p(scratch), st))
    med, lo, hi = event_median_us(fed, args.launches)
    print(json.dumps({"kernel": "metric_map_u16 (device maps) + score_gt_stats", "B": B, "H": H, "W": W, "out": [oh, ow], "us_median": round(med, 1),
                      "us_min": round(lo, 1), "us_max": round(hi, 1)}), flush=True)

# (2) the generator on the tree of tools/evaluate_e2e.py, without metric maps
root = tempfile.mkdtemp(prefix="gtmaps_")
base = os.path.join(root, "tree", "res_540")
H, W = 540, 720
g = np.random.Generator(np.random.PCG64(1)); yy, xx = np.mgrid[0:H, 0:W]
def img(i):
    x = np.stack([127 + 100 * np.sin(xx / (17.0 + i) + i), 127 + 100 * np.cos(yy / (23.0 + i)), (xx + yy + 31 * i) % 256], axis=2)
    return (x + g.normal(0, 8, x.shape)).clip(0, 255).astype(np.uint8)
for si, split in enumerate(("train", "test")):
    d = os.path.join(base, "s00000", split, "ours_1000")
    for k in ("renders", "gt"):
        os.makedirs(os.path.join(d, k))
    for i in range(args.images_per_split):
        shot = img(100 * si + i)  # a render is its captured image plus rendering error: blur on the right half, noise everywhere
        r = shot.astype(np.float64)
        r[:, W // 2:] = 0.5 * (r[:, W // 2:] + np.roll(r, 2, 1)[:, W // 2:])
        Image.fromarray(shot).save(os.path.join(d, "gt", f"frame_{i:05}.png"))
        Image.fromarray((r + g.normal(0, 4, r.shape)).clip(0, 255).astype(np.uint8)).save(os.path.join(d, "renders", f"frame_{i:05}.png"))
with open(os.path.join(base, "split.json"), "w") as f:
    json.dump({"test": ["s00000"]}, f)
bare = os.path.join(root, "tree")
filled = os.path.join(root, "filled")
for rnd in range(args.rounds):
    shutil.rmtree(filled, ignore_errors=True)
    shutil.copytree(bare, filled)
    res = generate(load_config("default_test", [f"data.dataset.path={filled}", "data.loader.validation.num_workers=8"]))
    ours, pil = [], []
    for f in res["written"][:: max(1, len(res["written"]) // 16)]:
        buf = io.BytesIO(); Image.fromarray(read_metric_map_u16(f)).save(buf, format="PNG")
        ours.append(os.path.getsize(f)); pil.append(buf.getbuffer().nbytes)
    print(json.dumps({"generator_round": rnd, "files": len(res["written"]), "seconds": round(res["seconds"], 3),
                      "files_per_sec": round(len(res["written"]) / res["seconds"], 1), "png_gpu_files": res["png_gpu_files"],
                      "bytes_ours_mean": int(np.mean(ours)), "bytes_pil_mean": int(np.mean(pil)), "ratio_to_pil": round(np.mean(ours) / np.mean(pil), 3)}), flush=True)

# (3) the test loop: files mode on the filled tree against compute mode on the bare one
arch = CrossScoreNet(model_config()).arch
sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(arch, 1).items()}
n = 2 * args.images_per_split
common = ["data.loader.validation.batch_size=8", "data.loader.validation.num_workers=8", "logger.test.write.flag.image_query=False",
          "logger.test.write.flag.image_reference=False", "logger.test.write.flag.item_path_json=False", "data.loader.validation.shuffle=False"]
metrics = {}
for rnd in range(args.rounds):
    for mode, tree in (("files", filled), ("compute", bare)):
        t0 = time.perf_counter()
        res = evaluate(load_config("default_test", common + [f"data.dataset.path={tree}", f"this_main.gt_metric_maps={mode}",
                                                             f"logger.test.out_dir={root}/out_{rnd}_{mode}"]), state_dict=sd, now="T")
        dt = time.perf_counter() - t0
        metrics[mode] = res["metrics"]
        print(json.dumps({"round": rnd, "gt_metric_maps": mode, "query_images": n, "input_stage": res["input_stage"].split(" ")[0],
                          "query_images_per_sec_loop": round(res["query_images_per_sec"], 1), "query_images_per_sec_wall": round(n / dt, 1),
                          "test/loss": res["metrics"]["test/loss"], "test/corr_cross": res["metrics"]["test/corr_cross"]}), flush=True)
print(json.dumps({"metrics_equal_in_both_modes": metrics["files"] == metrics["compute"]}), flush=True)
shutil.rmtree(root, ignore_errors=True)
