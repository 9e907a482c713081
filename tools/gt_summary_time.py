"""Ground-truth score summary on the device (cs_op_metric_map_sums_u16, cs_op_gt_metric_sums_u8): kernel time and the
program.

(1) HIP-event time (median over --launches after a warm-up; the window holds the op's memset of the 32 bytes per frame and the launch) of
    cs_op_metric_map_sums_u16 for 8 frames at 540 x 720 and 1200 x 1800, beside its algorithmic traffic 4 * H * W * B bytes over the HBM rate a
    float4 copy reaches (6.29 TB/s), and of cs_op_gt_metric_sums_u8 beside the two kinds of cs_op_gt_metric_map_u8 (whose work it does, less the
    stores) timed in the same loop.
(2) python -m crossscore_amd.summarise_gt on the tree of tools/evaluate_e2e.py (540 x 720, --images-per-split renders per split, maps written by
    crossscore_amd.metric_maps): frames per second of files and compute mode with both PNG decoders, --rounds rounds, and whether the four CSVs
    are the same bytes.
One JSON line per figure.  usage: python tools/gt_summary_time.py [--images-per-split 48] [--rounds 2] [--launches 30]"""
import argparse, ctypes as C, json, os, shutil, sys, tempfile
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
from PIL import Image
from crossscore_amd import _lib, summarise_gt
from crossscore_amd.config import load_config
from crossscore_amd.metric_maps import generate

ap = argparse.ArgumentParser()
ap.add_argument("--images-per-split", type=int, default=48)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--launches", type=int, default=30)
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


def line(name, B, H, W, t, traffic=None):
    d = {"kernel": name, "B": B, "H": H, "W": W, "us_median": round(t[0], 1), "us_min": round(t[1], 1), "us_max": round(t[2], 1)}
    if traffic:
        d.update(algorithmic_bytes=traffic, hbm_bound_us=round(traffic / (HBM_TBS * 1e6), 2), achieved_GBps_algorithmic=round(traffic / t[0] / 1e3, 1))
    print(json.dumps(d), flush=True)


# (1) the kernels
rng = np.random.default_rng(0)
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
B = 8
for H, W in ((540, 720), (1200, 1800)):
    ssim = torch.from_numpy(rng.integers(0, 65536, (B, H, W), dtype=np.uint16).view(np.int16)).to(dev)
    mae = torch.from_numpy(rng.integers(0, 65536, (B, H, W), dtype=np.uint16).view(np.int16)).to(dev)
    sums = torch.empty((B, 4), dtype=torch.int64, device=dev)
    t = event_median_us(lambda: _lib.check(lib.cs_op_metric_map_sums_u16(p(ssim), p(mae), B, H, W, W, H * W, p(sums), st)), args.launches)
    line("metric_map_sums_u16", B, H, W, t, 4 * H * W * B)
for H, W in ((518, 518), (540, 720)):
    a = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    b = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    out = torch.empty((B, H, W), dtype=torch.int16, device=dev)
    sums = torch.empty((B, 4), dtype=torch.int64, device=dev)
    ts = {}
    for kind, name in ((_lib.GTMAP_SSIM, "gt_ssim"), (_lib.GTMAP_MAE, "gt_mae")):
        ts[name] = event_median_us(lambda: _lib.check(lib.cs_op_gt_metric_map_u8(p(a), p(b), B, H, W, H * W * 3, kind, p(out), W, st)), args.launches)
        line(name + " (map form)", B, H, W, ts[name])
    t = event_median_us(lambda: _lib.check(lib.cs_op_gt_metric_sums_u8(p(a), p(b), B, H, W, H * W * 3, p(sums), st)), args.launches)
    line("gt_metric_sums_u8 (fused)", B, H, W, t)
    print(json.dumps({"H": H, "W": W, "fused_us": round(t[0], 1), "ssim_plus_mae_maps_us": round(ts["gt_ssim"][0] + ts["gt_mae"][0], 1),
                      "fused_over_sum": round(t[0] / (ts["gt_ssim"][0] + ts["gt_mae"][0]), 3)}), flush=True)

# (2) the program on the tree of tools/evaluate_e2e.py
root = tempfile.mkdtemp(prefix="gtsum_")
tree = os.path.join(root, "gaussian", "mfr")
base = os.path.join(tree, "res_540")
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
generate(load_config("default_test", [f"data.dataset.path={tree}", "data.loader.validation.num_workers=8"]))
csvs = {}
for rnd in range(args.rounds):
    for source in summarise_gt.SOURCES:
        for decoder in ("host", "gpu"):
            res = summarise_gt.summarise(base, os.path.join(root, f"out_{source}_{decoder}"), num_workers=8, force=True, source=source, png_decoder=decoder)
            csvs[(source, decoder)] = open(res["csv"], "rb").read()
            print(json.dumps({"round": rnd, "source": source, "png_decoder": decoder, "frames": res["frames"], "seconds": round(res["seconds"], 3),
                              "frames_per_sec": round(res["frames"] / res["seconds"], 1)}), flush=True)
print(json.dumps({"csv_equal_in_all_four": len(set(csvs.values())) == 1, "first_rows": csvs[("files", "host")].decode().splitlines()[:3]}), flush=True)
shutil.rmtree(root, ignore_errors=True)
