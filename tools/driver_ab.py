"""A/B of the predict, evaluate and fit_head drivers of two source trees, same box: do both trees write the same bytes and return the same results?

usage: driver_ab.py <parent tree> <new tree> [--jobs N] [--only predict|evaluate|fit_head] [--match TEXT] [--drop-result-key KEY ...]

Each tree is a checkout with its own built library (the parent e.g. as a `git worktree`).  The input trees are generated once (the geometry of the
driver tests: 5 queries and 4 references of 70 x 90 -> 56 x 72, batch 2, ViT-S two-layer synthetic weights; tests/nvs_tree.py for evaluate).  One
fresh child process per tree and case imports that tree's package, runs the driver with now= fixed inside a directory of its own, and prints one line:
a digest over (relative path, file bytes) of everything it wrote, and the result dictionary without query_images_per_sec (paths relative to the
case directory; the long values -- files, rows, batches, metrics -- as a count and a digest).  The two trees' listings must be identical.

predict:  cache on / off x fused_input_stage auto / False x png_decoder host / gpu x batches_in_flight 1 / 3; every writer flag on; JPEG queries
          with jpeg_decoder=gpu; neighbour strategy similar over input stage, decoder and batches in flight.
          reference_use with its images, score_pool, vis_sheet: each over fused_input_stage auto / False.
evaluate: cache x fused x png_decoder x gt_metric_maps files / compute x shuffle on / off; limit_test_batches=2; neighbour strategy similar,
          score_pool, vis_sheet: each over fused_input_stage auto / False.
fit_head: the overrides of tests/test_headfit_driver.py, two epochs; token cache on / off, gt_metric_maps files / compute.  Its digest is over
          fit_head.csv, the tensors of checkpoints/last.ckpt (not the file: a pickle) and the result dictionary.

--match keeps the cases whose name holds TEXT; --drop-result-key leaves a key out of both trees' result dictionaries (one that only the new
tree reports, e.g. reference_strategy: profiles/r15_reference_selection.txt).

Every child runs under its own time limit; the script stops at the first one that ends with a non-zero status (it may have faulted the GPU: nothing
more is started on it).  Written for the move of both drivers' loop into crossscore_amd/scoring.py (profiles/r13_driver_loop.txt).
"""
import argparse
import itertools
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACK = "synthetic/dinov2-small-2l"

CHILD = r'''
import hashlib, json, os, sys
tree, driver, case_dir, drop = sys.argv[1], sys.argv[2], sys.argv[3], [k for k in sys.argv[4].split(",") if k]
overrides = sys.argv[5:]
sys.path.insert(0, tree)
os.makedirs(case_dir)
os.chdir(case_dir)  # (evaluate's version directory is relative: log/<now>/test_empty_ckpt/version_0)
import numpy as np, torch
import crossscore_amd
assert os.path.dirname(os.path.abspath(crossscore_amd.__file__)) == os.path.join(os.path.abspath(tree), "crossscore_amd"), crossscore_amd.__file__
from crossscore_amd import synth
from crossscore_amd.config import load_config, model_config
from crossscore_amd.model import CrossScoreNet
back = [o.split("=", 1)[1] for o in overrides if o.startswith("model.backbone.from_pretrained=")][0]
sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(CrossScoreNet(model_config(**{"backbone.from_pretrained": back})).arch, 6).items()}
np.random.seed(0)
with torch.no_grad():
    if driver == "fit_head":
        from crossscore_amd.fit_head import fit_head
        res = fit_head(load_config("default_fit_head", overrides + ["logger.train.out_dir=" + os.path.join(case_dir, "out")]), state_dict=sd, now="T")
        ckpt = torch.load(res["checkpoint"], map_location="cpu", weights_only=False)["state_dict"]
        with open(res["checkpoint"], "wb") as f:  # the digest below then covers the tensors, key by key
            for k in sorted(ckpt):
                f.write(k.encode() + b"\0" + str(ckpt[k].dtype).encode() + str(tuple(ckpt[k].shape)).encode() + ckpt[k].contiguous().numpy().tobytes())
    elif driver == "predict":
        from crossscore_amd.predict import predict
        res = predict(load_config("default_predict", overrides + ["logger.predict.out_dir=" + os.path.join(case_dir, "out")]), state_dict=sd, now="T")
    else:
        from crossscore_amd.evaluate import evaluate
        res = evaluate(load_config("default_test", overrides + ["logger.test.out_dir=" + os.path.join(case_dir, "out")]), state_dict=sd, now="T")
h, n = hashlib.sha256(), 0
for d, ds, fs in os.walk(case_dir):
    ds.sort()
    for f in sorted(fs):
        p = os.path.join(d, f)
        h.update(os.path.relpath(p, case_dir).encode() + b"\0" + open(p, "rb").read() + b"\0")
        n += 1
rel = lambda v: os.path.relpath(v, case_dir) if os.path.isabs(v) else v
res.pop("query_images_per_sec", None)
for k in drop:
    res.pop(k, None)
if "files" in res:
    res["files"] = sorted(rel(f) for f in res["files"])
for k in ("out_dir", "version_dir", "csv", "checkpoint"):
    if k in res:
        res[k] = rel(res[k])
for k in ("files", "rows", "batches", "metrics", "losses"):
    if k in res:
        res[k] = "%d:%s" % (len(res[k]), hashlib.sha256(repr(res[k]).encode()).hexdigest()[:16])
print("%d files %s %s" % (n, h.hexdigest()[:32], json.dumps(res, sort_keys=True)))
'''


def make_inputs(root):
    """(predict overrides, evaluate overrides, JPEG query directory) over input trees generated under root."""
    from PIL import Image

    sys.path.insert(0, os.path.join(REPO, "tests"))
    from nvs_tree import make_tree

    rng = np.random.Generator(np.random.PCG64(7))
    base = os.path.join(root, "data", "gaussian", "mfr", "res_540", "s00001", "test", "ours_1000")
    dirs = {k: os.path.join(base, k) for k in ("renders", "gt", "renders_jpeg")}
    for d in dirs.values():
        os.makedirs(d)
    yy, xx = np.mgrid[0:70, 0:90]
    for kind, n, off in (("renders", 5, 0), ("gt", 4, 100)):
        for i in range(n):
            img = np.stack([(xx * 3 + i * 17 + off) % 256, (yy * 2 + i * 29) % 256, (xx + yy + i * 11) % 256], axis=2).astype(np.uint8)
            img = (img.astype(np.int32) + rng.integers(-20, 21, size=img.shape)).clip(0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(dirs[kind], f"frame_{i:05}.png"))
            if kind == "renders":
                Image.fromarray(img).save(os.path.join(dirs["renders_jpeg"], f"frame_{i:05}.jpg"), format="JPEG", quality=90)
    common = [f"model.backbone.from_pretrained={BACK}", "this_main.resize_short_side=56", "data.neighbour_config.deterministic=True"]
    pred = common + [f"data.dataset.query_dir={dirs['renders']}", f"data.dataset.reference_dir={dirs['gt']}", "data.neighbour_config.cross=3",
                     "data.loader.validation.batch_size=2", "logger.predict.write.config.score_map_colour_mode=gray"]
    ev = common + [f"data.dataset.path={make_tree(os.path.join(root, 'nvs'))}", "data.dataset.num_gaussians_iters=2",
                   "data.loader.validation.batch_size=4", "data.loader.validation.num_workers=2"]
    return pred, ev, dirs["renders_jpeg"]


def cases(pred, ev, jpeg_dir):
    no_imgs = ["logger.predict.write.flag.image_query=False", "logger.predict.write.flag.image_reference=False"]
    grid = [(c, f, d) for c in (True, False) for f in ("auto", False) for d in ("host", "gpu")]
    knobs = lambda c, f, d: [f"this_main.cache_reference_tokens={c}", f"this_main.fused_input_stage={f}", f"this_main.png_decoder={d}"]  # noqa: E731
    for (c, f, d), depth in itertools.product(grid, (1, 3)):
        yield "predict", f"predict cache={c} fused={f} png_decoder={d} in_flight={depth}", pred + no_imgs + knobs(c, f, d) + [f"this_main.batches_in_flight={depth}"]
    yield "predict", "predict every writer flag on", pred + [f"logger.predict.write.flag.{k}=True" for k in ("item_path_json", "score_map_gt", "attn_weights")] + \
        ["model.need_attn_weights=True", "model.need_attn_weights_head_id=1"]
    yield "predict", "predict JPEG queries jpeg_decoder=gpu", [o for o in pred if not o.startswith("data.dataset.query_dir=")] + no_imgs + \
        [f"data.dataset.query_dir={jpeg_dir}", "this_main.jpeg_decoder=gpu"]
    for f, d, depth in (("auto", "host", 3), (False, "gpu", 3), (False, "host", 1), ("auto", "gpu", 1)):
        yield "predict", f"predict strategy=similar fused={f} png_decoder={d} in_flight={depth}", \
            pred + no_imgs + knobs(True, f, d) + [f"this_main.batches_in_flight={depth}", "data.neighbour_config.strategy=similar", "logger.predict.write.flag.item_path_json=True"]
    for (c, f, d), gt, shuffle in itertools.product(grid, ("files", "compute"), (False, True)):
        yield "evaluate", f"evaluate cache={c} fused={f} png_decoder={d} gt_metric_maps={gt} shuffle={shuffle}", \
            ev + knobs(c, f, d) + [f"this_main.gt_metric_maps={gt}", f"data.loader.validation.shuffle={shuffle}"]
    yield "evaluate", "evaluate limit_test_batches=2", ev + ["trainer.limit_test_batches=2"]
    # what the scoring run has learnt since: each over both input stages (vis_sheet keeps auto on the two-launch stage)
    ev_no_imgs = [o.replace(".predict.", ".test.") for o in no_imgs]
    for f in ("auto", False):
        fused = [f"this_main.fused_input_stage={f}"]
        yield "predict", f"predict reference_use + images fused={f}", pred + no_imgs + fused + ["this_main.reference_use=True", "this_main.reference_use_images=True"]
        for key in ("score_pool", "vis_sheet"):
            yield "predict", f"predict {key} fused={f}", pred + no_imgs + fused + [f"this_main.{key}=True"]
            yield "evaluate", f"evaluate {key} fused={f}", ev + ev_no_imgs + fused + [f"this_main.{key}=True"]
        yield "evaluate", f"evaluate strategy=similar fused={f}", ev + ev_no_imgs + fused + \
            ["data.neighbour_config.strategy=similar", "data.neighbour_config.cross=2", "logger.test.write.flag.item_path_json=True"]
    fit = [o for o in ev if not o.startswith("data.loader.validation.")] + ["data.loader.train.batch_size=4", "data.loader.train.num_workers=2",
                                                                         "trainer.max_epochs=2", "trainer.lr_scheduler.step_size=1", "trainer.lr_scheduler.gamma=0.5"]
    for c, gt in ((True, "files"), (False, "files"), (True, "compute")):
        yield "fit_head", f"fit_head cache={c} gt_metric_maps={gt}", fit + [f"this_main.cache_reference_tokens={c}", f"this_main.gt_metric_maps={gt}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--jobs", type=int, default=1, help="children running side by side (each opens the GPU: keep it small)")
    ap.add_argument("--only", choices=("predict", "evaluate", "fit_head"))
    ap.add_argument("--match", help="only the cases whose name holds this text")
    ap.add_argument("--drop-result-key", action="append", default=[], help="a result key to leave out of the comparison (reported by one tree only)")
    args = ap.parse_args()
    trees = (("parent", os.path.abspath(args.parent)), ("new", os.path.abspath(args.new)))
    failed = []

    def child(tag, tree, root, k, driver, overrides):
        if failed:
            return None
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", CHILD, tree, driver, os.path.join(root, tag, f"case_{k:02}"), ",".join(args.drop_result_key)] + overrides,
                           capture_output=True, text=True)
        if r.returncode != 0:
            failed.append((tag, k, r.returncode, r.stdout[-1500:], r.stderr[-1500:]))
            return None
        return r.stdout.strip().splitlines()[-1]

    with tempfile.TemporaryDirectory() as root:
        todo = [c for c in cases(*make_inputs(root)) if args.only in (None, c[0]) and (args.match is None or args.match in c[1])]
        with ThreadPoolExecutor(max_workers=max(1, args.jobs)) as ex:
            futs = [[ex.submit(child, tag, tree, root, k, driver, over) for tag, tree in trees] for k, (driver, _, over) in enumerate(todo)]
            differ = 0
            for (driver, name, _), (fa, fb) in zip(todo, futs):
                a, b = fa.result(), fb.result()
                if failed:
                    break
                differ += a != b
                print(name)
                print("  parent " + a)
                print("  new    " + b if a != b else "  new    the same line")
    if failed:
        tag, k, rc, out, err = failed[0]
        print(out, err, sep="\n")
        sys.exit("driver_ab: the %s child of case %d ended with status %d; stopping" % (tag, k, rc))
    print("%d cases, %d differ between the trees" % (len(todo), differ))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
