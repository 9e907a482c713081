"""Scene builders and driver runners of the predict / evaluate / summary tests: synthetic image directories, the runs over them, and readers
of what the runs wrote."""
import csv
import os
import shutil

import numpy as np

from nets import TINY, arch_of, state_dict_for

# query index -> its copy's name in reference_dir (before, between and behind the others): make_scene_with_copies
COPIES = {1: "copy_b.png", 3: "copy_a.png", 4: "zz_copy.png"}


def make_scene(root, n_query=3, n_ref=4, h=70, w=84, seed=7):
    """<root>/<method>/<dataset>/<res>/<scene>/test/ours_1000/{renders,gt}/frame_XXXXX.png, the depth the reference's CSV
    grouping indexes into (score_summariser.py:180-212)."""
    from PIL import Image

    rng = np.random.Generator(np.random.PCG64(seed))
    base = os.path.join(root, "gaussian", "mfr", "res_540", "s00001", "test", "ours_1000")
    qd, rd = os.path.join(base, "renders"), os.path.join(base, "gt")
    os.makedirs(qd)
    os.makedirs(rd)
    yy, xx = np.mgrid[0:h, 0:w]
    for d, n, off in ((qd, n_query, 0), (rd, n_ref, 100)):
        for i in range(n):
            img = np.stack([(xx * 3 + i * 17 + off) % 256, (yy * 2 + i * 29) % 256, (xx + yy + i * 11) % 256], axis=2).astype(np.uint8)
            img = (img.astype(np.int32) + rng.integers(-20, 21, size=img.shape)).clip(0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(d, f"frame_{i:05}.png"))
    return qd, rd


def make_scene_with_copies(root, n_query=6, n_other=4, h=70, w=90, seed=7):
    """make_scene plus byte copies of the queries of COPIES under other names in the reference directory"""
    qd, rd = make_scene(root, n_query, n_other, h, w, seed)
    for i, name in COPIES.items():
        shutil.copyfile(os.path.join(qd, f"frame_{i:05}.png"), os.path.join(rd, name))
    return qd, rd


def tree_bytes(out_dir):
    """{relative path: bytes} of every file under out_dir"""
    files = {}
    for d, _, fs in os.walk(out_dir):
        for f in fs:
            p = os.path.join(d, f)
            files[os.path.relpath(p, out_dir)] = open(p, "rb").read()
    return files


def run_predict_similar(out, qd, rd, backbone, sd, *over):
    """predict with data.neighbour_config.strategy=similar, two references per query, gray score maps"""
    from crossscore_amd.config import load_config
    from crossscore_amd.predict import predict

    cfg = load_config("default_predict", [f"data.dataset.query_dir={qd}", f"data.dataset.reference_dir={rd}", f"model.backbone.from_pretrained={backbone}",
                                          "this_main.resize_short_side=56", "data.neighbour_config.cross=2", "data.neighbour_config.strategy=similar",
                                          "data.loader.validation.batch_size=2", f"logger.predict.out_dir={out}",
                                          "logger.predict.write.config.score_map_colour_mode=gray", "logger.predict.write.flag.item_path_json=True", *over])
    return predict(cfg, state_dict=sd, now="T")


def run_evaluate(tree, tmp_path, name, extra, back=TINY, seed=7):
    """crossscore_amd.evaluate over an nvs_tree.make_tree tree -> (result, captured batches, state dict, arch)"""
    import torch

    from crossscore_amd.config import load_config
    from crossscore_amd.evaluate import evaluate

    arch = arch_of(back)
    sd = state_dict_for(back, seed, arch)
    cfg = load_config("default_test", [f"data.dataset.path={tree}", f"model.backbone.from_pretrained={back}", "this_main.resize_short_side=56",
                                       "data.dataset.num_gaussians_iters=2", "data.loader.validation.batch_size=4",
                                       "data.loader.validation.num_workers=2", "data.neighbour_config.deterministic=True",
                                       f"logger.test.out_dir={tmp_path}/{name}"] + list(extra))
    cap = []
    np.random.seed(0)
    with torch.no_grad():
        res = evaluate(cfg, state_dict=sd, now="NOW", capture=cap)
    return res, cap, sd, arch


def read_csv_dicts(path):
    return list(csv.DictReader(open(path)))
