"""Golden vectors for the score summary: what the reference's SummaryWriterGroundTruth and SummaryReader (utils/io/score_summariser.py) make of
the tree of tests/nvs_tree.py.  Imports the reference module with a stub for imageio (absent offline), as make_golden_nvs.py does; pandas and
tqdm are needed.  Only names, printed numbers and verdicts are written: s0_gt_summary.json, with the temporary root replaced by a token.

The reference forms its values as fp32 means; crossscore_amd.summarise_gt forms them exactly from integer sums.  The golden comparison is string
equality of the "%.4f" fields, so before anything is written every exact value must lie farther from a rounding boundary than the reference's
own fp32 value lies from it (both computed here).  Seed 0 passes; should a change of the tree ever fail this, change the seed, not the test.
usage: python tests/golden/make_golden_summary.py <checkout of the reference>"""
import csv
import json
import math
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from nvs_tree import make_tree  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else None
TOKEN = "<ROOT>"
SEED = 0
FILTERS = {  # name: (method_list, scene_list, split_list, iter_list)
    "all": ([""], [""], [""], []),
    "scene_a_test_1000_7000": (["gaussian"], ["scene_a"], ["test"], [1000, 7000]),
}


def _import_reference():
    sys.modules["imageio"] = types.ModuleType("imageio")
    sys.path[:0] = [REF]
    sys.dont_write_bytecode = True
    from utils.io import score_summariser
    return score_summariser


def _read_rows(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def exact_values(path_ssim, path_mae):
    from PIL import Image

    cs = np.array(Image.open(path_ssim)).astype(np.int64)
    cm = np.array(Image.open(path_mae)).astype(np.int64)
    n = cs.size
    s1, s2, s3, s4 = int(cs.sum()), int(np.clip(cs, 32767, 65534).sum()), int(cm.sum()), int((cm * cm).sum())
    mse = s4 / (65535 * 65535 * n)
    return [s1 / (32767 * n) - 1.0, (s2 - 32767 * n) / (32767 * n), s3 / (65535 * n), mse, -10.0 * math.log10(mse)]


def boundary_distance(v):
    """distance of v from the nearest value at which "%.4f" changes its last digit"""
    return abs((v * 1e4) % 1.0 - 0.5) / 1e4


def records(df, root):
    out = []
    for rec in df.to_dict(orient="records"):
        out.append({k: (v.replace(root, TOKEN) if isinstance(v, str) else float(v)) for k, v in rec.items()})
    return out


def main():
    if REF is None:
        raise SystemExit(__doc__)
    ss = _import_reference()
    tmp = tempfile.mkdtemp()
    root = tmp.lstrip("/")  # rendered_dir loses the leading "/" (os.path.join of the split parts)
    tree = make_tree(os.path.join(tmp, "gaussian", "mfr"), seed=SEED)
    dir_in = os.path.join(tree, "res_540")
    gt_dir = os.path.join(tmp, "summary_gt")
    writer = ss.SummaryWriterGroundTruth(dir_in=dir_in, dir_out=gt_dir, num_workers=0, fast_debug=-1, force=True)
    writer.write_csv()
    columns, rows = _read_rows(writer.csv_path)
    assert columns == writer.columns, columns

    # the margin: exact value to the nearest rounding boundary against the reference's fp32 value to the exact one
    from glob import glob
    reader = ss.ScoreReader(sorted(glob(os.path.join(dir_in, "**/metric_map"), recursive=True)))
    assert len(reader) == len(rows)
    min_dist, max_dev = math.inf, 0.0
    for i in range(len(reader)):
        r = reader[i]
        ref = [float(r["ssim_-1_1"]), float(r["ssim_0_1"]), float(r["mae"]), float(r["mse"]), float(np.asarray(r["psnr"]).reshape(-1)[0])]
        path_ssim = str(r["path_ssim"])
        ex = exact_values(path_ssim, path_ssim.replace("/metric_map/ssim/", "/metric_map/mae/"))
        for name, e, f, printed in zip(columns[3:], ex, ref, rows[i][3:]):
            dev, dist = abs(f - e), boundary_distance(e)
            assert dist > dev, f"{path_ssim} {name}: exact {e!r} lies {dist:.3e} from a rounding boundary, the reference's fp32 value {dev:.3e} from it"
            assert "%.4f" % e == printed, (path_ssim, name, e, printed)
            min_dist, max_dev = min(min_dist, dist), max(max_dev, dev)

    # a predicted summary of the same frames (the layout writers.ScoreSummariser writes), for the reader
    pred_dir = os.path.join(tmp, "summary_pred")
    os.makedirs(os.path.join(pred_dir, "mfr"))
    pred_rows = [[r[0], r[1], r[2], "%.4f" % (0.25 + 0.5 * ((37 * i) % 17) / 17)] for i, r in enumerate(rows)]
    pred_rows.sort(key=lambda r: (r[0], r[1], r[2]))
    with open(os.path.join(pred_dir, "mfr", "gaussian.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(columns[:3] + ["pred_ssim_0_1"])
        w.writerows(pred_rows)

    read = {}
    for name, (methods, scenes, splits, iters) in FILTERS.items():
        gt = ss.SummaryReader.read_summary(gt_dir, "mfr", methods, scenes, splits, iters)
        pred = ss.SummaryReader.read_summary(pred_dir, "mfr", methods, scenes, splits, iters)
        read[name] = {"method_list": methods, "scene_list": scenes, "split_list": splits, "iter_list": iters,
                      "gt": records(gt, root), "pred": records(pred, root)}

    gt = ss.SummaryReader.read_summary(gt_dir, "mfr", [""], [""], [""], [])
    pred = ss.SummaryReader.read_summary(pred_dir, "mfr", [""], [""], [""], [])

    def verdict(a, b):
        try:
            ss.SummaryReader.check_summary_gt_prediction_rows(a, b)
            return None
        except ValueError as e:
            return str(e)

    swapped_dir = pred.copy()
    swapped_dir.loc[0, "rendered_dir"] = pred.loc[1, "rendered_dir"] + "_x"
    swapped_name = pred.copy()
    swapped_name.loc[0, "image_name"] = "99999.png"
    check = {"match": verdict(gt, pred), "length": verdict(gt, pred.iloc[:-1].reset_index(drop=True)),
             "rendered_dir": verdict(gt, swapped_dir), "image_name": verdict(gt, swapped_name)}
    assert check["match"] is None and all(check[k] for k in ("length", "rendered_dir", "image_name")), check

    out = {"root_token": TOKEN, "seed": SEED, "dataset": "mfr", "method": "gaussian", "columns": columns,
           "rows": [[c.replace(root, TOKEN) for c in r] for r in rows],
           "pred_columns": columns[:3] + ["pred_ssim_0_1"], "pred_rows": [[c.replace(root, TOKEN) for c in r] for r in pred_rows],
           "read_summary": read, "check": check,
           "margin": {"min_boundary_distance": min_dist, "max_reference_deviation": max_dev}}
    with open(os.path.join(HERE, "s0_gt_summary.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("rows", len(rows), "margin", out["margin"], "filters", {k: len(v["gt"]) for k, v in read.items()})


if __name__ == "__main__":
    main()
