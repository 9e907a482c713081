"""Reads the score-summary CSVs and lines the ground-truth side up with the predicted side (the reference's SummaryReader,
utils/io/score_summariser.py:253-315, and utils/evaluation/metric.py:26-30 on the result).  Host only: the csv module and numpy.

    python -m crossscore_amd.summary --gt <dir> --pred <dir> --dataset <name> [--methods ... --scenes ... --splits ... --iters ...]
                                     [--gt_column gt_ssim_0_1] [--pred_column <inferred when the CSV has one pred_* column>]

<dir>/<dataset>/<method>.csv is what crossscore_amd.summarise_gt writes (--gt: its --dir_out) and what predict / evaluate write under
<run>/score_summary (--pred).  A summary is a list of rows, each a dict: scene_name, rendered_dir and image_name as strings, every other column
as a float, plus method_name (the file's stem).
"""
from __future__ import annotations

import argparse
import csv
from pathlib import Path
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np

KEY_COLUMNS = ("scene_name", "rendered_dir", "image_name")
SORT_COLUMNS = ("scene_name", "rendered_dir", "image_name", "method_name")


def read_csv(path, method_name: str) -> List[dict]:
    """The rows of one CSV.  The key columns stay the strings the file holds.  This departs from the reference on purpose: pandas there infers
    an integer type for a scene_name or image_name column that is all digits ("00012" becomes 12, and sorts as a number); strings keep the
    names as written, compare equal between the two CSVs whatever each file's other rows look like, and sort as the directory listing does."""
    with open(path, newline="") as f:
        return [dict({k: (v if k in KEY_COLUMNS else float(v)) for k, v in row.items()}, method_name=method_name) for row in csv.DictReader(f)]


def read_summary(summary_dir, dataset: str, method_list: Sequence[str], scene_list: Sequence[str], split_list: Sequence[str],
                 iter_list: Sequence) -> List[dict]:
    """SummaryReader.read_summary: the rows of <summary_dir>/<dataset>/<method>.csv for the methods of method_list ([""]: every file there),
    filtered by scene_name (scene_list, [""]: all), by part -2 of rendered_dir (split_list, [""]: all; the matches of each split in list order)
    and by rendered_dir ending in "ours_<i>" (iter_list, empty: all), then sorted by (scene_name, rendered_dir, image_name, method_name)."""
    summary_dir = Path(summary_dir).expanduser() / dataset
    available = sorted(f.stem for f in summary_dir.iterdir() if f.is_file())
    if list(method_list) != [""]:
        for m in method_list:
            if m not in available:
                raise ValueError(f"{m} is not available in {summary_dir}")
        methods = list(method_list)
    else:
        methods = available
    if not methods:
        raise ValueError(f"no summary to read in {summary_dir}")
    rows: List[dict] = []
    for m in methods:
        rows += read_csv(summary_dir / f"{m}.csv", m)
    if list(scene_list) != [""]:
        rows = [r for r in rows if r["scene_name"] in scene_list]
    if list(split_list) != [""]:
        rows = [r for split in split_list for r in rows if (r["rendered_dir"].split("/")[-2:-1] or [None])[0] == split]
    if len(iter_list) > 0:
        rows = [r for i in iter_list for r in rows if r["rendered_dir"].endswith(f"ours_{i}")]
    rows.sort(key=lambda r: tuple(r[k] for k in SORT_COLUMNS))  # stable, as the reference's lexsort
    return rows


def check_summary_gt_prediction_rows(summary_gt: Sequence[dict], summary_prediction: Sequence[dict]) -> None:
    if len(summary_gt) != len(summary_prediction):
        raise ValueError("Summary GT and prediction have different length")
    if [r["rendered_dir"] for r in summary_gt] != [r["rendered_dir"] for r in summary_prediction]:
        raise ValueError("Summary GT and prediction have different rendered_dir")
    if [r["image_name"] for r in summary_gt] != [r["image_name"] for r in summary_prediction]:
        raise ValueError("Summary GT and prediction have different image_name")


def pearson(a: Sequence[float], b: Sequence[float]) -> float:
    """The off-diagonal entry of corrcoef of the two columns (metric.py:26-30), in fp64; nan below two rows or without variance."""
    x, y = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if x.size < 2:
        return float("nan")
    dx, dy = x - x.mean(), y - y.mean()
    den = np.sqrt(np.dot(dx, dx) * np.dot(dy, dy))
    return float(np.dot(dx, dy) / den) if den > 0 else float("nan")


def correlate(summary_gt: Sequence[dict], summary_prediction: Sequence[dict], gt_column: str, pred_column: str) -> Dict[str, object]:
    """Checks that the two summaries hold the same frames in the same order, then returns {"all": r, "scenes": {scene_name: r}}: the Pearson
    coefficient of gt_column against pred_column over all rows and per scene."""
    check_summary_gt_prediction_rows(summary_gt, summary_prediction)
    g = [r[gt_column] for r in summary_gt]
    p = [r[pred_column] for r in summary_prediction]
    scenes: Dict[str, List[int]] = {}
    for i, r in enumerate(summary_gt):
        scenes.setdefault(r["scene_name"], []).append(i)
    return {"all": pearson(g, p), "scenes": {s: pearson([g[i] for i in idx], [p[i] for i in idx]) for s, idx in scenes.items()}}


def infer_pred_column(summary_prediction: Sequence[dict]) -> str:
    cols = sorted({k for r in summary_prediction for k in r if k.startswith("pred_")})
    if len(cols) != 1:
        raise ValueError(f"--pred_column is needed: the predicted summary has the columns {cols}")
    return cols[0]


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Correlate the predicted score summary with the ground-truth one.")
    p.add_argument("--gt", required=True, help="directory of the ground-truth summary (summarise_gt's --dir_out)")
    p.add_argument("--pred", required=True, help="directory of the predicted summary (<run>/score_summary)")
    p.add_argument("--dataset", required=True, help="dataset type: the sub-directory of both that holds <method>.csv")
    p.add_argument("--methods", nargs="*", default=[""])
    p.add_argument("--scenes", nargs="*", default=[""])
    p.add_argument("--splits", nargs="*", default=[""])
    p.add_argument("--iters", nargs="*", default=[])
    p.add_argument("--gt_column", default="gt_ssim_0_1")
    p.add_argument("--pred_column", default=None)
    return p.parse_args(argv)


def main(argv: Optional[Iterable[str]] = None) -> int:
    a = parse_args(None if argv is None else list(argv))
    filters = (a.methods or [""], a.scenes or [""], a.splits or [""], a.iters)
    gt = read_summary(a.gt, a.dataset, *filters)
    pred = read_summary(a.pred, a.dataset, *filters)
    pred_column = a.pred_column or infer_pred_column(pred)
    res = correlate(gt, pred, a.gt_column, pred_column)
    print(f"[crossscore_amd.summary] {len(gt)} frames, {a.gt_column} against {pred_column}")
    print(f"[crossscore_amd.summary] correlation all: {res['all']:.6f}")
    for s, r in res["scenes"].items():
        print(f"[crossscore_amd.summary] correlation {s}: {r:.6f}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
