"""The ground-truth score summary's golden (tests/golden/s0_gt_summary.json, made by tests/golden/make_golden_summary.py from the reference's
SummaryWriterGroundTruth / SummaryReader over nvs_tree.make_tree(seed=GOLDEN["seed"])) and the CSV reader of its tests."""
import csv
import json
import os

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "s0_gt_summary.json")))
TOKEN = GOLDEN["root_token"]  # stands for the tree's root in the golden's paths


def read_rows(path):
    """-> (header, rows) of a CSV as lists of strings"""
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def golden_rows(key, root):
    return [[c.replace(TOKEN, root.lstrip("/")) for c in r] for r in GOLDEN[key]]
