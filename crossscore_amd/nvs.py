"""Test-phase data side: which files form a (render, GT metric map, N references) item of the multi-scene NvsDataset tree.

Mirrors, for the test path:
  get_dataset                      dataloading/data_manager.py:7-41        dataset.path a string or a list, concatenated in order
  NvsDataset.__init__ / get_paths  dataloading/dataset/nvs_dataset.py:87-147, 299-427
  NeighbourSelector                nvs_dataset.py:14-84                    index order scene -> gs_train, gs_test -> iteration -> image
The tree under <path>/<resolution>/:
  split.json                                  {"train": [...], "test": [...], ...}: scene names per data split
  <scene>/{train,test}/<name>_<iter>/renders/ the query images (renders of that split at that iteration)
  <scene>/{train,test}/<name>_<iter>/gt/      the captured images: the cross references of the OTHER split's queries
  <scene>/{train,test}/<name>_<iter>/metric_map/{ssim,mae}/   GT maps of the renders (16-bit PNG)
With this_main.gt_metric_maps=compute the maps are formed on the device from renders/<name> and gt/<name> of the same iteration directory
(cs_op_gt_metric_map_u8): items then carry "query/gt" and metric_map/ is not looked at.
Pixel work (decoding aside) is the GPU's: data.InputStage for the images and, for the maps, InputStage.metric_map.
"""
from __future__ import annotations

import json
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Union

from .data import EMPTY, sample_references

DATA_SPLITS = ("train", "test", "val", "val_small", "test_small")


def metric_load_dir(metric_type: str) -> str:
    """nvs_dataset.py:299-319: SSIM maps for ssim, MAE maps for mae and mse (mse is the MAE map squared)."""
    if metric_type in ("ssim", "mae"):
        return f"metric_map/{metric_type}"
    if metric_type == "mse":
        return "metric_map/mae"
    raise ValueError(f"Invalid metric type {metric_type}")


def get_paths(scene_paths: Sequence[Path], num_gaussians_iters: int, metric_dir: Optional[str]) -> Dict[str, dict]:
    """NvsDataset.get_paths (nvs_dataset.py:321-426): per scene and split, iteration -> sorted file lists, with the query / cross-reference
    pairing.  As in the reference, a missing metric directory is filled with as many "empty_image" placeholders as the split has iterations
    so far (nvs_dataset.py:380), and any list whose length differs from its iteration's gt list raises ValueError.
    metric_dir None (compute mode, this build's): no metric directory is looked at, every score map is "empty_image", and each query side
    also carries "gt", the captured images of its own split."""
    names = sorted(p.name for p in scene_paths)
    kinds = ("renders", "gt", "score_map")
    allp = {n: {s: {k: {} for k in kinds} for s in ("train", "test")} for n in names}
    for sp in scene_paths:
        sn = sp.name
        for split in ("train", "test"):
            d = Path(sp, split)
            iters = sorted(os.listdir(d), key=lambda x: int(x.split("_")[-1]))
            if num_gaussians_iters > 0:
                iters = iters[:num_gaussians_iters]
            for it in iters:
                num = int(it.split("_")[-1])
                for k in kinds:
                    if k == "score_map" and metric_dir is None:
                        allp[sn][split][k][num] = [EMPTY] * len(allp[sn][split]["gt"][num])
                        continue
                    img_dir = Path(d, it, metric_dir if k == "score_map" else k)
                    if os.path.exists(img_dir):
                        paths = [str(img_dir / f) for f in sorted(os.listdir(img_dir))]
                    else:
                        paths = [EMPTY] * len(allp[sn][split]["gt"])
                    allp[sn][split][k][num] = paths
            for k in kinds:
                for num, paths in allp[sn][split][k].items():
                    if len(paths) != len(allp[sn][split]["gt"][num]):
                        raise ValueError(f"Number of items mismatch in {sn}/{split}/{num}/{k}")
    out = {}
    for sn in names:
        out[sn] = {}
        for split, cross in (("train", "test"), ("test", "train")):
            renders = allp[sn][split]["renders"]
            out[sn][f"gs_{split}"] = {
                "query": {"images": renders, "score_map": allp[sn][split]["score_map"], "N_iters": len(renders),
                          "N_imgs_per_iter": len(next(iter(renders.values())))},
                "reference": {"cross": {"images": allp[sn][cross]["gt"]}},
            }
            if metric_dir is None:
                out[sn][f"gs_{split}"]["query"]["gt"] = allp[sn][split]["gt"]
    return out


class NvsItems:
    """Index -> file paths of one item, like get_dataset(...)[idx]["item_paths"] for the NvsDataset layout (ConcatDataset over the entries
    of `dataset_path`).  References are drawn when an item is asked for, by data.sample_references (numpy's global RNG unless
    deterministic), as NeighbourSelector.__getitem__ does.
    compute_gt (this_main.gt_metric_maps=compute): an item also carries "query/gt", the file of the same iteration and index in the gt/ list
    of the query's own split, its "query/score_map" is "empty_image", and no metric_map/ directory is looked at.
    candidates (neighbour strategy similar): nothing is drawn.  An item carries "reference/cross/imgs": None and
    "reference/cross/group", the place in `groups` of the `cross` list random would draw from -- the captured images of the other split of the
    query's scene and iteration; `groups` lists each distinct `cross` list once, in index order.  The views are chosen on the device."""

    def __init__(self, dataset_path: Union[str, Sequence[str]], resolution, data_split: str, neighbour_config, metric_type: str,
                 num_gaussians_iters: int = -1, compute_gt: bool = False, candidates: bool = False):
        if data_split not in DATA_SPLITS:
            raise ValueError(f"Unknown data_split {data_split}")
        if neighbour_config["strategy"] == "similar" and not candidates:
            raise NotImplementedError("neighbour strategy similar: without candidates=True this class draws an item's references on the host, "
                                      "which is what random does; the choice on the device needs the candidate lists (from_config asks for "
                                      "them).  Items without candidate lists serve similar for predict only (data.SimpleReferenceItems)")
        if neighbour_config["strategy"] not in (("random", "similar") if candidates else ("random",)):
            raise NotImplementedError(f"neighbour strategy {neighbour_config['strategy']} (sampler.py:60-66 only knows 'random'; this build adds 'similar')")
        if isinstance(dataset_path, str):
            roots = [dataset_path]
        elif isinstance(dataset_path, (list, tuple)):
            roots = list(dataset_path)
        else:
            raise ValueError("cfg.data.dataset.path should be a string or a list")
        self.n_cross = int(neighbour_config["cross"])
        self.deterministic = bool(neighbour_config["deterministic"])
        self.compute_gt = bool(compute_gt)
        self.candidates = bool(candidates)
        self.groups: List[List[str]] = []
        self._group_of: List[int] = []
        seen: Dict[tuple, int] = {}
        mdir = metric_load_dir(metric_type)  # (validates the metric type in both modes)
        if self.compute_gt:
            mdir = None
        # (query, score map, cross list[, gt]) per index, every dataset of the list in turn
        self._index: List[tuple] = []
        for root in roots:
            res = resolution if resolution is not None else os.listdir(root)[0]
            base = Path(root, res)
            with open(base / "split.json") as f:
                scenes = json.load(f)[data_split]
            scene_paths = [p for p in (base / n for n in sorted(scenes)) if p.exists()]
            paths = get_paths(scene_paths, int(num_gaussians_iters), mdir)
            for sn in sorted(paths):
                for split in ("train", "test"):
                    q = paths[sn][f"gs_{split}"]
                    per_iter = q["query"]["N_imgs_per_iter"]
                    iter_names = list(q["query"]["images"].keys())
                    for idx in range(q["query"]["N_iters"] * per_iter):
                        it, im = iter_names[idx // per_iter], idx % per_iter
                        entry = (q["query"]["images"][it][im], q["query"]["score_map"][it][im], q["reference"]["cross"]["images"][it])
                        self._index.append(entry + ((q["query"]["gt"][it][im],) if self.compute_gt else ()))
                        if self.candidates:
                            key = tuple(entry[2])
                            if key not in seen:
                                seen[key] = len(self.groups)
                                self.groups.append(list(key))
                            self._group_of.append(seen[key])

    def __len__(self) -> int:
        return len(self._index)

    def ground_truth_files(self):
        """(query path, ground-truth map path or "empty_image") of every item, in item order, without building the items: no reference is
        sampled, so the seeded generator is left as it is."""
        return [(entry[0], entry[1]) for entry in self._index]

    def __getitem__(self, idx: int) -> Dict[str, object]:
        query, score_map, cross = self._index[idx][:3]
        if self.candidates:  # no RNG is drawn
            item = {"query/img": query, "query/score_map": score_map, "reference/cross/imgs": None, "reference/cross/group": self._group_of[idx]}
        else:
            refs = sample_references(cross, self.n_cross, self.deterministic) if self.n_cross > 0 else []
            item = {"query/img": query, "query/score_map": score_map, "reference/cross/imgs": refs}
        if self.compute_gt:
            item["query/gt"] = self._index[idx][3]
        return item

    @classmethod
    def from_config(cls, cfg, compute_gt: bool = False) -> "NvsItems":
        """get_dataset(cfg, ..., cfg.this_main.data_split) of task/test.py:95-97."""
        d = cfg.data.dataset
        return cls(d.path, d.get("resolution"), cfg.this_main.data_split, cfg.data.neighbour_config, cfg.model.predict.metric.type,
                   int(d.get("num_gaussians_iters", -1)), compute_gt, candidates=str(cfg.data.neighbour_config.strategy) == "similar")


def random_order(n: int, seed: int) -> List[int]:
    """shuffle: True -- a permutation from torch.randperm with a generator seeded from lightning.seed.  Lightning's sampler draws differ;
    the per-image outputs do not depend on the order, the epoch correlation does (through the batch grouping)."""
    import torch

    g = torch.Generator()
    g.manual_seed(int(seed))
    return torch.randperm(n, generator=g).tolist()
