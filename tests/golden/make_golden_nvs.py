"""Golden vectors for the test phase's data side: what the reference's NvsDataset (dataloading/dataset/nvs_dataset.py) makes of the tree of
tests/nvs_tree.py.  Imports the reference module with stub modules for the packages absent offline (omegaconf, imageio), as make_golden.py
does, and stands in F.interpolate(mode="bilinear", antialias=True) for torchvision's T.Resize, as make_golden_preprocess.py does.  Only names
and numbers are written: n0_nvs_items.json (item paths relative to the tree) and n0_nvs_maps.npz (processed GT maps).
usage: python tests/golden/make_golden_nvs.py <checkout of the reference>"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from nvs_tree import make_tree  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else None


class _Attr(dict):
    __getattr__ = dict.__getitem__


def _import_reference():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    stub("imageio")
    stub("omegaconf", OmegaConf=types.SimpleNamespace(create=lambda d: _Attr(d)), DictConfig=dict, ListConfig=list)
    sys.path[:0] = [REF]
    sys.dont_write_bytecode = True
    from dataloading.dataset import nvs_dataset
    return nvs_dataset


def out_size(h, w, short):
    return (short, int(short * w / h)) if h <= w else (int(short * h / w), short)


class Resize:
    """T.Resize(short, BILINEAR, antialias=True) on float tensors (..., H, W)."""

    def __init__(self, short):
        self.size = [short]
        self.short = short

    def __call__(self, x):
        lead = x.shape[:-2]
        x4 = x.reshape(-1, 1, *x.shape[-2:])
        y = F.interpolate(x4, size=out_size(*x.shape[-2:], self.short), mode="bilinear", align_corners=False, antialias=True)
        return y.reshape(*lead, *y.shape[-2:])


def main():
    if REF is None:
        raise SystemExit(__doc__)
    torch.set_num_threads(1)
    nvs = _import_reference()
    tmp = tempfile.mkdtemp()
    path = make_tree(tmp)
    rel = lambda p: p if p == "empty_image" else os.path.relpath(p, path)  # noqa: E731
    cross = dict(strategy="random", cross=5, deterministic=True)
    items = {}
    for det in (True, False):
        ds = nvs.NvsDataset(path, None, "test", {}, dict(cross, deterministic=det), "ssim", 0, 1, num_gaussians_iters=2)
        np.random.seed(0 if det else 1)  # short lists are padded and permuted even when deterministic (sampler.py:22-27)
        sel = ds.neighbour_selector
        items["deterministic" if det else "random_seed1"] = [
            {k: (rel(v) if isinstance(v, str) else [rel(x) for x in v]) for k, v in sel[i].items()} for i in range(len(sel))]
    items["mae_score_maps"] = [rel(sel_it["query/score_map"]) for sel_it in (
        nvs.NvsDataset(path, None, "test", {}, cross, "mae", 0, 1, num_gaussians_iters=2).neighbour_selector[i] for i in range(9))]
    with open(os.path.join(HERE, "n0_nvs_items.json"), "w") as f:
        json.dump(items, f, indent=1)

    maps = {}
    modes = {"ssim_0_1": ("ssim", 0), "ssim_-1_1": ("ssim", -1), "mae": ("mae", 0), "mse": ("mse", 0)}
    cases = {  # name: (data split, item index, transforms)
        "a_noresize": ("test", 0, {"crop_integer_patches": "adaptive"}),
        "a_s518": ("test", 0, {"resize": Resize(518), "crop_integer_patches": "adaptive"}),
        "a_s37": ("test", 1, {"resize": Resize(37)}),
        "c_s518": ("val", 0, {"resize": Resize(518), "crop_integer_patches": "adaptive"}),
    }
    for cname, (split, idx, tf) in cases.items():
        for mname, (mt, mmin) in modes.items():
            ds = nvs.NvsDataset(path, None, split, tf, dict(cross, cross=1), mt, mmin, 1, num_gaussians_iters=2, return_item_paths=True)
            r = ds[idx]
            m = r["query/score_map"].numpy().astype(np.float32)
            key = f"{cname}/{mname}"
            maps[key + "/query"] = np.array(rel(r["item_paths"]["query/img"]))
            maps[key + "/shape"] = np.array(m.shape)
            if m.size <= 64 * 96:
                maps[key + "/out"] = m
            else:  # large: every 74th row, every 83rd column and the mean
                maps[key + "/rows"] = m[::74]
                maps[key + "/cols"] = m[:, ::83]
                maps[key + "/mean"] = np.array(m.mean(dtype=np.float64))
    np.savez_compressed(os.path.join(HERE, "n0_nvs_maps.npz"), **maps)
    print("items", {k: len(v) for k, v in items.items()}, "maps", len(maps))


if __name__ == "__main__":
    main()
