"""A seeded, small NvsDataset tree (the layout crossscore_amd/nvs.py reads) for the test-phase tests and tools/evaluate_e2e.py.

<root>/res_540/split.json      test: scene_a, scene_b and scene_gone (absent on disk: filtered out); train: scene_a; val: scene_c
scene_a  60 x 84   iterations 1000, 7000, 30000 (num_gaussians_iters=2 keeps two); train 3 images per iteration, test 2: with cross = 5
                   every reference list is short and gets "empty_image" padding.  GT maps under metric_map/ssim and metric_map/mae.
scene_b  60 x 84   one iteration, one image per split, no metric_map directory: placeholders ("empty_image")
scene_c  540 x 720 one iteration, one image per split (the resize path at the dataset's real size)
"""
import json
import os

import numpy as np

SCENES = {  # name: (h, w, iterations, images per iteration of train / test, metric maps)
    "scene_a": (60, 84, (30000, 1000, 7000), (3, 2), True),
    "scene_b": (60, 84, (1000,), (1, 1), False),
    "scene_c": (540, 720, (1000,), (1, 1), True),
}
SPLITS = {"test": ["scene_a", "scene_b", "scene_gone"], "train": ["scene_a"], "val": ["scene_c"]}


def _rgb(rng, h, w):
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    img[..., 1] = ((np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 2) % 256).astype(np.uint8)
    return img


def _map(rng, h, w):
    # a smooth field plus noise over the whole 16-bit range (the ends included)
    y, x = np.meshgrid(np.linspace(0, 3, h), np.linspace(0, 4, w), indexing="ij")
    base = (np.sin(y) * np.cos(x) + 1.0) * 0.5
    m = np.clip(base * 65535 + rng.normal(0, 4000, size=(h, w)), 0, 65535).astype(np.uint16)
    m[0, 0], m[0, 1] = 0, 65535
    return m


def make_tree(root, seed: int = 0, scenes=None) -> str:
    """Writes the tree under `root` (created) and returns the dataset path (the directory holding res_540)."""
    from PIL import Image

    rng = np.random.Generator(np.random.PCG64(seed))
    base = os.path.join(str(root), "res_540")
    os.makedirs(base, exist_ok=True)
    with open(os.path.join(base, "split.json"), "w") as f:
        json.dump(SPLITS, f)
    for name in sorted(scenes or SCENES):
        h, w, iters, counts, maps = SCENES[name]
        for split, n in zip(("train", "test"), counts):
            for it in iters:
                d = os.path.join(base, name, split, f"ours_{it}")
                kinds = ["renders", "gt"] + (["metric_map/ssim", "metric_map/mae"] if maps else [])
                for k in kinds:
                    os.makedirs(os.path.join(d, k), exist_ok=True)
                for i in range(n):
                    fn = f"frame_{i:05d}.png"
                    Image.fromarray(_rgb(rng, h, w)).save(os.path.join(d, "renders", fn))
                    Image.fromarray(_rgb(rng, h, w)).save(os.path.join(d, "gt", fn))
                    if maps:
                        Image.fromarray(_map(rng, h, w)).save(os.path.join(d, "metric_map/ssim", fn))
                        Image.fromarray(_map(rng, h, w)).save(os.path.join(d, "metric_map/mae", fn))
    return str(root)


if __name__ == "__main__":
    import sys

    print(make_tree(sys.argv[1]))
