"""The ground-truth metric-map definition of DESIGN.md section 6 (row f6), restated in torch on the CPU for the tests.

ssim_map(a, b, dtype, separable): a, b uint8 (H, W, 3) arrays; the SSIM map (H, W) in `dtype`, as a direct 11 x 11 conv2d with zero padding 5
(the definition; fp64 is the reference, fp32 the form whose own error is the tests' bar) or as the two 11-tap passes.
codes(m): the stored uint16 samples, trunc((m + 1) * 32767) in fp64.  mae_codes(a, b): (257 * sum_c |a_c - b_c|) // 3, integers only."""
import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2


def gauss(dtype=torch.float64):
    x = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-x * x / (2 * 1.5 ** 2))
    return (g / g.sum()).to(dtype)


def _chw(img, dtype):
    t = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1)
    return t.to(torch.float64).div(255).to(dtype)  # x / 255, rounded once to the working type


def moments(a, b, dtype=torch.float64, separable=False):
    """(mu_a, mu_b, s_aa, s_bb, s_ab) per channel, each (3, H, W)"""
    a, b = _chw(a, dtype), _chw(b, dtype)
    g = gauss(dtype)
    w2 = (gauss()[:, None] * gauss()[None, :]).to(dtype).view(1, 1, 11, 11)

    def blur(x):
        x = x[:, None]
        if separable:
            x = F.conv2d(F.conv2d(x, g.view(1, 1, 1, 11), padding=(0, 5)), g.view(1, 1, 11, 1), padding=(5, 0))
        else:
            x = F.conv2d(x, w2, padding=5)
        return x[:, 0]

    mu_a, mu_b = blur(a), blur(b)
    return mu_a, mu_b, blur(a * a) - mu_a * mu_a, blur(b * b) - mu_b * mu_b, blur(a * b) - mu_a * mu_b


def ssim_map(a, b, dtype=torch.float64, separable=False):
    mu_a, mu_b, s_aa, s_bb, s_ab = moments(a, b, dtype, separable)
    m = ((2 * mu_a * mu_b + C1) * (2 * s_ab + C2)) / ((mu_a * mu_a + mu_b * mu_b + C1) * (s_aa + s_bb + C2))
    return m.mean(0)


def codes(m):
    """metric_map_write for [-1, 1]: trunc((m + 1) * 32767) -> int64 tensor of uint16 values"""
    return ((m.to(torch.float64) + 1) * 32767).to(torch.int64)


def mae_codes(a, b):
    s = np.abs(a.astype(np.int64) - b.astype(np.int64)).sum(axis=2)
    return torch.from_numpy((257 * s) // 3)


# ---- the six case classes of the accuracy tests (seeded; uint8 (H, W, 3) pairs) ----------------------------------------------------------
def _smooth(h, w, seed):
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.zeros((3, h, w))
    for c in range(3):
        for _ in range(6):
            fx, fy, ph = r.uniform(0.005, 0.08), r.uniform(0.005, 0.08), r.uniform(0, 6.28)
            img[c] += r.uniform(0.05, 0.3) * np.sin(fx * xx * 6.28 + fy * yy * 6.28 + ph)
    return np.clip(img * 0.5 + 0.5, 0, 1)


def _u8(x):
    return np.ascontiguousarray(np.floor(x * 255 + 0.5).astype(np.uint8).transpose(1, 2, 0))


CASES = ("smooth+noise", "shift blend", "noise vs noise", "flat bright", "identical", "black vs sparse 1")


def case_pair(name, h, w, seed=3):
    """(render, captured image) of one case class at h x w"""
    rng = np.random.default_rng(seed)
    gt = _smooth(h, w, 1)
    if name == "smooth+noise":
        return _u8(np.clip(gt + rng.normal(0, 0.05, gt.shape), 0, 1)), _u8(gt)
    if name == "shift blend":
        r = gt.copy()
        r[:, :, w // 2:] = 0.5 * (r[:, :, w // 2:] + np.roll(gt, 3, 2)[:, :, w // 2:])
        return _u8(r), _u8(gt)
    if name == "noise vs noise":
        return _u8(rng.uniform(0, 1, gt.shape)), _u8(rng.uniform(0, 1, gt.shape))
    if name == "flat bright":
        flat = np.full_like(gt, 250 / 255)
        f2 = flat.copy()
        f2[:, h * 3 // 8: h * 5 // 8 + 1, w * 2 // 7: w * 3 // 7 + 1] = 249 / 255
        return _u8(f2), _u8(flat)
    if name == "identical":
        return _u8(gt), _u8(gt)
    if name == "black vs sparse 1":
        blk = np.zeros_like(gt)
        return _u8(blk + (rng.uniform(0, 1, gt.shape) < 0.1) / 255), _u8(blk)
    raise KeyError(name)
