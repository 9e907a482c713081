"""Synthetic networks and driver weights of the forward and driver tests, the oracle call and the bounds of the end-to-end parity tests."""
import numpy as np
import torch

from crossscore_amd import synth
from crossscore_amd.config import model_config
from crossscore_amd.model import CrossScoreNet
from oracle import crossscore_oracle as orc

TINY = "synthetic/dinov2-tiny"       # C = 128, 8 decoder heads of 16 (golden g0's net)
SMALL = "synthetic/dinov2-small-2l"  # the ViT-S width, 8 decoder heads of 48 (golden g8's net): what the one-pass (uint8) input stage takes

MAE_TOL = 1e-3     # the north-star bound
MAE_TARGET = 2e-4  # SURVEY.md 8c target, asserted on the reference's own goldens and the real backbones
MAX_TOL = 5e-3     # single-pixel worst case of an fp16-operand forward on peaky synthetic weights (measured 6e-4 - 8e-4)


def make_net(backbone, seed, dtype=None, device="cuda", **over):
    """-> (net on `device` with synth.make_state_dict(arch, seed) loaded, arch, that state dict); dtype: the net's operand_dtype, if given;
    over: model_config overrides"""
    net = CrossScoreNet(model_config(**{"backbone.from_pretrained": backbone, **over}))
    sd = synth.make_state_dict(net.arch, seed)
    net.load_numpy_state_dict(sd)
    if dtype is not None:
        net.operand_dtype = dtype
    return net.to(device), net.arch, sd


def arch_of(backbone):
    return CrossScoreNet(model_config(**{"backbone.from_pretrained": backbone})).arch


def state_dict_for(backbone, seed, arch=None):
    """the torch state dict a driver takes (predict / evaluate state_dict=...): synth.make_state_dict of the backbone's architecture"""
    return {k: torch.from_numpy(v) for k, v in synth.make_state_dict(arch or arch_of(backbone), seed).items()}


def oracle(arch, sd, q, r, need_w=False, head=0, **cfgover):
    W = orc.to_torch(sd)
    return orc.forward(W, dict(enc_heads=arch.enc_heads, **cfgover), torch.from_numpy(q), torch.from_numpy(r), need_w, head)


def check_compact(g, score):
    """a full-size score map against a compact golden (rows, per-patch means, image means) -> (MAE of the rows, of the patch grid, max |d mean|)"""
    P = 14
    s = score.cpu().numpy()
    B, Hs, Ws = s.shape
    assert tuple(g["shape"]) == (B, Hs, Ws)
    grid = s.reshape(B, Hs // P, P, Ws // P, P).mean(axis=(2, 4), dtype=np.float64)
    rows = s[:, g["rows_idx"], :]
    mae_rows = float(np.abs(rows - g["rows"]).mean())
    mae_grid = float(np.abs(grid - g["patch_mean"]).mean())
    dmean = float(np.abs(s.mean(axis=(1, 2), dtype=np.float64) - g["mean"]).max())
    return mae_rows, mae_grid, dmean
