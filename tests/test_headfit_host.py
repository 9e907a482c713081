"""Host-side checks of the head fit: the fp64 oracle against the goldens made from the reference's own head, its AdamW against
torch's three recorded steps, option handling, the checkpoint round trip, and that the kernel file is listed, declared and bound."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import headfit_oracle as ho  # noqa: E402
from crossscore_amd import _lib, build  # noqa: E402
from crossscore_amd.config import model_config  # noqa: E402
from crossscore_amd.model import CrossScoreNet, HeadFitState, load_lightning_checkpoint, save_lightning_checkpoint  # noqa: E402

CONFIGS = {"c0": (0, 1.0), "c1": (0, 2.0), "c2": (1, 1.0)}  # (act, p) of the golden's three configurations
KEYS = ("Wa", "ba", "Wb", "bb")


def load_golden(tag):
    g = np.load(os.path.join(HERE, "golden", f"{tag}_head_fit.npz"))
    B, gh, gw, Cc, P = (int(v) for v in g["shape"])
    return g, B, gh, gw, Cc, P


def golden_case(g, cname, gh, gw, P):
    X = torch.from_numpy(g["X"]).double()
    prm = [torch.from_numpy(g[k]).double() for k in KEYS]
    gt_rows = ho.to_rows(torch.from_numpy(g[f"{cname}_gt"]).double(), gh, gw, P)
    return X, prm, gt_rows


@pytest.mark.parametrize("tag", ["h0", "h1"])
@pytest.mark.parametrize("cname", sorted(CONFIGS))
def test_oracle_equals_golden(tag, cname):
    g, B, gh, gw, Cc, P = load_golden(tag)
    act, p = CONFIGS[cname]
    X, (Wa, ba, Wb, bb), gt_rows = golden_case(g, cname, gh, gw, P)
    A = ho.leaky(X @ Wa.T + ba)
    r = ho.backward(X, A, Wb, bb, gt_rows, act, p, 1.0 / gt_rows.numel())
    assert abs(float(r["loss"]) - float(g[f"{cname}_loss"])) <= 1e-12 * float(g[f"{cname}_loss"])
    for k in KEYS:
        want = torch.from_numpy(g[f"{cname}_d{k}"])
        assert float((r["d" + k] - want).abs().max()) <= 1e-12 * float(want.abs().max()), k


@pytest.mark.parametrize("cname", sorted(CONFIGS))
def test_oracle_adamw_equals_torch(cname):
    """three steps of AdamW(lr 5e-4) + StepLR(2, 0.5) as the golden script ran them in fp64; the bound is twice what torch's own fp32 run
    differs from its fp64 run by (recorded per parameter), plus the fp32 storage of the recorded change"""
    g, B, gh, gw, Cc, P = load_golden("h0")
    act, p = CONFIGS[cname]
    X, prm, gt_rows = golden_case(g, cname, gh, gw, P)
    _, got = ho.fit(X, prm, gt_rows, act, p, steps=3, lr=5e-4, step_size=2, gamma=0.5)
    for i, k in enumerate(KEYS):
        delta = torch.from_numpy(g[f"{cname}_step3_delta_{k}"]).double()
        err = (got[i] - prm[i] - delta).abs()
        assert float((err - (2.0 * float(g[f"{cname}_adam32_dev"][i]) + 2.0 ** -24 * delta.abs())).max()) <= 0, k


def test_step_lr():
    assert [ho.step_lr(1.0, 2, 0.5, n) for n in range(5)] == [1.0, 1.0, 0.5, 0.5, 0.25]


def _net(**over):
    return CrossScoreNet(model_config(**{"backbone.from_pretrained": "synthetic/dinov2-tiny", **over}))


def test_options():
    st = HeadFitState()
    assert (st.lr, st.betas, st.eps, st.weight_decay, st.step) == (5e-4, (0.9, 0.999), 1e-8, 1e-2, 0)
    net = _net()
    names = [n for n, _ in net.named_parameters()]
    assert [names[[id(q) for _, q in net.named_parameters()].index(id(p))] for p in net.head_parameters()] == list(CrossScoreNet.HEAD_KEYS)
    gt = torch.zeros((1, 42, 42))
    with pytest.raises(ValueError):
        net.fit_head_step(torch.zeros((1, 3, 42, 42)), None, gt, st)  # neither images nor tokens
    with pytest.raises(ValueError):
        net.fit_head_step(torch.zeros((1, 3, 42, 42)), torch.zeros((1, 1, 3, 42, 42)), gt, st, ref_tokens=torch.zeros((1, 1, 9, 128)))
    with pytest.raises(ValueError):
        net.fit_head_step(torch.zeros((1, 3, 42, 42)), torch.zeros((1, 1, 3, 42, 42)), gt, st)  # parameters not on a device
    with pytest.raises(ValueError):
        _net(do_reference_cross=False).head_parameters()


def test_checkpoint_round_trip(tmp_path):
    net = _net()
    with torch.no_grad():
        for i, p in enumerate(net.parameters()):
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(i)))
    path = str(tmp_path / "last.ckpt")
    save_lightning_checkpoint(path, net)
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert set(raw) == {"state_dict"} and all(k.startswith("model.") for k in raw["state_dict"])
    sd = load_lightning_checkpoint(path)
    want = net.state_dict()
    assert set(sd) == set(want)
    for k, v in want.items():
        assert torch.equal(sd[k], v), k
    other = _net()
    other.load_state_dict(sd, strict=True)


HEADFIT_SYMBOLS = ("cs_head_fit_supported", "cs_head_backward_workspace_bytes", "cs_op_head_grad_z", "cs_op_gemm_tn", "cs_op_head_backward",
                   "cs_head_backward", "cs_op_adamw", "cs_set_head_weights")


def test_headfit_listed_declared_and_bound():
    assert "headfit.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "headfit.hip"))
    header = open(os.path.join(REPO, "include", "crossscore_hip.h")).read()
    common = open(os.path.join(build.CSRC, "cs_common.h")).read()
    for name in HEADFIT_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SYMBOLS, name
    for launch in ("cs_head_grad_z_launch", "cs_gemm_tn_launch", "cs_head_backward_launch", "cs_adamw_launch"):
        assert launch in common, launch
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()  # binds every declared symbol: raises if the library lacks one
        assert lib.cs_head_fit_supported(384, 14) == 1
