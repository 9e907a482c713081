"""Host-side checks of the whole-layer fit: the fp64 oracle's six new gradients against torch.autograd of the layer the
reference's modules execute (the check of the ln2 in dx1 and of the in_proj scalars), the rounded oracle's own margin inside the op test's bounds,
the planted defects against those bounds (so that the GPU bounds are known to discriminate), the scope table and the driver's option, and that
the kernel file is listed, declared and bound."""
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import layerfit_helpers as lh  # noqa: E402
import layerfit_oracle as lo  # noqa: E402
import tailfit_helpers as th  # noqa: E402
from bits16 import MODES  # noqa: E402
from crossscore_amd import _lib, build, model  # noqa: E402
from crossscore_amd.config import load_config, model_config  # noqa: E402
from crossscore_amd.model import CrossScoreNet, HeadFitState, arch_from_cfg, check_fit_supported  # noqa: E402

F64 = torch.float64
DERIVATION_CASES = [(2, 2, 3, 5, 128, 8, True), (1, 3, 2, 3, 96, 2, False), (2, 1, 1, 2, 64, 4, True)]


def _unrounded(c, mutate=None):
    """a layer_case with every stored row recomputed without roundings, from its twenty-two tensors"""
    return lo.forward_backward(c["x0"], c["mem"], lh.params_of(c), c["gt_rows"], c["act"], c["p"], c["B"], c["h"], c["short_cut"], mutate=mutate)


@pytest.mark.parametrize("act,p", [(0, 1.0), (1, 1.0)])
@pytest.mark.parametrize("B,N,gh,gw,Cc,h,short_cut", DERIVATION_CASES)
def test_oracle_equals_autograd(B, N, gh, gw, Cc, h, short_cut, act, p):
    """operand roundings off: the written-out formulas against fp64 autograd through F.multi_head_attention_forward + residual + layer_norm in
    front of the cross-attention block and the tail, with and without the short cut; 1e-10 relative Frobenius error per tensor, all twenty-two"""
    c = lh.layer_case(B, N, gh, gw, Cc, h, act, p, False, seed=17 + Cc + act, short_cut=short_cut)
    r = _unrounded(c)
    loss, grads = lh.autograd_layer(c)
    assert abs(float(r["loss"]) - float(loss)) <= 1e-12 * float(loss)
    for name, want in zip(lo.KEYS, grads):
        if name in ("dbin", "dbin_s"):  # the K rows are zero in exact arithmetic: compared on the scale of the whole bias gradient
            assert float((r[name] - want).norm()) <= 1e-10 * float(want.norm()), name
        else:
            assert th.rel_fro(r[name], want) <= 1e-10, name


@pytest.mark.parametrize("short_cut", [True, False])
@pytest.mark.parametrize("which,part,factor", [("dx1_no_ln2", None, None), ("no_rsqrt_s", "dWq_s", 4.0), ("no_ln2_s", "dWk_s", 1.0 / lo.LN2)])
def test_scaling_factors_matter(which, part, factor, short_cut):
    """each scalar taken out in turn: without the ln2 of dx1 every one of the six new gradients leaves autograd's; without the 1 / sqrt(dh) of
    the Q rows or the ln2 of the K rows that block of in_proj is off by exactly that factor (dh = 16)"""
    c = lh.layer_case(2, 2, 3, 5, 128, 8, 0, 1.0, False, seed=5, short_cut=short_cut)
    r = _unrounded(c, mutate=which)
    _, grads = lh.autograd_layer(c)
    have, want = lh.split_layer(r, 128), lh.split_layer(grads[:6], 128)
    if part is None:
        for name in lh.LAYER_PARTS:
            if name != "dbk_s":
                assert th.rel_fro(have[name], want[name]) > 1e-3, name
    else:
        assert th.rel_fro(have[part], factor * want[part]) <= 1e-10
        for name in lh.LAYER_PARTS:
            if name not in (part, "dbk_s", "dbq_s" if part == "dWq_s" else part):
                assert th.rel_fro(have[name], want[name]) <= 1e-10, name


def _cases():
    return [(B, N, gh, gw, sc, Cc, h) for (B, N, gh, gw, sc) in lh.LAYER_OP_CASES for (Cc, h) in lh.WIDTHS]


_CACHE = {}


def _case(B, N, gh, gw, sc, Cc, h, bf16):
    """the op test's case with the oracle's own attention in place of cs_op_attention, its rounded reference and bounds; computed once"""
    key = (B, N, gh, gw, sc, Cc, h, bf16)
    if key not in _CACHE:
        c = lh.layer_case(B, N, gh, gw, Cc, h, 0, 1.0, bf16, seed=lh.case_seed(B, gh, gw, Cc), short_cut=sc)
        ref = lh.layer_oracle(c, bf16)
        _CACHE[key] = (c, ref, lh.layer_fro_bounds(ref, c, bf16))
    return _CACHE[key]


@MODES
@pytest.mark.parametrize("B,N,gh,gw,short_cut,Cc,h", _cases())
def test_rounded_oracle_stays_inside_the_bounds(B, N, gh, gw, short_cut, Cc, h, bf16):
    """the reference's own margin: on every case of the GPU op test the oracle with the 16-bit roundings on is inside the bounds against the
    fp64 definition on the same stored operands, and every bound is a small part of its gradient"""
    c, ref, bounds = _case(B, N, gh, gw, short_cut, Cc, h, bf16)
    exact = lh.split_layer(lh.layer_oracle(c, bf16, rounded=False), Cc)
    have = lh.split_layer(ref, Cc)
    for name in lh.LAYER_PARTS:
        err, nrm = float((have[name] - exact[name]).norm()), float(exact[name].norm())
        print(f"{name}: rounded vs fp64 err/bound {err / bounds[name]:.3f}, bound/|ref| {bounds[name] / max(nrm, 1e-300):.2e}")
        assert err <= bounds[name], (name, err / bounds[name])


@MODES
@pytest.mark.parametrize("B,N,gh,gw,short_cut,Cc,h", _cases())
def test_defects_exceed_the_op_bounds(B, N, gh, gw, short_cut, Cc, h, bf16):
    """Every case of test_layerfit_ops.test_layer_backward, on the CPU: each planted defect moves every part it reaches (layerfit_helpers.REACH)
    by more than 3 x that test's bound.  Without the short cut the two residual defects have nothing to change: they are checked to be exact
    no-ops there instead."""
    c, ref, bounds = _case(B, N, gh, gw, short_cut, Cc, h, bf16)
    want = lh.split_layer(ref, Cc)
    for defect in lo.MUTATIONS:
        got = lh.split_layer(lh.layer_oracle(c, bf16, mutate=defect), Cc)
        if not short_cut and defect in lh.NEEDS_SHORT_CUT:
            for name in lh.LAYER_PARTS:
                assert torch.equal(got[name], want[name]), (defect, name, "a no-op without the short cut")
            continue
        for name in lh.REACH[defect]:
            moved = float((got[name] - want[name]).norm())
            assert moved > 3.0 * bounds[name], (defect, name, moved / bounds[name])


def test_scope_table_and_options():
    from crossscore_amd import fit_head

    assert list(model.FIT_SCOPES) == ["head", "tail", "cross", "layer"] and fit_head.FIT_SCOPES == ("head", "tail", "cross", "layer")  # one table
    assert model.FIT_SCOPES["layer"] is model.FIT_LAYER and not hasattr(model, "ALL_FIT_SCOPES")
    assert [s.name for s in model.FIT_LAYER.chain()] == ["layer", "cross", "tail", "head"]
    net = CrossScoreNet(model_config(**{"backbone.from_pretrained": "synthetic/dinov2-tiny"}))
    keys = net.LAYER_KEYS
    last = f"ref_cross.attn.layers.{net.arch.dec_layers - 1}."
    assert len(keys) == 22 and len(set(keys)) == 22 and keys[6:] == net.CROSS_KEYS
    assert keys[:6] == tuple(last + k for k in ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight",
                                                "self_attn.out_proj.bias", "norm1.weight", "norm1.bias"))
    sd = net.state_dict()
    assert all(k in sd for k in keys)
    assert [tuple(p.shape) for p in net.layer_parameters()] == [tuple(sd[k].shape) for k in keys]
    with pytest.raises(ValueError):
        net.fit_layer_step(torch.zeros((1, 3, 42, 42)), None, torch.zeros((1, 42, 42)), HeadFitState())  # neither images nor tokens
    cfg = load_config("default_fit_head", ["this_main.fit_scope=layer"])
    fit_head.check_config(cfg)
    assert fit_head.fit_scope(cfg) == "layer"
    for bad in ("decoder", "Tail", "Cross", "Layer", ""):
        with pytest.raises(ValueError, match="fit_scope"):
            fit_head.check_config(load_config("default_fit_head", [f"this_main.fit_scope={bad}"]))


def test_layer_scope_needs_self_attention():
    """nothing to fit without the self-attention: a ValueError, raised before any weight is loaded"""
    cfg = load_config("default_fit_head", ["this_main.fit_scope=layer", "model.decoder_do_self_attn=False"])
    with pytest.raises(ValueError, match="decoder_do_self_attn"):
        check_fit_supported(arch_from_cfg(cfg), "layer")


LAYERFIT_SYMBOLS = ("cs_layer_fit_supported", "cs_layer_backward_workspace_bytes", "cs_op_layer_backward", "cs_fit_layer_keep", "cs_layer_backward",
                    "cs_debug_layer_inputs", "cs_set_layer_weights")


def test_layerfit_listed_declared_and_bound():
    assert "layerfit.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "layerfit.hip"))
    header = open(os.path.join(REPO, "include", "crossscore_hip.h")).read()
    common = open(os.path.join(build.CSRC, "cs_common.h")).read()
    for name in LAYERFIT_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SYMBOLS, name
    for launch in ("cs_layer_backward_launch", "cs_layer_backward_workspace", "cs_layer_backward_attn_params"):
        assert launch in common, launch
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for hidden in (128, 384, 768):
            assert lib.cs_layer_fit_supported(hidden, 8, 14, 1) == 1, hidden
            assert lib.cs_layer_fit_supported(hidden, 8, 14, 0) == 0, hidden
        assert lib.cs_layer_fit_supported(1024, 8, 14, 1) == 0 and lib.cs_layer_fit_supported(1536, 8, 14, 1) == 0
        assert lib.cs_layer_fit_supported(384, 8, 16, 1) == 0
        with pytest.raises(NotImplementedError):  # where the cross scope would refuse: head dim 128
            check_fit_supported(arch_from_cfg(load_config("default_fit_head", ["model.backbone.from_pretrained=facebook/dinov2-large"])), "layer")
