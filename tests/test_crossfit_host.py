"""Host-side checks of the cross-attention fit: the fp64 oracle's sixteen gradients against torch.autograd of the block the
reference's modules execute (the check of the ln2 and 1 / sqrt(dh) derivation), its AdamW trajectory against torch.optim.AdamW, the three
properties of the attention backward, the planted defects against the op tests' bounds (so that the GPU bounds are known to discriminate), the
driver's fit_scope option, the sixteen keys, and that the kernel files are listed, declared and bound."""
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import crossfit_helpers as ch  # noqa: E402
import crossfit_oracle as co  # noqa: E402
import tailfit_helpers as th  # noqa: E402
from bits16 import MODES, r16  # noqa: E402
from crossscore_amd import _lib, build  # noqa: E402
from crossscore_amd.config import load_config, model_config  # noqa: E402
from crossscore_amd.model import CrossScoreNet, HeadFitState  # noqa: E402

F64 = torch.float64
CONFIGS = [(0, 1.0), (0, 2.5), (1, 1.0)]  # (act, p)


def _unrounded(c):
    """a cross_case with every stored row recomputed without roundings, and its sixteen tensors in crossfit_oracle.PARAMS order"""
    params = [c[k] for k in co.PARAMS]
    return params, co.forward_backward(c["x1"], c["mem"], params, c["gt_rows"], c["act"], c["p"], c["B"], c["h"], c["short_cut"])


@pytest.mark.parametrize("act,p", CONFIGS)
@pytest.mark.parametrize("B,N,gh,gw,Cc,h,short_cut", [(2, 2, 3, 5, 128, 8, True), (1, 3, 2, 3, 96, 2, False), (2, 1, 1, 1, 64, 4, True)])
def test_oracle_equals_autograd(B, N, gh, gw, Cc, h, short_cut, act, p):
    """operand roundings off: the written-out formulas, with ln2 in the K rows and 1 / sqrt(dh) in the Q rows of in_proj, against fp64 autograd
    through F.multi_head_attention_forward + residual + layer_norm + the tail; 1e-10 relative Frobenius error per tensor"""
    c = ch.cross_case(B, N, gh, gw, Cc, h, act, p, False, seed=31 + Cc + act, short_cut=short_cut)
    _, r = _unrounded(c)
    loss, grads = ch.autograd_block(c)
    assert abs(float(r["loss"]) - float(loss)) <= 1e-12 * float(loss)
    for name, want in zip(co.KEYS, grads):
        if name == "dbin":  # the K rows are zero in exact arithmetic: compared on the scale of the whole bias gradient
            assert float((r[name] - want).norm()) <= 1e-10 * float(want.norm()), name
            assert float(r[name][Cc:2 * Cc].abs().max()) <= 1e-14 * float(want.abs().max())
        else:
            assert th.rel_fro(r[name], want) <= 1e-10, name


@pytest.mark.parametrize("which", ["no_ln2", "no_rsqrt"])
def test_scaling_factors_matter(which):
    """without the ln2 (K rows) or the 1 / sqrt(dh) (Q rows) the in_proj gradient is off by that factor against autograd"""
    c = ch.cross_case(2, 2, 3, 5, 128, 8, 0, 1.0, False, seed=4)
    params = [c[k] for k in co.PARAMS]
    blk = co.block_forward(c["x1"], c["mem"], *params[:6], c["B"], c["h"])
    import tailfit_oracle as to
    H, _, X, A = to.tail_forward(blk["x2"], *params[6:14])
    r = co.backward(c["x1"], blk["Qp"], blk["K"], blk["V"], blk["O"], blk["lse"], c["mem"], c["W1"], c["Wo"], c["bo"], c["g2"], blk["x2"], H, X, A, c["W2"],
                    c["b2"], c["g3"], c["Wa"], c["Wb"], c["bb"], c["gt_rows"], 0, 1.0, c["inv"], c["B"], c["h"], mutate=which)
    _, grads = ch.autograd_block(c)
    rows = slice(128, 256) if which == "no_ln2" else slice(0, 128)
    factor = 1.0 / co.LN2 if which == "no_ln2" else 4.0
    assert th.rel_fro(r["dWin"][rows], factor * grads[0][rows]) <= 1e-10


def test_oracle_adamw_equals_torch():
    """three steps of AdamW(lr 5e-4) + StepLR(2, 0.5) over the sixteen tensors: crossfit_oracle.fit against torch.optim.AdamW on autograd of the
    same block in fp64.  The bound is test_tailfit_host's: twice what torch's own fp32 run differs from its fp64 run by, plus the fp32 storage
    of the change."""
    c = ch.cross_case(2, 2, 3, 5, 64, 4, 0, 1.0, False, seed=5)
    params = [c[k] for k in co.PARAMS]

    def torch_run(dtype):
        cur = dict(c)
        prm = [t.to(dtype).clone().requires_grad_(True) for t in params]
        opt = torch.optim.AdamW(prm, lr=5e-4)
        sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
        for _ in range(3):
            cur.update({k: t.detach() for k, t in zip(co.PARAMS, prm)})
            _, grads = ch.autograd_block(cur)
            for t, g in zip(prm, grads):
                t.grad = g
            opt.step()
            sched.step()
        return [t.detach().double() - t0 for t, t0 in zip(prm, params)]

    d64, d32 = torch_run(F64), torch_run(torch.float32)
    _, got = co.fit(c["x1"], c["mem"], params, c["gt_rows"], 0, 1.0, c["B"], c["h"], steps=3, lr=5e-4, step_size=2, gamma=0.5)
    for k, name in enumerate(co.KEYS):
        dev = float((d32[k] - d64[k]).abs().max())
        err = (got[k] - params[k] - d64[k]).abs()
        assert float((err - (2.0 * dev + 2.0 ** -24 * d64[k].abs())).max()) <= 0, name


def test_attention_backward_properties():
    Qp, K, V, dO = ch.attn_case(37, 45, 16, False, 2)
    O, lse, _ = co.attention_forward(Qp, K, V)
    r = co.attention_backward(Qp, K, V, O, dO, lse)
    # sum_k dz[q, k] = 0: adding one vector to every key does not move a softmax, so the K bias gradient is zero in exact arithmetic
    scale = (r["P"] * (r["dP"].abs() + r["D"].abs()[..., None])).sum(-1)
    assert float((r["dz"].sum(-1).abs() / scale).max()) <= 64 * 2.0 ** -52
    assert float(r["dKu"].sum(-2).abs().max()) <= 1e-13 * float(r["dKu"].abs().max()) * 37
    # dQu of one query row does not depend on any other query row
    Q2, dO2 = Qp.clone(), dO.clone()
    Q2[..., 5:, :] += 1.0
    dO2[..., 5:, :] *= -2.0
    O2, lse2, _ = co.attention_forward(Q2, K, V)
    r2 = co.attention_backward(Q2, K, V, O2, dO2, lse2)
    assert torch.equal(r2["dQu"][..., :5, :], r["dQu"][..., :5, :])
    # dKu / dV of a key do not depend on how the keys are tiled: the keys in two blocks, each against the whole problem's lse and D
    for cut in (1, 32, 44):
        a = co.attention_backward(Qp, K[..., :cut, :], V[..., :cut, :], O, dO, lse)
        b = co.attention_backward(Qp, K[..., cut:, :], V[..., cut:, :], O, dO, lse)
        for name in ("dKu", "dV"):
            assert torch.equal(torch.cat([a[name], b[name]], -2), r[name]), (name, cut)
        assert float((a["dQu"] + b["dQu"] - r["dQu"]).abs().max()) <= 1e-13 * float(r["dQu"].abs().max())


# which of dQu, dKu, dV each planted defect reaches
REACH = {"no_D": ("dQu", "dKu"), "dP_for_dz": ("dQu", "dKu"), "natural_exp": co.ATTN, "wrong_head_lse": co.ATTN, "skip_ragged_keys": co.ATTN,
         "skip_ragged_queries": co.ATTN, "swap_kq": ("dKu",), "padded_keys": ("dQu",)}


def _plant_all(Qp, K, V, dO, bf16, reach_of, factor):
    """every defect of co.MUTATIONS into the oracle on one case: each tensor reach_of(defect) names moves by more than factor x the op test's
    bound, or stops being finite (a NaN or an inf fails the op test's finiteness assertion)"""
    rnd = lambda t: r16(t, bf16)  # noqa: E731
    O, lse, _ = co.attention_forward(Qp, K, V, rnd)
    lse = lse.float().double()
    ref = co.attention_backward(Qp, K, V, O, dO, lse, rnd)
    bounds = ch.attn_fro_bounds(ref, Qp, K, V, O, dO, lse, bf16)
    for defect in co.MUTATIONS:
        bad = co.attention_backward(Qp, K, V, O, dO, lse, rnd, mutate=defect)
        for name in reach_of(defect):
            moved = float((bad[name] - ref[name]).norm())
            assert not moved <= factor * bounds[name], (defect, name, moved / bounds[name])
    return lse


@MODES
@pytest.mark.parametrize("dh", ch.DHS)
@pytest.mark.parametrize("pair", range(5))
def test_attention_defects_exceed_the_op_bounds(pair, dh, bf16):
    """Every case of test_crossfit_ops.test_attention_backward, on the CPU: each defect planted into the oracle moves every tensor it reaches by
    more than 3 x that test's bound.  A defect reaches a tensor of a case unless the case leaves it nothing to change: natural exp, the wrong
    head's lse and D only act where there are two keys to weigh (Lk = 1 makes P = 1 and dz = 0 whatever the exponent's base; the wrong lse still
    moves P there, and with it dV), a ragged tile only exists where the length is no multiple of the tile, K and Q can only be swapped where
    Lq = Lk (the (65, 65) case), and a padded key counted as 2^(0 - lse) meets zero K and V rows, so it changes nothing while 2^(-lse) stays
    inside the operand type's range -- which it does in every case of the grid (test_special_cases below has the one where it does not)."""
    tq, tk = 64, 64
    Lq, Lk = ch.shape_pairs(tq, tk)[pair]

    def reach_of(defect):
        reach = REACH[defect]
        if Lk == 1:
            reach = {"natural_exp": (), "wrong_head_lse": ("dV",), "skip_ragged_keys": ("dV",), "skip_ragged_queries": ("dV",)}.get(defect, reach)
        if (defect == "skip_ragged_keys" and Lk % tk == 0) or (defect == "skip_ragged_queries" and Lq % tq == 0) or (defect == "swap_kq" and Lq != Lk):
            reach = ()
        return () if defect == "padded_keys" else reach

    _plant_all(*ch.attn_case(Lq, Lk, dh, bf16, seed=1000 * pair + dh), bf16, reach_of, 3.0)


# what the special cases of the op test leave a defect nothing (or less than a bound's worth) to change
SPECIAL_UNREACHED = {
    # key 0 holds P > 0.9: e^x and 2^x agree near x = 0, so dV = Ph^T dO barely moves; the three keys of the ragged tile (64 .. 66) hold P < 1e-3
    # between them, so skipping them moves dKu and dV by less than the bound (dQu still by 3 x)
    "peaky": {"natural_exp": ("dV",), "skip_ragged_keys": ("dKu", "dV")},
    "underflow": {}, "negative": {}, "raw_q": {}}


@MODES
@pytest.mark.parametrize("dh", ch.DHS)
@pytest.mark.parametrize("kind", sorted(ch.SPECIAL_CASES))
def test_special_cases_defects_exceed_the_op_bounds(kind, dh, bf16):
    """The peaky, underflow and negative-logit cases of the op test: every defect exceeds the bound (or leaves the finite numbers) in every tensor
    it reaches, SPECIAL_UNREACHED saying where a case leaves it less than a bound's worth.  No special case has Lq = Lk (swap_kq), and a padded
    key counted as 2^(0 - lse) reaches dQu exactly where 2^(-lse) leaves the operand type's range: the negative case, where every row of dQu
    turns NaN -- the case that pins the kernel's forced zeros in the ragged tile."""
    Lq, Lk, so = ch.SPECIAL_CASES[kind]

    def reach_of(defect):
        if defect == "swap_kq" or (defect == "padded_keys" and kind != "negative"):
            return ()
        return tuple(n for n in REACH[defect] if n not in SPECIAL_UNREACHED[kind].get(defect, ()))

    lse = _plant_all(*ch.attn_case(Lq, Lk, dh, bf16, so + dh, kind), bf16, reach_of, 1.0)
    if kind == "negative":
        assert float(lse.max()) < -128.0 and Lq % 64 and Lk % 64


@MODES
def test_raw_q_case_defects_exceed_the_op_bounds(bf16):
    """the q_scale = 0 case of the op test (Q' = the rounded product both kernels form): as the grid's ragged cases"""
    _plant_all(*ch.raw_q_case(bf16)[1:], bf16, lambda d: () if d in ("swap_kq", "padded_keys") else REACH[d], 3.0)


@MODES
@pytest.mark.parametrize("Cc,h", [(128, 8), (384, 8)])
@pytest.mark.parametrize("B,N,gh,gw,short_cut", ch.CROSS_OP_CASES)
def test_block_defects_exceed_the_op_bounds(B, N, gh, gw, short_cut, Cc, h, bf16):
    """Every case of test_crossfit_ops.test_cross_backward, on the CPU: the attention's defects, a missing ln2 or 1 / sqrt(dh), y2 without the
    residual and dx2 without the feed-forward term each exceed the bounds of the parts they reach"""
    c = ch.cross_case(B, N, gh, gw, Cc, h, 0, 1.0, bf16, seed=B * 100 + Cc + gh, short_cut=short_cut)
    ref = ch.cross_oracle(c, bf16)
    bounds = ch.cross_fro_bounds(ref, c, bf16)
    parts = lambda r: {**ch.split_in_proj(r, Cc), **{k: r[k] for k in ("dWo", "dbo", "dgamma2", "dbeta2")}}  # noqa: E731
    want = parts(ref)
    qk = ("dWq", "dbq", "dWk")
    everything = tuple(k for k in ch.CROSS_PARTS if k != "dbk")  # (dbk is rounding residue in every run)
    reach = {"no_D": qk, "dP_for_dz": qk, "natural_exp": qk + ("dWv", "dbv"), "wrong_head_lse": qk + ("dWv", "dbv"), "no_ln2": ("dWk",),
             "no_rsqrt": ("dWq", "dbq"), "y2_no_residual": tuple(k for k in everything if k != "dbeta2"),  # (dbeta2 = sum_m dx2 does not read y2)
             "dx2_no_ffn": everything}
    if not short_cut:
        reach["y2_no_residual"] = ()  # (there is no residual to leave out)
    for defect, names in reach.items():
        got = parts(ch.cross_oracle(c, bf16, mutate=defect))
        for name in names:
            moved = float((got[name] - want[name]).norm())
            assert moved > 3.0 * bounds[name], (defect, name, moved / bounds[name])


def test_fit_scope_option():
    from crossscore_amd.fit_head import FIT_SCOPES, check_config, fit_scope

    assert FIT_SCOPES == ("head", "tail", "cross", "layer")
    cfg = load_config("default_fit_head", ["this_main.fit_scope=cross"])
    check_config(cfg)
    assert fit_scope(cfg) == "cross"
    assert fit_scope(load_config("default_fit_head", [])) == "head"
    for bad in ("decoder", "Tail", "Cross", ""):
        with pytest.raises(ValueError, match="fit_scope"):
            check_config(load_config("default_fit_head", [f"this_main.fit_scope={bad}"]))


def test_cross_keys_and_options():
    net = CrossScoreNet(model_config(**{"backbone.from_pretrained": "synthetic/dinov2-tiny"}))
    keys = net.CROSS_KEYS
    last = f"ref_cross.attn.layers.{net.arch.dec_layers - 1}."
    assert len(keys) == 16 and len(set(keys)) == 16 and keys[6:] == net.TAIL_KEYS
    assert keys[:6] == tuple(last + k for k in ("multihead_attn.in_proj_weight", "multihead_attn.in_proj_bias", "multihead_attn.out_proj.weight",
                                                "multihead_attn.out_proj.bias", "norm2.weight", "norm2.bias"))
    sd = net.state_dict()
    Cc = net.arch.hidden
    assert [tuple(p.shape) for p in net.cross_parameters()] == [tuple(sd[k].shape) for k in keys]
    assert tuple(sd[keys[0]].shape) == (3 * Cc, Cc) and tuple(sd[keys[1]].shape) == (3 * Cc,)
    st, gt = HeadFitState(), torch.zeros((1, 42, 42))
    with pytest.raises(ValueError):
        net.fit_cross_step(torch.zeros((1, 3, 42, 42)), None, gt, st)  # neither images nor tokens
    with pytest.raises(ValueError):
        CrossScoreNet(model_config(**{"backbone.from_pretrained": "synthetic/dinov2-tiny", "do_reference_cross": False})).cross_parameters()


CROSSFIT_SYMBOLS = ("cs_attention_backward_workspace_bytes", "cs_attention_backward_tiles", "cs_op_attention_backward", "cs_cross_fit_supported",
                    "cs_cross_backward_workspace_bytes", "cs_op_cross_backward", "cs_fit_cross_keep", "cs_cross_backward", "cs_debug_cross_inputs",
                    "cs_set_cross_weights")


def test_crossfit_listed_declared_and_bound():
    for src in ("attnbwd.hip", "crossfit.hip"):
        assert src in build.SOURCES and os.path.exists(os.path.join(build.CSRC, src))
    header = open(os.path.join(REPO, "include", "crossscore_hip.h")).read()
    common = open(os.path.join(build.CSRC, "cs_common.h")).read()
    for name in CROSSFIT_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SYMBOLS, name
    for launch in ("cs_attnbwd_launch", "cs_attnbwd_check", "cs_cross_backward_launch"):
        assert launch in common, launch
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.cs_cross_fit_supported(128, 8, 14) == 1 and lib.cs_cross_fit_supported(384, 8, 14) == 1 and lib.cs_cross_fit_supported(768, 8, 14) == 1
        # dinov2-large / giant decoder widths: head dims 128 and 192 are not built; nor is what the tail refuses
        assert lib.cs_cross_fit_supported(1024, 8, 14) == 0 and lib.cs_cross_fit_supported(1536, 8, 14) == 0
        assert lib.cs_cross_fit_supported(384, 8, 16) == 0 and lib.cs_cross_fit_supported(384, 0, 14) == 0 and lib.cs_cross_fit_supported(384, 7, 14) == 0
