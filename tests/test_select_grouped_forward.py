"""cs_forward_select_grouped / CrossScoreNet.forward_select(group=...): each query chooses among the rows of its own group
of the bank, a group shorter than N is padded with the blank row's tokens.  Pinned from two sides, as the ungrouped forward is: the choice
equals cs_op_select_references_grouped on descriptors formed by the single ops, and everything behind the choice is bit-identical to
forward_cached on the chosen rows (-1 -> the blank row)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from crossscore_amd import _lib, synth  # noqa: E402
from crossscore_amd.model import SelectionBank  # noqa: E402
from crossscore_amd.pipeline import ForwardPipeline  # noqa: E402
from nets import SMALL, TINY, make_net  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("score_map_ref_cross", "score_mean_ref_cross", "attn_weights_map_ref_cross")
SIZES = (1, 4, 4)  # a group of one (padding with N = 2) and two that leave a choice; the blank row follows them
OFFSETS = np.array([0, 1, 5, 9], dtype=np.int32)
R, BLANK, N, B = 10, 9, 2, 3
GROUPS = np.array([1, 0, 2], dtype=np.int32)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _h(a):
    return a.ctypes.data_as(C.c_void_p)


def _images(n, H, W, seed):
    return torch.from_numpy(synth.make_inputs(n, 1, H, W, seed)[0]).cuda()


def _grouped_bank(net, imgs, blank_row=BLANK, offsets=OFFSETS, n=N):
    tokens = net.encode_references(imgs)
    mean, centre, unit = net.reference_descriptors(tokens, offsets)
    return SelectionBank(tokens, mean, centre, unit, n, offsets, blank_row)


def _bank_images(H, W, seed):
    imgs = _images(R, H, W, seed)
    imgs[BLANK] = -1.5  # a constant image stands in for the normalised all-zero placeholder
    return imgs


def _chosen_rows(bank, index):
    rows = index.long().clone()
    rows[rows < 0] = bank.blank_row
    return bank.tokens[rows]


def _ops_selection(net, q, bank, groups, exclude):
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    qt = net.encode_references(q)
    Bq, Np, Cc = qt.shape
    code = _lib.DTYPE_BF16 if qt.dtype == torch.bfloat16 else _lib.DTYPE_F16
    mean = torch.empty((Bq, Cc), dtype=torch.float32, device=q.device)
    index = torch.empty((Bq, N), dtype=torch.int32, device=q.device)
    sim = torch.empty((Bq, bank.longest_group), dtype=torch.float32, device=q.device)
    _lib.check(lib.cs_op_token_descriptors(_p(qt), Bq, Np, Cc, code, _p(mean), st))
    _lib.check(lib.cs_op_select_references_grouped(_p(mean), Bq, _h(groups), _p(bank.unit), _p(bank.centre), _h(bank.offsets), len(bank.offsets) - 1,
                                                   len(bank), Cc, _p(exclude), N, _p(index), _p(sim), st))
    return index, sim


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("H,W", [(70, 98), (42, 42)])
def test_grouped_forward_is_forward_cached_on_the_chosen_rows(H, W, dtype):
    net = make_net(TINY, 3, dtype)[0]
    bank = _grouped_bank(net, _bank_images(H, W, 21))
    q = _images(B, H, W, 22)
    for exclude in (None, torch.tensor([3, -1, 0], dtype=torch.int32).cuda()):  # a row of the query's group; none; a row of another group
        got = net.forward_select(q, bank, exclude, True, 1, True, group=GROUPS)
        index = got["reference_index"]
        assert index.dtype == torch.int32 and tuple(index.shape) == (B, N)
        rows = index.tolist()
        assert rows[1] == [0, -1]                                  # the group of one: its row, then padding
        assert all(1 <= r < 5 for r in rows[0]) and all(5 <= r < 9 for r in rows[2])
        if exclude is not None:
            assert 3 not in rows[0]
        want = net.forward_cached(q, _chosen_rows(bank, index), True, 1, True)
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(got[k], want[k]), k
        ops_index, ops_sim = _ops_selection(net, q, bank, GROUPS, exclude)
        assert torch.equal(index, ops_index)
        sim = got["reference_similarity"]
        assert bool(torch.isnan(sim[1, 1])) and bool(torch.isfinite(sim[0]).all()) and bool(torch.isfinite(sim[2]).all()) and bool(torch.isfinite(sim[1, 0]))
        lo = torch.from_numpy(OFFSETS[GROUPS].astype(np.int64)).cuda().unsqueeze(1)
        picked = torch.gather(ops_sim, 1, (index.long() - lo).clamp(min=0))
        assert torch.equal(sim[index >= 0], picked[index >= 0])
    # without a blank row the missing places are zeros, as today's gather gives for -1
    zeros = _grouped_bank(net, _bank_images(H, W, 21), blank_row=-1)
    got = net.forward_select(q, zeros, None, True, 1, True, group=GROUPS)
    fed = zeros.tokens[got["reference_index"].long().clamp(min=0)].clone()
    fed[got["reference_index"] < 0] = 0
    want = net.forward_cached(q, fed, True, 1, True)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    # the launches the grouped selection adds to the cached forward's, and nothing else
    index = net.forward_select(q, bank, None, True, 1, True, group=GROUPS)["reference_index"]
    sel = net.forward_stats()["kernels"]
    net.forward_cached(q, _chosen_rows(bank, index), True, 1, True)
    base = net.forward_stats()["kernels"]
    extra = {k: v for k, v in sel.items() if k.startswith("select_")}
    assert extra == {"select_desc": 1, "select_unit_grouped": 1, "select_sim_grouped": 1, "select_topn_grouped": 1, "select_gather_blank": 1}
    assert {k: v for k, v in sel.items() if k not in extra} == base


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_one_group_over_every_row_is_todays_forward_select(dtype):
    H, W = 70, 98
    net = make_net(TINY, 3, dtype)[0]
    imgs = _images(R, H, W, 51)
    tokens = net.encode_references(imgs)
    mean, centre, unit = net.reference_descriptors(tokens)
    plain = SelectionBank(tokens, mean, centre, unit, N)
    whole = np.array([0, R], dtype=np.int32)
    g_mean, g_centre, g_unit = net.reference_descriptors(tokens, whole)
    assert torch.equal(g_mean, mean) and torch.equal(g_centre[0], centre) and torch.equal(g_unit, unit)
    grouped = SelectionBank(tokens, g_mean, g_centre, g_unit, N, whole, -1)
    q = _images(B, H, W, 52)
    for exclude in (None, torch.tensor([-1, 4, 7], dtype=torch.int32).cuda()):
        want = net.forward_select(q, plain, exclude, True, 1, True)
        got = net.forward_select(q, grouped, exclude, True, 1, True, group=np.zeros(B, dtype=np.int32))
        torch.cuda.synchronize()
        for k in KEYS + ("reference_index", "reference_similarity"):
            assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_entry_points_and_batches_in_flight_give_the_same_bits(dtype):
    """fp32 and uint8 queries, one batch at a time and three in flight through ForwardPipeline: the same choice and the same maps"""
    from crossscore_amd.data import InputStage

    net = make_net(SMALL, 3, dtype)[0]
    dev = torch.device("cuda:0")
    stage = InputStage(dev, resize_short_side=70, integer_patches=True)
    rng = np.random.Generator(np.random.PCG64(17))
    raw = [rng.integers(0, 256, size=(90, 120, 3), dtype=np.uint8) for _ in range(R + 2 * B)]
    raw[BLANK] = np.zeros((90, 120, 3), dtype=np.uint8)
    size = stage.geometry(90, 120)[1][2:]

    def f32(imgs):
        out = torch.empty((len(imgs), 3) + size, device=dev)
        for i, im in enumerate(imgs):
            stage(im, out[i])
        return out

    bank = _grouped_bank(net, f32(raw[:R]))
    batches = [raw[R:R + B], raw[R + B:]]
    groups = [GROUPS, np.array([0, 2, 1], dtype=np.int32)]
    ex = torch.tensor([-1, 3, 6], dtype=torch.int32, device=dev)
    want = [net.forward_select(f32(b), bank, ex, True, 2, True, group=g) for b, g in zip(batches, groups)]
    assert net.u8_input_supported(stage.describe(raw[0]), size)
    for depth in (1, 3):
        pipe = ForwardPipeline(net, depth=depth)
        for u8 in (False, True):
            tickets = []
            for b, g in list(zip(batches, groups)) * 2:
                if u8:
                    tickets.append(pipe.submit_select(stage.batch([stage.describe(im) for im in b], size), bank, ex, True, 2, True, group=g))
                else:
                    tickets.append(pipe.submit_select(f32(b), bank, ex, True, 2, True, group=g))
            outs = [pipe.result(t) for t in tickets]
            torch.cuda.synchronize()
            for i, out in enumerate(outs):
                for k in KEYS + ("reference_index",):
                    assert torch.equal(out[k], want[i % 2][k]), (depth, u8, i, k)
                a, b_ = out["reference_similarity"], want[i % 2]["reference_similarity"]
                assert torch.equal(torch.isnan(a), torch.isnan(b_)) and torch.equal(a.nan_to_num(nan=0.0), b_.nan_to_num(nan=0.0)), (depth, u8, i)


def test_bad_arguments_raise_and_leave_the_handle_usable():
    H, W = 42, 42
    net = make_net(TINY, 3, "fp16")[0]
    imgs = _bank_images(H, W, 41)
    bank = _grouped_bank(net, imgs)
    q = _images(B, H, W, 42)
    good = net.forward_select(q, bank, None, False, 0, True, group=GROUPS)
    with pytest.raises(ValueError):  # a grouped bank needs the queries' groups
        net.forward_select(q, bank)
    with pytest.raises(ValueError):  # ... one per query
        net.forward_select(q, bank, group=GROUPS[:2])
    with pytest.raises(ValueError):  # ... inside [0, G)
        net.forward_select(q, bank, group=np.array([0, 1, 3]))
    with pytest.raises(NotImplementedError):
        net.forward_select(q, bank, group=GROUPS, n_references=33)
    plain_tokens = bank.tokens
    mean, centre, unit = net.reference_descriptors(plain_tokens)
    with pytest.raises(ValueError):  # group ids with a bank that has no groups
        net.forward_select(q, SelectionBank(plain_tokens, mean, centre, unit, N), group=GROUPS)
    for bad in ([1, 5, 9], [0, 5, 5, 9], [0, 5, 11]):  # not from 0, not increasing, past the bank
        with pytest.raises(ValueError):
            SelectionBank(bank.tokens, bank.mean, bank.centre, bank.unit, N, bad, -1)
    for blank in (4, R, -2):  # inside a group, outside the bank
        with pytest.raises(ValueError):
            SelectionBank(bank.tokens, bank.mean, bank.centre, bank.unit, N, OFFSETS, blank)
    # the C entry point refuses the same, queues nothing and leaves the handle usable
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    G = len(OFFSETS) - 1

    def call(offsets, groups, blank):
        index = torch.full((B, N), -7, dtype=torch.int32, device="cuda")
        score = torch.full((B, H, W), 3.25, dtype=torch.float32, device="cuda")
        rc = lib.cs_forward_select_grouped(net._handle, _p(q), _p(bank.tokens), _p(bank.unit), _p(bank.centre), R, _h(offsets), G, _h(groups), blank,
                                           None, B, N, H, W, _p(score), None, 0, None, _p(index), None, st)
        torch.cuda.synchronize()
        return rc, index, score

    i32 = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
    for offsets, groups, blank in ((i32(1, 2, 5, 9), GROUPS, BLANK), (i32(0, 5, 5, 9), GROUPS, BLANK), (i32(0, 1, 5, 11), GROUPS, -1),
                                   (OFFSETS, i32(1, 3, 2), BLANK), (OFFSETS, i32(1, -1, 2), BLANK), (OFFSETS, GROUPS, 8), (OFFSETS, GROUPS, R),
                                   (OFFSETS, GROUPS, -2)):
        rc, index, score = call(offsets, groups, blank)
        assert rc == _lib.CS_ERR_BAD_ARG, (offsets, groups, blank)
        assert bool((index == -7).all()) and bool((score == 3.25).all())
    rc, index, score = call(OFFSETS, GROUPS, BLANK)  # sim_out NULL: the similarities stay in the workspace, the choice is the same
    _lib.check(rc)
    assert torch.equal(index, good["reference_index"]) and torch.equal(score, good["score_map_ref_cross"])
    again = net.forward_select(q, bank, None, False, 0, True, group=GROUPS)
    torch.cuda.synchronize()
    for k in ("score_map_ref_cross", "score_mean_ref_cross", "reference_index"):
        assert torch.equal(again[k], good[k]), k
