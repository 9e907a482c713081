"""cs_forward_select / CrossScoreNet.forward_select: the forward that chooses each query's reference views on the device.
What it computes is pinned from two sides: the choice equals cs_op_select_references on descriptors formed by the single ops, and everything
behind the choice is bit-identical to forward_cached on the chosen rows."""
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


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _bank(net, imgs, N):
    tokens = net.encode_references(imgs)
    mean, centre, unit = net.reference_descriptors(tokens)
    return SelectionBank(tokens, mean, centre, unit, N)


def _images(n, H, W, seed):
    return torch.from_numpy(synth.make_inputs(n, 1, H, W, seed)[0]).cuda()


def _ops_selection(net, q, bank, N, exclude):
    """the choice formed by the single ops from the queries' own encode_references rows (the rounding the forward's 16-bit copy has)"""
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    qt = net.encode_references(q)
    B, Np, Cc = qt.shape
    code = _lib.DTYPE_BF16 if qt.dtype == torch.bfloat16 else _lib.DTYPE_F16
    mean = torch.empty((B, Cc), dtype=torch.float32, device=q.device)
    unit = torch.empty_like(mean)
    index = torch.empty((B, N), dtype=torch.int32, device=q.device)
    sim = torch.empty((B, len(bank)), dtype=torch.float32, device=q.device)
    _lib.check(lib.cs_op_token_descriptors(_p(qt), B, Np, Cc, code, _p(mean), st))
    _lib.check(lib.cs_op_descriptor_unit(_p(mean), B, Cc, _p(bank.centre), _p(unit), st))
    _lib.check(lib.cs_op_select_references(_p(unit), B, _p(bank.unit), len(bank), Cc, _p(exclude), N, _p(index), _p(sim), st))
    return index, sim, mean


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("H,W,B,N,R", [(70, 98, 1, 1, 4), (70, 98, 3, 2, 9), (42, 42, 3, 1, 9), (42, 42, 1, 2, 4)])
def test_forward_select_is_forward_cached_on_the_chosen_rows(H, W, B, N, R, dtype):
    net = make_net(TINY, 3, dtype)[0]
    bank = _bank(net, _images(R, H, W, 21), N)
    q = _images(B, H, W, 22)
    for exclude in (None, torch.tensor([(2 * b + 1) % R if b != 1 else -1 for b in range(B)], dtype=torch.int32).cuda()):
        if exclude is not None and N > R - 1:
            continue
        got = net.forward_select(q, bank, exclude, True, 1, True)
        index = got["reference_index"]
        assert index.dtype == torch.int32 and tuple(index.shape) == (B, N) and int(index.min()) >= 0 and int(index.max()) < R
        want = net.forward_cached(q, bank.tokens[index.long()], True, 1, True)
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(got[k], want[k]), k
        ops_index, ops_sim, _ = _ops_selection(net, q, bank, N, exclude)
        assert torch.equal(index, ops_index)
        assert torch.equal(got["reference_similarity"], torch.gather(ops_sim, 1, index.long()))
        if exclude is not None:
            for b in range(B):
                assert int(exclude[b]) not in index[b].tolist()
    # the launches the selection adds to the cached forward's, and nothing else
    index = net.forward_select(q, bank, None, True, 1, True)["reference_index"]
    sel = net.forward_stats()["kernels"]
    net.forward_cached(q, bank.tokens[index.long()], True, 1, True)
    base = net.forward_stats()["kernels"]
    extra = {k: v for k, v in sel.items() if k.startswith("select_")}
    assert extra == {"select_desc": 1, "select_unit": 1, "select_sim": 1, "select_topn": 1, "select_gather": 1}
    assert {k: v for k, v in sel.items() if k not in extra} == base


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_a_query_that_is_a_bank_image_picks_itself(dtype):
    H, W, R, N, j = 70, 98, 9, 2, 5
    net = make_net(TINY, 3, dtype)[0]
    imgs = _images(R, H, W, 31)
    bank = _bank(net, imgs, N)
    q = torch.stack([imgs[j], _images(1, H, W, 32)[0]])
    net.debug_capture(True)
    got = net.forward_select(q, bank, None, False, 0, True)
    pooled = net.debug_read("select_query_mean")
    net.debug_capture(False)
    torch.cuda.synchronize()
    assert int(got["reference_index"][0, 0]) == j
    assert abs(float(got["reference_similarity"][0, 0]) - 1.0) <= 1e-5
    assert torch.equal(pooled[0], bank.mean[j])  # the same rows, rounded the same way, pooled in the same order: bit for bit
    ex = torch.tensor([j, -1], dtype=torch.int32).cuda()
    again = net.forward_select(q, bank, ex, False, 0, True)
    assert j not in again["reference_index"][0].tolist()
    assert torch.equal(again["reference_index"][1], got["reference_index"][1])
    assert torch.equal(again["score_map_ref_cross"][1], got["score_map_ref_cross"][1])  # an item's result does not depend on its neighbours'


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_entry_points_and_batches_in_flight_give_the_same_bits(dtype):
    """fp32 and uint8 queries, one batch at a time and three in flight through ForwardPipeline: the same choice and the same maps"""
    from crossscore_amd.data import InputStage

    net = make_net(SMALL, 3, dtype)[0]
    dev = torch.device("cuda:0")
    stage = InputStage(dev, resize_short_side=70, integer_patches=True)
    rng = np.random.Generator(np.random.PCG64(17))
    R, N, B = 9, 2, 3
    raw = [rng.integers(0, 256, size=(90, 120, 3), dtype=np.uint8) for _ in range(R + 2 * B)]
    size = stage.geometry(90, 120)[1][2:]
    assert size == (70, 84)

    def f32(imgs):
        out = torch.empty((len(imgs), 3) + size, device=dev)
        for i, im in enumerate(imgs):
            stage(im, out[i])
        return out

    bank = _bank(net, f32(raw[:R]), N)
    batches = [raw[R:R + B], raw[R + B:]]
    ex = torch.tensor([-1, 3, -1], dtype=torch.int32, device=dev)
    want = [net.forward_select(f32(b), bank, ex, True, 2, True) for b in batches]
    assert net.u8_input_supported(stage.describe(raw[0]), size)
    for depth in (1, 3):
        pipe = ForwardPipeline(net, depth=depth)
        for u8 in (False, True):
            tickets = []
            for b in batches * 2:
                if u8:
                    tickets.append(pipe.submit_select(stage.batch([stage.describe(im) for im in b], size), bank, ex, True, 2, True))
                else:
                    tickets.append(pipe.submit_select(f32(b), bank, ex, True, 2, True))
            outs = [pipe.result(t) for t in tickets]
            torch.cuda.synchronize()
            for i, out in enumerate(outs):
                for k in KEYS + ("reference_index", "reference_similarity"):
                    assert torch.equal(out[k], want[i % 2][k]), (depth, u8, i, k)


def test_bad_arguments_raise_and_leave_the_handle_usable():
    H, W, R = 42, 42, 4
    net = make_net(TINY, 3, "fp16")[0]
    bank = _bank(net, _images(R, H, W, 41), 2)
    q = _images(2, H, W, 42)
    good = net.forward_select(q, bank, None, False, 0, True)
    with pytest.raises(ValueError):  # more views than the bank holds
        net.forward_select(q, bank, n_references=5)
    with pytest.raises(ValueError):  # ... than are eligible once a query may carry an exclusion
        net.forward_select(q, bank, torch.tensor([-1, -1], dtype=torch.int32).cuda(), n_references=4)
    with pytest.raises(NotImplementedError):
        net.forward_select(q, bank, n_references=33)
    with pytest.raises(ValueError):  # one exclusion per query
        net.forward_select(q, bank, torch.tensor([1], dtype=torch.int32).cuda())
    with pytest.raises(ValueError):  # the bank of another patch grid
        net.forward_select(_images(2, 70, 98, 43), bank)
    with pytest.raises(ValueError):  # tokens of the other operand type
        other = SelectionBank(bank.tokens.to(torch.bfloat16), bank.mean, bank.centre, bank.unit, 2)
        net.forward_select(q, other)
    lib = _lib.load()
    index = torch.empty((2, 2), dtype=torch.int32, device="cuda")
    score = torch.empty((2, 42, 42), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.cs_forward_select(net._handle, _p(q), _p(bank.tokens), None, _p(bank.centre), R, None, 2, 2, H, W, _p(score), None, 0, None, _p(index), None, st)
    assert rc == _lib.CS_ERR_BAD_ARG
    again = net.forward_select(q, bank, None, False, 0, True)
    torch.cuda.synchronize()
    for k in ("score_map_ref_cross", "score_mean_ref_cross", "reference_index"):
        assert torch.equal(again[k], good[k]), k
    # sim_out NULL: the similarities stay in the workspace, the choice is the same
    rc = lib.cs_forward_select(net._handle, _p(q), _p(bank.tokens), _p(bank.unit), _p(bank.centre), R, None, 2, 2, H, W, _p(score), None, 0, None, _p(index),
                               None, st)
    _lib.check(rc)
    torch.cuda.synchronize()
    assert torch.equal(index, good["reference_index"]) and torch.equal(score, good["score_map_ref_cross"])
