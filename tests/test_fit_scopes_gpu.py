"""The four fit scopes on one forward: head, tail, cross and layer are nested, so on the same kept forward the head's four gradients
and the loss come out with the same bits from cs_head_backward, cs_tail_backward, cs_cross_backward and cs_layer_backward, the tail's six from
the last three, the cross-attention block's six from the last two, and none of the four backwards, which share one workspace, writes into what
the forward left for them.  What the forward keeps is one region carved by level: a forward at a lower level and a larger batch re-carves it, and
the deeper backwards then refuse."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from nets import TINY, make_net  # noqa: E402
from crossscore_amd import _lib, synth  # noqa: E402

pytestmark = pytest.mark.gpu

P = 14


def _gt(score, seed):
    g = torch.Generator().manual_seed(seed)
    return (score.cpu() + 0.3 * (torch.rand(score.shape, generator=g) - 0.5)).cuda().contiguous()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_nested_scopes_agree_and_leave_their_inputs_alone(dtype):
    B, N, H, W = 2, 2, 42, 56  # 3 x 4 tokens an image: M = 24 rows, a ragged last row tile in every kernel
    M = B * (H // P) * (W // P)
    net = make_net(TINY, 3, dtype)[0]
    q, r = synth.make_inputs(B, N, H, W, 5)
    q, r = torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()
    net.fit_layer_keep(True)
    score = net(q, r)["score_map_ref_cross"]
    gt = _gt(score, 9)

    def inputs():
        return [t.clone() for t in net.head_inputs(M) + net.tail_inputs(M) + net.cross_inputs(M, N) + net.layer_inputs(M)]

    before = inputs()
    head = net.head_backward(gt)
    tail = net.tail_backward(gt)
    cross = net.cross_backward(gt)
    layer = net.layer_backward(gt)
    after = inputs()
    torch.cuda.synchronize()
    assert len(head) == 5 and len(tail) == 11 and len(cross) == 17 and len(layer) == 23
    names = ("X", "A", "x2", "H", "x1", "Qp", "O", "lse", "K", "V", "x0", "Qs", "Ks", "Vs", "Os", "lse_s")
    assert len(before) == len(after) == len(names)
    for name, a, b in zip(names, before, after):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
    for i in range(5):  # dWa, dba, dWb, dbb, loss
        assert bool(torch.isfinite(head[i]).all()) and float(head[i].abs().max()) > 0
        assert torch.equal(head[i], tail[6 + i]) and torch.equal(head[i], cross[12 + i]), i
    for i in range(6):  # dW1, db1, dW2, db2, dg3, db3
        assert float(tail[i].abs().max()) > 0
        assert torch.equal(tail[i], cross[6 + i]), i
    for i in range(6):
        assert bool(torch.isfinite(cross[i]).all()) and float(cross[i].abs().max()) > 0
    for i in range(17):  # the cross backward's seventeen outputs, bit for bit
        assert torch.equal(cross[i], layer[6 + i]), i
    for i in range(6):  # dWin_s, dbin_s, dWo_s, dbo_s, dg1, db1
        assert bool(torch.isfinite(layer[i]).all()) and float(layer[i].abs().max()) > 0


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_kept_region_is_carved_again_at_a_lower_level_and_a_larger_batch(dtype):
    """One handle: a forward at the layer level (M = 24) and its backward, then a forward at the tail level with a larger batch (M = 36).  The
    kept region is carved again -- fewer pieces, each longer -- so the tail backward must read x2 and H where the second forward wrote them: it
    equals, bit for bit, the tail backward of a fresh net with the same weights after the same forward.  The deeper backwards refuse."""
    N, H, W = 2, 42, 56
    net = make_net(TINY, 3, dtype)[0]
    q, r = synth.make_inputs(3, N, H, W, 5)
    q, r = torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()
    net.fit_layer_keep(True)
    score = net(q[:2], r[:2])["score_map_ref_cross"]
    first = net.layer_backward(_gt(score, 9))
    assert all(bool(torch.isfinite(t).all()) for t in first)
    net.fit_layer_keep(False)
    net.fit_tail_keep(True)
    gt = _gt(net(q, r)["score_map_ref_cross"], 11)
    got = net.tail_backward(gt)

    fresh = make_net(TINY, 3, dtype)[0]
    fresh.fit_tail_keep(True)
    fresh(q, r)
    want = fresh.tail_backward(gt)
    torch.cuda.synchronize()
    assert len(got) == len(want) == 11
    for i, (a, b) in enumerate(zip(got, want)):
        assert float(b.abs().max()) > 0 and torch.equal(a, b), i
    with pytest.raises(_lib.CrossScoreHipError, match="cs_fit_cross_keep off"):
        net.cross_backward(gt)
    with pytest.raises(_lib.CrossScoreHipError, match="cs_fit_layer_keep off"):
        net.layer_backward(gt)
