"""The three fit scopes on one forward: head, tail and cross are nested, so on the same kept forward the head's four gradients and
the loss come out with the same bits from cs_head_backward, cs_tail_backward and cs_cross_backward, the tail's six from the last two, and none
of the three backwards, which share one workspace, writes into what the forward left for them."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from nets import TINY, make_net  # noqa: E402
from crossscore_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

P = 14


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_nested_scopes_agree_and_leave_their_inputs_alone(dtype):
    B, N, H, W = 2, 2, 42, 56  # 3 x 4 tokens an image: M = 24 rows, a ragged last row tile in every kernel
    M = B * (H // P) * (W // P)
    net = make_net(TINY, 3, dtype)[0]
    q, r = synth.make_inputs(B, N, H, W, 5)
    q, r = torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()
    net.fit_cross_keep(True)
    score = net(q, r)["score_map_ref_cross"]
    g = torch.Generator().manual_seed(9)
    gt = (score.cpu() + 0.3 * (torch.rand(score.shape, generator=g) - 0.5)).cuda().contiguous()

    def inputs():
        return [t.clone() for t in net.head_inputs(M) + net.tail_inputs(M) + net.cross_inputs(M, N)]

    before = inputs()
    head = net.head_backward(gt)
    tail = net.tail_backward(gt)
    cross = net.cross_backward(gt)
    after = inputs()
    torch.cuda.synchronize()
    assert len(head) == 5 and len(tail) == 11 and len(cross) == 17
    for name, a, b in zip(("X", "A", "x2", "H", "x1", "Qp", "O", "lse", "K", "V"), before, after):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
    for i in range(5):  # dWa, dba, dWb, dbb, loss
        assert bool(torch.isfinite(head[i]).all()) and float(head[i].abs().max()) > 0
        assert torch.equal(head[i], tail[6 + i]) and torch.equal(head[i], cross[12 + i]), i
    for i in range(6):  # dW1, db1, dW2, db2, dg3, db3
        assert float(tail[i].abs().max()) > 0
        assert torch.equal(tail[i], cross[6 + i]), i
    for i in range(6):
        assert bool(torch.isfinite(cross[i]).all()) and float(cross[i].abs().max()) > 0
