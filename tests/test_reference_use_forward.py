"""need_reference_use / cs_request_reference_use through the forward: the four outputs against the eight one-head attention maps
need_attn_weights returns, every other output bit for bit as without the request, one launch more in the census, the one-shot rule, and the same
bits through every entry point and any number of batches in flight."""
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
import guard  # noqa: E402
import reference_use_oracle as oracle  # noqa: E402

pytestmark = pytest.mark.gpu

USE = ("ref_use_share", "ref_use_peak_prob", "ref_use_peak_index", "ref_use_entropy")
# The forward's outputs against the fp64 recomputation from the eight fp32 maps of need_attn_weights_head_id = 0 .. 7.  Both sides use the same
# lse and operand values; they differ by the order of the fp32 dot products (MFMA against a scalar chain) and the fp32 sums.  Bounds: 4 x the
# maxima measured on an MI355X over the cases below, as fractions of the caps of reference_use_oracle.check_values -- which they
# may never exceed.
MEASURED_OF_CAP = {"share": 0.0006, "peak_prob": 0.0024, "entropy": 0.0005}
BOUND_OF_CAP = {k: min(1.0, 4 * v) for k, v in MEASURED_OF_CAP.items()}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _inputs(B, N, H, W, seed):
    q, r = synth.make_inputs(B, N, H, W, seed)
    return torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()


def _same(a, b, keys):
    torch.cuda.synchronize()
    for k in keys:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("backbone,H,W,B,N", [(TINY, 70, 98, 3, 2), (TINY, 42, 42, 2, 3), (SMALL, 70, 84, 2, 3)])
def test_outputs_equal_what_the_eight_attention_maps_give(backbone, H, W, B, N, dtype):
    net = make_net(backbone, 3, dtype)[0]
    q, r = _inputs(B, N, H, W, 5)
    got = net(q, r, need_reference_use=True)
    P = net.arch.patch
    h, w = H // P, W // P
    Np, heads = h * w, net.arch.dec_heads
    assert heads == 8
    assert tuple(got["ref_use_share"].shape) == (B, N, h, w) and tuple(got["ref_use_entropy"].shape) == (B, h, w)
    assert got["ref_use_peak_index"].dtype == torch.int32 and tuple(got["ref_use_peak_index"].shape) == (B, N, h, w)
    maps = [net(q, r, True, hd)["attn_weights_map_ref_cross"].double().cpu().numpy().reshape(B, Np, N * Np) for hd in range(heads)]
    p = np.stack(maps, axis=1)  # (B, heads, Lq, Lk)
    pm = p.mean(axis=1).reshape(B, Np, N, Np)
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = np.where(p > 0, -p * np.log2(p), 0.0).sum(axis=-1).mean(axis=1)
    want = {"share": pm.sum(axis=-1).transpose(0, 2, 1), "peak_prob": pm.max(axis=-1).transpose(0, 2, 1),
            "peak_index": pm.argmax(axis=-1).transpose(0, 2, 1), "entropy": ent, "pm": pm}
    mine = {k[len("ref_use_"):]: got[k].cpu().numpy().reshape((B, N, Np) if got[k].dim() == 4 else (B, Np)) for k in USE}
    fig = oracle.check_values(mine, want, f"{backbone} {dtype}")
    inside, total = oracle.check_peak_index(mine["peak_index"], want, Np)
    print(f"{backbone} {dtype} {H}x{W} B {B} N {N}: of their caps: " + ", ".join(f"{k} {v:.4f}" for k, v in fig.items() if k != "sum") +
          f"; |sum - 1| {fig['sum']:.2e}; {inside} of {total} peak cases inside the margin")
    for k, bound in BOUND_OF_CAP.items():
        assert fig[k] <= bound, (k, fig[k], bound)
    assert inside <= oracle.MAX_INSIDE * total, (inside, total)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("backbone,H,W", [(TINY, 70, 98), (SMALL, 70, 84)])
def test_other_outputs_keep_their_bits_and_the_census_gains_one_launch(backbone, H, W, dtype):
    net = make_net(backbone, 3, dtype)[0]
    q, r = _inputs(2, 2, H, W, 6)
    keys = ("score_map_ref_cross", "score_mean_ref_cross", "attn_weights_map_ref_cross")
    plain = net(q, r, False, 0, False, True)
    census = net.forward_stats()
    assert "ref_use" not in census["kernels"]
    use = net(q, r, False, 0, False, True, need_reference_use=True)
    census_use = net.forward_stats()
    _same(plain, use, keys)
    assert census_use["kernels"] == dict(census["kernels"], ref_use=1) and census_use["launches"] == census["launches"] + 1
    # beside need_attn_weights: legal, both launches, the same bits on every side
    attn = net(q, r, True, 3, False, True)
    census_attn = net.forward_stats()
    both = net(q, r, True, 3, False, True, need_reference_use=True)
    assert net.forward_stats()["kernels"] == dict(census_attn["kernels"], ref_use=1)
    _same(attn, both, keys)
    _same(use, both, USE)
    # and the forward behind it is the plain one again
    again = net(q, r, False, 0, False, True)
    assert net.forward_stats() == dict(census, host_enqueue_ms=net.forward_stats()["host_enqueue_ms"])
    assert not any(k in again for k in USE)
    _same(plain, again, keys)


def _guarded_request(net, B, N, h, w):
    """arms the request on net's handle with outputs inside guard bands -> ({name: view}, [check])"""
    views, checks = {}, []
    for name in USE:
        shape = (B, h, w) if name.endswith("entropy") else (B, N, h, w)
        v, chk = guard.guarded_out(shape, torch.int32 if name.endswith("index") else torch.float32, guard_rows=64)
        views[name] = v
        checks.append(chk)
    _lib.check(_lib.load().cs_request_reference_use(net._handle, *(_p(views[k]) for k in USE)))
    return views, checks


def _untouched(views):
    torch.cuda.synchronize()
    return all(bool((v.view(torch.int32) == guard._signed(guard.SENTINEL[v.dtype], 4)).all()) for v in views.values())


def test_the_request_is_one_shot_and_a_failing_forward_clears_it():
    H, W, B, N = 70, 98, 2, 2
    net = make_net(TINY, 3, "fp16")[0]
    q, r = _inputs(B, N, H, W, 7)
    want = net(q, r, need_reference_use=True)
    # armed through the C ABI: the next forward fills the buffers and nothing around them ...
    views, checks = _guarded_request(net, B, N, 5, 7)
    net(q, r)
    for chk in checks:
        chk()
    _same(views, want, USE)
    # ... and the one behind it writes nothing into them
    kept = {k: v.clone() for k, v in views.items()}
    for v in views.values():
        v.view(torch.int32).fill_(guard._signed(guard.SENTINEL[v.dtype], 4))
    out = net(q, r)
    assert _untouched(views) and not any(k in out for k in USE)
    # a forward that fails its argument check takes the request with it
    views, checks = _guarded_request(net, B, N, 5, 7)
    with pytest.raises(ValueError):
        net(q, r, True, 99)
    net(q, r)
    assert _untouched(views)
    # all pointers null cancels
    views, checks = _guarded_request(net, B, N, 5, 7)
    _lib.check(_lib.load().cs_request_reference_use(net._handle, None, None, None, None))
    net(q, r)
    assert _untouched(views)
    # encoding references is no forward: the request stays armed across it
    views, checks = _guarded_request(net, B, N, 5, 7)
    net.encode_references(r[:, 0].contiguous())
    assert _untouched(views)
    net(q, r)
    for chk in checks:
        chk()
    _same(views, kept, USE)
    # any subset of the outputs
    share, chk = guard.guarded_out((B, N, 5, 7), torch.float32, guard_rows=64)
    _lib.check(_lib.load().cs_request_reference_use(net._handle, _p(share), None, None, None))
    net(q, r)
    chk()
    assert torch.equal(share, want["ref_use_share"])


def test_no_reference_views_with_a_request_is_an_error():
    net = make_net(TINY, 3, "fp16")[0]
    q, r = _inputs(2, 1, 42, 42, 8)
    with pytest.raises(ValueError):
        net(q, r[:, :0], need_reference_use=True)
    out = net(q, r)  # the handle is usable and the request is gone
    assert not any(k in out for k in USE)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_every_entry_point_and_any_depth_give_the_same_bits(dtype):
    """plain, cached, uint8, cached uint8 and select on the same references; one batch at a time and three in flight"""
    from crossscore_amd.data import InputStage

    net = make_net(SMALL, 3, dtype)[0]
    dev = torch.device("cuda:0")
    stage = InputStage(dev, resize_short_side=70, integer_patches=True)
    rng = np.random.Generator(np.random.PCG64(19))
    B, N = 2, 2
    raw_q = [rng.integers(0, 256, size=(90, 120, 3), dtype=np.uint8) for _ in range(B)]
    raw_r = [rng.integers(0, 256, size=(90, 120, 3), dtype=np.uint8) for _ in range(B * N)]
    size = stage.geometry(90, 120)[1][2:]

    def f32(imgs):
        out = torch.empty((len(imgs), 3) + size, device=dev)
        for i, im in enumerate(imgs):
            stage(im, out[i])
        return out

    def u8(imgs):
        return stage.batch([stage.describe(im) for im in imgs], size)

    q, r = f32(raw_q), f32(raw_r)
    keys = USE + ("score_map_ref_cross",)
    want = net(q, r.view(B, N, 3, *size), need_reference_use=True)
    tokens = net.encode_references(r)
    _same(net.forward_cached(q, tokens.view(B, N, *tokens.shape[1:]), need_reference_use=True), want, keys)
    assert net.u8_input_supported(stage.describe(raw_q[0]), size)
    _same(net.forward(u8(raw_q), u8(raw_r), need_reference_use=True), want, keys)
    _same(net.forward_cached(u8(raw_q), tokens.view(B, N, *tokens.shape[1:]), need_reference_use=True), want, keys)
    # select: whatever it chooses, the outputs are those of the cached forward on the chosen rows
    mean, centre, unit = net.reference_descriptors(tokens)
    bank = SelectionBank(tokens, mean, centre, unit, N)
    sel = net.forward_select(q, bank, need_reference_use=True)
    _same(sel, net.forward_cached(q, bank.tokens[sel["reference_index"].long()], need_reference_use=True), keys)
    _same(net.forward_select(u8(raw_q), bank, need_reference_use=True), sel, keys + ("reference_index",))
    for depth in (1, 3):
        pipe = ForwardPipeline(net, depth=depth)
        tickets = [pipe.submit(q, r.view(B, N, 3, *size), need_reference_use=True) for _ in range(4)]
        tickets += [pipe.submit_cached(q, tokens.view(B, N, *tokens.shape[1:]), need_reference_use=True) for _ in range(2)]
        plain = pipe.submit(q, r.view(B, N, 3, *size))
        for t in tickets:
            _same(pipe.result(t), want, keys)
        assert not any(k in pipe.result(plain) for k in USE)
