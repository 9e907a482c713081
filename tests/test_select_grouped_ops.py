"""The grouped forms of the reference selection (select.hip): cs_op_group_descriptors, cs_op_select_references_grouped and
cs_op_gather_tokens_ex.  No new oracle: a grouped call gives, for every query, bit for bit what the ungrouped ops (tests/test_select_ops.py pins
those against tests/select_oracle.py) give on the sliced group -- centre, units, similarities, and the local indices plus the group's offset."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from guard import guarded_out, poisoned_in  # noqa: E402
from crossscore_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

# groups of 1 (a row equal to its centre: zero unit), 5 (no multiple of the four centre lanes), 70 (more than a wave) and 300 rows (more than the 256
# threads of the top-N workgroup), and two rows behind them that belong to no group
SIZES = (1, 5, 70, 300)
OFFSETS = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
R = int(OFFSETS[-1]) + 2
G = len(SIZES)
NP = 35  # 7 x 5 patches: odd against the 32 row lanes of the descriptor kernel
GROUPS = np.array([3, 0, 2, 2, 1, 3, 0], dtype=np.int32)
B, N = len(GROUPS), 3
S = max(SIZES)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _h(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib_ungrouped():
    lib = _lib.load()

    def means(tok):
        I, Np, C_ = tok.shape
        out = torch.empty((I, C_), dtype=torch.float32, device=tok.device)
        _lib.check(lib.cs_op_token_descriptors(_p(tok), I, Np, C_, _lib.DTYPE_BF16 if tok.dtype == torch.bfloat16 else _lib.DTYPE_F16, _p(out), _st()))
        return out

    def centre(mean):
        out = torch.empty((mean.shape[1],), dtype=torch.float32, device=mean.device)
        _lib.check(lib.cs_op_descriptor_centre(_p(mean), mean.shape[0], mean.shape[1], _p(out), _st()))
        return out

    def unit(mean, mu):
        out = torch.empty_like(mean)
        _lib.check(lib.cs_op_descriptor_unit(_p(mean), mean.shape[0], mean.shape[1], _p(mu), _p(out), _st()))
        return out

    def select(q, bank, n, exclude=None):
        index = torch.full((q.shape[0], n), -7, dtype=torch.int32, device=q.device)
        sim = torch.full((q.shape[0], bank.shape[0]), float("nan"), dtype=torch.float32, device=q.device)
        _lib.check(lib.cs_op_select_references(_p(q), q.shape[0], _p(bank), bank.shape[0], q.shape[1], _p(exclude), n, _p(index), _p(sim), _st()))
        return index, sim

    return means, centre, unit, select


def group_descriptors(mean, offsets, centre=None, unit=None):
    Rr, C_ = mean.shape
    g = len(offsets) - 1
    centre = centre if centre is not None else torch.empty((g, C_), dtype=torch.float32, device=mean.device)
    unit = unit if unit is not None else torch.zeros((Rr, C_), dtype=torch.float32, device=mean.device)
    _lib.check(_lib.load().cs_op_group_descriptors(_p(mean), Rr, C_, _h(offsets), g, _p(centre), _p(unit), _st()))
    return centre, unit


def select_grouped(q_mean, groups, bank_unit, centre, offsets, n, exclude=None, index=None, sim=None):
    Bq, C_ = q_mean.shape
    s = int(np.diff(offsets).max())
    index = index if index is not None else torch.full((Bq, n), -7, dtype=torch.int32, device=q_mean.device)
    sim = sim if sim is not None else torch.zeros((Bq, s), dtype=torch.float32, device=q_mean.device)
    _lib.check(_lib.load().cs_op_select_references_grouped(_p(q_mean), Bq, _h(groups), _p(bank_unit), _p(centre), _h(offsets), len(offsets) - 1,
                                                           bank_unit.shape[0], C_, _p(exclude), n, _p(index), _p(sim), _st()))
    return index, sim


def gather_ex(bank, index, blank_row, out=None):
    Rr, Np, C_ = bank.shape
    Bq, n = index.shape
    out = out if out is not None else torch.empty((Bq, n, Np, C_), dtype=bank.dtype, device=bank.device)
    _lib.check(_lib.load().cs_op_gather_tokens_ex(_p(bank), Rr, Np, C_, _p(index), Bq, n, _p(out), _st(), blank_row))
    return out


_CASES = {}


def _case(C_, bf16):
    """the case's tokens, means and the per-slice results of today's ops: formed once, shared by the tests, never written"""
    key = (C_, bf16)
    if key not in _CASES:
        means, centre, unit, _ = _lib_ungrouped()
        rng = np.random.Generator(np.random.PCG64(1000 + C_ + int(bf16)))
        x = rng.normal(size=(R + B, NP, C_)) * 0.8 + rng.normal(size=(1, NP, C_)) * 0.5 + rng.normal(size=(R + B, 1, C_)) * 0.3
        tok = torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16 if bf16 else torch.float16).cuda()
        m = means(tok)
        bank_mean, q_mean = m[:R].contiguous(), m[R:].contiguous()
        slice_centre = [centre(bank_mean[OFFSETS[g]:OFFSETS[g + 1]].contiguous()) for g in range(G)]
        slice_unit = [unit(bank_mean[OFFSETS[g]:OFFSETS[g + 1]].contiguous(), slice_centre[g]) for g in range(G)]
        torch.cuda.synchronize()
        _CASES[key] = (tok[:R].contiguous(), bank_mean, q_mean, slice_centre, slice_unit)
    return _CASES[key]


def _slice_selection(C_, bf16, b, n, exclude_row=None, q_mean=None):
    """query b against its group alone through today's ops -> (global indices padded with -1 (n), similarities (group size))"""
    _, _, q_all, slice_centre, slice_unit = _case(C_, bf16)
    _, _, unit, select = _lib_ungrouped()
    g = int(GROUPS[b])
    lo, size = int(OFFSETS[g]), SIZES[g]
    q = unit((q_all if q_mean is None else q_mean)[b:b + 1].contiguous(), slice_centre[g])
    ex = None
    eligible = size
    if exclude_row is not None:
        local = exclude_row - lo if lo <= exclude_row < lo + size else -1
        ex = torch.tensor([local], dtype=torch.int32).cuda()
        eligible = size - 1  # today's op counts an exclusion array as one entry less, whatever it holds
    take = min(n, eligible)
    if take == 0:
        _, sim = select(q, slice_unit[g], 1)
        return [-1] * n, sim[0]
    index, sim = select(q, slice_unit[g], take, ex)
    picks = [i + lo if i >= 0 else -1 for i in index[0].tolist()]
    return picks + [-1] * (n - take), sim[0]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("C_", [128, 384])
def test_group_descriptors_equal_the_ops_on_each_slice(C_, bf16):
    _, bank_mean, _, slice_centre, slice_unit = _case(C_, bf16)
    mu_out, mu_check = guarded_out((G, C_), torch.float32)
    sentinel = torch.full((R, C_), 7.5, dtype=torch.float32, device="cuda")
    e_out, e_check = guarded_out((R, C_), torch.float32, init=sentinel)
    mu, e = group_descriptors(poisoned_in(bank_mean), OFFSETS, mu_out, e_out)
    mu_check("centres")
    e_check("units")
    for g in range(G):
        assert torch.equal(mu[g], slice_centre[g]), g
        assert torch.equal(e[OFFSETS[g]:OFFSETS[g + 1]], slice_unit[g]), g
    assert bool((e[0] == 0).all())                  # the group of one: its row is its centre
    assert bool((e[OFFSETS[G]:] == 7.5).all())      # the rows behind the last group are left alone
    # one group over every row is today's bank
    means, centre, unit, _ = _lib_ungrouped()
    whole = np.array([0, R], dtype=np.int32)
    mu1, e1 = group_descriptors(bank_mean, whole)
    want_mu = centre(bank_mean)
    assert torch.equal(mu1[0], want_mu) and torch.equal(e1, unit(bank_mean, want_mu))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("C_", [128, 384])
def test_grouped_selection_equals_the_ops_on_each_slice(C_, bf16):
    _, bank_mean, q_mean, _, _ = _case(C_, bf16)
    mu, e = group_descriptors(bank_mean, OFFSETS)
    idx_out, idx_check = guarded_out((B, N), torch.int32)
    sim_out, sim_check = guarded_out((B, S), torch.float32)
    index, sim = select_grouped(poisoned_in(q_mean), GROUPS, poisoned_in(e), mu, OFFSETS, N, None, idx_out, sim_out)
    idx_check("index")
    sim_check("similarities")
    index, sim = index.clone(), sim.clone()
    for b in range(B):
        size = SIZES[GROUPS[b]]
        want_index, want_sim = _slice_selection(C_, bf16, b, N)
        assert index[b].tolist() == want_index, (b, index[b].tolist(), want_index)
        assert torch.equal(sim[b, :size], want_sim), b
        assert bool(torch.isnan(sim[b, size:]).all()), b  # written, as a NaN: the buffer held zeros / the sentinel
    lo = int(OFFSETS[0])
    assert index[1].tolist() == [lo, -1, -1] and index[6].tolist() == [lo, -1, -1]  # the group of one
    # every query alone equals the query at any place of the batch
    for b in range(B):
        one_i, one_s = select_grouped(q_mean[b:b + 1].contiguous(), GROUPS[b:b + 1].copy(), e, mu, OFFSETS, N)
        size = SIZES[GROUPS[b]]
        assert torch.equal(one_i[0], index[b]) and torch.equal(one_s[0, :size], sim[b, :size]), b
    order = np.array([4, 2, 6, 0, 5, 1, 3])
    mixed_i, mixed_s = select_grouped(q_mean[torch.from_numpy(order).cuda()].contiguous(), GROUPS[order].copy(), e, mu, OFFSETS, N)
    assert torch.equal(mixed_i, index[torch.from_numpy(order).cuda()])
    assert torch.equal(mixed_s.nan_to_num(nan=-9.0), sim[torch.from_numpy(order).cuda()].nan_to_num(nan=-9.0))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("C_", [128, 384])
def test_exclusions_inside_and_outside_the_group(C_, bf16):
    _, bank_mean, q_mean, _, _ = _case(C_, bf16)
    mu, e = group_descriptors(bank_mean, OFFSETS)
    plain, _ = select_grouped(q_mean, GROUPS, e, mu, OFFSETS, N)
    plain = plain.cpu().numpy()
    # query 0, 2, 4: their own best (inside); 1: the only row of its group; 3: a row of another group; 5: the blank tail; 6: none
    ex = np.array([plain[0, 0], OFFSETS[0], plain[2, 0], plain[0, 0], plain[4, 0], R - 1, -1], dtype=np.int32)
    index, _ = select_grouped(q_mean, GROUPS, e, mu, OFFSETS, N, torch.from_numpy(ex).cuda())
    index = index.cpu().numpy()
    for b in range(B):
        want, _ = _slice_selection(C_, bf16, b, N, int(ex[b])) if ex[b] >= 0 else (plain[b].tolist(), None)
        assert index[b].tolist() == want, (b, index[b].tolist(), want)
    assert index[1].tolist() == [-1, -1, -1]                      # its group's one row excluded: nothing left
    assert np.array_equal(index[3], plain[3]) and np.array_equal(index[5], plain[5]) and np.array_equal(index[6], plain[6])
    for b in (0, 2, 4):
        assert ex[b] not in index[b] and index[b, 0] == plain[b, 1]


def test_equal_rows_give_the_lower_index_and_nan_rows_never_qualify():
    C_, bf16 = 384, False
    _, bank_mean, q_mean, _, _ = _case(C_, bf16)
    m = bank_mean.clone()
    lo70, lo300 = int(OFFSETS[2]), int(OFFSETS[3])
    m[lo300 + 280] = m[lo300 + 11]   # a later copy (behind the workgroup's first 256 rows) of row 11 of the 300
    m[lo70 + 3] = m[lo70 + 40]       # ... and an earlier copy of row 40 of the 70
    q = q_mean.clone()
    q[0], q[2] = m[lo300 + 11], m[lo70 + 40]
    mu, e = group_descriptors(m, OFFSETS)
    index, sim = select_grouped(q, GROUPS, e, mu, OFFSETS, N)
    index, sim = index.cpu().numpy(), sim.cpu().numpy()
    assert sim[0, 11].tobytes() == sim[0, 280].tobytes() and sim[2, 3].tobytes() == sim[2, 40].tobytes()
    assert index[0, :2].tolist() == [lo300 + 11, lo300 + 280] and index[2, :2].tolist() == [lo70 + 3, lo70 + 40]
    ex = torch.tensor([lo300 + 11, -1, lo70 + 3, -1, -1, -1, -1], dtype=torch.int32).cuda()
    index, _ = select_grouped(q, GROUPS, e, mu, OFFSETS, N, ex)
    assert int(index[0, 0]) == lo300 + 280 and int(index[2, 0]) == lo70 + 40
    # a NaN row of the bank's units never qualifies, wherever its similarity would rank
    e_nan = e.clone()
    lo5 = int(OFFSETS[1])
    e_nan[lo5 + 1] = float("nan")
    e_nan[lo5 + 4] = float("nan")
    index, sim = select_grouped(q, GROUPS, e_nan, mu, OFFSETS, 5)
    got = index[4].tolist()  # query 4 chooses from the group of five
    assert sorted(got[:3]) == [lo5, lo5 + 2, lo5 + 3] and got[3:] == [-1, -1]
    assert bool(torch.isnan(sim[4, 1])) and bool(torch.isnan(sim[4, 4]))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("C_", [128, 384])
def test_gather_with_and_without_a_blank_row(C_, bf16):
    bank, _, _, _, _ = _case(C_, bf16)
    index = np.array([[0, -1, 5], [R, 377, -1]], dtype=np.int32)
    raw = bank.view(torch.int16)
    for blank in (-1, R - 1, R - 2):
        out, check = guarded_out((2, 3, NP, C_), bank.dtype)
        flat = poisoned_in(bank.reshape(R * NP, C_)).reshape(R, NP, C_)
        got = gather_ex(flat, torch.from_numpy(index).cuda(), blank, out)
        check("gathered tokens")
        got = got.view(torch.int16)
        for b in range(2):
            for n in range(3):
                i = int(index[b, n])
                want = raw[i] if 0 <= i < R else (raw[blank] if blank >= 0 else torch.zeros_like(raw[0]))
                assert torch.equal(got[b, n], want), (blank, b, n)
    # blank_row = -1 is today's entry point
    plain = torch.empty((2, 3, NP, C_), dtype=bank.dtype, device="cuda")
    _lib.check(_lib.load().cs_op_gather_tokens(_p(bank), R, NP, C_, _p(torch.from_numpy(index).cuda()), 2, 3, _p(plain), _st()))
    assert torch.equal(plain.view(torch.int16), gather_ex(bank, torch.from_numpy(index).cuda(), -1).view(torch.int16))


def test_bad_arguments_queue_nothing_and_leave_the_library_usable():
    C_ = 128
    bank, bank_mean, q_mean, _, _ = _case(C_, False)
    mu, e = group_descriptors(bank_mean, OFFSETS)
    good_i, good_s = select_grouped(q_mean, GROUPS, e, mu, OFFSETS, N)
    lib = _lib.load()

    def off(*v):
        return np.array(v, dtype=np.int32)

    bad_offsets = [off(1, 6, 76, 300, 376), off(0, 6, 6, 76, 376), off(0, 6, 5, 76, 376), off(0, 1, 6, 76, R + 1)]
    for o in bad_offsets:
        mu_s = torch.full((G, C_), 3.25, dtype=torch.float32, device="cuda")
        e_s = torch.full((R, C_), 3.25, dtype=torch.float32, device="cuda")
        rc = lib.cs_op_group_descriptors(_p(bank_mean), R, C_, _h(o), G, _p(mu_s), _p(e_s), _st())
        assert rc == _lib.CS_ERR_BAD_ARG, o
        idx_s = torch.full((B, N), -7, dtype=torch.int32, device="cuda")
        sim_s = torch.full((B, S), 3.25, dtype=torch.float32, device="cuda")
        rc = lib.cs_op_select_references_grouped(_p(q_mean), B, _h(GROUPS), _p(e), _p(mu), _h(o), G, R, C_, None, N, _p(idx_s), _p(sim_s), _st())
        assert rc == _lib.CS_ERR_BAD_ARG, o
        torch.cuda.synchronize()
        assert bool((mu_s == 3.25).all()) and bool((e_s == 3.25).all()) and bool((idx_s == -7).all()) and bool((sim_s == 3.25).all())
    for groups in (np.array([3, 0, 2, 2, 1, 4, 0], dtype=np.int32), np.array([3, 0, -1, 2, 1, 3, 0], dtype=np.int32)):
        idx_s = torch.full((B, N), -7, dtype=torch.int32, device="cuda")
        sim_s = torch.full((B, S), 3.25, dtype=torch.float32, device="cuda")
        rc = lib.cs_op_select_references_grouped(_p(q_mean), B, _h(groups), _p(e), _p(mu), _h(OFFSETS), G, R, C_, None, N, _p(idx_s), _p(sim_s), _st())
        assert rc == _lib.CS_ERR_BAD_ARG
        torch.cuda.synchronize()
        assert bool((idx_s == -7).all()) and bool((sim_s == 3.25).all())
    idx_s = torch.full((B, 33), -7, dtype=torch.int32, device="cuda")
    sim_s = torch.full((B, S), 3.25, dtype=torch.float32, device="cuda")
    rc = lib.cs_op_select_references_grouped(_p(q_mean), B, _h(GROUPS), _p(e), _p(mu), _h(OFFSETS), G, R, C_, None, 33, _p(idx_s), _p(sim_s), _st())
    assert rc == _lib.CS_ERR_UNSUPPORTED
    index = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    for blank in (-2, R):
        out_s = torch.full((1, 2, NP, C_), 3.25, dtype=bank.dtype, device="cuda")
        rc = lib.cs_op_gather_tokens_ex(_p(bank), R, NP, C_, _p(index), 1, 2, _p(out_s), _st(), blank)
        assert rc == _lib.CS_ERR_BAD_ARG
        torch.cuda.synchronize()
        assert bool((out_s == 3.25).all())
    # N larger than a group is legal, and the library is usable afterwards
    again_i, again_s = select_grouped(q_mean, GROUPS, e, mu, OFFSETS, N)
    torch.cuda.synchronize()
    assert torch.equal(again_i, good_i) and torch.equal(again_s.nan_to_num(nan=-9.0), good_s.nan_to_num(nan=-9.0))
