"""The single-op entry points of the reference selection (select.hip) against tests/select_oracle.py: pooled descriptors,
centre, unit vectors, similarities + the N best per query, and the gather of the chosen token blocks.  Bounds come from the oracle's
fp32-sequential restatement on each case's own input (select_oracle.tolerance), never from what a kernel returns."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import select_oracle as so  # noqa: E402
from guard import guarded_out, poisoned_in  # noqa: E402
from crossscore_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

DESC_SHAPES = [(1, 1, 128), (3, 7, 128), (2, 64, 384), (2, 65, 384), (1, 1369, 384), (2, 35, 1536)]  # (I, Np, C)
SELECT_SHAPES = [(1, 1, 1), (1, 5, 5), (3, 33, 5), (8, 64, 5), (2, 257, 32), (2, 4099, 5)]            # (B, R, N)
# seeds for which every query's first N + 1 similarities (fp64 oracle) lie at least 1e-4 apart -- with and without the exclusions of
# _exclusions below; found by counting up from 0 on the CPU, and asserted again by every test that relies on it
SELECT_SEEDS = {(128, 1, 1, 1): 0, (128, 1, 5, 5): 0, (128, 3, 33, 5): 0, (128, 8, 64, 5): 0, (128, 2, 257, 32): 9, (128, 2, 4099, 5): 0,
                (384, 1, 1, 1): 0, (384, 1, 5, 5): 0, (384, 3, 33, 5): 0, (384, 8, 64, 5): 1, (384, 2, 257, 32): 1291, (384, 2, 4099, 5): 3}
MIN_GAP = 1e-4


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tokens(I, Np, C_, seed, bf16):
    """(I, Np, C) 16-bit tokens like a decoder input: unit-scale rows on top of a position pattern every image shares; -> (device tensor, fp64)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.normal(size=(I, Np, C_)) * 0.8 + rng.normal(size=(1, Np, C_)) * 0.5 + rng.normal(size=(I, 1, C_)) * 0.3
    t = torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16 if bf16 else torch.float16)
    return t.cuda(), t.to(torch.float64).numpy()


def token_descriptors(tok, out=None):
    I, Np, C_ = tok.shape
    out = out if out is not None else torch.empty((I, C_), dtype=torch.float32, device=tok.device)
    code = _lib.DTYPE_BF16 if tok.dtype == torch.bfloat16 else _lib.DTYPE_F16
    _lib.check(_lib.load().cs_op_token_descriptors(_p(tok), I, Np, C_, code, _p(out), _st()))
    return out


def descriptor_centre(mean, out=None):
    R, C_ = mean.shape
    out = out if out is not None else torch.empty((C_,), dtype=torch.float32, device=mean.device)
    _lib.check(_lib.load().cs_op_descriptor_centre(_p(mean), R, C_, _p(out), _st()))
    return out


def descriptor_unit(mean, centre, out=None):
    I, C_ = mean.shape
    out = out if out is not None else torch.empty((I, C_), dtype=torch.float32, device=mean.device)
    _lib.check(_lib.load().cs_op_descriptor_unit(_p(mean), I, C_, _p(centre), _p(out), _st()))
    return out


def select_references(q, bank, N, exclude=None, index=None, sim=None):
    B, C_ = q.shape
    R = bank.shape[0]
    index = index if index is not None else torch.full((B, N), -7, dtype=torch.int32, device=q.device)
    sim = sim if sim is not None else torch.full((B, R), float("nan"), dtype=torch.float32, device=q.device)
    _lib.check(_lib.load().cs_op_select_references(_p(q), B, _p(bank), R, C_, _p(exclude), N, _p(index), _p(sim), _st()))
    return index, sim


def gather_tokens(bank, index, out=None):
    R, Np, C_ = bank.shape
    B, N = index.shape
    out = out if out is not None else torch.empty((B, N, Np, C_), dtype=bank.dtype, device=bank.device)
    _lib.check(_lib.load().cs_op_gather_tokens(_p(bank), R, Np, C_, _p(index), B, N, _p(out), _st()))
    return out


# ------------------------------------------------------------------------------------------------------------------- descriptors
@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("I,Np,C_", DESC_SHAPES)
def test_token_descriptors(I, Np, C_, bf16):
    """mean against fp64 within the case's own bound; an image's mean has the same bits alone and at any position of a larger call; nothing is
    written outside the output and nothing is read outside the tokens (poisoned padding)"""
    tok, t64 = _tokens(I, Np, C_, 100 + I + Np + C_, bf16)
    want = so.mean(t64)
    tol = so.tolerance(want, so.mean_seq32(t64))
    out, check = guarded_out((I, C_), torch.float32)
    got = token_descriptors(poisoned_in(tok.reshape(I * Np, C_)).reshape(I, Np, C_), out)
    check("mean")
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"token_descriptors ({I},{Np},{C_}) {'bf16' if bf16 else 'fp16'}: max |err| {err:.3e}, bound {tol:.3e}")
    assert err <= tol, (err, tol)
    # the same images inside a larger call, at other positions, and each alone
    more, _ = _tokens(3, Np, C_, 7, bf16)
    mixed = torch.cat([more[:2], tok.flip(0), more[2:]])
    big = token_descriptors(mixed)
    assert torch.equal(big[2:2 + I], got.flip(0))
    for i in range(I):
        assert torch.equal(token_descriptors(tok[i:i + 1].contiguous())[0], got[i]), i


def test_token_descriptor_arguments():
    tok, _ = _tokens(1, 3, 128, 1, False)
    out = torch.empty((1, 128), dtype=torch.float32, device="cuda")
    lib = _lib.load()
    with pytest.raises(ValueError):
        _lib.check(lib.cs_op_token_descriptors(_p(tok), 1, 3, 128, _lib.DTYPE_F32, _p(out), _st()))
    with pytest.raises(NotImplementedError):
        _lib.check(lib.cs_op_token_descriptors(_p(tok), 1, 4, 96, _lib.DTYPE_F16, _p(out), _st()))
    with pytest.raises(ValueError):
        _lib.check(lib.cs_op_token_descriptors(None, 1, 3, 128, _lib.DTYPE_F16, _p(out), _st()))


@pytest.mark.parametrize("R,C_", [(1, 128), (3, 128), (7, 384), (64, 384), (257, 384), (35, 1536)])
def test_centre_and_unit(R, C_):
    """centre and unit vectors against fp64 from the same fp32 means, bounds formed like the descriptors'; guard bands around both outputs"""
    rng = np.random.Generator(np.random.PCG64(R * 1000 + C_))
    m32 = (rng.normal(size=(R, C_)) * 0.1 + rng.normal(size=(1, C_)) * 0.6).astype(np.float32)
    m = torch.from_numpy(m32).cuda()
    mu_want = so.centre(m32.astype(np.float64))
    mu_out, mu_check = guarded_out((C_,), torch.float32)
    mu = descriptor_centre(poisoned_in(m), mu_out)
    mu_check("centre")
    tol = so.tolerance(mu_want, so.centre_seq32(m32))
    err = float(np.abs(mu.cpu().numpy().astype(np.float64) - mu_want).max())
    print(f"centre ({R},{C_}): max |err| {err:.3e}, bound {tol:.3e}")
    assert err <= tol, (err, tol)
    # unit vectors from the centre the device formed (the fp64 side starts from the same fp32 numbers)
    mu32 = mu.cpu().numpy()
    e_want = so.unit(m32.astype(np.float64), mu32.astype(np.float64))
    e_out, e_check = guarded_out((R, C_), torch.float32)
    e = descriptor_unit(poisoned_in(m), mu.contiguous(), e_out)
    e_check("unit")
    tol = so.tolerance(e_want, so.unit_seq32(m32, mu32))
    err = float(np.abs(e.cpu().numpy().astype(np.float64) - e_want).max())
    print(f"unit ({R},{C_}): max |err| {err:.3e}, bound {tol:.3e}")
    assert err <= tol, (err, tol)
    if R == 1:  # the only row IS the centre
        assert bool((e == 0).all())


def test_a_row_equal_to_the_centre_gives_zeros():
    rng = np.random.Generator(np.random.PCG64(4))
    mu = torch.from_numpy(rng.normal(size=(384,)).astype(np.float32)).cuda()
    m = torch.from_numpy(rng.normal(size=(3, 384)).astype(np.float32)).cuda()
    m[1] = mu
    e = descriptor_unit(m, mu)
    assert bool((e[1] == 0).all()) and bool(torch.isfinite(e).all())
    assert abs(float(e[0].double().pow(2).sum()) - 1.0) < 1e-5


# ------------------------------------------------------------------------------------------------------------------- selection
def _units(B, R, C_, seed):
    """synthetic unit descriptors (fp32) and their fp64 similarities"""
    rng = np.random.Generator(np.random.PCG64(seed))
    q, e = rng.normal(size=(B, C_)), rng.normal(size=(R, C_))
    q32 = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    e32 = (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)
    return q32, e32, so.similarity(q32.astype(np.float64), e32.astype(np.float64))


def _exclusions(sim, R):
    """per query: its best entry, none, its third entry, ... (so that an exclusion changes the answer), as int32 (B)"""
    order = np.argsort(-sim, axis=1, kind="stable")
    ex = np.array([[order[b, 0], -1, order[b, min(2, R - 1)]][b % 3] for b in range(sim.shape[0])], dtype=np.int32)
    return ex


def separated(C_, B, R, N):
    """the case's inputs, after asserting on the oracle that an exact comparison is meaningful for them"""
    q32, e32, sim = _units(B, R, C_, SELECT_SEEDS[(C_, B, R, N)])
    assert min(so.top_gaps(sim, N)) >= MIN_GAP, so.top_gaps(sim, N)
    if R > 1:
        ex = _exclusions(sim, R)
        n_ex = min(N, R - 1)
        assert min(so.top_gaps(sim, n_ex, ex)) >= MIN_GAP, so.top_gaps(sim, n_ex, ex)
    return q32, e32, sim


@pytest.mark.parametrize("B,R,N", SELECT_SHAPES)
@pytest.mark.parametrize("C_", [128, 384])
def test_select_references(C_, B, R, N):
    q32, e32, sim = separated(C_, B, R, N)
    q, e = torch.from_numpy(q32).cuda(), torch.from_numpy(e32).cuda()
    idx_out, idx_check = guarded_out((B, N), torch.int32)
    sim_out, sim_check = guarded_out((B, R), torch.float32)
    index, got = select_references(poisoned_in(q), poisoned_in(e), N, None, idx_out, sim_out)
    idx_check("index")
    sim_check("similarities")
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - sim).max())
    print(f"select ({B},{R},{N}) C {C_}: max |sim err| {err:.3e}")
    assert err <= 1e-5, err
    assert np.array_equal(index.cpu().numpy(), so.select(sim, N))
    if R > 1:  # exclusions, N = R - 1 at the most
        ex = _exclusions(sim, R)
        n_ex = min(N, R - 1)
        index, _ = select_references(q, e, n_ex, torch.from_numpy(ex).cuda())
        want = so.select(sim, n_ex, ex)
        assert np.array_equal(index.cpu().numpy(), want)
        for b in range(B):
            assert ex[b] < 0 or ex[b] not in want[b]


def test_exact_duplicates_give_the_lower_index():
    q32, e32, _ = _units(3, 40, 384, 5)
    e32[31] = e32[4]    # a later copy of row 4
    e32[17] = e32[22]   # ... and an earlier copy of row 22
    q32[0], q32[1] = e32[4], e32[22]
    q, e = torch.from_numpy(q32).cuda(), torch.from_numpy(e32).cuda()
    index, sim = select_references(q, e, 5)
    index, sim = index.cpu().numpy(), sim.cpu().numpy()
    assert sim[0, 4].tobytes() == sim[0, 31].tobytes() and sim[1, 17].tobytes() == sim[1, 22].tobytes()  # the same instruction sequence per pair
    assert list(index[0, :2]) == [4, 31] and list(index[1, :2]) == [17, 22]
    one, _ = select_references(q, e, 1)
    assert list(one.cpu().numpy()[:2, 0]) == [4, 17]
    # excluding the lower of a pair leaves the higher one first
    ex = torch.tensor([4, 17, -1], dtype=torch.int32).cuda()
    index, _ = select_references(q, e, 2, ex)
    assert index[0, 0] == 31 and index[1, 0] == 22 and 4 not in index[0].tolist() and 17 not in index[1].tolist()
    # a bank of equal rows: ascending indices
    same = e[:1].repeat(9, 1).contiguous()
    index, _ = select_references(q, same, 9)
    assert index.cpu().tolist() == [list(range(9))] * 3


def test_select_arguments():
    q32, e32, _ = _units(2, 64, 128, 1)
    q, e = torch.from_numpy(q32).cuda(), torch.from_numpy(e32).cuda()
    ex = torch.tensor([-1, -1], dtype=torch.int32).cuda()
    with pytest.raises(ValueError):          # N beyond the bank
        select_references(q, e[:4].contiguous(), 5)
    with pytest.raises(ValueError):          # ... and beyond the eligible entries when any query may carry an exclusion
        select_references(q, e[:5].contiguous(), 5, ex)
    select_references(q, e[:5].contiguous(), 5)
    select_references(q, e[:5].contiguous(), 4, ex)
    with pytest.raises(NotImplementedError):
        select_references(q, e, 33)
    index, _ = select_references(q, e, 32)   # the handle-free path is usable afterwards
    torch.cuda.synchronize()
    assert int(index.min()) >= 0


# ------------------------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("R,Np,C_", DESC_SHAPES)
def test_gather_tokens(R, Np, C_, bf16):
    """bank[index] bit for bit, sizes that are no multiple of the 16-KiB piece a workgroup copies; indices -1 and R give zero slots"""
    bank, _ = _tokens(R, Np, C_, 50 + Np, bf16)
    rng = np.random.Generator(np.random.PCG64(Np))
    B, N = 2, 3
    index = rng.integers(0, R, size=(B, N)).astype(np.int32)
    index[0, 1], index[1, 2] = -1, R
    out, check = guarded_out((B, N, Np, C_), bank.dtype)
    flat = poisoned_in(bank.reshape(R * Np, C_)).reshape(R, Np, C_)
    got = gather_tokens(flat, torch.from_numpy(index).cuda(), out)
    check("gathered tokens")
    raw, braw = got.view(torch.int16).cpu(), bank.view(torch.int16).cpu()
    for b in range(B):
        for n in range(N):
            i = int(index[b, n])
            want = braw[i] if 0 <= i < R else torch.zeros_like(braw[0])
            assert torch.equal(raw[b, n], want), (b, n, i)
