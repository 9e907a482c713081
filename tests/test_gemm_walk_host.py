"""Host-side proof of what tests/test_hip_gemm_walk.py relies on (no GPU): the operand data of tests/gemm_walk_data.py keeps every exact case
exact, and it separates tiles, K slices and epilogue steps: each way a persistent GEMM block can read the wrong thing between two tiles is applied
to the REFERENCE here and must change the expected output of the tile concerned."""
import numpy as np
import pytest

import gemm_walk_data as wd

_OPS = {}


def _ops(M, N, K):
    if (M, N, K) not in _OPS:
        d = wd.operands(M, N, K)
        d["y"] = wd.product(d["A"], d["W"], d["b"])
        d["S"] = np.abs(d["A"]).astype(np.float64) @ np.abs(d["W"]).astype(np.float64).T + np.abs(d["b"])
        _OPS[(M, N, K)] = d
    return _OPS[(M, N, K)]


def _assert_16bit(y, bf16):
    assert np.abs(y).max() <= (256 if bf16 else 2048), np.abs(y).max()
    assert (y == np.round(y)).all()


# ------------------------------------------------------------------------------------------------ the conditions, on every case of the GPU tests
def test_exact_cases_stay_exact():
    """16-bit outputs: integers within +-2048 (fp16) / +-256 (bf16); every fp32 sum, in any order, below 2^24; operands exact in both types"""
    for M, N, K, epi in wd.HALF128:
        _assert_16bit(_ops(M, N, K)["y"], False)
    for what in ("bias", "relu"):
        _assert_16bit(_ops(*wd.BF16_128[what])["y"], True)
    for M, N, K, epi in wd.G256:
        d = _ops(M, N, K)
        if epi in ("bias", "gelu"):
            _assert_16bit(d["y"], True)  # run in fp16 and bf16
        assert (d["S"] + 64).max() < 2 ** 24
    for M, N, K, _ in wd.RESID128:
        d = _ops(M, N, K)
        assert (d["S"] + 64).max() < 2 ** 24 and np.abs(d["r"]).max() <= 64
    for M, Cc, K in wd.RESID_LN128 + [wd.BF16_128["resid-ln"]]:
        d = _ops(M, Cc, K)
        assert (d["S"] + 64).max() < 2 ** 24
        assert np.abs(d["y"] + d["r"]).max() <= 256  # the 16-bit copy of x holds it exactly in fp16 and bf16
    for pc in wd.PATCH128:
        d = _ops(pc["I"] * pc["Np"], pc["Cc"], pc["K"])
        pos = wd.pos_rows(pc["Np"], pc["Cc"])
        assert (d["S"] + 32).max() < 2 ** 24 and np.abs(pos).max() <= 32 and np.abs(d["y"]).max() + 32 <= 256
    for d in _OPS.values():
        assert np.abs(d["A"]).max() <= 2 and np.abs(d["W"]).max() <= 1 and np.abs(d["b"]).max() <= 8


def test_layernorm_rows_are_exact_and_their_statistics_differ():
    for BM, cases in ((128, wd.LN128), (256, wd.LN256)):
        for M, Cc, N, _ in cases:
            x = wd.ln_rows(M, Cc, BM)
            Wp, s, c = wd.ln_weights(N, Cc)
            assert np.abs(x).max() <= 18 and (x == np.round(x)).all()              # exact in fp16 and bf16 (8 significant bits hold 18)
            assert (Wp * 64 == np.round(Wp * 64)).all() and np.abs(Wp).max() <= 1 / 16
            assert (s.astype(np.float64) == Wp.astype(np.float64).sum(1)).all()     # s is exact in fp32
            part = wd.row_partials128(x, wd.bn128(Cc, "wide")) if BM == 128 else None
            if part is not None:
                assert (part.astype(np.float32) == part).all() and part.max() < 2 ** 24
            mu = x.astype(np.float64).mean(1)
            pm = np.array([mu[p * BM:(p + 1) * BM].mean() for p in range(-(-M // BM))])
            # consecutive panels of one XCD (8 apart) and neighbours differ by whole units of the mean
            for gap in (1, 8):
                if len(pm) > gap:
                    assert np.abs(pm[gap:] - pm[:-gap]).min() > 2.0, (M, Cc, gap)


def _groups():
    g = {}
    for M, N, K, e in wd.HALF128:
        g.setdefault(e, []).append((M, N, wd.bn128(N)))
    for M, N, K, mode in wd.RESID128:
        g.setdefault("resid" + ("-pipe" if K >= 320 and mode != "none" else ""), []).append((M, N, wd.bn128(N)))
    for M, Cc, K in wd.RESID_LN128:
        g.setdefault("resid-ln", []).append((M, Cc, wd.bn128(Cc, "wide")))
    for M, Cc, N, e in wd.LN128:
        g.setdefault(e, []).append((M, N, wd.bn128(N, "wide")))
    g["patch"] = [(pc["I"] * pc["Np"], pc["Cc"], wd.bn128(pc["Cc"], "wide")) for pc in wd.PATCH128]
    h = wd.HEAD128
    g["head"] = [(h["B"] * h["gh"] * h["gw"], 196, 128)]
    return g


def test_every_epilogue_meets_both_hand_over_orders_and_both_flush_arms():
    for name, shapes in _groups().items():
        seen, last = set(), set()
        for M, N, BN in shapes:
            for blocks in (8, 16):
                s, l = wd.orders(M, N, 128, BN, blocks)
                seen |= s
                last |= l
        assert {"full>ragged", "ragged>full"} <= seen, (name, seen)
        assert {"last-full", "last-ragged"} <= last, (name, last)


def test_the_walks_contain_idle_blocks_uneven_xcds_and_both_bias_paths():
    w = wd.walk(300, 136, 128, 128, 8)
    assert sorted(b for b, t in w.items() if not t) == [3, 4, 5, 6, 7]                 # five of eight blocks own nothing
    w = wd.walk(2176, 136, 128, 128, 8)
    assert [len(w[b]) for b in range(8)] == [6] + [4] * 7                               # XCD 0 owns 3 panels, the others 2
    w = wd.walk(1147, 136, 128, 128, 8)
    assert w[0] == [(0, 0), (0, 128), (1024, 0), (1024, 128)]                          # a full panel, then a ragged one
    w = wd.walk(1147, 384, 128, 128, 16)                                                # N <= 1536: blocks with 2+ tiles keep the bias in LDS,
    assert {len(t) for t in w.values()} >= {1, 2, 3}                                    # single-tile blocks of the same launch read it from memory
    assert wd.grid_of(300, 136, 128, 128, 16) == 16 and wd.grid_of(300, 128, 128, 128, 16) == 8 and wd.grid_of(128, 128, 128, 128, 0) == 8
    # every tile exactly once, whatever the grid
    for M, N, BM, BN in ((1147, 136, 128, 128), (2176, 576, 128, 192), (2301, 512, 256, 256), (300, 1664, 128, 128)):
        want = sorted((m, n) for m in range(0, M, BM) for n in range(0, N, BN))
        for blocks in (8, 16, 24, 512):
            assert sorted(t for ts in wd.walk(M, N, BM, BN, blocks).values() for t in ts) == want


# ------------------------------------------------------------------------------------------------ the mutations, at the smallest walk shapes
M0, N0, K0, BM, BN = 1147, 136, 320, 128, 128


def _changed(a, b, tile, M, N, BN_=BN, rows=None):
    rs, cs = wd.region(tile, M, N, BM, BN_)
    if rows is not None:
        rs = slice(rs.start + rows.start, min(rs.start + rows.stop, rs.stop))
    return int((a[rs, cs] != b[rs, cs]).sum()), (rs.stop - rs.start) * (cs.stop - cs.start)


@pytest.mark.parametrize("M,N", [(M0, N0), (2176, 136), (1147, 384)])
def test_a_rows_of_another_panel_change_every_tile_of_the_panel(M, N):
    d = _ops(M, N, K0)
    panels = -(-M // BM)
    pairs = {(p, q) for p in range(panels) for q in range(panels) if p != q and (abs(p - q) == 1 or (p - q) % 8 == 0)}
    assert (0, 8) in pairs and (8, 0) in pairs
    for p, q in sorted(pairs):
        A = d["A"].copy()
        rows = np.arange(p * BM, min((p + 1) * BM, M))
        A[rows] = d["A"][np.minimum(rows - p * BM + q * BM, M - 1)]
        y = wd.product(A, d["W"], d["b"])
        for n0 in range(0, N, wd.bn128(N)):
            n, size = _changed(y, d["y"], (p * BM, n0), M, N, wd.bn128(N))
            assert n > size // 2, (p, q, n0, n, size)


@pytest.mark.parametrize("N", [136, 384, 576])
def test_w_rows_and_bias_of_another_column_tile_change_the_tile(N):
    d = _ops(M0, N, K0)
    bn = wd.bn128(N)
    tiles = -(-N // bn)
    for t in range(tiles):
        for u in range(tiles):
            if t == u:
                continue
            cols = np.arange(t * bn, min((t + 1) * bn, N))
            src = np.minimum(cols - t * bn + u * bn, N - 1)
            for what in ("W", "b"):
                W, b = d["W"].copy(), d["b"].copy()
                if what == "W":
                    W[cols] = d["W"][src]
                else:
                    b[cols] = d["b"][src]
                y = wd.product(d["A"], W, b)
                for m0 in (0, 1024):
                    n, size = _changed(y, d["y"], (m0, t * bn), M0, N, bn)
                    assert n > size // 2, (what, t, u, m0, n, size)


def test_col_s_and_c_of_another_column_tile_change_the_tile():
    M, Cc, N = 1147, 128, 200
    x = wd.ln_rows(M, Cc, BM)
    Wp, s, c = wd.ln_weights(N, Cc)
    mu, rstd = wd.ln_stats(wd.row_partials128(x, 128), Cc, 1e-6)
    ref = wd.ln_folded(x, Wp, s, c, mu, rstd)
    for t, u in ((0, 1), (1, 0)):
        cols = np.arange(t * 128, min((t + 1) * 128, N))
        src = np.minimum(cols - t * 128 + u * 128, N - 1)
        for what in ("s", "c"):
            s2, c2 = s.copy(), c.copy()
            (s2 if what == "s" else c2)[cols] = (s if what == "s" else c)[src]
            y = wd.ln_folded(x, Wp, s2, c2, mu, rstd)
            n, size = _changed(y, ref, (0, t * 128), M, N)
            assert n > size // 2 and np.abs(y - ref).max() > 0.2, (what, t, u, n, size)


@pytest.mark.parametrize("K", [64, 256, 320])
def test_a_k_slice_from_the_same_ring_slot_or_the_one_before_changes_the_tile(K):
    """slice kt of a tile replaced by the slice 3 (the same slot of the 3-slot ring) or 1 before it in the block's slice stream, which runs on
    through the previous tile: the first, a middle and the last slice of every tile a block of the 8-block walk computes after its first"""
    d = _ops(M0, N0, K)
    nk = K // 32
    for b, tiles in wd.walk(M0, N0, BM, BN, 8).items():
        for pos in range(1, len(tiles)):
            rs, cs = wd.region(tiles[pos], M0, N0, BM, BN)
            for kt in sorted({0, nk // 2, nk - 1}):
                for back in (1, 3):
                    if pos * nk + kt - back < 0:  # (K = 64: the stream is only two slices old at the second tile's first slice)
                        continue
                    y = wd.tile_product_with_slice_from(d["A"], d["W"], d["b"], tiles, pos, kt, back, BM, BN)
                    n = int((y != d["y"][rs, cs]).sum())
                    assert n > y.size // 2, (b, pos, kt, back, n, y.size)


def test_residual_position_rows_and_row_statistics_of_the_previous_tile_change_the_tile():
    d = _ops(M0, N0, K0)
    full = d["y"] + d["r"]
    Np = 63
    pos = wd.pos_rows(Np, N0)
    m = np.arange(M0 // Np * Np)
    patch = d["y"][m] + pos[m % Np + 1]
    x = wd.ln_rows(M0, 128, BM)
    Wp, s, c = wd.ln_weights(N0, 128)
    mu, rstd = wd.ln_stats(wd.row_partials128(x, 128), 128, 1e-6)
    ln = wd.ln_folded(x, Wp, s, c, mu, rstd)
    for blocks in (8, 16):
        for tiles in wd.walk(M0, N0, BM, BN, blocks).values():
            for prev, cur in zip(tiles, tiles[1:]):
                dr, dc, sr, sc = wd.take_from(cur, prev, M0, N0, BM, BN)
                r = d["r"].copy()
                r[np.ix_(dr, dc)] = d["r"][np.ix_(sr, sc)]
                n, size = _changed(d["y"] + r, full, cur, M0, N0)
                assert n > size // 2, ("resid", prev, cur, n, size)
                # the position row of patch row m is pos[m % Np + 1]: the previous tile's rows are other patches of other images
                keep = dr < len(m)
                pm = d["y"][dr[keep]][:, dc] + pos[sr[keep] % Np + 1][:, sc]
                n = int((pm != patch[dr[keep]][:, dc]).sum())
                assert n > pm.size // 2, ("pos", prev, cur, n, pm.size)
                if prev[0] != cur[0]:  # (within a panel the rows, hence their statistics, are the same: the stash differs in s and c, above)
                    mu2, rs2 = mu.copy(), rstd.copy()
                    mu2[dr], rs2[dr] = mu[sr], rstd[sr]
                    y = wd.ln_folded(x, Wp, s, c, mu2, rs2)
                    n, size = _changed(y, ln, cur, M0, N0)
                    assert n > size // 2 and np.abs(y - ln).max() > 0.5, ("ln stats", prev, cur, n, size)


def test_an_epilogue_step_of_the_previous_tile_changes_the_step():
    """one 16-row step of a tile replaced by the same step of the tile the block computed before it (a stale register set or patch)"""
    d = _ops(M0, N0, K0)
    for blocks in (8, 16):
        for tiles in wd.walk(M0, N0, BM, BN, blocks).values():
            for prev, cur in zip(tiles, tiles[1:]):
                for step in range(8):
                    rows = slice(16 * step, 16 * step + 16)
                    dr, dc, sr, sc = wd.take_from(cur, prev, M0, N0, BM, BN, rows=rows)
                    if not len(dr):
                        continue
                    y = d["y"].copy()
                    y[np.ix_(dr, dc)] = d["y"][np.ix_(sr, sc)]
                    n, size = _changed(y, d["y"], cur, M0, N0, rows=rows)
                    assert n > size // 2, (prev, cur, step, n, size)
