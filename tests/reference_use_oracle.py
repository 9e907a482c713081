"""fp64 numpy restatement of the reference-use outputs, for the tests of csrc/refuse.hip and of need_reference_use.

Keys are N segments of Np rows: key k = n * Np + j is patch j of reference n.  With the base-2 logits s[b, hd, q, k] = q . k of head hd (Q
already carries log2(e) / sqrt(dh)) and lse[b, hd, q]:
    e = s - lse,  p = 2^e,  pm[b, q, k] = mean over the heads of p
    share[b, n, q]      = sum_j pm[b, q, n Np + j]
    peak_prob[b, n, q]  = max_j pm[b, q, n Np + j],  peak_index its j, the lowest on equal values
    entropy[b, q]       = mean over the heads of sum_k -p e        (bits)
lse is taken as given (the attention kernel's), nothing is renormalised.

The keyword switches restate four mistakes a tiled kernel can make; the host tests show that each one moves most of the values it concerns, so
the GPU tests, which compare with the switch-free oracle, would see it:
    count_padded     the zero-filled keys of each reference's ragged last 64-key tile (s = 0, p = 2^-lse) are counted into its share / peak
    tail_to_next     the last key of reference n is credited to reference n + 1 (a tile that straddles two references)
    max_before_mean  the peak is taken per head and the head mean after it
    ties_high        equal values keep the highest index"""
import numpy as np

TILE = 64


def logits(Q, K, heads, dh):
    """Q (B, Lq, >= heads dh), K (B, Lk, >= heads dh): the operands' values -> s (B, heads, Lq, Lk) fp64"""
    Q = np.asarray(Q, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64)
    B, Lq, Lk = Q.shape[0], Q.shape[1], K.shape[1]
    q = Q[:, :, :heads * dh].reshape(B, Lq, heads, dh)
    k = K[:, :, :heads * dh].reshape(B, Lk, heads, dh)
    return np.einsum("bqhd,bkhd->bhqk", q, k)


def lse_of(s):
    """the exact base-2 log-sum-exp of s over its last axis"""
    m = s.max(axis=-1, keepdims=True)
    return (m + np.log2(np.exp2(s - m).sum(axis=-1, keepdims=True)))[..., 0]


def head_mean_probs(s, lse):
    """-> (p (B, heads, Lq, Lk), e, pm (B, Lq, Lk))"""
    e = s - np.asarray(lse, dtype=np.float64)[..., None]
    p = np.exp2(e)
    return p, e, p.mean(axis=1)


def _argmax(v, ties_high):
    """argmax over the last axis: the lowest index on equal values, or the highest"""
    if not ties_high:
        return v.argmax(axis=-1)
    return v.shape[-1] - 1 - v[..., ::-1].argmax(axis=-1)


def reference_use(s, lse, N, Np, count_padded=False, tail_to_next=False, max_before_mean=False, ties_high=False):
    """s (B, heads, Lq, N Np) fp64 logits, lse (B, heads, Lq) -> dict of share, peak_prob (B, N, Lq) fp64, peak_index (B, N, Lq) int64,
    entropy (B, Lq) fp64 and pm (B, Lq, N, Np), the head-mean probabilities the peak rules are stated on"""
    s = np.asarray(s, dtype=np.float64)
    B, heads, Lq, Lk = s.shape
    assert Lk == N * Np, (Lk, N, Np)
    p, e, pm = head_mean_probs(s, lse)
    entropy = (-(p * e)).sum(axis=-1).mean(axis=1)
    seg = pm.reshape(B, Lq, N, Np).copy()
    per_head = p.reshape(B, heads, Lq, N, Np)
    pad = (-Np) % TILE
    if count_padded and pad:
        ppad = np.exp2(-np.asarray(lse, dtype=np.float64))  # s = 0
        per_head = np.concatenate([per_head, np.broadcast_to(ppad[..., None, None], (B, heads, Lq, N, pad))], axis=-1)
        seg = per_head.mean(axis=1)
    if tail_to_next and N > 1:
        seg = seg.copy()
        last = seg[:, :, :-1, Np - 1].copy()
        seg[:, :, :-1, Np - 1] = 0.0
        seg[:, :, 1:, 0] += last  # (counted with the next reference's first key)
        per_head = None
    share = seg.sum(axis=-1)
    if max_before_mean:
        assert per_head is not None
        peak_prob = per_head.max(axis=-1).mean(axis=1)
        peak_index = _argmax(per_head.mean(axis=1), ties_high)
    else:
        peak_prob = seg.max(axis=-1)
        peak_index = _argmax(seg, ties_high)
    tr = (0, 2, 1)
    return {"share": share.transpose(tr), "peak_prob": peak_prob.transpose(tr), "peak_index": peak_index.transpose(tr).astype(np.int64),
            "entropy": entropy, "pm": pm.reshape(B, Lq, N, Np)}


# ---- the bounds of the GPU tests (the issue's caps, from the project's own lse bound of 5e-4: 2^(5e-4) - 1 = 3.5e-4) ----
REL = 5e-4


def check_values(got, want, what=""):
    """share / peak_prob within 5e-4 relative + 1e-6, sum over the references within 5e-4 of 1, entropy within 5e-4 (1 + entropy) + 1e-5.
    Returns the measured maxima (in units of each cap) for the record."""
    out = {}
    for k in ("share", "peak_prob"):
        if got.get(k) is None:
            continue
        d = np.abs(np.asarray(got[k], dtype=np.float64) - want[k])
        cap = REL * want[k] + 1e-6
        out[k] = float((d / cap).max())
        assert (d <= cap).all(), f"{what} {k}: {float((d / cap).max()):.3f} x the cap at {np.unravel_index((d / cap).argmax(), d.shape)}"
    if got.get("share") is not None:
        tot = np.asarray(got["share"], dtype=np.float64).sum(axis=1)
        out["sum"] = float(np.abs(tot - 1.0).max())
        assert out["sum"] <= REL, f"{what} sum of shares off 1 by {out['sum']:.3e}"
    if got.get("entropy") is not None:
        d = np.abs(np.asarray(got["entropy"], dtype=np.float64) - want["entropy"])
        cap = REL * (1.0 + want["entropy"]) + 1e-5
        out["entropy"] = float((d / cap).max())
        assert (d <= cap).all(), f"{what} entropy: {float((d / cap).max()):.3f} x the cap"
    return out


MARGIN = 2e-3


MAX_INSIDE = 0.03


def check_peak_index(index, want, Np, what=""):
    """The margin rule: the oracle's pm at the kernel's index is at least (1 - 2e-3) of the oracle's maximum; the index equals the oracle's
    wherever the oracle's best exceeds its second best by more than 2e-3 relative.  Returns (cases inside that margin, cases): the caller sums
    them over its shapes and asserts that at most MAX_INSIDE of the cases lie inside, so that the equality test cannot go empty."""
    index = np.asarray(index).astype(np.int64)
    pm = want["pm"].transpose(0, 2, 1, 3)  # (B, N, Lq, Np)
    assert index.shape == pm.shape[:3], (index.shape, pm.shape)
    assert ((index >= 0) & (index < Np)).all(), f"{what} peak_index outside [0, {Np})"
    at = np.take_along_axis(pm, index[..., None], axis=-1)[..., 0]
    best = pm.max(axis=-1)
    assert (at >= (1.0 - MARGIN) * best).all(), f"{what} peak_index names a key below (1 - 2e-3) of the maximum"
    if Np > 1:
        second = np.sort(pm, axis=-1)[..., -2]
        clear = best - second > MARGIN * best
    else:
        clear = np.ones_like(best, dtype=bool)
    assert (index[clear] == want["peak_index"][clear]).all(), f"{what} peak_index differs from the oracle's outside the margin"
    return int(clear.size - clear.sum()), int(clear.size)
