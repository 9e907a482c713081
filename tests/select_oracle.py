"""Oracle of the reference selection by similarity (tests only): the five steps in numpy fp64 from the same 16-bit tokens,
and an fp32 SEQUENTIAL restatement of each arithmetic step that is used only to size tolerances (tolerance below): how far plain fp32 arithmetic
in the simplest order lands from fp64 on the very input of a test case.  Nothing here looks at what a kernel returns."""
import numpy as np


def widen(tokens, bf16=False):
    """16-bit tokens as fp64, exactly: numpy float16 arrays as they are; bfloat16 given as its raw uint16 bits"""
    t = np.asarray(tokens)
    if bf16:
        return (t.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    assert t.dtype == np.float16, t.dtype
    return t.astype(np.float64)


# ---- the definition, fp64 ----
def mean(t64):
    """(I, Np, C) -> (I, C): step 1"""
    return t64.sum(axis=1) / t64.shape[1]


def centre(m64):
    """(R, C) -> (C): step 2"""
    return m64.sum(axis=0) / m64.shape[0]


def unit(m64, mu64):
    """(I, C), (C) -> (I, C): step 3"""
    d = m64 - mu64
    return d / np.maximum(np.sqrt((d * d).sum(axis=1, keepdims=True)), 1e-12)


def similarity(eq64, er64):
    """(B, C), (R, C) -> (B, R): step 4"""
    return eq64 @ er64.T


def select(sim, N, exclude=None):
    """(B, R) similarities -> (B, N) indices: step 5.  Descending similarity, ties to the lower index, exclude[b] >= 0 left out."""
    B, R = sim.shape
    out = np.full((B, N), -1, dtype=np.int32)
    for b in range(B):
        cand = [r for r in range(R) if exclude is None or int(exclude[b]) != r]
        cand.sort(key=lambda r: (-sim[b, r], r))
        out[b, :min(N, len(cand))] = cand[:N]
    return out


def descriptors(bank_tokens64):
    """bank tokens (R, Np, C) fp64 -> (mean, centre, unit)"""
    m = mean(bank_tokens64)
    mu = centre(m)
    return m, mu, unit(m, mu)


def choose(query_tokens64, bank_tokens64, N, exclude=None):
    """the whole definition: (indices (B, N), similarities (B, R))"""
    _, mu, e = descriptors(bank_tokens64)
    s = similarity(unit(mean(query_tokens64), mu), e)
    return select(s, N, exclude), s


def top_gaps(sim, N, exclude=None):
    """per query the smallest difference between consecutive similarities among its first min(N + 1, candidates) entries in selection order
    (inf when there is a single one): a selection is comparable exactly, order included, only where this is well above the arithmetic's error"""
    B, R = sim.shape
    gaps = []
    for b in range(B):
        s = np.sort(np.array([sim[b, r] for r in range(R) if exclude is None or int(exclude[b]) != r]))[::-1][:N + 1]
        gaps.append(float(np.min(s[:-1] - s[1:])) if len(s) > 1 else float("inf"))
    return gaps


# ---- fp32, sequential: one accumulator, ascending index, one rounding per operation ----
def mean_seq32(t64):
    t = t64.astype(np.float32)  # exact: the values are 16-bit
    acc = np.zeros((t.shape[0], t.shape[2]), dtype=np.float32)
    for p in range(t.shape[1]):
        acc = acc + t[:, p]
    return acc / np.float32(t.shape[1])


def centre_seq32(m32):
    acc = np.zeros((m32.shape[1],), dtype=np.float32)
    for r in range(m32.shape[0]):
        acc = acc + m32[r]
    return acc / np.float32(m32.shape[0])


def unit_seq32(m32, mu32):
    d = (m32 - mu32).astype(np.float32)
    ss = np.zeros((d.shape[0],), dtype=np.float32)
    for c in range(d.shape[1]):
        ss = ss + d[:, c] * d[:, c]
    return d / np.maximum(np.sqrt(ss), np.float32(1e-12))[:, None]


def tolerance(ref64, seq32, floor_rel=1e-7):
    """The bound of a case: 4 x the largest deviation of the fp32-sequential restatement from fp64 on this input, and at least floor_rel of the
    largest reference magnitude (a case the restatement happens to hit exactly still allows the last bit of an fp32 result)."""
    dev = float(np.max(np.abs(seq32.astype(np.float64) - ref64))) if ref64.size else 0.0
    return max(4.0 * dev, floor_rel * float(np.max(np.abs(ref64))) if ref64.size else 0.0)
