"""The reference-use launch at the cfg-2 decoder shape (8 items x 8 heads x 1369 queries x 5 references of 1369 keys, dh 48) beside what it
stands next to, same box, alternating child processes, HIP events: the cross-attention launch that writes its lse (cs_op_attention), the
ref_use launch itself (cs_op_reference_use), and eight one-head attn_weights launches (cs_op_attention_weights) -- the only way to the same
information without it, 300 MB of fp32 each.  Also prints the launch's algorithmic floors: 57.6 GFLOP at the dense 16-bit MFMA peak, and K read
once per 64-row query block at the HBM rate.  Stops at the first child that ends with a non-zero status.
usage: refuse_time.py [timed launches per child, default 50] [children, default 4]"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, HEADS, LQ, N, NP, DH = 8, 8, 1369, 5, 1369, 48
child = r'''
import ctypes as C, sys, torch, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r + "/tests")
from crossscore_amd import _lib
import hip_helpers as hh
B, heads, Lq, N, Np, dh = %d, %d, %d, %d, %d, %d
iters = int(sys.argv[1])
g = np.random.default_rng(0)
Cc, Lk = heads * dh, N * Np
Q = hh.prescale_q(torch.from_numpy(1.5 * g.standard_normal((B, Lq, Cc), dtype=np.float32)).cuda().half(), dh)
KV = torch.from_numpy(g.standard_normal((B, Lk, 4 * Cc), dtype=np.float32)).cuda().half()  # the forward's kv buffer: K and V of two layers per row
K, V = KV[:, :, :Cc], KV[:, :, Cc:2 * Cc]
lse = torch.zeros((B, heads, Lq), device="cuda")
O = torch.zeros((B, Lq, Cc), dtype=torch.float16, device="cuda")
share = torch.empty((B, N, Lq), device="cuda"); peak = torch.empty_like(share); ent = torch.empty((B, Lq), device="cuda")
index = torch.empty((B, N, Lq), dtype=torch.int32, device="cuda")
W = torch.empty((B, Lq, Lk), device="cuda")
lib, p, st = _lib.load(), hh._p, hh._stream

def attn():
    hh.attention(Q, K, V, heads, dh, q_scale=1.0, O=O, L=lse)
def use():
    _lib.check(lib.cs_op_reference_use(p(Q), p(K), Q.stride(1), K.stride(1), Q.stride(0), K.stride(0), B, heads, Lq, N, Np, dh, 1.0, p(lse),
                                       p(share), p(peak), p(index), p(ent), st()))
def weights8():
    for hd in range(heads):
        hh.attention_weights(Q, K, heads, dh, lse, hd, q_scale=1.0, out=W)

res = []
for fn in (attn, use, weights8):
    for _ in range(3): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters): fn()
    b.record(); torch.cuda.synchronize()
    res.append(1e3 * a.elapsed_time(b) / iters)
assert abs(float(share.sum(1).mean()) - 1.0) < 5e-4
print(*res)
''' % (REPO, REPO, B, HEADS, LQ, N, NP, DH)


def main():
    iters = sys.argv[1] if len(sys.argv) > 1 else "50"
    children = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    rows = []
    for _ in range(children):
        r = subprocess.run([sys.executable, "-c", child, iters], capture_output=True, text=True)
        if r.returncode != 0:  # a child that failed may have faulted the GPU: nothing more is started on it
            print(r.stdout[-800:], r.stderr[-800:], sep="\n")
            sys.exit("refuse_time: a child ended with status %d; stopping" % r.returncode)
        rows.append([float(v) for v in r.stdout.strip().splitlines()[-1].split()])
    for k, name in enumerate(("cross-attention (cs_op_attention, lse written)", "ref_use (cs_op_reference_use)", "8 x attn_weights (one head each)")):
        print("%-48s %s us" % (name, " | ".join("%.1f" % row[k] for row in rows)))
    flop = 2.0 * B * HEADS * LQ * N * NP * DH
    k_bytes = B * ((LQ + 63) // 64) * N * NP * HEADS * DH * 2.0
    print("floors: %.1f GFLOP at 2.5 PFLOP/s = %.1f us; K once per 64-row query block = %.0f MB at 8 TB/s = %.1f us (an upper estimate: the blocks "
          "of an item share their K through the caches)" % (flop / 1e9, flop / 2.5e15 * 1e6, k_bytes / 1e6, k_bytes / 8e12 * 1e6))


if __name__ == "__main__":
    main()
