"""A/B of two library builds on the token-panel kernel alone, same box, alternating subprocesses: the cfg-2 encoder launch (48 images x 1370
rows, out-projection + MLP + next norm1), random operands, HIP events.  Each child packs its own weight image (the layout belongs to the build).
Stops at the first child that ends with a non-zero status.  usage: panel_ab_libs.py <libA.so> <libB.so> [timed launches per child, default 200]"""
import os, subprocess, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
child = r'''
import sys, torch
sys.path.insert(0, %r); sys.path.insert(0, %r + "/tests")
from crossscore_amd import _lib
_lib.LIB_PATH = sys.argv[1]
import hip_helpers as hh
from panel_data import make, reference
N = int(sys.argv[2])
dev = torch.device("cuda:0")
M = 48 * 1370
x, o, w = make(M, 1, dev)
img = hh.panel_pack(w["wo"], w["ls1"], w["w1"], w["g2"], w["w2"], w["ls2"])
xk = x.clone()
hh.encoder_panel(xk, o, img, w["bo"], w["b1"], w["b2"])
ref, _ = reference(x[:512], o[:512], w, True, emulate=True)
err = (xk[:512] - ref).abs().max().item()
assert err < 4e-3, err
for _ in range(5): hh.encoder_panel(x, o, img, w["bo"], w["b1"], w["b2"])
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
a.record()
for _ in range(N): hh.encoder_panel(x, o, img, w["bo"], w["b1"], w["b2"])
b.record(); torch.cuda.synchronize()
print(1e3 * a.elapsed_time(b) / N)
''' % (REPO, REPO)
libs = sys.argv[1:3]
iters = sys.argv[3] if len(sys.argv) > 3 else "200"
out = {l: [] for l in libs}
for rep in range(4):
    for l in libs:
        r = subprocess.run([sys.executable, "-c", child, l, iters], capture_output=True, text=True)
        if r.returncode != 0:  # a child that failed may have faulted the GPU: nothing more is started on it
            print(r.stdout[-800:], r.stderr[-800:], sep="\n")
            sys.exit("panel_ab_libs: child for %s ended with status %d; stopping" % (l, r.returncode))
        out[l].append(float(r.stdout.strip().splitlines()[-1]))
flop = 4.0 * 48 * 1370 * 384 * 1536 + 2.0 * 48 * 1370 * 384 * 384
for l in libs:
    print(l, " | ".join("%.1f us" % v for v in out[l]), "  (%.0f-%.0f TFLOP/s)" % (flop / max(out[l]) / 1e6, flop / min(out[l]) / 1e6))
