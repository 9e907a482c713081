"""A/B of two builds of the library on the whole forward, same box: are the outputs bit-identical, and is the speed where it was?

usage: forward_split_ab.py <parent.so> <new.so> [--no-timing] [--steps K]

1. Outputs.  One fresh child process per library runs every case of tests/golden/make_forward_census.py with the debug taps on and saves the score
   maps, per-image means, attention-weight maps, encoded reference tokens and every tap; this process compares the two sets with exact array equality.
2. Speed.  Alternating children (parent, new, parent, new) time the cfg-2 and cfg-4 workloads the way bench.py runs them (its Workload, its
   pipeline, its timed_steps): query-images/s and the host's enqueue time per forward.  The two parent runs against each other are the noise.

Every child runs under its own time limit and the script stops at the first one that ends with a non-zero status (it may have faulted the GPU:
nothing more is started on it).  Written for the split of csrc/api.hip into api.hip / forward.hip / ops.hip (profiles/forward_split_ab.txt).
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRELUDE = r'''
import importlib.util, json, os, statistics, sys
sys.path.insert(0, %r)
from crossscore_amd import _lib
_lib.LIB_PATH = sys.argv[1]
''' % REPO

DUMP = PRELUDE + r'''
import numpy as np
spec = importlib.util.spec_from_file_location("mfc", os.path.join(%r, "tests", "golden", "make_forward_census.py"))
mfc = importlib.util.module_from_spec(spec); spec.loader.exec_module(mfc)
for name in mfc.CASES:
    record, arrays = mfc.run_case(name, capture=True)
    np.savez(os.path.join(sys.argv[2], name + ".npz"), **arrays)
    print(name, len(arrays), "arrays", flush=True)
''' % REPO

TIME = PRELUDE + r'''
import torch, bench
name, steps = sys.argv[2], int(sys.argv[3])
dev = torch.device("cuda", 0); torch.cuda.set_device(dev)
sync = lambda: torch.cuda.synchronize(dev)
wl = bench.Workload(name, 0, dev).start_pipeline()
elapsed, ticket = bench.timed_steps(wl.step, sync, steps, 3, dev)
wl.pipe.result(ticket)
host = []
for _ in range(steps):  # host time of the enqueueing call, forward by forward (cs_forward_stats of the replica that ran it)
    wl.pipe.result(wl.step()); sync()
    host.append(wl.pipe.last_replica().forward_stats()["host_enqueue_ms"])
print(json.dumps({"workload": name, "q_per_s": wl.B * steps / elapsed, "ms_per_step": 1e3 * elapsed / steps,
                  "host_enqueue_ms_per_forward_median": statistics.median(host), "host_enqueue_ms_per_forward_min": min(host)}))
'''


def child(code, args, limit):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", code] + args, capture_output=True, text=True, cwd=REPO)
    if r.returncode != 0:
        print(r.stdout[-1500:], r.stderr[-1500:], sep="\n")
        sys.exit("forward_split_ab: the child for %s ended with status %d; stopping" % (args[0], r.returncode))
    return r.stdout


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("parent"); ap.add_argument("new")
    ap.add_argument("--no-timing", action="store_true"); ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    parent, new, steps = os.path.abspath(args.parent), os.path.abspath(args.new), args.steps
    print("parent:", parent, "\nnew:   ", new)
    with tempfile.TemporaryDirectory() as tmp:
        dirs = {}
        for tag, lib in (("parent", parent), ("new", new)):
            dirs[tag] = os.path.join(tmp, tag)
            os.makedirs(dirs[tag])
            child(DUMP, [lib, dirs[tag]], 300)
        bad = total = 0
        for f in sorted(os.listdir(dirs["parent"])):
            a, b = np.load(os.path.join(dirs["parent"], f)), np.load(os.path.join(dirs["new"], f))
            differ = [k for k in a.files if k not in b.files or a[k].shape != b[k].shape or not np.array_equal(a[k], b[k], equal_nan=True)]
            differ += [k for k in b.files if k not in a.files]
            total += len(a.files)
            bad += len(differ)
            print("%-26s %3d arrays  %s" % (f[:-4], len(a.files), "all equal" if not differ else "DIFFER: " + ", ".join(differ)))
        print("outputs: %d arrays in %d cases, %d differ" % (total, len(os.listdir(dirs["parent"])), bad))
    if not args.no_timing:
        import json
        for wl in ("cfg2", "cfg4"):
            for rep in range(2):
                for tag, lib in (("parent", parent), ("new", new)):
                    r = json.loads(child(TIME, [lib, wl, str(steps)], 280).strip().splitlines()[-1])
                    print("%s %-6s run %d: %8.1f query-images/s  %7.3f ms/step  host enqueue per forward %.3f ms median, %.3f ms min"
                          % (wl, tag, rep + 1, r["q_per_s"], r["ms_per_step"], r["host_enqueue_ms_per_forward_median"], r["host_enqueue_ms_per_forward_min"]))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
