"""Reference selection on the device against what it replaces, at cfg-2: ViT-S, 518 x 518, B = 8 queries, N = 5 views, a bank of
R = 64 and 1024 references.  Per R, wall time per batch (host clock around `steps` forwards that end in a device synchronise), the three forms
alternating inside every round, the median over the rounds:

  select   forward_select: descriptors, similarities, top-N and gather between encoder and decoder
  stack    the parent's cached path: torch.stack of the N token tensors per query on the host's say-so (ReferenceTokenCache.gather), forward_cached
  cached   forward_cached on tokens gathered beforehand (neither a choice nor a gather: the floor the two above add to)
  grouped1 forward_select(group=...) on the same bank as ONE group over all rows, blank_row -1 (the test phase's form: per-query slices, the
           triples uploaded with the call); the same bits as select
  grouped16 (banks of at least 16 x N rows) the bank as 16 equal groups, query b in group b % 16: similarities and top-N over R / 16 rows

and the bank build per reference: encode_references in chunks of 32 alone, and with the copy into the contiguous bank and the descriptors behind it.
Needs the GPU; prints what it measured (--out FILE: also written there)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from crossscore_amd import synth  # noqa: E402
from crossscore_amd.config import model_config  # noqa: E402
from crossscore_amd.model import CrossScoreNet, SelectionBank  # noqa: E402

B, N, H, W, CHUNK = 8, 5, 518, 518, 32


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--banks", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("select_ab.py measures on the GPU; there is none here")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    net = CrossScoreNet(model_config())
    net.load_numpy_state_dict(synth.make_state_dict(net.arch, 1))
    net = net.cuda()
    q = torch.from_numpy(synth.make_inputs(B, 1, H, W, 1)[0]).cuda()
    gen = torch.Generator(device="cuda").manual_seed(5)
    say(f"cfg-2: {net.arch.name}, {H} x {W}, B = {B}, N = {N}; {args.rounds} rounds x {args.steps} steps per form, forms alternating, median of the rounds")
    for R in args.banks:
        imgs = [torch.randn((min(CHUNK, R - r0), 3, H, W), generator=gen, device="cuda") for r0 in range(0, R, CHUNK)]
        tokens = None

        def encode_only():
            for x in imgs:
                net.encode_references(x)

        def build():
            nonlocal tokens
            r0 = 0
            for x in imgs:
                t = net.encode_references(x)
                if tokens is None:
                    tokens = torch.empty((R,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
                tokens[r0:r0 + len(t)] = t
                r0 += len(t)
            return net.reference_descriptors(tokens)

        build()  # warm: workspace, tables, the bank tensor
        enc = statistics.median(timed(encode_only, 1) for _ in range(3))
        full = statistics.median(timed(build, 1) for _ in range(3))
        desc = statistics.median(timed(lambda: net.reference_descriptors(tokens), 5) for _ in range(3))
        bank = SelectionBank(tokens, *build(), N)
        say(f"R = {R}: bank build {full / R * 1e6:.1f} us per reference (encode_references alone {enc / R * 1e6:.1f} us; the descriptors of the whole bank "
            f"{desc * 1e6:.1f} us = {desc / R * 1e6:.2f} us per reference)")
        first = net.forward_select(q, bank, None, False, 0, True)
        index = first["reference_index"].cpu().tolist()
        pre = tokens[first["reference_index"].long()]

        def stack():
            tok = torch.stack([torch.stack([tokens[i] for i in row]) for row in index])
            return net.forward_cached(q, tok, False, 0, True)

        whole = np.array([0, R], dtype=np.int32)
        bank1 = SelectionBank(tokens, *net.reference_descriptors(tokens, whole), N, whole, -1)
        zeros = np.zeros(B, dtype=np.int32)
        forms = {"select": lambda: net.forward_select(q, bank, None, False, 0, True), "stack": stack,
                 "cached": lambda: net.forward_cached(q, pre, False, 0, True),
                 "grouped1": lambda: net.forward_select(q, bank1, None, False, 0, True, group=zeros)}
        for k, fn in forms.items():
            out = fn()
            assert torch.equal(out["score_map_ref_cross"], first["score_map_ref_cross"]), k  # the forms score the same rows: the same bits
        if R >= 16 * N and R % 16 == 0:
            sixteen = np.arange(0, R + 1, R // 16, dtype=np.int32)
            gdesc = statistics.median(timed(lambda: net.reference_descriptors(tokens, sixteen), 5) for _ in range(3))
            say(f"R = {R}: the descriptors of the whole bank in 16 groups {gdesc * 1e6:.1f} us (ungrouped {desc * 1e6:.1f} us)")
            bank16 = SelectionBank(tokens, *net.reference_descriptors(tokens, sixteen), N, sixteen, -1)
            groups16 = (np.arange(B) % 16).astype(np.int32)
            forms["grouped16"] = lambda: net.forward_select(q, bank16, None, False, 0, True, group=groups16)
            forms["grouped16"]()
        seen = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                seen[k].append(timed(fn, args.steps))
        med = {k: statistics.median(v) for k, v in seen.items()}
        say(f"R = {R}: per batch  select {med['select'] * 1e3:.3f} ms   stack + forward_cached {med['stack'] * 1e3:.3f} ms   forward_cached alone "
            f"{med['cached'] * 1e3:.3f} ms   (spread of the rounds: " + ", ".join(f"{k} {min(v) * 1e3:.3f}-{max(v) * 1e3:.3f}" for k, v in seen.items()) + ")")
        say(f"R = {R}: the choice and the gather on the device add {(med['select'] - med['cached']) * 1e6:.0f} us to the cached forward, the host-side "
            f"stack adds {(med['stack'] - med['cached']) * 1e6:.0f} us")
        say(f"R = {R}: per batch  grouped (G = 1) {med['grouped1'] * 1e3:.3f} ms = select {(med['grouped1'] - med['select']) * 1e6:+.0f} us" +
            (f"   grouped (G = 16) {med['grouped16'] * 1e3:.3f} ms = select {(med['grouped16'] - med['select']) * 1e6:+.0f} us" if "grouped16" in med else ""))
        net.forward_select(q, bank, None, False, 0, True)
        st = net.forward_stats()
        say(f"R = {R}: forward_select enqueues {st['launches']} launches in {st['host_enqueue_ms']:.2f} ms of host time")
        bank = bank1 = bank16 = tokens = pre = imgs = None
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
