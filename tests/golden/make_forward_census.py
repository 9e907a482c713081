"""The forward's launch census, case by case: which kernels one forward enqueues, how many, and the workspace it asks for.

    python tests/golden/make_forward_census.py [OUT.json]     # default: tests/golden/forward_census.json (needs the GPU)

Uses only the package's public Python surface, so the same file runs on any commit that has that surface: the fixture was written by the
commit BEFORE the host code of the forward was split into api.hip / forward.hip / ops.hip, and tests/test_forward_census.py holds every later
commit to it.  The cases are the smallest shapes that reach each routing branch of the forward (panel / fold256 / fold / plain / SwiGLU layers,
row-complete or GEMM + LayerNorm decoder closings, one or more lanes, cached and uint8 entry points, profiling).

`run_case(name, capture=True)` also returns every output array and debug tap of the case (tools/forward_split_ab.py compares two library
builds with it); the census itself is taken with capture off.
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from crossscore_amd import _lib, synth  # noqa: E402
from crossscore_amd.config import model_config  # noqa: E402
from crossscore_amd.model import CrossScoreNet  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "forward_census.json")
TINY, SMALL2, BASE2, SWIGLU2 = "synthetic/dinov2-tiny", "synthetic/dinov2-small-2l", "synthetic/dinov2-base-2l", "synthetic/dinov2-swiglu-2l"
TINY_SHAPE = (2, 2, 75, 90)
WIDE_SHAPE = (2, 3, 98, 112)  # g8's: 8 images x 57 tokens = 456 encoder rows
# every profile family the library records: the GEMM epilogues (0..9), attention (16 + dh / 16), small kernels (32), panel (40), patch (41), rowln (42)
FAMILIES = list(range(0, 10)) + [16 + dh // 16 for dh in (16, 48, 64, 96, 128, 192)] + [32, 40, 41, 42]

# name -> backbone, (B, N, H, W), module attributes, config overrides, process-wide debug switches, how it is driven
CASES = {
    "tiny_one_lane": dict(back=TINY, shape=TINY_SHAPE, attrs=dict(lanes=1)),
    "tiny_default_lanes": dict(back=TINY, shape=TINY_SHAPE),
    "tiny_ln_fold_1": dict(back=TINY, shape=TINY_SHAPE, attrs=dict(ln_fold=1)),
    "tiny_no_self_attn": dict(back=TINY, shape=TINY_SHAPE, over={"decoder_do_self_attn": False}),
    "tiny_no_short_cut": dict(back=TINY, shape=TINY_SHAPE, over={"decoder_do_short_cut": False}),
    "tiny_attn_weights_head_1": dict(back=TINY, shape=TINY_SHAPE, attn_head=1),
    "tiny_remainder_chunk": dict(back=TINY, shape=TINY_SHAPE, attrs=dict(enc_chunk_images=4)),  # 6 images: a chunk of 2 first, then one of 4
    "vits_default": dict(back=SMALL2, shape=WIDE_SHAPE),  # two lanes: chunks of 228 rows, QKV on the 128-row GEMM
    "vits_one_lane": dict(back=SMALL2, shape=WIDE_SHAPE, attrs=dict(lanes=1)),  # one chunk of 456 rows: QKV on the 256-tile GEMM
    "vits_two_lanes": dict(back=SMALL2, shape=WIDE_SHAPE, attrs=dict(lanes=2)),
    "vits_unfused": dict(back=SMALL2, shape=WIDE_SHAPE, attrs=dict(enc_fused=1), switches=dict(rowln=0)),
    "vits_rowln_no_next": dict(back=SMALL2, shape=WIDE_SHAPE, switches=dict(rowln=2)),
    "vits_panel4": dict(back=SMALL2, shape=WIDE_SHAPE, switches=dict(panel_impl=1)),
    "vits_bf16": dict(back=SMALL2, shape=WIDE_SHAPE, attrs=dict(operand_dtype="bf16")),
    "vits_cached": dict(back=SMALL2, shape=WIDE_SHAPE, drive="cached"),
    "vits_u8": dict(back=SMALL2, shape=(2, 2, 70, 84), drive="u8"),
    "vits_profile": dict(back=SMALL2, shape=WIDE_SHAPE, drive="profile"),
    # the wide backbones fold their LayerNorms into the 256-tile GEMM only for chunks of >= 256 rows: one lane keeps the 456 rows in one chunk
    "vitb_default": dict(back=BASE2, shape=WIDE_SHAPE),  # two lanes: a fold256 handle whose chunks (228 rows) take the LayerNorm launches
    "vitb_folded": dict(back=BASE2, shape=WIDE_SHAPE, attrs=dict(lanes=1)),
    "vitb_ln_fold_2": dict(back=BASE2, shape=WIDE_SHAPE, attrs=dict(lanes=1, ln_fold=2)),
    "vitb_gemm256_off": dict(back=BASE2, shape=WIDE_SHAPE, attrs=dict(lanes=1), switches=dict(gemm256=0)),
    "swiglu_default": dict(back=SWIGLU2, shape=WIDE_SHAPE),
    "swiglu_one_lane": dict(back=SWIGLU2, shape=WIDE_SHAPE, attrs=dict(lanes=1)),
}


def _u8_inputs(net, B, N, dev):
    """Decoded uint8 images of three sizes, all -> the 70 x 84 window; one placeholder reference (as tests/test_preprocess.py drives it)."""
    from crossscore_amd.data import InputStage
    stage = InputStage(dev, resize_short_side=70, integer_patches=True)
    rng = np.random.Generator(np.random.PCG64(11))
    sizes = [(120, 160), (90, 120), (120, 160), (150, 200), (90, 120), (120, 160)]
    imgs = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
    size = stage.geometry(*sizes[0])[1][2:]
    refs = []
    for b in range(B):
        for n in range(N):
            refs.append(stage.placeholder(size) if (b, n) == (1, 1) else stage.describe(imgs[B + b * N + n]))
    return stage.batch([stage.describe(imgs[b]) for b in range(B)], size), stage.batch(refs, size)


def run_case(name, capture=False):
    """Runs one case in this process.  Returns (record, arrays): the census record of the fixture, and (capture on) the outputs and taps."""
    case = CASES[name]
    lib = _lib.load()
    B, N, H, W = case["shape"]
    sw = case.get("switches", {})
    drive = case.get("drive", "forward")
    dev = torch.device("cuda:0")
    arrays, calls = {}, []
    try:
        if "rowln" in sw:
            lib.cs_debug_rowln_enable(sw["rowln"])
        if "gemm256" in sw:
            lib.cs_debug_gemm256_enable(sw["gemm256"])
        if "panel_impl" in sw:
            lib.cs_debug_panel_impl(sw["panel_impl"])  # read when the handle is created
        net = CrossScoreNet(model_config(**{"backbone.from_pretrained": case["back"], **case.get("over", {})}))
        net.load_numpy_state_dict(synth.make_state_dict(net.arch, 8))
        for k, v in case.get("attrs", {}).items():
            setattr(net, k, v)
        net = net.cuda()
        net.debug_capture(capture)

        def note(tag, out=None):
            torch.cuda.synchronize()
            s = net.forward_stats()
            calls.append({"call": tag, "kernels": s["kernels"], "launches": s["launches"]})
            for k, v in (out or {}).items():
                if v is not None:
                    arrays[f"{tag}.{k}"] = v
            if capture:
                taps = ["embeddings", "featmap_query", "featmap_ref", "head_pre_activation"]
                taps += [f"enc_layer_{l}" for l in range(net.arch.enc_layers)] + [f"dec{l}_out" for l in range(net.arch.dec_layers)]
                for t in taps:
                    try:
                        arrays[f"{tag}.tap.{t}"] = net.debug_read(t)
                    except _lib.CrossScoreHipError:
                        pass  # this call does not write that tap (a cached forward has no reference rows in its encoder, ...)

        head = case.get("attn_head")
        q, r = (torch.from_numpy(a).to(dev) for a in synth.make_inputs(B, N, H, W, 8))
        if drive == "u8":
            q8, r8 = _u8_inputs(net, B, N, dev)
            note("forward_u8", net.forward(q8, r8, True, 3, return_mean=True))
            tok = net.encode_references(r8)
            note("encode_references_u8", {"tokens": tok})
            note("forward_cached_u8", net.forward_cached(q8, tok.reshape((B, N) + tuple(tok.shape[1:])), False, 0, True))
        elif drive == "cached":
            tok = net.encode_references(r.reshape(B * N, 3, H, W))
            note("encode_references", {"tokens": tok})
            note("forward_cached", net.forward_cached(q, tok.reshape((B, N) + tuple(tok.shape[1:])), False, 0, True))
        else:
            if drive == "profile":
                net(q, r, False, 0, False)  # the handle exists from here on
                net.profile_enable(True)
            note("forward", net(q, r, head is not None, head or 0, False, return_mean=True))
        record = {"calls": calls, "workspace_bytes": int(lib.cs_workspace_bytes(net._handle, B, N, H, W))}
        if drive == "profile":
            prof = {}
            for fam in FAMILIES:
                _, n, flops = net.profile_read(fam)
                if n:
                    prof[str(fam)] = [int(n), float(flops), float(net.profile_read_bytes(fam))]
            record["profile"] = prof
            net.profile_enable(False)
        arrays = {k: v.float().cpu().numpy() if v.dtype == torch.bfloat16 else v.cpu().numpy() for k, v in arrays.items()}
        del net
        return record, arrays
    finally:
        lib.cs_debug_rowln_enable(1)
        lib.cs_debug_gemm256_enable(1)
        lib.cs_debug_panel_impl(0)


if __name__ == "__main__":
    out = {}
    for name in CASES:
        out[name], _ = run_case(name)
        print(name, json.dumps(out[name]))
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)
