"""References and expected-value helpers that more than one kernel test module uses: the packed-half GELU's fitting tool and compiled constants,
the attention reference and one-hot codes, the GEMM's LayerNorm partial sums.  (Panel operands: panel_data.py; GEMM walk operands:
gemm_walk_data.py; patch tiles: patch_tile_data.py.)"""
import importlib.util
import math
import os
import re

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- packed-half GELU of the token-panel kernels ------------------------------------------------------------------------------------------
def gelu_tool():
    """tools/gelu_pk16_fit.py as a module"""
    spec = importlib.util.spec_from_file_location("gelu_pk16_fit", os.path.join(REPO, "tools", "gelu_pk16_fit.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def gelu_kernel_constants():
    """{name: half value} of pk_gelu_consts() in panel_shared.h (both halves of every packed constant must be equal)."""
    src = open(os.path.join(REPO, "crossscore_amd", "csrc", "panel_shared.h")).read()  # (shared by panel.hip and panel4.hip since round 6)
    out = {}
    for name, hexv in re.findall(r'asm volatile\("[sv]_mov_b32 %0, 0x([0-9a-f]{8})" : "=[sv]"\(k\.(\w+)\)\)', src):
        name, hexv = hexv, name
        lo, hi = int(hexv[4:], 16), int(hexv[:4], 16)
        assert lo == hi, (name, hexv)
        out[name] = float(np.array([lo], dtype=np.uint16).view(np.float16)[0])
    return out


def gelu_compiled(k):
    """the constants in the order the tool's kernel_gelu takes them"""
    return np.asarray([k["c0"], k["c1"], k["c2"], k["c3"], k["c4"], k["c5"], k["vc6"]])


# ---- attention ------------------------------------------------------------------------------------------------------------------------
def attn_ref(Q, K, V, heads, dh):
    """fp32 reference for a Q that carries log2(e)/sqrt(dh) already (hip_helpers.prescale_q): natural-log logits are q.k * ln 2"""
    B, Lq, _ = Q.shape
    Lk = K.shape[1]
    q = Q.float().view(B, Lq, heads, dh).transpose(1, 2)
    k = K.float().view(B, Lk, heads, dh).transpose(1, 2)
    v = V.float().view(B, Lk, heads, dh).transpose(1, 2)
    s = (q @ k.transpose(-1, -2)) * math.log(2.0)
    p = torch.softmax(s, dim=-1)
    return (p @ v).transpose(1, 2).reshape(B, Lq, heads * dh), torch.logsumexp(s, dim=-1)


def attn_code(i, nbits=11):
    """11-bit codes in +-16: q.k is maximal (11 * 256) for the matching key only, 512 less for the nearest other one"""
    return (((i[..., None] >> torch.arange(nbits, device=i.device)) & 1).float() * 2 - 1) * 16


# ---- GEMM with the LayerNorm producer epilogue ------------------------------------------------------------------------------------------
def row_partials(x, sp):
    """(sum, sumsq) of each row of x over the column ranges the 128-row kernel's (column tile, wave) pairs own"""
    M, Cc = x.shape
    tiles = sp // 4
    bn = Cc // tiles if Cc % 192 == 0 else 128
    wn = bn // 4
    out = torch.zeros((M, sp, 2), device=x.device)
    for t in range(tiles):
        for w in range(4):
            seg = x[:, t * bn + w * wn:min(t * bn + w * wn + wn, Cc)]
            out[:, t * 4 + w, 0] = seg.sum(1)
            out[:, t * 4 + w, 1] = (seg * seg).sum(1)
    return out
