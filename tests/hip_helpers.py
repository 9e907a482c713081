"""torch-tensor wrappers over the single-op C-ABI entry points (tests only).  Outputs are allocated here unless the caller passes them (views into
guarded buffers: tests/guard.py); every row pitch passed to the library is the tensor's own stride, so strided views go through unchanged."""
import contextlib
import ctypes as C

import torch

from crossscore_amd import _lib

# the library's process-wide debug switches: keyword of switches() -> (setter, the library's default).  The ABI has no getters.
SWITCHES = {"bf16": ("cs_debug_set_op_operand_dtype", 0), "gemm256": ("cs_debug_gemm256_enable", 1), "panel_impl": ("cs_debug_panel_impl", 0),
            "rowln": ("cs_debug_rowln_enable", 1), "grid": ("cs_debug_gemm_grid", 0)}


@contextlib.contextmanager
def switches(lib=None, **given):
    """Sets exactly the switches it is given (bf16=, gemm256=, panel_impl=, rowln=, grid=; None: not given) for the duration of a block and puts
    exactly those back to the library's defaults on every way out, a refused operand type during entry included.  Managers over different
    switches nest; `lib` is the loaded library unless a test passes a stand-in."""
    given = {k: int(v) for k, v in given.items() if v is not None}
    assert set(given) <= set(SWITCHES), sorted(set(given) - set(SWITCHES))
    lib = lib or _lib.load()
    try:
        for name, v in given.items():
            rc = getattr(lib, SWITCHES[name][0])(v)
            assert name != "bf16" or rc == 0, rc
        yield
    finally:
        for name in given:
            getattr(lib, SWITCHES[name][0])(SWITCHES[name][1])


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ld(t):
    """row pitch in elements of a 2-D operand whose rows are contiguous"""
    assert t.stride(-1) == 1, t.stride()
    return t.stride(0)


def gemm(A, W, bias=None, epi=_lib.EPI_BIAS_F16, resid=None, out=None, pos=None, Np=0, gw=0, P=0, act=0, powp=1.0,
         K=None, ldc=None, out_f16=None, stats_out=None, ln_part=None, col_s=None, ln_eps=1e-6):
    """A:(M,K) fp16, W:(N,K) fp16 (rows lda / ldw apart) -> out (allocated here unless given)."""
    lib = _lib.load()
    M, N = A.shape[0], W.shape[0]
    K = K or A.shape[1]
    if out is None:
        dt = torch.float16 if (epi <= _lib.EPI_BIAS_LEAKY_F16 or epi in (_lib.EPI_LN_F16, _lib.EPI_LN_GELU_F16)) else torch.float32
        out = torch.zeros((M, N), dtype=dt, device=A.device)
    ldc = ldc or _ld(out)
    rc = lib.cs_op_gemm(_p(A), _ld(A), _p(W), _ld(W), M, N, K, _p(bias), _p(resid), _ld(resid) if resid is not None else 0,
                        _p(out), ldc, epi, _p(pos), Np, gw, P, act, powp, _p(out_f16), _p(stats_out),
                        stats_out.shape[1] if stats_out is not None else 0, _p(ln_part), ln_part.shape[1] if ln_part is not None else 0,
                        _p(col_s), ln_eps, _stream())
    _lib.check(rc)
    return out


def head_sp(P):
    """per-row partial-sum slots of the head's mean (cs_op_head_score mean_part)"""
    return 4 * ((P * P + 127) // 128 if (P * P) % 192 else (P * P) // 192)


def head_score(A, W, bias, B, gh, gw, P, act=0, powp=1.0, want_mean=True, cnt=None, score=None, part=None, mean=None):
    """The head's last linear + activation + jigsaw and the per-image mean from the same launch -> (score (B, gh P, gw P), mean (B,), counters)."""
    lib = _lib.load()
    M, K = A.shape
    Np = gh * gw
    if score is None:
        score = torch.full((B, gh * P, gw * P), 777.0, dtype=torch.float32, device=A.device)
    if want_mean and part is None:
        part = torch.full((M, head_sp(P)), float("nan"), dtype=torch.float32, device=A.device)
    if want_mean and cnt is None:
        cnt = torch.zeros((B,), dtype=torch.int32, device=A.device)
    if want_mean and mean is None:
        mean = torch.full((B,), 777.0, dtype=torch.float32, device=A.device)
    if not want_mean:
        part = mean = None
    _lib.check(lib.cs_op_head_score(_p(A), _ld(A), _p(W), _ld(W), M, K, _p(bias), _p(score), Np, gw, P, act, powp, _p(part),
                                    _p(cnt) if want_mean else None, _p(mean), _stream()))
    return score, mean, cnt


def ln_finalize(part, Cc, eps=1e-6, stat=None):
    """(M, sp, 2) partial sums of the 256-tile GEMM's residual epilogue -> (ceil(M / 256) * 256, 1, 2) finalised (mean, rstd) rows."""
    lib = _lib.load()
    M, sp, _ = part.shape
    Mpad = (M + 255) // 256 * 256
    if stat is None:
        stat = torch.full((Mpad, 1, 2), 777.0, dtype=torch.float32, device=part.device)
    _lib.check(lib.cs_op_ln_finalize(_p(part), M, stat.shape[0], sp, Cc, eps, _p(stat), _stream()))
    return stat


def silu_mul(x):
    """in place on x (M, 2F) 16-bit rows (a view: rows x.stride(0) apart): x[:, :F] = silu(x[:, :F]) * x[:, F:]"""
    lib = _lib.load()
    M, F2 = x.shape
    _lib.check(lib.cs_op_silu_mul(_p(x), M, F2 // 2, _ld(x), _stream()))
    return x


def prescale_q(Q, dh):
    """Q * log2(e)/sqrt(dh) in fp32, rounded to fp16 once: what the forward's Q projections emit (the factor is folded into their weights)."""
    return (Q.float() * (1.4426950408889634 / dh ** 0.5)).to(torch.float16)


def attention(Q, K, V, heads, dh, lse=False, q_scale=0.0, O=None, L=None):
    """Q:(B,Lq,heads*dh) K,V:(B,Lk,heads*dh) fp16 (any row / batch strides) -> O (B,Lq,heads*dh) fp16 [, lse (B,heads,Lq), base 2].
    q_scale=1: Q is prescale_q(..) already; 0: raw Q, scaled (and re-rounded) inside the kernel.  O / L: caller-provided outputs."""
    lib = _lib.load()
    B, Lq, Cq = Q.shape
    Lk = K.shape[1]
    if O is None:
        O = torch.zeros((B, Lq, heads * dh), dtype=torch.float16, device=Q.device)
    if lse and L is None:
        L = torch.zeros((B, heads, Lq), dtype=torch.float32, device=Q.device)
    if L is not None:
        assert L.is_contiguous()
    rc = lib.cs_op_attention(_p(Q), _p(K), _p(V), _p(O), Q.stride(1), K.stride(1), V.stride(1), O.stride(1), Q.stride(0), K.stride(0),
                             V.stride(0), O.stride(0), B, heads, Lq, Lk, dh, q_scale, _p(L), _stream())
    _lib.check(rc)
    return (O, L) if L is not None else O


def attention_weights(Q, K, heads, dh, lse, head, q_scale=0.0, out=None):
    lib = _lib.load()
    B, Lq, _ = Q.shape
    Lk = K.shape[1]
    if out is None:
        out = torch.zeros((B, Lq, Lk), dtype=torch.float32, device=Q.device)
    assert out.is_contiguous()
    rc = lib.cs_op_attention_weights(_p(Q), _p(K), Q.stride(1), K.stride(1), Q.stride(0), K.stride(0), B, heads, Lq, Lk, dh, q_scale,
                                     _p(lse), head, _p(out), _stream())
    _lib.check(rc)
    return out


def layernorm(x, g, b, eps, want_f32=True, want_f16=True, of=None, ob=None):
    lib = _lib.load()
    M, Cc = x.shape
    assert x.is_contiguous()
    if want_f32 and of is None:
        of = torch.zeros_like(x)
    if want_f16 and ob is None:
        ob = torch.zeros((M, Cc), dtype=torch.float16, device=x.device)
    _lib.check(lib.cs_op_layernorm(_p(x), M, Cc, _p(g), _p(b), eps, _p(of), _p(ob), _stream()))
    return of, ob


def im2col(x, P, Kp, out=None):
    lib = _lib.load()
    I, _, H, W = x.shape
    if out is None:
        out = torch.zeros((I * (H // P) * (W // P), Kp), dtype=torch.float16, device=x.device)
    assert out.is_contiguous() and out.shape[1] == Kp
    _lib.check(lib.cs_op_im2col(_p(x), _p(out), I, H, W, P, Kp, _stream()))
    return out


def pos_bicubic(pos, G, gh, gw, legacy=None, out=None):
    lib = _lib.load()
    Cc = pos.shape[-1]
    if out is None:
        out = torch.zeros((1 + gh * gw, Cc), dtype=torch.float32, device=pos.device)
    if legacy is None:
        _lib.check(lib.cs_op_pos_bicubic(_p(pos), G, Cc, gh, gw, _p(out), _stream()))
    else:
        _lib.check(lib.cs_op_pos_bicubic_ex(_p(pos), G, Cc, gh, gw, int(legacy), _p(out), _stream()))
    return out


def pe_bilinear(pe, gh, gw):
    lib = _lib.load()
    ph, pw, Cc = pe.shape
    out = torch.zeros((gh * gw, Cc), dtype=torch.float32, device=pe.device)
    _lib.check(lib.cs_op_pe_bilinear(_p(pe), ph, pw, Cc, gh, gw, _p(out), _stream()))
    return out


def linear_layernorm(A, W, bias, resid, gamma, beta, eps, want_f32=True, want_f16=True, of=None, oh=None):
    """LN(resid + A W^T + bias) in one launch (csrc/rowln.hip): A (M,C) fp16, W (C,C) fp16 -> (out_f32, out_f16)"""
    lib = _lib.load()
    M, Cc = A.shape
    if want_f32 and of is None:
        of = torch.zeros((M, Cc), dtype=torch.float32, device=A.device)
    if want_f16 and oh is None:
        oh = torch.zeros((M, Cc), dtype=torch.float16, device=A.device)
    _lib.check(lib.cs_op_linear_layernorm(_p(A), _p(W), _p(bias), _p(resid), _p(gamma), _p(beta), eps, _p(of), _p(oh), M, Cc, _stream()))
    return of, oh


def linear_layernorm_linear(A, W, bias, resid, gamma, beta, eps, W2, bias2, act2, want_f32=True, want_f16=False, out2=None, of=None, oh=None):
    """the same with the sub-block's next linear in the launch: -> (out_f32, out_f16, out2 (M, n2) fp16); out2 may be A itself"""
    lib = _lib.load()
    M, Cc = A.shape
    n2 = W2.shape[0]
    if want_f32 and of is None:
        of = torch.zeros((M, Cc), dtype=torch.float32, device=A.device)
    if want_f16 and oh is None:
        oh = torch.zeros((M, Cc), dtype=torch.float16, device=A.device)
    o2 = torch.zeros((M, n2), dtype=torch.float16, device=A.device) if out2 is None else out2
    _lib.check(lib.cs_op_linear_layernorm_linear(_p(A), _p(W), _p(bias), _p(resid), _p(gamma), _p(beta), eps, _p(of), _p(oh), _p(W2), _p(bias2),
                                                 n2, int(act2), _p(o2), M, Cc, _stream()))
    return of, oh, o2


def pe_interp(pe, gh, gw, mode, out=None):
    """mode 0 bilinear, 1 bicubic (align_corners=True): model.pos_enc.multi_view.interpolate_mode"""
    lib = _lib.load()
    ph, pw, Cc = pe.shape
    if out is None:
        out = torch.zeros((gh * gw, Cc), dtype=torch.float32, device=pe.device)
    _lib.check(lib.cs_op_pe_interp(_p(pe), ph, pw, Cc, gh, gw, int(mode), _p(out), _stream()))
    return out


def pack_f16(w, ldo=None, row_scale=None, col_scale=None, out=None):
    """fp32 (rows, K) -> 16-bit rows `ldo` apart, zero-padded to ldo; out: a caller-provided (rows, ldo) output (its row pitch is passed)"""
    lib = _lib.load()
    rows, K = w.shape
    if out is None:
        out = torch.zeros((rows, ldo or K), dtype=torch.float16, device=w.device)
    _lib.check(lib.cs_op_pack_f16(_p(w), rows, K, _p(out), _ld(out), _p(row_scale), _p(col_scale), _stream()))
    return out


def ln_fold_consts(w_packed, w, beta, bias, s=None, c=None):
    lib = _lib.load()
    N, K = w.shape
    s = torch.zeros(N, device=w.device) if s is None else s
    c = torch.zeros(N, device=w.device) if c is None else c
    _lib.check(lib.cs_op_ln_fold_consts(_p(w_packed), _ld(w_packed), _p(w), _p(beta), _p(bias), N, K, _p(s), _p(c), _stream()))
    return s, c


def column_tiles(N):
    return _lib.load().cs_gemm_column_tiles(N)


def panel_pack(wo, ls1, w1, g2, w2, ls2, img=None):
    """fp32 weights -> the unit stream of the encoder token-panel kernel (uint8 tensor of cs_panel_image_bytes)."""
    lib = _lib.load()
    n = lib.cs_panel_image_bytes(1 if wo is not None else 0)
    if img is None:
        img = torch.zeros(n, dtype=torch.uint8, device=w1.device)
    assert img.numel() == n
    _lib.check(lib.cs_op_panel_pack(_p(wo), _p(ls1), _p(w1), _p(g2), _p(w2), _p(ls2), _p(img), _stream()))
    return img


def encoder_panel(x, attn_o, img, bo, b1, b2, want_u=True, eps=1e-6, u=None):
    """In place on x (M,384) fp32; returns u (M,384) fp16 or None."""
    lib = _lib.load()
    M = x.shape[0]
    if want_u and u is None:
        u = torch.zeros((M, x.shape[1]), dtype=torch.float16, device=x.device)
    _lib.check(lib.cs_op_encoder_panel(_p(x), _p(attn_o), _p(img), _p(bo), _p(b1), _p(b2), _p(u), M, eps, _stream()))
    return u


def patch_embed_fused(x, w, bias, pos, P, out=None):
    """one-launch form (csrc/patch.hip): same contract as patch_embed(centred=True)"""
    lib = _lib.load()
    I, _, H, W = x.shape
    C_ = w.shape[0]
    Np = (H // P) * (W // P)
    if out is None:
        out = torch.full((I * (1 + Np), C_), 7.0, dtype=torch.float32, device=x.device)
    _lib.check(lib.cs_op_patch_embed_fused(_p(x), _p(w), _p(bias), _p(pos), I, H, W, P, C_, _p(out), _stream()))
    return out


def patch_embed_fused_u8(imgs_u8, rs, crop, mean, std, w, bias, pos, P, out=None):
    """imgs_u8 (I, h, >= w*3) uint8 device, rows of w*3 bytes (+ padding: the row pitch is the tensor's stride) -> token rows as
    patch_embed_fused of the input stage's output.  The images are h rows apart: a view with a gap between images is refused."""
    lib = _lib.load()
    I, h = imgs_u8.shape[:2]
    row = imgs_u8.stride(1)
    assert imgs_u8.stride(2) == 1 and imgs_u8.stride(0) == h * row, imgs_u8.stride()
    y0, x0, H, W, in_w = crop
    C_ = w.shape[0]
    Np = (H // P) * (W // P)
    if out is None:
        out = torch.full((I * (1 + Np), C_), 7.0, dtype=torch.float32, device=imgs_u8.device)
    _lib.check(lib.cs_op_patch_embed_fused_u8(_p(imgs_u8), I, h, in_w, row, rs[0], rs[1], y0, x0, H, W, (C.c_float * 3)(*mean), (C.c_float * 3)(*std),
                                              _p(w), _p(bias), _p(pos), P, C_, _p(out), _stream()))
    return out


def patch_embed(x, w, bias, pos, P, centred, out=None):
    """(I,3,H,W) images -> (I * (1 + Np), C) fp32 token rows (patch rows written, CLS rows left at 7.0)."""
    lib = _lib.load()
    I, _, H, W = x.shape
    C_ = w.shape[0]
    Np = (H // P) * (W // P)
    if out is None:
        out = torch.full((I * (1 + Np), C_), 7.0, dtype=torch.float32, device=x.device)
    _lib.check(lib.cs_op_patch_embed(_p(x), _p(w), _p(bias), _p(pos), I, H, W, P, C_, int(centred), _p(out), _stream()))
    return out


def preprocess_u8(img, in_w, rs, crop, out_hw, mean, std, out=None):
    """img (in_h, row_bytes) uint8 rows of in_w * 3 bytes (+ padding: the row pitch is the tensor's stride) -> fp32 (3, out_h, out_w)"""
    lib = _lib.load()
    in_h = img.shape[0]
    oh, ow = out_hw
    if out is None:
        out = torch.empty((3, oh, ow), dtype=torch.float32, device=img.device)
    scratch = torch.empty((in_h * rs[1] * 3,), dtype=torch.float32, device=img.device) if tuple(rs) != (in_h, in_w) else None
    _lib.check(lib.cs_op_preprocess_u8(_p(img), in_h, in_w, _ld(img), rs[0], rs[1], crop[0], crop[1], oh, ow, (C.c_float * 3)(*mean),
                                       (C.c_float * 3)(*std), _p(out), _p(scratch), _stream()))
    return out


def metric_map_u16(maps, B, in_h, in_w, mode, rs, crop, out_hw, out=None):
    """maps (B, in_h, row_elems) 16-bit maps (int16 / uint16 bits; rows the tensor's stride apart, maps in_h rows apart) or None (placeholders)
    -> fp32 (B, out_h, out_w)"""
    lib = _lib.load()
    oh, ow = out_hw
    dev = out.device if out is not None else maps.device
    if out is None:
        out = torch.empty((B, oh, ow), dtype=torch.float32, device=dev)
    row = in_w
    if maps is not None:
        row = maps.stride(1)
        assert maps.stride(2) == 1 and maps.stride(0) == in_h * row, maps.stride()
    scratch = torch.empty((B * in_h * rs[1],), dtype=torch.float32, device=dev) if maps is not None and tuple(rs) != (in_h, in_w) else None
    _lib.check(lib.cs_op_metric_map_u16(_p(maps), B, in_h, in_w, row, mode, rs[0], rs[1], crop[0], crop[1], oh, ow, _p(out), _p(scratch), _stream()))
    return out


def score_to_gray16(score, signed_range, out=None):
    lib = _lib.load()
    n = score.numel()
    out = torch.empty((n,), dtype=torch.int16, device=score.device) if out is None else out
    _lib.check(lib.cs_op_score_to_gray16(_p(score), n, int(signed_range), _p(out), _stream()))
    return out


def score_to_rgb(score, vmin, vmax, lut, out=None):
    lib = _lib.load()
    n = score.numel()
    out = torch.empty((n, 3), dtype=torch.uint8, device=score.device) if out is None else out
    _lib.check(lib.cs_op_score_to_rgb(_p(score), n, vmin, vmax, _p(lut), _p(out), _stream()))
    return out


def score_gt_stats(score, gt, out=None, scratch=None):
    """score, gt (B, H, W) fp32 -> (B, 6) fp64 sums"""
    lib = _lib.load()
    B, H, W = score.shape
    out = torch.empty((B, 6), dtype=torch.float64, device=score.device) if out is None else out
    if scratch is None:
        scratch = torch.empty((lib.cs_score_gt_workspace_bytes(B, H, W),), dtype=torch.uint8, device=score.device)
    _lib.check(lib.cs_op_score_gt_stats(_p(score), _p(gt), B, H, W, _p(out), _p(scratch), _stream()))
    return out
