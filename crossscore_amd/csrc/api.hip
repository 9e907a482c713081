// C ABI of the CrossScore gfx950 path (see include/crossscore_hip.h): the handle's life cycle, weight packing, and the stats / debug /
// profile / lane accessors.  Host-side only.  The forward itself is forward.hip, the single-op entry points are ops.hip, fitting is fit_host.hip;
// what the four share is cs_model.h.
#include "cs_model.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace cs_host {

int g_debug_stream_log = 0;
int g_panel_impl = 0;
int g_rowln_off = 0;
int g_rowln_no_next = 0;
int g_op_bf16 = 0;

static thread_local std::string g_err;
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

}  // namespace cs_host

namespace {

std::vector<std::string> expected_names(const cs_config& c) {
  std::vector<std::string> n;
  n.push_back("img_mean_std");
  const std::string e = "backbone.embeddings.";
  n.push_back(e + "cls_token"); n.push_back(e + "mask_token"); n.push_back(e + "position_embeddings");
  n.push_back(e + "patch_embeddings.projection.weight"); n.push_back(e + "patch_embeddings.projection.bias");
  for (int l = 0; l < c.enc_layers; ++l) {
    const std::string p = "backbone.encoder.layer." + std::to_string(l) + ".";
    for (const char* s : {"norm1.weight", "norm1.bias", "attention.attention.query.weight", "attention.attention.query.bias",
                          "attention.attention.key.weight", "attention.attention.key.bias", "attention.attention.value.weight",
                          "attention.attention.value.bias", "attention.output.dense.weight", "attention.output.dense.bias",
                          "layer_scale1.lambda1", "norm2.weight", "norm2.bias", "layer_scale2.lambda1"})
      n.push_back(p + s);
    if (c.swiglu) for (const char* s : {"mlp.weights_in.weight", "mlp.weights_in.bias", "mlp.weights_out.weight", "mlp.weights_out.bias"}) n.push_back(p + s);
    else for (const char* s : {"mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"}) n.push_back(p + s);
  }
  n.push_back("backbone.layernorm.weight"); n.push_back("backbone.layernorm.bias");
  n.push_back("pos_enc_fn.PE");
  for (int l = 0; l < c.dec_layers; ++l) {
    const std::string p = "ref_cross.attn.layers." + std::to_string(l) + ".";
    std::vector<std::string> blocks;
    if (c.do_self_attn) blocks.push_back("self_attn");
    blocks.push_back("multihead_attn");
    for (auto& b : blocks)
      for (const char* s : {".in_proj_weight", ".in_proj_bias", ".out_proj.weight", ".out_proj.bias"}) n.push_back(p + b + s);
    for (const char* s : {"linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias",
                          "norm2.weight", "norm2.bias", "norm3.weight", "norm3.bias"})
      n.push_back(p + s);
  }
  for (const char* s : {"ref_cross.head.0.weight", "ref_cross.head.0.bias", "ref_cross.head.2.weight", "ref_cross.head.2.bias"})
    n.push_back(s);
  return n;
}

}  // namespace

extern "C" {

const char* cs_last_error(void) { return g_err.c_str(); }

cs_handle cs_create(const cs_config* cfg) {
  if (!cfg) { fail(CS_ERR_BAD_ARG, "cs_create: null config"); return nullptr; }
  const cs_config& c = *cfg;
  if (c.hidden <= 0 || c.hidden % 64 || c.hidden > 1536) { fail(CS_ERR_UNSUPPORTED, "hidden=%d must be a multiple of 64 and <= 1536", c.hidden); return nullptr; }
  if (c.enc_layers <= 0 || c.enc_heads <= 0 || c.hidden % c.enc_heads) { fail(CS_ERR_BAD_ARG, "bad encoder layers/heads"); return nullptr; }
  if (!supported_dh(c.hidden / c.enc_heads)) { fail(CS_ERR_UNSUPPORTED, "encoder head dim %d not in {16,48,64,96,128,192}", c.hidden / c.enc_heads); return nullptr; }
  if (c.dec_heads <= 0 || c.hidden % c.dec_heads || !supported_dh(c.hidden / c.dec_heads)) { fail(CS_ERR_UNSUPPORTED, "decoder head dim %d not in {16,48,64,96,128,192}", c.dec_heads > 0 ? c.hidden / c.dec_heads : 0); return nullptr; }
  if (c.dec_layers <= 0 || c.patch <= 0 || (c.patch * c.patch) % 4 || c.pos_grid <= 0 || c.pe_h <= 0 || c.pe_w <= 0 || c.mlp_ratio <= 0) { fail(CS_ERR_BAD_ARG, "bad config"); return nullptr; }
  if (c.act != 0 && c.act != 1) { fail(CS_ERR_BAD_ARG, "act must be 0 (sigmoid) or 1 (tanh)"); return nullptr; }
  if (c.act == 1 && c.pow_p != 1.0f) { fail(CS_ERR_BAD_ARG, "power factor applies only to the sigmoid range"); return nullptr; }
  if (c.pe_interp_mode != 0 && c.pe_interp_mode != 1) { fail(CS_ERR_BAD_ARG, "pe_interp_mode must be 0 (bilinear) or 1 (bicubic)"); return nullptr; }
  if (c.operand_dtype != 0 && c.operand_dtype != 1) { fail(CS_ERR_BAD_ARG, "operand_dtype must be 0 (fp16) or 1 (bf16)"); return nullptr; }
  if (c.operand_dtype == 1 && c.ln_fold == 1) { fail(CS_ERR_UNSUPPORTED, "the LayerNorm-folded epilogues (ln_fold = 1) are built for fp16 operands only"); return nullptr; }
  if (c.swiglu != 0 && c.swiglu != 1) { fail(CS_ERR_BAD_ARG, "swiglu must be 0 or 1"); return nullptr; }
  if (c.swiglu && ffn_hidden(c) % 64) { fail(CS_ERR_UNSUPPORTED, "SwiGLU hidden features %d must be a multiple of 64 (the GEMM's K)", ffn_hidden(c)); return nullptr; }
  if (c.swiglu && c.ln_fold == 1) { fail(CS_ERR_UNSUPPORTED, "ln_fold = 1 is built for the GELU MLP only"); return nullptr; }
  cs_model* m = new cs_model();
  m->cfg = c;
  m->names = expected_names(c);
  m->Kp = ((3 * c.patch * c.patch + 63) / 64) * 64;
  // the 256 x 256 x 64-tile GEMM (gemm256.hip) needs whole 256-column tiles and K >= 384 in multiples of 128
  m->qkv_n = (c.hidden >= 384 && c.hidden % 128 == 0) ? ((3 * c.hidden + 255) / 256) * 256 : 3 * c.hidden;
  m->ln_sp = 4 * cs_gemm_column_tiles(c.hidden);
  // opt-in: measured slower than separate LayerNorm kernels on cfg-2 (kernel-time sum 10.2 vs 9.5 ms: the folded consumers run
  // at the 256-register limit and their tile-switch loads drain the LDS-DMA queue)
  m->lnfold = c.ln_fold == 1 && (m->ln_sp == 4 || m->ln_sp == 8 || m->ln_sp == 16);
  // default for ViT-S: out-proj + norm2 + MLP + next norm1 in one launch per layer, the 4C hidden never leaves the registers
  m->panel = c.enc_fused != 1 && !m->lnfold && !c.swiglu && cs_panel_supported(c.hidden, c.mlp_ratio);
  m->panel_impl = g_panel_impl;
  // wide backbones (r5): the encoder's LayerNorms ride in the 256-tile GEMM's epilogues; ln_fold = 2 keeps the separate LayerNorm launches
  m->fold256 = c.ln_fold == 0 && !m->panel && !c.swiglu && c.hidden >= 512 && c.hidden % 256 == 0 && (c.mlp_ratio * c.hidden) % 256 == 0;
  return m;
}

void cs_destroy(cs_handle h) {
  if (!h) return;
  // waits explicitly for THIS handle's work (its last forward's completion event and its lane streams; a forward that failed half-way may have
  // left lane work that no event covers).  The hipFree calls below synchronise the device on top of that in today's runtime -- which is also
  // what covers caller-stream work of a half-failed forward -- so siblings of a pipeline do stall while one handle is torn down; nothing here
  // relies on them not stalling, and nothing of this handle is freed before its own streams have drained.
  if (h->ev_done) hipEventSynchronize(h->ev_done);
  for (int l = 0; l < CS_MAX_LANES; ++l) if (h->lane_st[l]) hipStreamSynchronize(h->lane_st[l]);
  for (auto& r : h->retired) hipEventSynchronize(r.ev);
  for (auto& kv : h->w) if (kv.second.d) hipFree(kv.second.d);
  for (void* p : h->owned) hipFree(p);
  for (auto& t : h->tables) { if (t.pos_owned) hipFree(t.pos_tab); if (t.pe_owned) hipFree(t.pe_tab); }
  reap_retired(h, true);
  if (h->ws) hipFree(h->ws);
  if (h->hfit_ws) hipFree(h->hfit_ws);
  if (h->fit_kept) hipFree(h->fit_kept);
  if (h->ev_done) hipEventDestroy(h->ev_done);
  if (h->ev_kv0) hipEventDestroy(h->ev_kv0);
  if (h->ev_kv1) hipEventDestroy(h->ev_kv1);
  for (int l = 0; l < CS_MAX_LANES; ++l) {
    if (h->lane_st[l]) hipStreamDestroy(h->lane_st[l]);
    if (h->ev_join[l]) hipEventDestroy(h->ev_join[l]);
    if (h->ev_stag[l]) hipEventDestroy(h->ev_stag[l]);
  }
  for (hipStream_t o : h->lane_st_old) hipStreamDestroy(o);
  if (h->ev_fork) hipEventDestroy(h->ev_fork);
  if (h->nonfinite) hipFree(h->nonfinite);
  for (auto& u : h->u8_slot) { if (u.host) hipHostFree(u.host); if (u.ev) hipEventDestroy(u.ev); }
  stage_free(h->sel_ring);
  for (auto& r : h->recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
  for (auto& kv : h->taps) if (kv.second.d) hipFree(kv.second.d);
  delete h;
}

int cs_num_weights(cs_handle h) { return h ? (int)h->names.size() : 0; }
const char* cs_weight_name(cs_handle h, int i) { return (h && i >= 0 && i < (int)h->names.size()) ? h->names[i].c_str() : nullptr; }

// dtype: CS_DTYPE_F32 / F16 / BF16 of the SOURCE buffer; the handle keeps fp32 copies (exact for all three) and packs its fp16
// operand images from those in cs_finalize
int cs_set_weight_typed(cs_handle h, const char* name, const void* data, int is_device, int dtype, int ndim, const int64_t* shape) {
  if (!h || !name || !data || ndim < 1 || !shape) return fail(CS_ERR_BAD_ARG, "cs_set_weight: null argument");
  if (dtype != CS_DTYPE_F32 && dtype != CS_DTYPE_F16 && dtype != CS_DTYPE_BF16) return fail(CS_ERR_BAD_ARG, "cs_set_weight: unknown dtype %d", dtype);
  if (h->finalized) return fail(CS_ERR_STATE, "cs_set_weight after cs_finalize");
  if (std::find(h->names.begin(), h->names.end(), name) == h->names.end()) return fail(CS_ERR_BAD_ARG, "unexpected key %s", name);
  Tensor t;
  t.numel = 1;
  for (int i = 0; i < ndim; ++i) { if (shape[i] <= 0) return fail(CS_ERR_BAD_ARG, "%s: bad shape", name); t.shape.push_back(shape[i]); t.numel *= (size_t)shape[i]; }
  auto it = h->w.find(name);
  if (it != h->w.end() && it->second.d) { hipFree(it->second.d); it->second.d = nullptr; }
  HIPCHK(hipMalloc(&t.d, t.numel * sizeof(float)));
  if (dtype == CS_DTYPE_F32) {
    HIPCHK(hipMemcpy(t.d, data, t.numel * sizeof(float), is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  } else {
    // 16-bit sources are widened on the host (checkpoint loading is set-up work; a device source is read back first)
    std::vector<uint16_t> src(t.numel);
    HIPCHK(hipMemcpy(src.data(), data, t.numel * sizeof(uint16_t), is_device ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
    std::vector<float> wide(t.numel);
    for (size_t i = 0; i < t.numel; ++i) {
      if (dtype == CS_DTYPE_BF16) {
        const uint32_t u = (uint32_t)src[i] << 16;
        std::memcpy(&wide[i], &u, 4);
      } else {
        wide[i] = (float)__builtin_bit_cast(_Float16, src[i]);  // host side: IEEE half -> float
      }
    }
    HIPCHK(hipMemcpy(t.d, wide.data(), t.numel * sizeof(float), hipMemcpyHostToDevice));
  }
  h->w[name] = t;
  return 0;
}

int cs_set_weight(cs_handle h, const char* name, const float* data, int is_device, int ndim, const int64_t* shape) {
  return cs_set_weight_typed(h, name, data, is_device, CS_DTYPE_F32, ndim, shape);
}

int cs_finalize(cs_handle h) {
  if (!h) return fail(CS_ERR_BAD_ARG, "null handle");
  if (h->finalized) return 0;
  const cs_config& c = h->cfg;
  const int64_t C = c.hidden, P = c.patch, F = ffn_hidden(c), F1 = c.swiglu ? 2 * F : F;  // F1: rows of the first projection (x1 | x2 for SwiGLU)
  auto need = [&](const std::string& n, std::vector<int64_t> shp) -> Tensor* {
    auto it = h->w.find(n);
    if (it == h->w.end()) { fail(CS_ERR_STATE, "missing key %s", n.c_str()); return nullptr; }
    if (it->second.shape != shp) {
      std::string got, want;
      for (auto v : it->second.shape) got += std::to_string(v) + ",";
      for (auto v : shp) want += std::to_string(v) + ",";
      fail(CS_ERR_BAD_ARG, "size mismatch for %s: got (%s) expected (%s)", n.c_str(), got.c_str(), want.c_str());
      return nullptr;
    }
    return &it->second;
  };
  hipStream_t st = nullptr;
  auto pack = [&](const float* src, int rows, int K, int ldo, h16_t* dst, const float* row_scale = nullptr,
                  const float* col_scale = nullptr) -> int {
    HIPCHK(cs_pack_f16_launch(src, rows, K, dst, ldo, row_scale, col_scale, c.operand_dtype, st));
    return 0;
  };
  auto alloc_bf = [&](size_t n) -> h16_t* { void* p = nullptr; if (hipMalloc(&p, n * sizeof(h16_t)) != hipSuccess) return nullptr; h->owned.push_back(p); return (h16_t*)p; };
  auto alloc_f = [&](size_t n) -> float* { void* p = nullptr; if (hipMalloc(&p, n * sizeof(float)) != hipSuccess) return nullptr; h->owned.push_back(p); return (float*)p; };
#define NEED(var, name, ...) Tensor* var = need(name, {__VA_ARGS__}); if (!var) return CS_ERR_STATE;
#define ALLOC_BF(var, n) h16_t* var = alloc_bf(n); if (!var) return fail(CS_ERR_HIP, "hipMalloc failed");
#define ALLOC_F(var, n) float* var = alloc_f(n); if (!var) return fail(CS_ERR_HIP, "hipMalloc failed");
#define D2D(dst, src, n) HIPCHK(hipMemcpy(dst, src, (n) * sizeof(float), hipMemcpyDeviceToDevice))

  const std::string e = "backbone.embeddings.";
  NEED(t_ms, "img_mean_std", 6) (void)t_ms;
  NEED(t_cls, e + "cls_token", 1, 1, C)
  NEED(t_mask, e + "mask_token", 1, C) (void)t_mask;
  NEED(t_pos, e + "position_embeddings", 1, (int64_t)c.pos_grid * c.pos_grid + 1, C)
  NEED(t_pw, e + "patch_embeddings.projection.weight", C, 3, P, P)
  NEED(t_pb, e + "patch_embeddings.projection.bias", C)
  h->cls = t_cls->d; h->pos = t_pos->d; h->bpatch = t_pb->d;
  { ALLOC_BF(wp, (size_t)C * h->Kp) if (int r = pack(t_pw->d, (int)C, (int)(3 * P * P), h->Kp, wp)) return r; h->Wpatch = wp; }
  { ALLOC_F(ws, (size_t)3 * C) HIPCHK(cs_patch_wsum_launch(t_pw->d, (int)C, (int)P, ws, st)); h->wsum = ws; }
  if (P == 14 && C % 384 == 0) {
    ALLOC_BF(wf, cs_patch_pack_elems((int)C))
    HIPCHK(cs_patch_pack_launch(t_pw->d, (int)C, wf, c.operand_dtype, st));
    h->Wpatch_frag = wf;
  }
  // softmax scale folded into the Q projections: the attention kernel takes Q pre-multiplied by log2(e)/sqrt(dh) (scale_log2e = 1),
  // so the factor is applied to the fp32 weights and biases before their single fp16 rounding instead of to fp16 Q values
  ALLOC_F(qs_enc, (size_t)C) ALLOC_F(qs_dec, (size_t)C)
  {
    std::vector<float> hv((size_t)C, LOG2E / std::sqrt((float)(C / c.enc_heads)));
    HIPCHK(hipMemcpy(qs_enc, hv.data(), (size_t)C * sizeof(float), hipMemcpyHostToDevice));
    std::fill(hv.begin(), hv.end(), LOG2E / std::sqrt((float)(C / c.dec_heads)));
    HIPCHK(hipMemcpy(qs_dec, hv.data(), (size_t)C * sizeof(float), hipMemcpyHostToDevice));
    h->qs_dec = qs_dec;
  }
  h->enc.resize(c.enc_layers);
  for (int l = 0; l < c.enc_layers; ++l) {
    const std::string p = "backbone.encoder.layer." + std::to_string(l) + ".";
    EncLayer& L = h->enc[l];
    NEED(n1w, p + "norm1.weight", C) NEED(n1b, p + "norm1.bias", C) NEED(n2w, p + "norm2.weight", C) NEED(n2b, p + "norm2.bias", C)
    NEED(qw, p + "attention.attention.query.weight", C, C) NEED(qb, p + "attention.attention.query.bias", C)
    NEED(kw, p + "attention.attention.key.weight", C, C) NEED(kb, p + "attention.attention.key.bias", C)
    NEED(vw, p + "attention.attention.value.weight", C, C) NEED(vb, p + "attention.attention.value.bias", C)
    NEED(ow, p + "attention.output.dense.weight", C, C) NEED(ob, p + "attention.output.dense.bias", C)
    NEED(l1, p + "layer_scale1.lambda1", C) NEED(l2, p + "layer_scale2.lambda1", C)
    NEED(f1w, p + (c.swiglu ? "mlp.weights_in.weight" : "mlp.fc1.weight"), F1, C) NEED(f1b, p + (c.swiglu ? "mlp.weights_in.bias" : "mlp.fc1.bias"), F1)
    NEED(f2w, p + (c.swiglu ? "mlp.weights_out.weight" : "mlp.fc2.weight"), C, F) NEED(f2b, p + (c.swiglu ? "mlp.weights_out.bias" : "mlp.fc2.bias"), C)
    L.ln1g = n1w->d; L.ln1b = n1b->d; L.ln2g = n2w->d; L.ln2b = n2b->d; L.b1 = f1b->d;
    // LayerScale (x += lambda * (a Wo^T + bo), HF:367-370,376-378) is folded into the projection: rows of Wo / W2 and the
    // biases are scaled by lambda once, so the GEMM epilogue is a plain residual add
    ALLOC_F(bo_s, (size_t)C) ALLOC_F(b2_s, (size_t)C)
    HIPCHK(cs_vec_mul_launch(ob->d, l1->d, bo_s, (int)C, st));
    HIPCHK(cs_vec_mul_launch(f2b->d, l2->d, b2_s, (int)C, st));
    L.bo = bo_s; L.b2 = b2_s;
    const size_t NQ = (size_t)h->qkv_n;  // >= 3C: the padding rows of the weights and the padding entries of the bias / fold vectors are zero
    ALLOC_BF(wqkv, NQ * C) ALLOC_F(bqkv, NQ)
    if (NQ > 3 * C) { HIPCHK(hipMemset(wqkv + 3 * C * C, 0, (NQ - 3 * C) * C * sizeof(h16_t))); HIPCHK(hipMemset(bqkv + 3 * C, 0, (NQ - 3 * C) * sizeof(float))); }
    const bool fold = h->lnfold || h->panel || h->fold256;
    const float* g1 = fold ? n1w->d : nullptr;  // LayerNorm gamma folded into the columns of the consuming projection
    const float* g2 = fold ? n2w->d : nullptr;
    if (int r = pack(qw->d, (int)C, (int)C, (int)C, wqkv, qs_enc, g1)) return r;
    if (int r = pack(kw->d, (int)C, (int)C, (int)C, wqkv + C * C, nullptr, g1)) return r;
    if (int r = pack(vw->d, (int)C, (int)C, (int)C, wqkv + 2 * C * C, nullptr, g1)) return r;
    HIPCHK(cs_vec_mul_launch(qb->d, qs_enc, bqkv, (int)C, st));
    D2D(bqkv + C, kb->d, C); D2D(bqkv + 2 * C, vb->d, C);
    ALLOC_BF(wo, (size_t)C * C) ALLOC_BF(w1, (size_t)F1 * C) ALLOC_BF(w2, (size_t)C * F)
    if (int r = pack(ow->d, (int)C, (int)C, (int)C, wo, l1->d)) return r;
    if (int r = pack(f1w->d, (int)F1, (int)C, (int)C, w1, nullptr, g2)) return r;
    if (int r = pack(f2w->d, (int)C, (int)F, (int)F, w2, l2->d)) return r;
    L.Wqkv = wqkv; L.bqkv = bqkv; L.Wo = wo; L.W1 = w1; L.W2 = w2;
    L.s_qkv = L.c_qkv = L.s_1 = L.c_1 = nullptr;
    L.panel_img = nullptr;
    if (h->panel) {
      ALLOC_BF(img, (h->panel_impl ? cs_panel4_image_bytes(1) : cs_panel8_image_bytes(1)) / sizeof(h16_t))
      if (h->panel_impl) HIPCHK(cs_panel4_pack_launch(ow->d, l1->d, f1w->d, n2w->d, f2w->d, l2->d, img, c.operand_dtype, st));
      else HIPCHK(cs_panel_pack_launch(ow->d, l1->d, f1w->d, n2w->d, f2w->d, l2->d, img, c.operand_dtype, st));
      L.panel_img = img;
    }
    if (fold) {
      ALLOC_F(sq, NQ) ALLOC_F(cq, NQ) ALLOC_F(s1v, (size_t)F) ALLOC_F(c1v, (size_t)F)
      if (NQ > 3 * C) { HIPCHK(hipMemset(sq + 3 * C, 0, (NQ - 3 * C) * sizeof(float))); HIPCHK(hipMemset(cq + 3 * C, 0, (NQ - 3 * C) * sizeof(float))); }
      const float* wsrc[3] = {qw->d, kw->d, vw->d};
      const float* bsrc[3] = {qb->d, kb->d, vb->d};
      for (int part = 0; part < 3; ++part)
        HIPCHK(cs_ln_fold_consts_launch(wqkv + (size_t)part * C * C, (int)C, wsrc[part], n1b->d, bsrc[part], (int)C, (int)C,
                                        sq + part * C, cq + part * C, c.operand_dtype, st));
      HIPCHK(cs_vec_mul_launch(cq, qs_enc, cq, (int)C, st));  // c = b + W beta of the Q rows carries the softmax scale too
      HIPCHK(cs_ln_fold_consts_launch(w1, (int)C, f1w->d, n2b->d, f1b->d, (int)F, (int)C, s1v, c1v, c.operand_dtype, st));
      L.s_qkv = sq; L.c_qkv = cq; L.s_1 = s1v; L.c_1 = c1v;
    }
  }
  { NEED(g, "backbone.layernorm.weight", C) NEED(b, "backbone.layernorm.bias", C) h->lnfg = g->d; h->lnfb = b->d; }
  if (h->panel || h->fold256) {
    ALLOC_F(on, (size_t)C) ALLOC_F(ze, (size_t)C)
    std::vector<float> hv((size_t)C, 1.0f);
    HIPCHK(hipMemcpy(on, hv.data(), (size_t)C * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(ze, 0, (size_t)C * sizeof(float)));
    h->ones = on; h->zeros = ze;
  }
  { NEED(pe, "pos_enc_fn.PE", 1, c.pe_h, c.pe_w, C) h->pe = pe->d; }
  h->dec.resize(c.dec_layers);
  { ALLOC_BF(wkv, (size_t)c.dec_layers * 2 * C * C) ALLOC_F(bkv, (size_t)c.dec_layers * 2 * C) h->Wkv_all = wkv; h->bkv_all = bkv; }
  for (int l = 0; l < c.dec_layers; ++l) {
    const std::string p = "ref_cross.attn.layers." + std::to_string(l) + ".";
    DecLayer& L = h->dec[l];
    std::memset(&L, 0, sizeof L);
    if (c.do_self_attn) {
      NEED(iw, p + "self_attn.in_proj_weight", 3 * C, C) NEED(ib, p + "self_attn.in_proj_bias", 3 * C)
      NEED(ow, p + "self_attn.out_proj.weight", C, C) NEED(ob, p + "self_attn.out_proj.bias", C)
      ALLOC_BF(w, (size_t)3 * C * C) ALLOC_F(bin, (size_t)3 * C)
      if (int r = pack(iw->d, (int)C, (int)C, (int)C, w, qs_dec)) return r;
      if (int r = pack(iw->d + C * C, (int)(2 * C), (int)C, (int)C, w + C * C)) return r;
      HIPCHK(cs_vec_mul_launch(ib->d, qs_dec, bin, (int)C, st));
      D2D(bin + C, ib->d + C, 2 * C);
      ALLOC_BF(wo, (size_t)C * C) if (int r = pack(ow->d, (int)C, (int)C, (int)C, wo)) return r;
      L.sa_Win = w; L.sa_bin = bin; L.sa_Wo = wo; L.sa_bo = ob->d;
    }
    NEED(iw, p + "multihead_attn.in_proj_weight", 3 * C, C) NEED(ib, p + "multihead_attn.in_proj_bias", 3 * C)
    NEED(ow, p + "multihead_attn.out_proj.weight", C, C) NEED(ob, p + "multihead_attn.out_proj.bias", C)
    ALLOC_BF(wq, (size_t)C * C) ALLOC_F(bq, (size_t)C)
    if (int r = pack(iw->d, (int)C, (int)C, (int)C, wq, qs_dec)) return r;
    HIPCHK(cs_vec_mul_launch(ib->d, qs_dec, bq, (int)C, st));
    // rows [C:3C) = [Wk;Wv] of this layer -> rows [l*2C, (l+1)*2C) of the fused KV projection (same memory for both layers)
    if (int r = pack(iw->d + C * C, (int)(2 * C), (int)C, (int)C, h->Wkv_all + (size_t)l * 2 * C * C)) return r;
    D2D(h->bkv_all + (size_t)l * 2 * C, ib->d + C, 2 * C);
    ALLOC_BF(wo, (size_t)C * C) if (int r = pack(ow->d, (int)C, (int)C, (int)C, wo)) return r;
    L.ca_Wq = wq; L.ca_bq = bq; L.ca_Wo = wo; L.ca_bo = ob->d;
    NEED(l1w, p + "linear1.weight", C, C) NEED(l1b, p + "linear1.bias", C) NEED(l2w, p + "linear2.weight", C, C) NEED(l2b, p + "linear2.bias", C)
    ALLOC_BF(w1, (size_t)C * C) if (int r = pack(l1w->d, (int)C, (int)C, (int)C, w1)) return r;
    ALLOC_BF(w2, (size_t)C * C) if (int r = pack(l2w->d, (int)C, (int)C, (int)C, w2)) return r;
    L.l1W = w1; L.l1b = l1b->d; L.l2W = w2; L.l2b = l2b->d;
    NEED(n1g, p + "norm1.weight", C) NEED(n1b, p + "norm1.bias", C) NEED(n2g, p + "norm2.weight", C) NEED(n2b, p + "norm2.bias", C)
    NEED(n3g, p + "norm3.weight", C) NEED(n3b, p + "norm3.bias", C)
    L.n1g = n1g->d; L.n1b = n1b->d; L.n2g = n2g->d; L.n2b = n2b->d; L.n3g = n3g->d; L.n3b = n3b->d;
  }
  {
    const int64_t PP = P * P;
    NEED(h0w, "ref_cross.head.0.weight", C, C) NEED(h0b, "ref_cross.head.0.bias", C)
    NEED(h2w, "ref_cross.head.2.weight", PP, C) NEED(h2b, "ref_cross.head.2.bias", PP)
    ALLOC_BF(w0, (size_t)C * C) if (int r = pack(h0w->d, (int)C, (int)C, (int)C, w0)) return r;
    ALLOC_BF(w2, (size_t)PP * C) if (int r = pack(h2w->d, (int)PP, (int)C, (int)C, w2)) return r;
    h->Wh0 = w0; h->bh0 = h0b->d; h->Wh2 = w2; h->bh2 = h2b->d;
  }
  if (!h->nonfinite) {
    HIPCHK(hipMalloc(&h->nonfinite, 16));
    HIPCHK(hipMemset(h->nonfinite, 0, 16));
  }
  HIPCHK(hipDeviceSynchronize());
  // fp32 copies of the big matrices are no longer needed
  for (auto& kv : h->w) {
    const std::string& n = kv.first;
    const bool big = kv.second.shape.size() >= 2 && n.find("weight") != std::string::npos && n.find("norm") == std::string::npos;
    if (big && kv.second.d) { hipFree(kv.second.d); kv.second.d = nullptr; }
  }
  h->finalized = true;
  return 0;
}

// What the last forward-class call on this handle launched, and what it cost the host: `launches` = kernel launches (memcpy taps of capture
// mode not counted; the two copies of cs_fit_tail_keep counted as tail_keep=2, the one more of cs_fit_cross_keep as cross_keep=1, the two more of cs_fit_layer_keep as layer_keep=2), `host_ms` = wall time of the call on the calling thread (everything is enqueued, nothing waited for), `names` (optional,
// `names_bytes` long) = "kernel=count kernel=count ..." by kernel: gemm256 / gemm128 (cs_gemm256_kernel / cs_gemm_kernel), attn<dh>, panel,
// rowln, patch, im2col, ln1 / ln2 / ln (layernorm_kernel), cls, final_ln, score_check, ...
int cs_forward_stats(cs_handle h, int* launches, double* host_ms, char* names, size_t names_bytes) {
  if (!h) return fail(CS_ERR_BAD_ARG, "null handle");
  int n = 0;
  std::string txt;
  for (const auto& kv : h->census) { n += kv.second; txt += (txt.empty() ? "" : " ") + kv.first + "=" + std::to_string(kv.second); }
  if (launches) *launches = n;
  if (host_ms) *host_ms = h->host_enqueue_ms;
  if (names && names_bytes) { std::strncpy(names, txt.c_str(), names_bytes - 1); names[names_bytes - 1] = 0; }
  return 0;
}

// Debug taps for the stage-level parity tests: with capture on, every forward also copies its intermediate tensors (stream-ordered
// device-to-device copies into library-owned buffers): "embeddings", "enc_layer_<l>" (fp32 [I][T][C], images in the reference's
// batch-major (query, refs) order), "featmap_query" (fp32 [B][Np][C]), "featmap_ref" (16 bit [B][N*Np][C]), "dec<l>_out" (fp32
// [B][Np][C]), "head_pre_activation" (fp32 [B][Np][P*P]).  Not for timed runs: the first captured forward of a shape allocates.
int cs_debug_capture(cs_handle h, int on) {
  if (!h) return fail(CS_ERR_BAD_ARG, "null handle");
  h->capture = on != 0;
  return 0;
}

// Copies tap `name` of the last captured forward to `dst` (device memory, dst_bytes >= the tap's size) on `stream`; reports its element
// type (CS_DTYPE_*), rank and shape.  dst == NULL: only reports.  CS_ERR_STATE when no forward has captured that tap.
int cs_debug_read(cs_handle h, const char* name, void* dst, size_t dst_bytes, int* dtype, int* ndim, int64_t* shape4, cs_stream stream) {
  if (!h || !name) return fail(CS_ERR_BAD_ARG, "null argument");
  auto it = h->taps.find(name);
  if (it == h->taps.end() || !it->second.d) return fail(CS_ERR_STATE, "no tap named '%s' was captured (cs_debug_capture before the forward?)", name);
  const cs_model::Tap& t = it->second;
  if (dtype) *dtype = t.dtype;
  if (ndim) *ndim = t.ndim;
  if (shape4) for (int k = 0; k < 4; ++k) shape4[k] = t.shape[k];
  if (!dst) return 0;
  if (dst_bytes < t.bytes) return fail(CS_ERR_BAD_ARG, "tap '%s' holds %zu bytes, destination %zu", name, t.bytes, dst_bytes);
  hipStream_t st = (hipStream_t)stream;
  if (int r = call_enter(h, st)) return r;
  HIPCHK(hipMemcpyAsync(dst, t.d, t.bytes, hipMemcpyDeviceToDevice, st));
  return 0;
}

int cs_profile_enable(cs_handle h, int on) {
  if (!h) return fail(CS_ERR_BAD_ARG, "null handle");
  hipDeviceSynchronize();
  for (auto& r : h->recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
  h->recs.clear();
  h->prof = on != 0;
  return 0;
}

// Lanes of the following forwards: 0 = as configured (cs_config.lanes), n >= 1 = at most n.  Same launches either way (score maps are
// bit-identical); for CrossScoreNet.calibrate_lanes, which times the two-lane forward against the one-lane one on the same handle.
int cs_set_lanes(cs_handle h, int lanes) {
  if (!h || lanes < 0 || lanes > CS_MAX_LANES) return fail(CS_ERR_BAD_ARG, "cs_set_lanes: bad arguments");
  h->lanes_now = lanes;
  return 0;
}

// Gives the handle's lane streams back; the next forward draws new ones (and probes them, cs_forward).  A set-up call: waits for the
// lanes' work.  The remedy when a two-lane forward turns out not to overlap although its streams passed the probe.
int cs_redraw_lane_streams(cs_handle h) {
  if (!h) return fail(CS_ERR_BAD_ARG, "null handle");
  for (int l = 0; l < CS_MAX_LANES; ++l)
    if (h->lane_st[l]) {
      HIPCHK(hipStreamSynchronize(h->lane_st[l]));
      // kept alive until the next forward has created the replacements: a stream destroyed now would hand its hardware queue
      // straight back to the very next hipStreamCreate
      h->lane_st_old.push_back(h->lane_st[l]);
      h->lane_st[l] = nullptr;
    }
  return 0;
}

int cs_profile_read_bytes(cs_handle h, int family, double* bytes) {
  if (!h || !bytes) return fail(CS_ERR_BAD_ARG, "null argument");
  double b = 0;
  for (auto& r : h->recs)
    if (r.family == family) b += r.bytes;
  *bytes = b;
  return 0;
}

int cs_profile_read(cs_handle h, int family, double* total_ms, int* launches, double* flops) {
  if (!h) return fail(CS_ERR_BAD_ARG, "null handle");
  HIPCHK(hipDeviceSynchronize());
  double ms = 0, fl = 0; int n = 0;
  for (auto& r : h->recs) {
    if (r.family != family) continue;
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, r.a, r.b));
    ms += t; fl += r.flops; ++n;
  }
  if (total_ms) *total_ms = ms;
  if (launches) *launches = n;
  if (flops) *flops = fl;
  return 0;
}

// Non-finite values the score maps of this handle's forwards held since the last call (and resets the count).  Waits for the handle's
// last forward (an explicit check, not part of the hot loop): an fp16 operand that overflowed upstream reaches the output as NaN.
int cs_nonfinite_count(cs_handle h, long long* count) {
  if (!h || !count) return fail(CS_ERR_BAD_ARG, "null argument");
  *count = 0;
  if (!h->nonfinite) return 0;
  if (h->ev_done) HIPCHK(hipEventSynchronize(h->ev_done));
  unsigned v = 0;
  HIPCHK(hipMemcpy(&v, h->nonfinite, sizeof v, hipMemcpyDeviceToHost));
  if (v) HIPCHK(hipMemset(h->nonfinite, 0, sizeof v));
  *count = (long long)v;
  return 0;
}

// ---- process-wide debug switches ----
void cs_debug_stream_probe_log(int on) { g_debug_stream_log = on; }
void cs_debug_rowln_enable(int on) { g_rowln_off = on == 0 ? 1 : 0; g_rowln_no_next = on == 2 ? 1 : 0; }
void cs_debug_panel_impl(int impl) { g_panel_impl = impl ? 1 : 0; }

// Head fit: changed head weights back into the finalised handle.  The four fp32 device arrays are re-packed into the buffers
// cs_finalize allocated (Wh0 / Wh2 in the handle's operand type, the biases in fp32), on `stream`, behind the handle's last call.
int cs_set_head_weights(cs_handle h, const float* w0, const float* b0, const float* w2, const float* b2, cs_stream stream) {
  if (!h) return fail(CS_ERR_BAD_ARG, "null handle");
  if (!h->finalized) return fail(CS_ERR_STATE, "cs_set_head_weights before cs_finalize");
  if (!w0 || !b0 || !w2 || !b2) return fail(CS_ERR_BAD_ARG, "cs_set_head_weights: null pointer");
  if (((uintptr_t)w0 | (uintptr_t)b0 | (uintptr_t)w2 | (uintptr_t)b2) & 3) return fail(CS_ERR_BAD_ARG, "cs_set_head_weights: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  const int C = h->cfg.hidden, PP = h->cfg.patch * h->cfg.patch;
  if (int r = call_enter(h, st)) return r;
  HIPCHK(cs_pack_f16_launch(w0, C, C, h->Wh0, C, nullptr, nullptr, h->cfg.operand_dtype, st));
  HIPCHK(cs_pack_f16_launch(w2, PP, C, h->Wh2, C, nullptr, nullptr, h->cfg.operand_dtype, st));
  HIPCHK(hipMemcpyAsync(h->bh0, b0, (size_t)C * 4, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(h->bh2, b2, (size_t)PP * 4, hipMemcpyDeviceToDevice, st));
  return call_leave(h, st);
}

// Tail fit: a persistent switch like cs_debug_capture, off by default.  With it on, every forward that runs the decoder
// keeps the last layer's norm2 output and its ReLU rows (two stream-ordered copies) for cs_tail_backward; nothing else of the forward changes.
int cs_fit_tail_keep(cs_handle h, int on) {
  if (!h) return fail(CS_ERR_BAD_ARG, "null handle");
  h->tail_keep = on != 0;
  return 0;
}

// The six changed tensors of the last decoder layer's feed-forward block and norm3 back into the finalised handle: w1 / w2 (C, C) re-packed into
// the layer's existing operand buffers, the biases and norm3's weight and bias copied, on `stream`, behind the handle's last call.
int cs_set_tail_weights(cs_handle h, const float* w1, const float* b1, const float* w2, const float* b2, const float* g3, const float* b3,
                        cs_stream stream) {
  if (!h) return fail(CS_ERR_BAD_ARG, "null handle");
  if (!h->finalized) return fail(CS_ERR_STATE, "cs_set_tail_weights before cs_finalize");
  if (h->dec.empty()) return fail(CS_ERR_STATE, "cs_set_tail_weights: the handle has no decoder layer");
  if (!w1 || !b1 || !w2 || !b2 || !g3 || !b3) return fail(CS_ERR_BAD_ARG, "cs_set_tail_weights: null pointer");
  if (((uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)w2 | (uintptr_t)b2 | (uintptr_t)g3 | (uintptr_t)b3) & 3) return fail(CS_ERR_BAD_ARG, "cs_set_tail_weights: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  const int C = h->cfg.hidden;
  const DecLayer& D = h->dec.back();
  if (int r = call_enter(h, st)) return r;
  HIPCHK(cs_pack_f16_launch(w1, C, C, D.l1W, C, nullptr, nullptr, h->cfg.operand_dtype, st));
  HIPCHK(cs_pack_f16_launch(w2, C, C, D.l2W, C, nullptr, nullptr, h->cfg.operand_dtype, st));
  HIPCHK(hipMemcpyAsync(D.l1b, b1, (size_t)C * 4, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(D.l2b, b2, (size_t)C * 4, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(D.n3g, g3, (size_t)C * 4, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(D.n3b, b3, (size_t)C * 4, hipMemcpyDeviceToDevice, st));
  return call_leave(h, st);
}

// Cross-attention fit: a persistent switch that implies cs_fit_tail_keep's copies; in addition the last layer's cross-attention
// writes its lse and x1 is copied in front of the norm2 closing.  Nothing else of the forward changes.
int cs_fit_cross_keep(cs_handle h, int on) {
  if (!h) return fail(CS_ERR_BAD_ARG, "null handle");
  h->cross_keep = on != 0;
  return 0;
}

// The six changed tensors of the last decoder layer's cross-attention block back into the finalised handle, exactly as cs_finalize packs them:
// rows [0, C) of in_proj into ca_Wq / ca_bq with log2(e) / sqrt(dh) folded in, rows [C, 3C) into the layer's 2C rows of the fused K | V
// projection, out_proj re-packed, its bias and norm2 copied; on `stream`, behind the handle's last call.
int cs_set_cross_weights(cs_handle h, const float* in_w, const float* in_b, const float* out_w, const float* out_b, const float* g2, const float* b2,
                         cs_stream stream) {
  if (!h) return fail(CS_ERR_BAD_ARG, "null handle");
  if (!h->finalized) return fail(CS_ERR_STATE, "cs_set_cross_weights before cs_finalize");
  if (h->dec.empty()) return fail(CS_ERR_STATE, "cs_set_cross_weights: the handle has no decoder layer");
  if (!in_w || !in_b || !out_w || !out_b || !g2 || !b2) return fail(CS_ERR_BAD_ARG, "cs_set_cross_weights: null pointer");
  if (((uintptr_t)in_w | (uintptr_t)in_b | (uintptr_t)out_w | (uintptr_t)out_b | (uintptr_t)g2 | (uintptr_t)b2) & 3) return fail(CS_ERR_BAD_ARG, "cs_set_cross_weights: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  const size_t C = h->cfg.hidden, l = h->dec.size() - 1;
  const int bf = h->cfg.operand_dtype;
  const DecLayer& D = h->dec.back();
  if (int r = call_enter(h, st)) return r;
  HIPCHK(cs_pack_f16_launch(in_w, (int)C, (int)C, D.ca_Wq, (int)C, h->qs_dec, nullptr, bf, st));
  HIPCHK(cs_vec_mul_launch(in_b, h->qs_dec, D.ca_bq, (int)C, st));
  HIPCHK(cs_pack_f16_launch(in_w + C * C, (int)(2 * C), (int)C, h->Wkv_all + l * 2 * C * C, (int)C, nullptr, nullptr, bf, st));
  HIPCHK(hipMemcpyAsync(h->bkv_all + l * 2 * C, in_b + C, 2 * C * 4, hipMemcpyDeviceToDevice, st));
  HIPCHK(cs_pack_f16_launch(out_w, (int)C, (int)C, D.ca_Wo, (int)C, nullptr, nullptr, bf, st));
  HIPCHK(hipMemcpyAsync(D.ca_bo, out_b, C * 4, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(D.n2g, g2, C * 4, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(D.n2b, b2, C * 4, hipMemcpyDeviceToDevice, st));
  return call_leave(h, st);
}

// Whole-layer fit: a persistent switch that implies cs_fit_cross_keep's (and with it cs_fit_tail_keep's) copies; in addition the
// last layer's self-attention writes its lse into the handle's region, and x0 and Os are copied there in front of the launches that overwrite them.
// Nothing else of the forward changes.
int cs_fit_layer_keep(cs_handle h, int on) {
  if (!h) return fail(CS_ERR_BAD_ARG, "null handle");
  h->layer_keep = on != 0;
  return 0;
}

// The six changed tensors of the last decoder layer's self-attention block back into the finalised handle, exactly as cs_finalize packs them: rows
// [0, C) of in_proj into sa_Win / sa_bin with log2(e) / sqrt(dh) folded in, rows [C, 3C) behind them unscaled, out_proj re-packed, its bias and
// norm1 copied -- the buffers both the GEMM path and the row-complete kernel read; on `stream`, behind the handle's last call.
int cs_set_layer_weights(cs_handle h, const float* in_w, const float* in_b, const float* out_w, const float* out_b, const float* g1, const float* b1,
                         cs_stream stream) {
  if (!h) return fail(CS_ERR_BAD_ARG, "null handle");
  if (!h->finalized) return fail(CS_ERR_STATE, "cs_set_layer_weights before cs_finalize");
  if (h->dec.empty()) return fail(CS_ERR_STATE, "cs_set_layer_weights: the handle has no decoder layer");
  if (!h->cfg.do_self_attn) return fail(CS_ERR_UNSUPPORTED, "cs_set_layer_weights: the decoder has no self-attention (decoder_do_self_attn = 0)");
  if (!in_w || !in_b || !out_w || !out_b || !g1 || !b1) return fail(CS_ERR_BAD_ARG, "cs_set_layer_weights: null pointer");
  if (((uintptr_t)in_w | (uintptr_t)in_b | (uintptr_t)out_w | (uintptr_t)out_b | (uintptr_t)g1 | (uintptr_t)b1) & 3) return fail(CS_ERR_BAD_ARG, "cs_set_layer_weights: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  const size_t C = h->cfg.hidden;
  const int bf = h->cfg.operand_dtype;
  const DecLayer& D = h->dec.back();
  if (int r = call_enter(h, st)) return r;
  HIPCHK(cs_pack_f16_launch(in_w, (int)C, (int)C, D.sa_Win, (int)C, h->qs_dec, nullptr, bf, st));
  HIPCHK(cs_pack_f16_launch(in_w + C * C, (int)(2 * C), (int)C, D.sa_Win + C * C, (int)C, nullptr, nullptr, bf, st));
  HIPCHK(cs_vec_mul_launch(in_b, h->qs_dec, D.sa_bin, (int)C, st));
  HIPCHK(hipMemcpyAsync(D.sa_bin + C, in_b + C, 2 * C * 4, hipMemcpyDeviceToDevice, st));
  HIPCHK(cs_pack_f16_launch(out_w, (int)C, (int)C, D.sa_Wo, (int)C, nullptr, nullptr, bf, st));
  HIPCHK(hipMemcpyAsync(D.sa_bo, out_b, C * 4, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(D.n1g, g1, C * 4, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(D.n1b, b1, C * 4, hipMemcpyDeviceToDevice, st));
  return call_leave(h, st);
}

int cs_debug_set_op_operand_dtype(int dtype) {
  if (dtype != 0 && dtype != 1) return fail(CS_ERR_BAD_ARG, "operand dtype must be 0 (fp16) or 1 (bf16)");
  g_op_bf16 = dtype;
  return 0;
}

}  // extern "C"
