// What the four host files share: api.hip (handle life cycle, weights, accessors), forward.hip (plan + the forward's steps), ops.hip
// (single-op entry points) and fit_host.hip (the fit scopes' checks, operators and backwards on a handle).  The handle, its packed layers, the
// workspace plan, the launch helper that keeps the census / profile records, and the library's one error slot.  Host-side only; no kernel file
// includes this.
#pragma once
#include "../../include/crossscore_hip.h"
#include "cs_common.h"
#include "fit_shared.h"

#include <algorithm>
#include <map>
#include <string>
#include <vector>

// (everything but the handle itself sits in a namespace: the library is loaded into processes that carry many other C++ libraries)
namespace cs_host {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int CS_MAX_LANES = 4;

// api.hip: records the message cs_last_error returns (ONE thread-local for the whole library) and hands `code` back
int fail(int code, const char* fmt, ...);
#define HIPCHK(expr)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) return fail(CS_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// process-wide debug switches (api.hip)
extern int g_debug_stream_log;  // cs_debug_stream_probe_log: one stderr line per lane-stream candidate of the overlap probe
extern int g_panel_impl;        // cs_debug_panel_impl: which token-panel kernel new handles and the cs_op_panel_* entry points use: 0 = panel.hip (8 waves), 1 = panel4.hip (4 waves)
extern int g_rowln_off;         // cs_debug_rowln_enable(0): the decoder goes back to GEMM + LayerNorm launches (A/B runs and tests)
extern int g_rowln_no_next;     // cs_debug_rowln_enable(2): linear + LayerNorm in one launch, the following linear as a GEMM of its own (round 4's first form)
extern int g_op_bf16;           // operand type of the cs_op_* entry points (a handle carries its own: cs_config.operand_dtype)

struct Tensor {
  std::vector<int64_t> shape;
  float* d = nullptr;
  size_t numel = 0;
};

struct EncLayer {
  float *ln1g, *ln1b, *ln2g, *ln2b, *bqkv, *bo, *b1, *b2;
  h16_t *Wqkv, *Wo, *W1, *W2;
  // LayerNorm fold (CS_EPI_LN_*): Wqkv / W1 above are then the gamma-scaled versions and these hold s[n], c[n]
  float *s_qkv, *c_qkv, *s_1, *c_1;
  h16_t* panel_img;  // token-panel kernel (panel.hip): packed unit stream [Wo | W1 / W2 interleaved]; Wqkv / c_qkv / c_1 are then the LN-folded ones
};
struct DecLayer {
  float *sa_bin, *sa_bo, *ca_bq, *ca_bo, *l1b, *l2b, *n1g, *n1b, *n2g, *n2b, *n3g, *n3b;
  h16_t *sa_Win, *sa_Wo, *ca_Wq, *ca_Wo, *l1W, *l2W;
};

struct ProfRec { hipEvent_t a, b; int family; double flops; double bytes; };

// Small host arrays on their way to the device (the grouped selection's offsets and per-query triples): a ring of pinned buffers, each reused
// only behind the event recorded after its asynchronous copy -- the copy of SLOTS calls ago, long done -- so that no call waits for its own.
// A slot can also own device memory: where the copy lands, and scratch of the kernels that read it (the single-op entry points have no
// workspace); its event is then recorded behind those kernels.
struct StageRing {
  static constexpr int SLOTS = 4;
  struct Slot { void* host = nullptr; void* dev = nullptr; size_t cap = 0, dev_cap = 0; int device = -1; hipEvent_t ev = nullptr; bool used = false; };
  Slot slot[SLOTS];
  int next = 0;
};
int stage_take(StageRing& r, size_t bytes, size_t dev_bytes, StageRing::Slot** out);  // forward.hip
void stage_free(StageRing& r);

}  // namespace cs_host
using namespace cs_host;

struct cs_model {
  cs_config cfg{};
  std::vector<std::string> names;
  std::map<std::string, Tensor> w;
  bool finalized = false;
  int Kp = 0;  // padded patch K
  int qkv_n = 0;  // columns of the encoder's packed QKV projection: 3C, or 3C padded to whole 256-column tiles (zero rows) when that lets the
                  // large-tile GEMM take it (ViT-S: 1152 -> 1280; measured 47.5 -> 36.9 us per 24-image chunk, r4); attention reads with this stride
  // launch census of the last forward (cs_forward_stats): kernel launches by kernel, and the host time the call spent enqueueing them
  std::map<std::string, int> census;
  double host_enqueue_ms = 0.0;
  int panel_impl = 0;   // which panel kernel the images of this handle were packed for (g_panel_impl at cs_finalize)
  bool panel = false;   // encoder layers run as QKV GEMM + attention + ONE token-panel kernel (panel.hip; hidden == 384 only)
  float *ones = nullptr, *zeros = nullptr;  // [C]: layer 0's norm1 without gamma/beta (they are folded into its QKV projection)
  bool lnfold = false;  // encoder LayerNorms folded into the QKV / fc1 projections (no separate LN pass)
  bool fold256 = false; // the same fold on the 256-tile GEMM (gemm256.hip LN = 1 / 2; r5): the default of the wide backbones (hidden 768 / 1024) for chunks of >= 256 rows
  int ln_sp = 0;        // partial-sum slots per row the producing epilogues write (4 per column tile)
  std::vector<void*> owned;  // device allocations of packed weights
  // packed
  h16_t* Wpatch = nullptr; float* bpatch = nullptr;
  h16_t* Wpatch_frag = nullptr;  // fragment-ordered copy for the one-launch patch embedding (patch.hip); null when C is not 384 n or P != 14
  float* wsum = nullptr;  // [3][C] fp32 sums of the patch weights per channel (mean-centred patch embedding)
  std::vector<EncLayer> enc;
  std::vector<DecLayer> dec;
  h16_t* Wkv_all = nullptr; float* bkv_all = nullptr;
  h16_t *Wh0 = nullptr, *Wh2 = nullptr; float *bh0 = nullptr, *bh2 = nullptr;
  float *lnfg = nullptr, *lnfb = nullptr, *cls = nullptr, *pos = nullptr, *pe = nullptr;
  // per-(gh,gw,square) tables: built once per shape and kept (a shape change never overwrites a table that queued work may read)
  struct Tables { int gh, gw, sq; float *pos_tab, *pe_tab; bool pos_owned, pe_owned; };
  std::vector<Tables> tables;
  float *pos_tab = nullptr, *pe_tab = nullptr;  // the current shape's (point into `tables` or at the parameters)
  // workspace; a workspace that had to grow is retired behind an event and freed once that event has completed
  void* ws = nullptr; size_t ws_bytes = 0;
  struct Retired { void* p; hipEvent_t ev; };
  std::vector<Retired> retired;
  // lanes: internal streams that run independent image chunks / batch groups concurrently (forked from and joined to
  // the caller's stream with events), so one kernel's tail and the memory-bound stages overlap another's MFMA work
  hipStream_t lane_st[CS_MAX_LANES] = {};
  // one-pass input stage: pinned host copies of the per-image descriptors of the last U8_SLOTS forwards (the upload is asynchronous; a slot is
  // reused only behind the event recorded after its copy)
  static constexpr int U8_SLOTS = 4;
  struct U8Slot { CsU8Desc* host = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool used = false; };
  U8Slot u8_slot[U8_SLOTS];
  int u8_next = 0;
  StageRing sel_ring;  // cs_forward_select_grouped: the queries' triples on their way to the workspace, staged the same way
  std::vector<hipStream_t> lane_st_old;  // given back by cs_redraw_lane_streams; destroyed once the next forward has drawn their replacements
  int lanes_now = 0;  // cs_set_lanes: lanes of the next forwards (0 = as configured)
  hipStream_t last_stream = nullptr; hipEvent_t ev_done = nullptr;  // ordering of calls that arrive on different streams
  hipEvent_t ev_kv0 = nullptr, ev_kv1 = nullptr;                    // decoder: K/V projection on a side stream
  hipEvent_t ev_fork = nullptr, ev_join[CS_MAX_LANES] = {}, ev_stag[CS_MAX_LANES] = {};
  // cs_request_reference_use: armed for the next cs_forward* call on this handle, which takes it and clears it whether it succeeds or fails
  struct RefUse {
    float* share = nullptr; float* peak_prob = nullptr; int32_t* peak_index = nullptr; float* entropy = nullptr;
    bool any() const { return share || peak_prob || peak_index || entropy; }
  };
  RefUse ref_use;
  // fitting (fit_host.hip): what the last forward-class call left behind, and the backwards' own workspace
  struct LastForward {
    bool ok = false; int mode = -1, B = 0, H = 0, W = 0; const float* xq = nullptr; const h16_t* dhid = nullptr;
    FitScope kept = FIT_HEAD;  // the deepest scope this forward kept for: fit_kept is carved at this level (cs_fit::kept_carve)
    // kept >= FIT_CROSS: the last layer's cross-attention as the forward left it in the workspace -- Q' (M, C), the layer's K block of the packed
    // K | V rows (Mk, ldkv; V is C columns further), O (M, C), lse (B, heads, Np) -- and the reference tokens its K / V projection read (Mk, C)
    int N = 0; const h16_t* dq = nullptr; const h16_t* k = nullptr; int ldkv = 0; const h16_t* dob = nullptr;
    const float* lse = nullptr; const h16_t* mem = nullptr;
    // kept >= FIT_LAYER: the last layer's packed self-attention projection rows Q' | K | V (M, 3C) where the forward left them
    const h16_t* dqkv = nullptr;
  };
  LastForward last_fwd;
  void* hfit_ws = nullptr; size_t hfit_ws_bytes = 0;  // X in 16 bits (M, C), then the workspace of the deepest scope a backward has run (cs_*_backward_workspace: each begins with its parent's)
  // The keep switches (cs_fit_tail_keep, cs_fit_cross_keep, cs_fit_layer_keep), independent of one another: a forward keeps for the deepest scope
  // whose switch is on, which implies its parents' pieces (what is copied, and when: Fwd::keep_rows in forward.hip).  All of it goes into ONE region,
  // carved by cs_fit::kept_carve (fit_shared.h) and grown like the workspace.
  bool tail_keep = false, cross_keep = false, layer_keep = false;
  void* fit_kept = nullptr; size_t fit_kept_bytes = 0;
  float* qs_dec = nullptr;  // [C] log2(e) / sqrt(dh) of the decoder: the row scale of the packed query projections (cs_set_cross_weights and cs_set_layer_weights pack with it again)
  unsigned* nonfinite = nullptr;  // device counter: non-finite score-map values seen since the last cs_nonfinite_count
  // profiling
  bool prof = false;
  std::vector<ProfRec> recs;
  // debug taps (cs_debug_capture / cs_debug_read): copies of intermediate tensors of the last forward, for the stage-level parity tests
  bool capture = false;
  struct Tap { void* d = nullptr; size_t bytes = 0; int dtype = 0; int ndim = 0; int64_t shape[4] = {0, 0, 0, 0}; };
  std::map<std::string, Tap> taps;
};

namespace cs_host {

// hidden features of the encoder's MLP: mlp_ratio * hidden, or the SwiGLU form's (int(hidden * mlp_ratio * 2 / 3) + 7) / 8 * 8 (HF modeling_dinov2.py:303-305)
inline int ffn_hidden(const cs_config& c) {
  const int f = c.mlp_ratio * c.hidden;
  return c.swiglu ? ((int)((double)f * 2 / 3) + 7) / 8 * 8 : f;
}

// the sizes cs_op_select_references and cs_forward_select take: B queries against a bank of R unit descriptors C wide, N picks per query.  The
// exclusions live on the device, so with an `exclude` array every query may carry one and only R - 1 entries count as eligible.  In the grouped
// forms N may exceed a group (the places left over are padded), so only the sizes are checked.
inline int select_check(int B, int R, int C, int N, bool grouped, bool has_exclude) {
  const char* op = grouped ? "select_references_grouped" : "select_references";
  if (B <= 0 || R <= 0 || C <= 0 || N <= 0) return fail(CS_ERR_BAD_ARG, "%s: empty batch, bank or selection", op);
  if (N > 32 || R > 65536 || C % 4 || B > 65535) return fail(CS_ERR_UNSUPPORTED, "%s: built for N <= 32, R <= 65536, C a multiple of 4 (N %d, R %d, C %d)", op, N, R, C);
  if (!grouped && N > R - (has_exclude ? 1 : 0))
    return fail(CS_ERR_BAD_ARG, "select_references: N = %d exceeds the %d eligible bank entries (R = %d%s)", N, R - (has_exclude ? 1 : 0), R, has_exclude ? ", one excluded" : "");
  return 0;
}

// offsets (G + 1) of a grouped bank of R rows: start at 0, increase strictly, end inside the bank.  *S_out: the longest group.
inline int group_offsets_check(const int32_t* offsets, int G, int R, int* S_out) {
  if (!offsets || G <= 0 || G > 65535 || R <= 0) return fail(CS_ERR_BAD_ARG, "grouped bank: offsets missing, or G = %d outside [1, 65535]", G);
  if (offsets[0] != 0) return fail(CS_ERR_BAD_ARG, "grouped bank: offsets[0] = %d, must be 0", offsets[0]);
  int S = 0;
  for (int g = 0; g < G; ++g) {
    if (offsets[g + 1] <= offsets[g]) return fail(CS_ERR_BAD_ARG, "grouped bank: offsets must increase strictly (offsets[%d] = %d, offsets[%d] = %d)", g, offsets[g], g + 1, offsets[g + 1]);
    S = std::max(S, offsets[g + 1] - offsets[g]);
  }
  if (offsets[G] > R) return fail(CS_ERR_BAD_ARG, "grouped bank: offsets[G] = %d exceeds the bank's %d rows", offsets[G], R);
  if (S_out) *S_out = S;
  return 0;
}

// the row whose tokens fill a query's missing places: -1 (zeros), or a bank row that belongs to no group
inline int blank_row_check(int blank_row, const int32_t* offsets, int G, int R) {
  if (blank_row < -1 || blank_row >= R || (blank_row >= 0 && blank_row < offsets[G]))
    return fail(CS_ERR_BAD_ARG, "grouped bank: blank_row = %d must be -1 or a row in [%d, %d), behind every group", blank_row, offsets[G], R);
  return 0;
}

inline int query_groups_check(const int32_t* query_group, int B, int G) {
  if (!query_group) return fail(CS_ERR_BAD_ARG, "grouped selection: query_group missing");
  for (int b = 0; b < B; ++b)
    if (query_group[b] < 0 || query_group[b] >= G) return fail(CS_ERR_BAD_ARG, "grouped selection: query %d names group %d of %d", b, query_group[b], G);
  return 0;
}

inline void fill_triples(const int32_t* query_group, int B, const int32_t* offsets, CsSelTriple* trip) {
  for (int b = 0; b < B; ++b) {
    const int g = query_group[b];
    trip[b] = CsSelTriple{offsets[g], offsets[g + 1] - offsets[g], g};
  }
}

inline bool supported_dh(int dh) { return dh == 16 || dh == 48 || dh == 64 || dh == 96 || dh == 128 || dh == 192; }

// fit_host.hip: every check of a scope's backward (its parent's is its first part), then its launches
int head_backward_run(const char* op, const CsHeadBackward& q, void* ws, int bf, hipStream_t st);
int tail_backward_run(const char* op, const CsTailBackward& q, void* ws, int bf, hipStream_t st);
int cross_backward_run(const char* op, const CsCrossBackward& q, void* ws, int bf, hipStream_t st);
int layer_backward_run(const char* op, const CsLayerBackward& q, void* ws, int bf, hipStream_t st);

// forward.hip
void reap_retired(cs_model* m, bool all);                        // frees retired workspaces whose last use has completed (never blocks unless `all`)
// *buf holds at least `need` bytes afterwards: a smaller one is retired behind an event recorded on `st` (freed by reap_retired) and replaced
int grow_retired(cs_model* m, void** buf, size_t* bytes, size_t need, hipStream_t st);
// The bracket of a call that works on the handle's buffers on `st`: call_enter orders it behind the handle's last call (which may have come on
// another stream; calls on one stream are ordered anyway), call_leave makes it the last call.
int call_enter(cs_model* m, hipStream_t st);
int call_leave(cs_model* m, hipStream_t st);
int streams_overlap(hipStream_t a, hipStream_t b, bool* yes);  // do kernels queued on a and b run side by side? (waits for both)

// The forward's workspace, carved 256-byte aligned: make_plan(h, ..., nullptr).total is what cs_workspace_bytes reports.
struct Plan {
  int B, N, H, W, gh, gw, Np, T, I, Ic, C, lanes;
  size_t total;
  // encoder chunk buffers, one set per lane
  float* x[CS_MAX_LANES]; h16_t* u[CS_MAX_LANES]; h16_t* r1[CS_MAX_LANES];
  h16_t* ob[CS_MAX_LANES]; float* stats[CS_MAX_LANES];  // LayerNorm fold: attention output, per-row partial sums
  float* lnstat[CS_MAX_LANES];                           // fold256: finalised (mean, rstd) per row, whole 256-row tiles
  float* pmean[CS_MAX_LANES];                            // per-patch channel means removed by im2col
  // decoder
  float *xq, *y, *lse; h16_t *q_bf, *mem_bf, *kv, *dqkv, *dq, *dob, *dhid;
  float* mean_part; unsigned* mean_cnt;  // the head launch's per-image mean (CsGemmParams::mean_*)
  CsU8Desc* u8desc;                      // one-pass input stage: B query descriptors, then B * N_enc reference descriptors
  float *sel_mean, *sel_unit, *sel_sim;  // cs_forward_select: the queries' pooled / unit descriptors (B, C), similarities (B, R) unless the caller keeps them
  CsSelTriple* sel_trip;                 // cs_forward_select_grouped: the queries' triples (B)
};

inline CsGemmParams gp(const h16_t* A, int lda, const h16_t* W, int ldw, int M, int N, int K, const float* bias, void* out, int ldc) {
  CsGemmParams g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.M = M; g.N = N; g.K = K; g.bias = bias; g.out = out; g.ldc = ldc;
  g.powp = 1.f;
  return g;
}

// the optional second stage of Launcher::rowln: the sub-block's following linear, out (M, n) = act(LN rows x W^T + b)
struct NextLinear { const h16_t* W = nullptr; const float* b = nullptr; h16_t* out = nullptr; int n = 0, act = 0; };

// Enqueues kernels on one stream: checks the parameters, counts the launch in the census, brackets it with profiling events when enabled.
// The first error sticks in `rc` and stops every later launch through this Launcher.
struct Launcher {
  cs_model* m; hipStream_t st; int rc = 0;
  int bpc = 0;  // GEMM blocks per CU hint (CsGemmParams::bpc)
  bool open = false;  // a profile record waits for its second event
  void begin(int family, double flops, double bytes = 0) {  // family < 0: not part of the profile (the score check)
    if (!m->prof || family < 0) return;
    ProfRec r{}; r.family = family; r.flops = flops; r.bytes = bytes;
    hipEventCreate(&r.a); hipEventCreate(&r.b);
    hipEventRecord(r.a, st);
    m->recs.push_back(r);
    open = true;
  }
  void end() { if (open) hipEventRecord(m->recs.back().b, st); open = false; }
  // behind the launch that begin() opened: closes the profile record, counts the launch under `kernel`, keeps the first error
  bool launched(const std::string& kernel, const char* what, hipError_t e) {
    end();
    m->census[kernel]++;
    if (e != hipSuccess) { rc = fail(CS_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e)); return false; }
    return true;
  }
  bool gemm(CsGemmParams g, int epi, double k_real = 0) {
    if (rc) return false;
    g.bpc = bpc;
    g.bf16 = m->cfg.operand_dtype;  // before the check: its "bf16 with a LayerNorm-folded epilogue" guard reads it
    if (const char* e = cs_gemm_check(&g, epi)) { rc = fail(CS_ERR_BAD_ARG, "%s", e); return false; }
    // algorithmic HBM bytes of one launch: A and W once (fp16), bias, the output once, the residual / position addend once
    const double mn = (double)g.M * g.N;
    const bool f32out = epi == CS_EPI_RESID_F32 || epi == CS_EPI_RESID_F32_LN || epi == CS_EPI_PATCH_F32 || epi == CS_EPI_HEAD_SCORE;
    double bytes = 2.0 * g.M * g.K + 2.0 * g.N * g.K + 4.0 * g.N + mn * (f32out ? 4.0 : 2.0);
    if ((epi == CS_EPI_RESID_F32 || epi == CS_EPI_RESID_F32_LN) && g.resid) bytes += 4.0 * mn;
    if (epi == CS_EPI_PATCH_F32) bytes += 4.0 * g.Np * g.N;
    begin(epi, 2.0 * g.M * g.N * (k_real > 0 ? k_real : g.K), bytes);
    return launched(cs_gemm256_supported(&g, epi) ? "gemm256" : "gemm128", "gemm", cs_gemm_launch(&g, epi, st));
  }
  // out (M, C) = resid + A (M, K) W^T + bias in fp32; with `u16` the epilogue also writes the rows in 16 bits and their LayerNorm partial sums
  // (`sp` slots per row) for the projection that consumes them (CS_EPI_RESID_F32_LN)
  bool resid_gemm(const h16_t* A, int lda, const h16_t* W, int K, int M, const float* bias, const float* resid, float* out,
                  h16_t* u16 = nullptr, float* stats = nullptr, int sp = 0) {
    const int C = m->cfg.hidden;
    CsGemmParams g = gp(A, lda, W, K, M, C, K, bias, out, C);
    g.resid = resid; g.ldr = C;
    if (u16) { g.out_f16 = u16; g.stats_out = stats; g.stats_sp = sp; }
    return gemm(g, u16 ? CS_EPI_RESID_F32_LN : CS_EPI_RESID_F32);
  }
  bool attn(CsAttnParams a, int dh, int batch) {
    if (rc) return false;
    a.bf16 = m->cfg.operand_dtype;
    if (const char* e = cs_attn_check(&a, dh, batch)) { rc = fail(CS_ERR_BAD_ARG, "%s", e); return false; }
    // Q and O once, K and V once per (batch, head): 2 bytes each
    begin(16 + dh / 16, 4.0 * batch * a.heads * (double)a.Lq * a.Lk * dh, 2.0 * batch * a.heads * dh * (2.0 * a.Lq + 2.0 * a.Lk));
    return launched("attn" + std::to_string(dh), "attention", cs_attn_launch(&a, dh, batch, st));
  }
  bool panel(CsPanelParams q) {
    if (rc) return false;
    q.bf16 = m->cfg.operand_dtype;
    if (const char* e = cs_panel_check(&q)) { rc = fail(CS_ERR_BAD_ARG, "%s", e); return false; }
    const double M = q.M, C = m->cfg.hidden, F = (double)m->cfg.mlp_ratio * C;
    // algorithmic bytes: x read + written (fp32), attention output read, u written (fp16), the weight stream once
    begin(40, 2.0 * M * C * C * (q.attn_o ? 1 : 0) + 4.0 * M * C * F,
          M * C * (8.0 + (q.attn_o ? 2.0 : 0.0) + (q.u_out ? 2.0 : 0.0)) + (double)(2 * (q.attn_o ? 1 : 0) + 16) * C * C);
    return launched(m->panel_impl ? "panel4" : "panel", "panel", m->panel_impl ? cs_panel4_launch(&q, st) : cs_panel_launch(&q, st));
  }
  // out = LN(resid + A W^T + bias): the decoder's out-projection / linear2 + residual + LayerNorm in one launch (rowln.hip; C = 384)
  bool rowln(const h16_t* A, const h16_t* W, const float* bias, const float* resid, const float* gamma, const float* beta, float eps,
             float* out_f32, h16_t* out_f16, int M, NextLinear next = NextLinear{}) {
    if (rc) return false;
    const int C = m->cfg.hidden;
    CsRowLnParams q{};
    q.A = A; q.lda = C; q.W = W; q.ldw = C; q.bias = bias; q.resid = resid; q.ldr = C; q.gamma = gamma; q.beta = beta; q.eps = eps;
    q.out_f32 = out_f32; q.out_f16 = out_f16; q.M = M;
    q.W2 = next.W; q.ldw2 = C; q.bias2 = next.b; q.out2 = next.out; q.ld2 = next.n; q.n2 = next.n; q.act2 = next.act;
    if (const char* e = cs_rowln_check(&q, C)) { rc = fail(CS_ERR_BAD_ARG, "%s", e); return false; }
    // algorithmic bytes: A and W once, the residual rows in, the normalised rows out (fp32, and 16-bit where asked); second stage: W2 in, rows out
    begin(42, 2.0 * M * C * (double)(C + next.n),
          2.0 * M * C + 2.0 * C * C + (resid ? 4.0 : 0.0) * M * C + (out_f32 ? 4.0 : 0.0) * M * C + (out_f16 ? 2.0 : 0.0) * M * C + 2.0 * next.n * C + 2.0 * M * next.n);
    return launched("rowln", "linear + LayerNorm", cs_rowln_launch(&q, C, m->cfg.operand_dtype, st));
  }
  // Every other kernel, census name `what`: `launch` is a callable that enqueues it on `st` and returns the hipError_t, so that the profile
  // record's first event is on the stream BEFORE the kernel.
  template <class Fn> bool misc(const char* what, int family, double flops, double bytes, Fn&& launch) {
    if (rc) return false;
    begin(family, flops, bytes);
    return launched(what, what, launch());
  }
  template <class Fn> bool small(const char* what, Fn&& launch) { return misc(what, 32, 0, 0, launch); }  // the memory-bound helpers: family 32, no flops
};

}  // namespace cs_host
