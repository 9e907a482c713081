// The forward of the CrossScore gfx950 path: workspace plan, position tables, lanes, encoder, decoder, and the six cs_forward* /
// cs_encode_references* entry points of the C ABI (include/crossscore_hip.h).  Host-side only: validates shapes and enqueues the HIP kernels on
// the caller's stream and the handle's lane streams.  Restates the control flow of CrossScoreNet.forward / get_featmaps (task/core.py:58-161),
// CrossReferenceNet.forward (model/cross_reference.py:52-94) and the post-norm decoder layer (transformer.py:157-173).
// forward_body at the end of the file is the sequence; the functions before it are its steps, in order.
#include "cs_model.h"

#include <chrono>
#include <cstdio>
#include <initializer_list>
#include <utility>

namespace cs_host {

// Frees retired workspaces whose last use has completed (never blocks).
void reap_retired(cs_model* m, bool all) {
  for (size_t i = 0; i < m->retired.size();) {
    if (all || hipEventQuery(m->retired[i].ev) == hipSuccess) {
      hipFree(m->retired[i].p); hipEventDestroy(m->retired[i].ev);
      m->retired.erase(m->retired.begin() + i);
    } else {
      ++i;
    }
  }
}

// Grows one of the handle's buffers.  The old one may still be in use by work queued earlier (on this or another stream), so it is retired
// behind an event recorded on `st` (which is ordered after every earlier call) and freed by a later call once that event has completed -- no
// wait here.
int grow_retired(cs_model* m, void** buf, size_t* bytes, size_t need, hipStream_t st) {
  if (need <= *bytes) return 0;
  if (*buf) {
    cs_model::Retired r{*buf, nullptr};
    HIPCHK(hipEventCreateWithFlags(&r.ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(r.ev, st));
    m->retired.push_back(r);
  }
  *buf = nullptr; *bytes = 0;
  HIPCHK(hipMalloc(buf, need));
  *bytes = need;
  return 0;
}

int call_enter(cs_model* m, hipStream_t st) {
  if (m->ev_done && m->last_stream != st) HIPCHK(hipStreamWaitEvent(st, m->ev_done, 0));
  return 0;
}

int call_leave(cs_model* m, hipStream_t st) {
  if (!m->ev_done) HIPCHK(hipEventCreateWithFlags(&m->ev_done, hipEventDisableTiming));
  HIPCHK(hipEventRecord(m->ev_done, st));
  m->last_stream = st;
  return 0;
}

// Do kernels queued on streams a and b run side by side?  The HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues,
// and hardware queues onto the pipes of the compute micro-engine.  Two streams on one queue serialise outright; two queues on one
// pipe are dispatched one kernel at a time, so a grid that does not fit the chip at once holds back the other stream's kernel until
// its last round (a two-lane forward then runs at the one-lane time although tiny kernels on the two streams overlap).  Probe, both
// released by one event: on `a` a grid of 4 workgroups per CU that fit two to a CU (64 KiB of LDS each) and idle 60 us each, i.e.
// two rounds; on `b` one wave that idles 2 us.  `b` finishes within a few microseconds when the two dispatch side by side and
// after >= 60 us when it has to wait for a's second round.  Waits for both streams (set-up only, ~0.4 ms).
int streams_overlap(hipStream_t a, hipStream_t b, bool* yes) {
  int dev = 0, cus = 0;
  HIPCHK(hipGetDevice(&dev));
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  hipEvent_t e0 = nullptr, eb = nullptr, ea = nullptr;
  HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&eb)); HIPCHK(hipEventCreate(&ea));
  int rc = 0;
  float best = 1e30f;
  for (int rep = 0; rep < 3 && !rc; ++rep) {  // the first round also absorbs the kernel's load
    hipError_t e = hipEventRecord(e0, a);
    if (e == hipSuccess) e = hipStreamWaitEvent(b, e0, 0);
    if (e == hipSuccess) e = cs_spin_launch(6000, 4 * cus, 64 * 1024, a);
    if (e == hipSuccess) e = cs_spin_launch(200, 1, 0, b);
    if (e == hipSuccess) e = hipEventRecord(eb, b);
    if (e == hipSuccess) e = hipEventRecord(ea, a);
    if (e == hipSuccess) e = hipEventSynchronize(ea);
    if (e == hipSuccess) e = hipEventSynchronize(eb);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, eb);
    if (e != hipSuccess) { rc = fail(CS_ERR_HIP, "stream overlap probe: %s", hipGetErrorString(e)); break; }
    if (rep > 0 && ms < best) best = ms;
  }
  hipEventDestroy(e0); hipEventDestroy(eb); hipEventDestroy(ea);
  if (!rc) *yes = best < 0.040f;
  return rc;
}

// the next slot of the ring with at least `bytes` of pinned memory and, on the current device, `dev_bytes` of device memory
int stage_take(StageRing& r, size_t bytes, size_t dev_bytes, StageRing::Slot** out) {
  StageRing::Slot& s = r.slot[r.next];
  r.next = (r.next + 1) % StageRing::SLOTS;
  if (s.used) HIPCHK(hipEventSynchronize(s.ev));  // the work of four calls ago: long done
  s.used = false;
  int dev = -1;
  if (dev_bytes) HIPCHK(hipGetDevice(&dev));
  if (s.cap < bytes) {
    if (s.host) HIPCHK(hipHostFree(s.host));
    s.host = nullptr; s.cap = 0;
    const size_t cap = std::max(bytes, (size_t)4096);
    HIPCHK(hipHostMalloc(&s.host, cap, hipHostMallocDefault));
    s.cap = cap;
  }
  if (dev_bytes && (s.dev_cap < dev_bytes || s.device != dev)) {
    if (s.dev) HIPCHK(hipFree(s.dev));
    s.dev = nullptr; s.dev_cap = 0;
    const size_t cap = std::max(dev_bytes, (size_t)4096);
    HIPCHK(hipMalloc(&s.dev, cap));
    s.dev_cap = cap; s.device = dev;
  }
  if (!s.ev) HIPCHK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
  *out = &s;
  return 0;
}

void stage_free(StageRing& r) {
  for (StageRing::Slot& s : r.slot) {
    if (s.host) hipHostFree(s.host);
    if (s.dev) hipFree(s.dev);
    if (s.ev) hipEventDestroy(s.ev);
    s = StageRing::Slot{};
  }
}

}  // namespace cs_host

namespace {

struct Arena {  // carve 256-byte aligned pieces out of the workspace
  char* base; size_t off = 0;
  template <typename T> T* take(size_t n) {
    T* p = reinterpret_cast<T*>(base + off);
    off += (n * sizeof(T) + 255) & ~size_t(255);
    return p;
  }
};

Plan make_plan(const cs_model* m, int B, int N, int N_enc, int H, int W, char* base, int R_sel = 0, bool own_sim = false, bool grouped = false) {
  Plan p{};
  const cs_config& c = m->cfg;
  p.B = B; p.N = N; p.H = H; p.W = W; p.C = c.hidden;
  p.gh = H / c.patch; p.gw = W / c.patch; p.Np = p.gh * p.gw; p.T = p.Np + 1; p.I = B * (1 + N_enc);
  p.lanes = m->prof ? 1 : (c.lanes <= 0 ? 2 : std::min(c.lanes, CS_MAX_LANES));  // profiling times kernels in isolation
  if (m->lanes_now > 0) p.lanes = std::min(p.lanes, m->lanes_now);               // cs_set_lanes (the workspace holds the configured number)
  // cfg-2: 2 lanes x 24 images measured best (7.51 vs 7.70 ms with 12).  ViT-B: with the 256-row-tile GEMM (gemm256.hip) a chunk has to hold
  // many row tiles per CU: cfg-4 449 q/s at 48 or 16 images per chunk, 419 at 6, 407 at 12; cfg-3 247 at 44, 248 at 11 (tools/lanes_sweep_b.py, r3)
  int ic = c.enc_chunk_images > 0 ? c.enc_chunk_images : (c.hidden <= 384 ? 24 : 48);
  // balanced chunks: a multiple of the lane count, near-equal sizes
  if (c.enc_chunk_images > 0) {
    p.Ic = std::min(ic, p.I);  // explicit: used verbatim (a shorter remainder chunk runs first)
  } else {
    // whole batch items per chunk (so a lane can decode what it just encoded), about `ic` images, balanced over the lanes
    const int per_item = 1 + N_enc;
    int items = std::max(1, ic / per_item);
    int passes = (B + items - 1) / items;
    if (B >= p.lanes) passes = ((passes + p.lanes - 1) / p.lanes) * p.lanes;
    passes = std::min(passes, B);
    items = (B + passes - 1) / passes;
    p.Ic = items * per_item;
  }
  const size_t C = c.hidden, Mc = (size_t)p.Ic * p.T, M = (size_t)B * p.Np, Mk = (size_t)B * N * p.Np;
  Arena a{base};
  const int nsets = c.lanes <= 0 ? 2 : std::min(c.lanes, CS_MAX_LANES);  // independent of the profiling mode
  for (int l = 0; l < nsets; ++l) {
    p.x[l] = a.take<float>(Mc * C);
    p.u[l] = a.take<h16_t>(Mc * C);
    p.r1[l] = a.take<h16_t>(std::max(Mc * (size_t)(c.swiglu ? 2 * ffn_hidden(c) : ffn_hidden(c)), std::max(Mc * (size_t)m->qkv_n, (size_t)p.Ic * p.Np * m->Kp)));
    p.ob[l] = a.take<h16_t>(m->lnfold || m->fold256 ? Mc * C : 0);
    p.pmean[l] = a.take<float>((size_t)p.Ic * p.Np * 4);
    const size_t Mpad = (Mc + 255) / 256 * 256;
    p.stats[l] = a.take<float>(m->lnfold ? Mc * (size_t)m->ln_sp * 2 : (m->fold256 ? Mpad * (C / 64) * 2 : 0));
    p.lnstat[l] = a.take<float>(m->fold256 ? Mpad * 2 : 0);
  }
  p.xq = a.take<float>(M * C);
  p.y = a.take<float>(M * C);
  p.q_bf = a.take<h16_t>(M * C);
  p.mem_bf = a.take<h16_t>(Mk * C);
  p.kv = a.take<h16_t>(Mk * 2 * C * c.dec_layers);
  p.dqkv = a.take<h16_t>(M * 3 * C);
  p.dq = a.take<h16_t>(M * C);
  p.dob = a.take<h16_t>(M * C);
  p.dhid = a.take<h16_t>(M * C);
  p.lse = a.take<float>((size_t)B * c.dec_heads * p.Np);
  p.mean_part = a.take<float>(M * 4 * (size_t)cs_gemm_column_tiles(c.patch * c.patch));
  p.mean_cnt = a.take<unsigned>((size_t)B);
  p.u8desc = a.take<CsU8Desc>((size_t)p.I);
  // cs_forward_select (R_sel > 0): the queries' pooled and unit descriptors, and the similarities when the caller keeps none; the gathered rows
  // are mem_bf above.  Nothing for the other modes: their plan and cs_workspace_bytes stay as they were.
  p.sel_mean = a.take<float>(R_sel > 0 ? (size_t)B * C : 0);
  p.sel_unit = a.take<float>(R_sel > 0 ? (size_t)B * C : 0);
  p.sel_sim = a.take<float>(own_sim ? (size_t)B * R_sel : 0);
  p.sel_trip = a.take<CsSelTriple>(grouped ? (size_t)B : 0);  // (a grouped call's R_sel is the longest group: its similarities are (B, S))
  p.total = a.off;
  return p;
}

int ensure_tables(cs_model* m, int gh, int gw, bool square, hipStream_t st) {
  const cs_config& c = m->cfg;
  const int sq = square ? 1 : 0;
  for (auto& t : m->tables)
    if (t.gh == gh && t.gw == gw && t.sq == sq) { m->pos_tab = t.pos_tab; m->pe_tab = t.pe_tab; return 0; }
  // first forward of this patch grid: allocate and fill its tables on the caller's stream (stream-ordered with the kernels that
  // read them).  Tables of other grids stay as they are -- work queued on any stream may still read them -- so there is nothing to
  // wait for; only past 16 distinct grids are the oldest dropped, behind a device synchronisation.
  if (m->tables.size() >= 16) {
    HIPCHK(hipDeviceSynchronize());
    for (auto& t : m->tables) { if (t.pos_owned) hipFree(t.pos_tab); if (t.pe_owned) hipFree(t.pe_tab); }
    m->tables.clear();
  }
  cs_model::Tables t{gh, gw, sq, nullptr, nullptr, false, false};
  const int Np = gh * gw, C = c.hidden;
  if (Np == c.pos_grid * c.pos_grid && square) {  // HF:71 -- parameter used as is
    t.pos_tab = m->pos;
  } else {
    HIPCHK(hipMalloc(&t.pos_tab, (size_t)(1 + Np) * C * sizeof(float)));
    t.pos_owned = true;
    HIPCHK(cs_pos_bicubic_launch(m->pos, c.pos_grid, C, gh, gw, c.pos_interp_legacy ? 0.1f : 0.0f, t.pos_tab, st));
  }
  if (gh == c.pe_h && gw == c.pe_w) {  // positional_encoding.py:51-56
    t.pe_tab = m->pe;
  } else {
    HIPCHK(hipMalloc(&t.pe_tab, (size_t)Np * C * sizeof(float)));
    t.pe_owned = true;
    HIPCHK(cs_pe_interp_launch(m->pe, c.pe_h, c.pe_w, C, gh, gw, c.pe_interp_mode, t.pe_tab, st));
  }
  m->tables.push_back(t);
  m->pos_tab = t.pos_tab; m->pe_tab = t.pe_tab;
  return 0;
}


// Debug tap: copies `bytes` of `src` into the tap `name` at byte offset `off` on stream `st` (stream-ordered behind the kernel that wrote src).
// The tap buffer holds `total` bytes and is (re)allocated here when its size changes: capture mode is for tests, not for timed runs.
int tap_buffer(cs_model* m, const std::string& name, size_t total, int dtype, std::initializer_list<int64_t> shape, void** out) {
  cs_model::Tap& t = m->taps[name];
  if (t.bytes != total) {
    if (t.d) { HIPCHK(hipDeviceSynchronize()); hipFree(t.d); t.d = nullptr; t.bytes = 0; }
    HIPCHK(hipMalloc(&t.d, total));
    t.bytes = total;
  }
  t.dtype = dtype; t.ndim = (int)shape.size();
  int k = 0;
  for (int64_t v : shape) t.shape[k++] = v;
  *out = t.d;
  return 0;
}
int tap_copy(cs_model* m, const std::string& name, const void* src, size_t off, size_t bytes, size_t total, int dtype,
             std::initializer_list<int64_t> shape, hipStream_t st) {
  if (!m->capture) return 0;
  void* d = nullptr;
  if (int r = tap_buffer(m, name, total, dtype, shape, &d)) return r;
  if (off + bytes > total) return fail(CS_ERR_STATE, "debug tap %s: copy out of range", name.c_str());
  HIPCHK(hipMemcpyAsync(static_cast<char*>(d) + off, src, bytes, hipMemcpyDeviceToDevice, st));
  return 0;
}

// the images of a forward as decoded uint8 (cs_forward_u8 and its siblings): host arrays of cs_u8_image
struct U8In { const cs_u8_image* query; const cs_u8_image* refs; const float* mean3; const float* std3; };

// How a chunk's layers run -- decided once per chunk, the same for every layer of it (a layer's producer feeds the next layer's consumer):
enum class Route {
  Panel,    // QKV GEMM + attention + ONE token-panel kernel per layer (hidden 384)
  Fold256,  // wide backbones (r5): LayerNorm folded into the 256-tile GEMM's epilogues, row statistics finalised by a kernel of their own
  Fold,     // ln_fold = 1: LayerNorm folded into the 128-row GEMM's epilogues
  Plain,    // LayerNorm launches + GEMMs with bias / GELU / residual epilogues; also a fold256 handle's chunk that the 256-tile kernel declines
  SwiGLU,   // Plain with the gated MLP
};

struct Chunk {
  int slot, i0, ic, Mc;  // lane buffers, first image, images, token rows
  Route route;
  float* x; h16_t *u, *r1, *ob; float *stats, *lnstat;
};

// One forward-class call: its arguments, and what the steps below work out for the later ones.
// mode 0: full forward (query + reference images); mode 1: query images + cached reference tokens (`ref_tokens`, fp16
// [B][N][Np][C]); mode 2: encode `B` images as references into `tokens_out` (fp16 [B][Np][C]), no decoder; mode 3: query images + a bank of
// reference tokens (`ref_tokens`, [R][Np][C]) from which each query's N views are selected by similarity and gathered (`sel`).
// Grouped (offsets != null): centre is (G, C), sim_out (B, S); offsets (G + 1) and query_group (B) are HOST arrays, blank_row fills missing places.
struct SelectIn {
  const float *bank_unit, *centre; int R; const int32_t* exclude; int32_t* index_out; float* sim_out;
  const int32_t* offsets = nullptr; int G = 0; const int32_t* query_group = nullptr; int blank_row = -1;
};
struct Fwd {
  cs_model* h; int mode;
  const float *query, *refs; const h16_t* ref_tokens; h16_t* tokens_out;
  int B, N, H, W;
  float *score_out, *attn_out; int head_id; float* mean_out;
  hipStream_t st;    // the caller's stream
  const U8In* u8;    // null: fp32 images
  const SelectIn* sel = nullptr;  // mode 3
  int bf = 0;        // 16-bit operand type of every activation buffer and packed weight: 0 IEEE half, 1 bfloat16
  int N_enc = 0;     // reference views that go through the encoder with their query
  int S_sel = 0;     // (grouped selection) rows of the longest group
  cs_model::RefUse use{};  // cs_request_reference_use, taken off the handle by forward_impl
  Plan p{};          // (workspace)
  int u8_span = 0;   // (uint8 descriptors) source rows one patch row reaches, at most
  int NL = 1;        // (lanes) lanes of this call, and their streams: the caller's when there is one lane
  hipStream_t lst[CS_MAX_LANES] = {};
  // (decoder) each sub-block closes with LN(x + Linear(.)): one launch where the row-complete kernel is built (C = 384), else GEMM + LayerNorm
  // ... and where it is, the sub-block's NEXT linear rides in the same launch when it is C wide (second stage of rowln.hip)
  bool fused_ln = false, fuse_next = false;
  // (fit keeps) the deepest scope this call keeps for -- FIT_TAIL: the two copies cs_tail_backward works on; FIT_CROSS: the copy of x1 as well, with
  // lse written; FIT_LAYER: the copies of x0 and Os as well, with the self-attention's lse written -- and the handle's kept region carved for it
  FitScope kept = FIT_HEAD;
  cs_fit::Kept kp{};

  // ---- step 1: arguments ----
  int validate() {
    if (!h) return fail(CS_ERR_BAD_ARG, "null handle");
    if (!h->finalized) return fail(CS_ERR_STATE, "cs_forward before cs_finalize");
    const cs_config& c = h->cfg;
    const bool have_q = u8 ? u8->query != nullptr : query != nullptr, have_r = u8 ? u8->refs != nullptr : refs != nullptr;
    if (mode == 0 && (!have_q || !have_r || !score_out)) return fail(CS_ERR_BAD_ARG, "null tensor (ref_cross_imgs is required when do_reference_cross)");
    if (mode == 1 && (!have_q || !ref_tokens || !score_out)) return fail(CS_ERR_BAD_ARG, "null tensor");
    if (mode == 2 && (!have_q || !tokens_out)) return fail(CS_ERR_BAD_ARG, "null tensor");
    if (mode == 3) {
      if (!have_q || !ref_tokens || !score_out || !sel || !sel->bank_unit || !sel->centre || !sel->index_out) return fail(CS_ERR_BAD_ARG, "null tensor");
      if (B > 0 && N > 0)
        if (int r = select_check(B, sel->R, c.hidden, N, sel->offsets != nullptr, sel->exclude != nullptr)) return r;
      if (sel->offsets) {
        if (int r = group_offsets_check(sel->offsets, sel->G, sel->R, &S_sel)) return r;
        if (int r = blank_row_check(sel->blank_row, sel->offsets, sel->G, sel->R)) return r;
        if (int r = query_groups_check(sel->query_group, B, sel->G)) return r;
      }
      if ((long long)B * N > 65535) return fail(CS_ERR_UNSUPPORTED, "cs_forward_select: more than 65535 reference slots in one call; split the batch");
    }
    if (u8 && (!u8->mean3 || !u8->std3 || !(u8->std3[0] > 0.f) || !(u8->std3[1] > 0.f) || !(u8->std3[2] > 0.f)))
      return fail(CS_ERR_BAD_ARG, "uint8 input: mean / std missing or std not positive");
    if (B <= 0 || (mode != 2 && N <= 0)) return fail(CS_ERR_BAD_ARG, "empty batch or no reference views");
    if (H < c.patch || W < c.patch) return fail(CS_ERR_BAD_ARG, "image smaller than one patch");
    if (attn_out && (head_id < 0 || head_id >= c.dec_heads)) return fail(CS_ERR_BAD_ARG, "need_attn_weights_head_id %d out of range", head_id);
    const long long Np = (long long)(H / c.patch) * (W / c.patch);
    if ((long long)B * N * Np * 2 * c.hidden * c.dec_layers >= (1ll << 31)) return fail(CS_ERR_UNSUPPORTED, "batch too large for 32-bit offsets; split the batch");
    if (attn_out && Np > 65535) return fail(CS_ERR_UNSUPPORTED, "need_attn_weights with more than 65535 patches per image is not built");
    bf = c.operand_dtype;
    N_enc = mode == 0 ? N : 0;
    return 0;
  }

  // ---- step 2: workspace (grown when this call needs more), carved into p ----
  int ensure_workspace() {
    const int N_plan = mode == 2 ? 0 : N;
    const bool grouped = mode == 3 && sel->offsets;
    const int R_sel = mode == 3 ? (grouped ? S_sel : sel->R) : 0;
    const bool own_sim = mode == 3 && !sel->sim_out;
    const size_t need = make_plan(h, B, N_plan, N_enc, H, W, nullptr, R_sel, own_sim, grouped).total;
    reap_retired(h, false);
    if (int r = grow_retired(h, &h->ws, &h->ws_bytes, need, st)) return r;  // st already waits for the previous call's stream (forward_impl)
    p = make_plan(h, B, N_plan, N_enc, H, W, static_cast<char*>(h->ws), R_sel, own_sim, grouped);
    return 0;
  }

  // ---- step 3 (grouped selection): the queries' triples -> workspace, the way the uint8 descriptors travel below ----
  int stage_select_triples() {
    if (mode != 3 || !sel->offsets) return 0;
    StageRing::Slot* sl = nullptr;
    if (int r = stage_take(h->sel_ring, (size_t)B * sizeof(CsSelTriple), 0, &sl)) return r;
    fill_triples(sel->query_group, B, sel->offsets, static_cast<CsSelTriple*>(sl->host));
    HIPCHK(hipMemcpyAsync(p.sel_trip, sl->host, (size_t)B * sizeof(CsSelTriple), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(sl->ev, st));
    sl->used = true;
    return 0;
  }

  // ---- step 4: one-pass input stage: per-image descriptors (filter tables of the image's resize geometry, crop corner) -> workspace ----
  int stage_u8_descriptors() {
    if (!u8) return 0;
    const int P = h->cfg.patch;
    if (h->lnfold || !h->Wpatch_frag || !cs_patch_fused_supported(H, W, P, h->cfg.hidden))
      return fail(CS_ERR_UNSUPPORTED, "uint8 input needs the one-launch patch embedding (14-pixel patches, hidden a multiple of 384, LayerNorm fold off)");
    const int n_desc = p.I;  // B + B * N_enc
    cs_model::U8Slot& sl = h->u8_slot[h->u8_next];
    h->u8_next = (h->u8_next + 1) % cs_model::U8_SLOTS;
    if (sl.used) HIPCHK(hipEventSynchronize(sl.ev));  // the copy of four forwards ago: long done
    if (sl.cap < (size_t)n_desc) {
      if (sl.host) HIPCHK(hipHostFree(sl.host));
      sl.host = nullptr; sl.cap = 0;
      HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&sl.host), (size_t)n_desc * sizeof(CsU8Desc), hipHostMallocDefault));
      sl.cap = (size_t)n_desc;
    }
    if (!sl.ev) HIPCHK(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
    // (the table cache holds 64 geometries and is dropped as a whole when a 65th arrives: if that happens while this call gathers its tables, the
    //  pointers gathered before the drop are gone -- gather again; a second drop means the call itself names more than 64 geometries)
    for (int attempt = 0;; ++attempt) {
      unsigned gen0 = 0, gen = 0;
      bool moved = false;
      u8_span = 0;
      for (int i = 0; i < n_desc; ++i) {
        const cs_u8_image& im = i < B ? u8->query[i] : u8->refs[i - B];
        CsU8Desc d{};
        if (im.h <= 0 || im.w <= 0 || im.rs_h <= 0 || im.rs_w <= 0 || im.row_bytes < 3 * im.w || im.crop_y < 0 || im.crop_x < 0 ||
            im.crop_y + H > im.rs_h || im.crop_x + W > im.rs_w)
          return fail(CS_ERR_BAD_ARG, "uint8 input %d: bad sizes (the %d x %d window must lie inside the resized image %d x %d)", i, H, W, im.rs_h, im.rs_w);
        int span = 0;
        HIPCHK(cs_preprocess_tables(im.h, im.w, im.rs_h, im.rs_w, im.crop_y, p.gh, P, &d.t, &span, &gen));
        if (i == 0) gen0 = gen;
        moved = moved || gen != gen0;
        d.data = im.data; d.row_bytes = im.row_bytes; d.crop_y = im.crop_y; d.crop_x = im.crop_x;
        u8_span = std::max(u8_span, span);
        sl.host[i] = d;
      }
      if (!moved) break;
      if (attempt) return fail(CS_ERR_UNSUPPORTED, "uint8 input: more than 64 distinct image geometries in one call");
    }
    if (cs_patch_u8_runs(W, u8_span) <= 0)
      return fail(CS_ERR_UNSUPPORTED, "uint8 input: a patch row reaches %d source rows, more than the one-pass form holds; use cs_op_preprocess_u8 + cs_forward", u8_span);
    HIPCHK(hipMemcpyAsync(p.u8desc, sl.host, (size_t)n_desc * sizeof(CsU8Desc), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(sl.ev, st));
    sl.used = true;
    return 0;
  }

  // ---- step 5: lanes: the handle's internal streams and the events that fork them from / join them to the caller's stream ----
  // A new lane stream that shares a hardware queue with the previous lane would run after it, not beside it: probe, and take another
  // stream until the two overlap (the rejected streams are released afterwards so that the runtime does not hand the same
  // queue back at once); one-time set-up cost of ~0.3 ms per probe, with a wait for the probe kernels
  int draw_lane_stream(int l) {
    HIPCHK(hipStreamCreateWithFlags(&h->lane_st[l], hipStreamNonBlocking));
    if (l == 0) return 0;
    std::vector<hipStream_t> rejected;
    for (int attempt = 0; attempt < 8; ++attempt) {
      bool ok = false;
      if (int r = streams_overlap(h->lane_st[l - 1], h->lane_st[l], &ok)) return r;
      if (g_debug_stream_log) fprintf(stderr, "[crossscore_hip] lane %d stream candidate %d: %s\n", l, attempt, ok ? "overlaps" : "serialises");
      if (ok) break;
      rejected.push_back(h->lane_st[l]);
      h->lane_st[l] = nullptr;
      HIPCHK(hipStreamCreateWithFlags(&h->lane_st[l], hipStreamNonBlocking));
    }
    for (hipStream_t r : rejected) hipStreamDestroy(r);
    return 0;
  }

  int ensure_lanes() {
    NL = p.lanes;
    for (hipStream_t& s : lst) s = st;
    if (NL < 2) return 0;
    for (int l = 0; l < NL; ++l) {
      if (!h->lane_st[l])
        if (int r = draw_lane_stream(l)) return r;
      if (!h->ev_join[l]) HIPCHK(hipEventCreateWithFlags(&h->ev_join[l], hipEventDisableTiming));
      if (!h->ev_stag[l]) HIPCHK(hipEventCreateWithFlags(&h->ev_stag[l], hipEventDisableTiming));
      lst[l] = h->lane_st[l];
    }
    if (!h->ev_fork) HIPCHK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    if (!h->ev_kv0) HIPCHK(hipEventCreateWithFlags(&h->ev_kv0, hipEventDisableTiming));  // the decoder's K/V projection on lane stream 1
    if (!h->ev_kv1) HIPCHK(hipEventCreateWithFlags(&h->ev_kv1, hipEventDisableTiming));
    for (hipStream_t o : h->lane_st_old) hipStreamDestroy(o);  // the replacements exist now
    h->lane_st_old.clear();
    return 0;
  }

  // ---- steps 6 and 8: everything stays stream-ordered on the caller's stream ----
  int fork_lanes() {
    if (NL == 1) return 0;
    HIPCHK(hipEventRecord(h->ev_fork, st));
    for (int l = 0; l < NL; ++l) HIPCHK(hipStreamWaitEvent(lst[l], h->ev_fork, 0));
    return 0;
  }

  int join_lanes() {
    if (NL == 1) return 0;
    for (int l = 0; l < NL; ++l) {
      HIPCHK(hipEventRecord(h->ev_join[l], lst[l]));
      HIPCHK(hipStreamWaitEvent(st, h->ev_join[l], 0));
    }
    return 0;
  }

  // ================= step 7: encoder (Dinov2Model.forward, HF:451-477): image chunks, alternating lanes =================

  Chunk make_chunk(int slot, int i0, int ic) {
    const int C = h->cfg.hidden, F = ffn_hidden(h->cfg), Mc = ic * p.T;
    Chunk k{slot, i0, ic, Mc, Route::Plain, p.x[slot], p.u[slot], p.r1[slot], p.ob[slot], p.stats[slot], p.lnstat[slot]};
    if (h->panel) k.route = Route::Panel;
    else if (h->lnfold) k.route = Route::Fold;
    else if (h->cfg.swiglu) k.route = Route::SwiGLU;
    else if (h->fold256 && Mc >= 256) {
      // The LayerNorm-folded epilogues (statistics layouts: consumer ln_sp == 1, producer stats_sp == N / 64) exist only in the 256-tile kernel:
      // a chunk takes that branch only if the kernel accepts ALL of its folded shapes.  Whatever makes it decline (cs_debug_gemm256_enable(0),
      // cs_debug_gemm256_kmin above C, a chunk below 256 rows or beyond the kernel's 32-bit byte offsets) leaves the chunk on the plain path, which
      // is correct for a fold256 handle (LayerNorm launches with ones / zeros, gamma in the packed weights, beta in the c vectors).
      const EncLayer& E0 = h->enc[0];
      CsGemmParams cq = gp(k.u, C, E0.Wqkv, C, Mc, h->qkv_n, C, E0.c_qkv, k.r1, h->qkv_n);
      cq.col_s = E0.s_qkv; cq.ln_part = k.lnstat; cq.ln_sp = 1;
      CsGemmParams c1 = gp(k.u, C, E0.W1, C, Mc, F, C, E0.c_1, k.r1, F);
      c1.col_s = E0.s_1; c1.ln_part = k.lnstat; c1.ln_sp = 1;
      CsGemmParams po = gp(k.ob, C, E0.Wo, C, Mc, C, C, E0.bo, k.x, C);
      po.resid = k.x; po.ldr = C; po.out_f16 = k.u; po.stats_out = k.stats; po.stats_sp = C / 64;
      CsGemmParams p2 = gp(k.r1, F, E0.W2, F, Mc, C, F, E0.b2, k.x, C);
      p2.resid = k.x; p2.ldr = C; p2.out_f16 = k.u; p2.stats_out = k.stats; p2.stats_sp = C / 64;
      if (cs_gemm256_supported(&cq, CS_EPI_LN_F16) && cs_gemm256_supported(&c1, CS_EPI_LN_GELU_F16) &&
          cs_gemm256_supported(&po, CS_EPI_RESID_F32_LN) && cs_gemm256_supported(&p2, CS_EPI_RESID_F32_LN))
        k.route = Route::Fold256;
    }
    return k;
  }

  // tap: the chunk's rows of the residual stream into the (I, T, C) tap `name`
  void enc_tap(Launcher& L, const Chunk& k, const std::string& name) {
    const size_t C = p.C;
    if (h->capture && !L.rc)
      L.rc = tap_copy(h, name, k.x, (size_t)k.i0 * p.T * C * 4, (size_t)k.Mc * C * 4, (size_t)p.I * p.T * C * 4, 0, {p.I, p.T, p.C}, L.st);
  }

  // CLS rows + patch embedding + position rows -> x (Dinov2Embeddings, HF:97-116)
  void enc_embed(Launcher& L, const Chunk& k) {
    const int C = p.C, P = h->cfg.patch, ic = k.ic, i0 = k.i0;
    hipStream_t s = L.st;
    const bool fold = k.route == Route::Fold;  // then layer 0's QKV wants fp16 rows + LayerNorm partial sums from here
    L.small("cls", [&] { return cs_cls_rows_launch(k.x, ic, p.T, C, h->cls, h->pos_tab, fold ? k.u : nullptr, fold ? k.stats : nullptr, h->ln_sp, bf, s); });
    if (u8) {
      // one launch fed from the decoded uint8 images (stage_u8_descriptors checked that this form is available)
      L.misc("patch_u8", 41, 2.0 * ic * p.Np * C * 3.0 * P * P, 3.0 * ic * H * W + 4.0 * ic * p.Np * C + 4.0 * p.Np * C, [&] {
        return cs_patch_fused_u8_launch(p.u8desc, B, N_enc, i0, ic, H, W, C, u8_span, u8->mean3, u8->std3, h->Wpatch_frag, h->bpatch, h->pos_tab,
                                        h->wsum, k.x, bf, s);
      });
    } else if (!fold && h->Wpatch_frag && cs_patch_fused_supported(H, W, P, C)) {
      // one launch: strip -> centred fp16 tile in LDS -> MFMA -> token rows (patch.hip).  Algorithmic bytes: the images once, the rows once
      L.misc("patch", 41, 2.0 * ic * p.Np * C * 3.0 * P * P, 12.0 * ic * H * W + 4.0 * ic * p.Np * C + 4.0 * p.Np * C, [&] {
        return cs_patch_fused_launch(query, refs, N_enc, i0, ic, H, W, C, h->Wpatch_frag, h->bpatch, h->pos_tab, h->wsum, k.x, bf, s);
      });
    } else {
      // patches are mean-centred per channel before the fp16 rounding; the patch GEMM adds mean * sum(W) back in fp32
      float* pmean = p.pmean[k.slot];
      L.small("im2col", [&] { return cs_im2col_launch(query, refs, N_enc, i0, k.r1, ic, H, W, P, h->Kp, pmean, bf, s); });
      CsGemmParams g = gp(k.r1, h->Kp, h->Wpatch, h->Kp, ic * p.Np, C, h->Kp, h->bpatch, k.x, C);
      g.pos = h->pos_tab; g.Np = p.Np; g.pmean = pmean; g.wsum = h->wsum;
      if (fold) { g.out_f16 = k.u; g.stats_out = k.stats; g.stats_sp = h->ln_sp; }
      L.gemm(g, CS_EPI_PATCH_F32, 3.0 * P * P);
    }
    enc_tap(L, k, "embeddings");
  }

  // u = 16-bit LayerNorm(x) as a launch of its own (`what`: ln1 / ln2).  `unit`: without gamma / beta, which are then folded into the consuming
  // projection (gamma in its packed weights, beta in its c vector)
  void enc_ln(Launcher& L, const Chunk& k, const char* what, const float* gamma, const float* beta, bool unit) {
    L.small(what, [&] { return cs_layernorm_launch(k.x, k.Mc, p.C, unit ? h->ones : gamma, unit ? h->zeros : beta, 1e-6f, nullptr, k.u, bf, L.st); });
  }

  // The LayerNorm consumers (QKV, fc1): r1 (Mc, n) = epi(u W^T + bias).  With `ln_part` the LayerNorm itself rides in the epilogue (CS_EPI_LN_*):
  // rstd * (acc - mean * s[n]) + c[n] from the row statistics in ln_part (ln_sp slots per row), bias = c
  void enc_proj(Launcher& L, const Chunk& k, const h16_t* W, const float* bias, int n, int epi, const float* col_s = nullptr,
                const float* ln_part = nullptr, int ln_sp = 0) {
    const int C = p.C;
    CsGemmParams g = gp(k.u, C, W, C, k.Mc, n, C, bias, k.r1, n);
    if (ln_part) { g.col_s = col_s; g.ln_part = ln_part; g.ln_sp = ln_sp; g.ln_eps = 1e-6f; }
    L.gemm(g, epi);
  }

  // Panel: u = fp16 normalised rows (norm1 without gamma / beta: folded into Wqkv / c_qkv), written by the previous layer's panel kernel; layer 0
  // gets it from the LayerNorm kernel.  Out-projection + norm2 + MLP + the next layer's norm1 are the one panel launch.
  void enc_layer_panel(Launcher& L, const Chunk& k, int l, CsAttnParams a) {
    const EncLayer& E = h->enc[l];
    if (l == 0) enc_ln(L, k, "ln1", nullptr, nullptr, true);
    enc_proj(L, k, E.Wqkv, E.c_qkv, h->qkv_n, CS_EPI_BIAS_F16);
    a.O = k.u;
    L.attn(a, p.C / h->cfg.enc_heads, k.ic);
    CsPanelParams q{};
    q.x = k.x; q.attn_o = k.u; q.img = E.panel_img; q.bo = E.bo; q.b1 = E.c_1; q.b2 = E.b2; q.u_out = l == h->cfg.enc_layers - 1 ? nullptr : k.u;
    q.M = k.Mc; q.eps = 1e-6f;
    L.panel(q);
  }

  // Fold / Fold256: no LayerNorm pass over the fp32 stream.  The residual epilogues (out-projection, fc2) also write u = 16-bit(x) and per-row
  // partial sums; the consuming projection (QKV, fc1) applies the LayerNorm in its epilogue.  The two differ in the statistics' layout: the
  // 128-row kernel's consumers read the producers' partial sums as they are (ln_sp slots); the 256-tile kernel's producers write C / 64 slots, a
  // row-statistics kernel (one thread per row) turns them into (mean, rstd), and layer 0's norm1 -- its rows come from the patch embedding, which
  // writes no sums there -- is a LayerNorm launch (gamma is in the packed weights, beta in c).
  void enc_layer_folded(Launcher& L, const Chunk& k, int l, CsAttnParams a) {
    const EncLayer& E = h->enc[l];
    const int C = p.C, F = ffn_hidden(h->cfg), Mc = k.Mc;
    const bool f256 = k.route == Route::Fold256, last = l == h->cfg.enc_layers - 1;
    const int sp_out = f256 ? C / 64 : h->ln_sp, sp_in = f256 ? 1 : h->ln_sp;
    const float* stat = f256 ? k.lnstat : k.stats;
    auto row_stats = [&] {
      if (f256) L.small("ln_stats", [&] { return cs_ln_finalize_launch(k.stats, Mc, (Mc + 255) / 256 * 256, sp_out, C, 1e-6f, k.lnstat, L.st); });
    };
    if (f256 && l == 0) {
      enc_ln(L, k, "ln1", nullptr, nullptr, true);
      enc_proj(L, k, E.Wqkv, E.c_qkv, h->qkv_n, CS_EPI_BIAS_F16);
    } else {
      enc_proj(L, k, E.Wqkv, E.c_qkv, h->qkv_n, CS_EPI_LN_F16, E.s_qkv, stat, sp_in);
    }
    a.O = k.ob;
    L.attn(a, C / h->cfg.enc_heads, k.ic);
    L.resid_gemm(k.ob, C, E.Wo, C, Mc, E.bo, k.x, k.x, k.u, k.stats, sp_out);
    row_stats();
    enc_proj(L, k, E.W1, E.c_1, F, CS_EPI_LN_GELU_F16, E.s_1, stat, sp_in);
    if (last) {
      L.resid_gemm(k.r1, F, E.W2, F, Mc, E.b2, k.x, k.x);  // the final LayerNorm reads the fp32 stream
    } else {
      L.resid_gemm(k.r1, F, E.W2, F, Mc, E.b2, k.x, k.x, k.u, k.stats, sp_out);
      row_stats();
    }
  }

  // Plain / SwiGLU.  (A fold256 handle's chunk lands here with gamma folded into its packed weights and beta into the c vectors: LayerNorm
  // without gamma / beta then, as in the panel path.)
  void enc_layer_plain(Launcher& L, const Chunk& k, int l, CsAttnParams a) {
    const EncLayer& E = h->enc[l];
    const int C = p.C, F = ffn_hidden(h->cfg), Mc = k.Mc;
    const bool unit = h->fold256;
    enc_ln(L, k, "ln1", E.ln1g, E.ln1b, unit);
    enc_proj(L, k, E.Wqkv, unit ? E.c_qkv : E.bqkv, h->qkv_n, CS_EPI_BIAS_F16);
    a.O = k.u;
    L.attn(a, C / h->cfg.enc_heads, k.ic);
    L.resid_gemm(k.u, C, E.Wo, C, Mc, E.bo, k.x, k.x);
    enc_ln(L, k, "ln2", E.ln2g, E.ln2b, unit);
    if (k.route == Route::SwiGLU) {
      // Dinov2SwiGLUFFN (HF:300-316): [x1 | x2] = LN2(x) Win^T + b (2F columns), hidden = silu(x1) * x2 in place over the x1 half, x += hidden Wout'^T + b'
      enc_proj(L, k, E.W1, E.b1, 2 * F, CS_EPI_BIAS_F16);
      L.misc("silu_mul", 32, 0, 6.0 * Mc * F, [&] { return cs_silu_mul_launch(k.r1, Mc, F, 2 * F, bf, L.st); });
      L.resid_gemm(k.r1, 2 * F, E.W2, F, Mc, E.b2, k.x, k.x);
    } else {
      enc_proj(L, k, E.W1, unit ? E.c_1 : E.b1, F, CS_EPI_BIAS_GELU_F16);
      L.resid_gemm(k.r1, F, E.W2, F, Mc, E.b2, k.x, k.x);
    }
  }

  // attention over `heads` heads of C / heads columns: Q (Lq rows per batch item, row stride ldq), K and V (Lk rows, stride ldkv) -> O (stride C);
  // the softmax scale is folded into the Q projections (cs_finalize)
  CsAttnParams attn_params(const h16_t* Q, int ldq, const h16_t* K, const h16_t* V, int ldkv, h16_t* O, int Lq, int Lk, int heads, float* lse = nullptr) {
    CsAttnParams a{};
    a.bf16 = bf;
    a.Q = Q; a.K = K; a.V = V; a.O = O; a.ldq = ldq; a.ldk = a.ldv = ldkv; a.ldo = p.C;
    a.q_bs = (long long)Lq * ldq; a.k_bs = a.v_bs = (long long)Lk * ldkv; a.o_bs = (long long)Lq * p.C;
    a.Lq = Lq; a.Lk = Lk; a.heads = heads; a.scale_log2e = 1.0f; a.lse = lse;
    return a;
  }

  // one encoder layer of one chunk (Dinov2Layer, HF:361-380)
  void enc_layer(Launcher& L, const Chunk& k, int l) {
    const int C = p.C, NQ = h->qkv_n;  // NQ: row stride of the packed QKV rows (3C, or padded to whole 256-column GEMM tiles)
    const CsAttnParams a = attn_params(k.r1, NQ, k.r1 + C, k.r1 + 2 * C, NQ, nullptr, p.T, p.T, h->cfg.enc_heads);
    switch (k.route) {
      case Route::Panel: enc_layer_panel(L, k, l, a); break;
      case Route::Fold256: case Route::Fold: enc_layer_folded(L, k, l, a); break;
      case Route::Plain: case Route::SwiGLU: enc_layer_plain(L, k, l, a); break;
    }
    enc_tap(L, k, "enc_layer_" + std::to_string(l));
  }

  // final LayerNorm of the patch rows + multi-view PE -> the decoder's query rows / memory rows (or the caller's token buffer, mode 2)
  void enc_finish(Launcher& L, const Chunk& k) {
    L.small("final_ln", [&] {
      return cs_final_ln_split_launch(k.x, k.ic, k.i0, p.Np, p.C, mode == 2 ? -1 : N_enc, h->lnfg, h->lnfb, 1e-6f, h->pe_tab, p.xq, p.q_bf,
                                      mode == 2 ? tokens_out : p.mem_bf, bf, L.st);
    });
  }

  // Chunk k runs on lane k % NL.  The host enqueues the chunks of one round (one per lane) step by step in turn -- embedding, layer 0, ...,
  // final LayerNorm -- so that every lane has work from the first microsecond of the step (a whole chunk is ~90 launches = 0.3 ms of enqueue
  // time, during which the other lanes would idle).
  int encoder_rounds(Launcher* LL) {
    // chunk sizes: the short remainder (if any) goes FIRST so that it overlaps the long chunks instead of trailing them
    std::vector<std::pair<int, int>> chunks;  // (first image, images)
    int i0 = 0;
    const int rem = p.I % p.Ic;
    if (rem) { chunks.push_back({0, rem}); i0 = rem; }
    for (; i0 < p.I; i0 += p.Ic) chunks.push_back({i0, p.Ic});
    for (size_t base = 0; base < chunks.size(); base += NL) {
      const int n = (int)std::min<size_t>(NL, chunks.size() - base);
      Chunk k[CS_MAX_LANES];
      for (int l = 0; l < n; ++l) k[l] = make_chunk(l, chunks[base + l].first, chunks[base + l].second);
      // The lanes run the same kernel sequence: started together they stay in lockstep (panel beside panel, attention beside
      // attention) and overlap nothing useful -- which is what happens whenever their streams sit on separate hardware queues.  Lane l
      // therefore starts its first chunk when lane l-1 has finished its patch embedding (about half a layer's time): from then on one
      // lane's QKV + attention runs beside the other's panel kernel.
      const bool stagger = base == 0 && NL >= 2;
      for (int l = 0; l < n; ++l) {
        if (stagger && l > 0 && hipStreamWaitEvent(lst[l], h->ev_stag[l - 1], 0) != hipSuccess) return fail(CS_ERR_HIP, "lane stagger wait failed");
        enc_embed(LL[l], k[l]);
        if (stagger && hipEventRecord(h->ev_stag[l], lst[l]) != hipSuccess) return fail(CS_ERR_HIP, "lane stagger record failed");
      }
      for (int layer = 0; layer < h->cfg.enc_layers; ++layer)
        for (int l = 0; l < n; ++l) enc_layer(LL[l], k[l], layer);
      for (int l = 0; l < n; ++l) enc_finish(LL[l], k[l]);
    }
    return 0;
  }

  // ---- step 8b (mode 3): the queries' descriptors from the 16-bit copy of their decoder input -- the rows final_ln_split rounds exactly as it
  // rounds a reference's (one ln_store for both) -- then similarities against the bank, the N best per query, and their token rows -> mem_bf ----
  void select_references(Launcher& L) {
    const int C = p.C;
    float* sim = sel->sim_out ? sel->sim_out : p.sel_sim;
    // grouped: every query against its own slice of the bank and that slice's centre, missing places take the blank row's tokens; plain: no
    // triples, which the kernels read as "the whole bank" (select.hip)
    const bool grouped = sel->offsets != nullptr;
    const CsSelTriple* trip = grouped ? p.sel_trip : nullptr;
    const int R = sel->R, G = grouped ? sel->G : 1, S = grouped ? S_sel : R, blank = grouped ? sel->blank_row : -1;
    L.small("select_desc", [&] { return cs_token_descriptors_launch(p.q_bf, B, p.Np, C, bf, p.sel_mean, L.st); });
    L.small(grouped ? "select_unit_grouped" : "select_unit", [&] { return cs_query_unit_launch(p.sel_mean, B, C, trip, R, G, sel->centre, p.sel_unit, L.st); });
    L.small(grouped ? "select_sim_grouped" : "select_sim", [&] { return cs_similarity_launch(p.sel_unit, B, sel->bank_unit, R, G, C, trip, S, sim, L.st); });
    L.small(grouped ? "select_topn_grouped" : "select_topn", [&] { return cs_topn_launch(sim, B, S, R, G, trip, sel->exclude, N, sel->index_out, L.st); });
    L.misc(grouped ? "select_gather_blank" : "select_gather", 32, 0, 4.0 * B * N * p.Np * C,
           [&] { return cs_gather_tokens_launch(ref_tokens, R, p.Np, C, sel->index_out, B * N, blank, p.mem_bf, L.st); });
  }

  // ---- step 9: taps: the decoder's inputs = final LayerNorm of the patch tokens + multi-view PE (core.py:141-153,93-98): query rows fp32, reference rows 16 bit ----
  int tap_featmaps() {
    if (!h->capture) return 0;
    const int C = p.C;
    const int dt16 = bf ? 2 : 1;
    if (mode == 2)
      return tap_copy(h, "featmap_ref", tokens_out, 0, (size_t)B * p.Np * C * 2, (size_t)B * p.Np * C * 2, dt16, {B, p.Np, C}, st);
    if (int r = tap_copy(h, "featmap_query", p.xq, 0, (size_t)B * p.Np * C * 4, (size_t)B * p.Np * C * 4, 0, {B, p.Np, C}, st)) return r;
    if (mode == 3) {
      if (int r = tap_copy(h, "select_query_mean", p.sel_mean, 0, (size_t)B * C * 4, (size_t)B * C * 4, 0, {B, C}, st)) return r;
      if (int r = tap_copy(h, "select_query_unit", p.sel_unit, 0, (size_t)B * C * 4, (size_t)B * C * 4, 0, {B, C}, st)) return r;
    }
    const h16_t* mem = mode == 1 ? ref_tokens : p.mem_bf;
    return tap_copy(h, "featmap_ref", mem, 0, (size_t)B * N * p.Np * C * 2, (size_t)B * N * p.Np * C * 2, dt16, {B, (int64_t)N * p.Np, C}, st);
  }

  // ================= step 10: decoder (transformer.py:213-268, post-norm layers :157-173) + head =================
  // Closes a sub-block: xq = LN(resid + A W^T + b), q_bf its 16-bit copy.  Returns whether `next` (if any) rode along in the same launch -- its
  // input is then the normalised rows and q_bf is not written; otherwise the caller runs that linear as a GEMM from q_bf.
  bool dec_close(Launcher& L, const h16_t* A, const h16_t* W, const float* b, const float* resid, const float* gamma, const float* beta,
                 const char* norm, NextLinear next = NextLinear{}) {
    const int M = B * p.Np;
    if (fused_ln) {
      const bool ride = fuse_next && next.W;
      L.rowln(A, W, b, resid, gamma, beta, 1e-5f, p.xq, ride ? nullptr : p.q_bf, M, ride ? next : NextLinear{});
      return ride;
    }
    L.resid_gemm(A, p.C, W, p.C, M, b, resid, p.y);
    L.small(norm, [&] { return cs_layernorm_launch(p.y, M, p.C, gamma, beta, 1e-5f, p.xq, p.q_bf, bf, L.st); });
    return false;
  }

  // Behind the last layer's cross-attention, on its stream: the four reference-use outputs from its Q, K and lse (refuse.hip)
  void reference_use(Launcher& L, const CsAttnParams& a, int dh) {
    CsRefUseParams r{};
    r.Q = a.Q; r.K = a.K; r.ldq = a.ldq; r.ldk = a.ldk; r.q_bs = a.q_bs; r.k_bs = a.k_bs; r.Lq = a.Lq; r.N = N; r.Np = p.Np; r.heads = a.heads; r.nbatch = B;
    r.scale_log2e = a.scale_log2e; r.lse = a.lse; r.bf16 = bf;
    r.share = use.share; r.peak_prob = use.peak_prob; r.peak_index = use.peak_index; r.entropy = use.entropy;
    if (L.rc) return;
    if (const char* e = cs_refuse_check(&r, dh)) { L.rc = fail(CS_ERR_BAD_ARG, "%s", e); return; }
    L.small("ref_use", [&] { return cs_refuse_launch(&r, dh, L.st); });
  }

  // What a forward keeps for the backwards.  The level is the deepest scope whose switch is on; the layer switch counts
  // for its own pieces only where there is a self-attention to keep them from, and as the cross switch otherwise.
  FitScope keep_level() const {
    if (h->cfg.dec_layers <= 0) return FIT_HEAD;
    if (h->layer_keep) return h->cfg.do_self_attn ? FIT_LAYER : FIT_CROSS;
    return h->cross_keep ? FIT_CROSS : h->tail_keep ? FIT_TAIL : FIT_HEAD;
  }
  // the handle's kept region, grown like the workspace and carved for this call's level (the backwards read the same carve: cs_fit::kept_carve)
  int ensure_kept(hipStream_t s) {
    kept = keep_level();
    if (kept == FIT_HEAD) return 0;
    const int heads = h->cfg.dec_heads;
    if (int r = grow_retired(h, &h->fit_kept, &h->fit_kept_bytes, cs_fit::kept_carve(nullptr, kept, B, p.Np, p.C, heads).end, s)) return r;
    kp = cs_fit::kept_carve(h->fit_kept, kept, B, p.Np, p.C, heads);
    return 0;
  }
  // One kept piece: M C elements copied on s into the kept region, counted in the census under the switch's name.  The decoder below keeps
  //   FIT_TAIL: x2 = p.xq and H = relu(linear1(x2)) = p.dhid between the last layer's norm2 and norm3 closings; both are overwritten by the time
  //     the forward returns.
  //   FIT_CROSS: x1 = p.xq, the rows that entered the cross-attention block (norm1's output, or the layer's input without self-attention), in front
  //     of the norm2 closing that overwrites it.  Q', the packed K | V rows, O and lse stay where they are: nothing behind the last layer's
  //     cross-attention writes p.dq (only a NOT-last layer's closing projects the next query into it), p.kv (written once, before the first layer),
  //     p.dob (the self-attention writes it, in front of the cross-attention) or p.lse, and mem is the caller's ref_tokens or p.mem_bf, which only
  //     the encoder / the gather write.
  //   FIT_LAYER: x0 = p.xq in front of the last layer's self-attention (the norm1 closing overwrites it) and Os = p.dob behind it (the
  //     cross-attention's output overwrites it); the self-attention writes its lse straight into kp.lse_s, since p.lse ends up with the
  //     cross-attention's.  The packed Q' | K | V rows stay where they are: nothing behind the last layer's self-attention writes p.dqkv.
  int keep_rows(void* dst, const void* src, size_t elem_bytes, const char* switch_name, hipStream_t s) {
    HIPCHK(hipMemcpyAsync(dst, src, (size_t)B * p.Np * p.C * elem_bytes, hipMemcpyDeviceToDevice, s));
    h->census[switch_name] += 1;
    return 0;
  }

  // The decoder runs as ONE group on the caller's stream, after the join: its kernels are small, and splitting the batch over streams only
  // makes them smaller (cfg-2, tools/dec_lanes.py: 1 group 8.77 ms, 2 groups 8.80, 3 groups 8.79, 4 groups 9.31).  Decoding each chunk's
  // items on its lane right after encoding them (no global join) was measured SLOWER too (833 vs 875 query-images/s on cfg-2): it doubles the
  // number of small decoder launches and the host enqueue rate becomes the limit.
  void decoder(Launcher& L) {
    const cs_config& c = h->cfg;
    const int C = p.C, P = c.patch, dec_dh = C / c.dec_heads, KV = 2 * C * c.dec_layers;
    const int M = B * p.Np, Mk = B * N * p.Np;
    hipStream_t s = L.st;
    const h16_t* mem = mode == 1 ? ref_tokens : p.mem_bf;
    // The next linears that ride along: the cross-attention's Q projection behind norm1, linear1 + ReLU behind norm2, the head's first linear +
    // LeakyReLU behind the last norm3 -- 16 launches per decoder + head instead of 21, at the same kernel time (34.5 vs 33.3 us per pair at
    // 10 952 rows).  The next layer's packed QKV projection (3 C wide) stays a GEMM of its own: in this kernel's 64-row shape it costs 62.5 us against 45.7.
    fused_ln = cs_rowln_supported(C) != 0 && !g_rowln_off;
    fuse_next = fused_ln && !g_rowln_no_next;
    auto next_of = [&](const h16_t* W, const float* b, h16_t* out, int act) { NextLinear x; x.W = W; x.b = b; x.out = out; x.n = C; x.act = act; return x; };
    // K/V projection of the memory (both layers at once).  Nothing before the first cross-attention depends on it, so with lanes
    // it runs on lane stream 1 next to layer 0's self-attention branch (the decoder phase has one small kernel in flight otherwise).
    const CsGemmParams kvp = gp(mem, C, h->Wkv_all, C, Mk, KV, C, h->bkv_all, p.kv, KV);
    const bool kv_side = NL >= 2 && c.do_self_attn && !h->prof;
    if (kv_side) {
      if (hipEventRecord(h->ev_kv0, s) != hipSuccess || hipStreamWaitEvent(lst[1], h->ev_kv0, 0) != hipSuccess) L.rc = CS_ERR_HIP;
      Launcher LK{h, lst[1]};
      LK.gemm(kvp, CS_EPI_BIAS_F16);
      if (LK.rc) L.rc = LK.rc;
      if (!L.rc && hipEventRecord(h->ev_kv1, lst[1]) != hipSuccess) L.rc = CS_ERR_HIP;
    } else {
      L.gemm(kvp, CS_EPI_BIAS_F16);
    }
    if (!L.rc) L.rc = ensure_kept(s);
    bool have_q = false, have_head0 = false;  // which projection a closing launch has already made
    for (int l = 0; l < c.dec_layers; ++l) {
      const DecLayer& D = h->dec[l];
      const bool last_l = l == c.dec_layers - 1;
      const float* shortcut = c.do_short_cut ? p.xq : nullptr;
      if (c.do_self_attn) {
        L.gemm(gp(p.q_bf, C, D.sa_Win, C, M, 3 * C, C, D.sa_bin, p.dqkv, 3 * C), CS_EPI_BIAS_F16);
        const bool keep_l = last_l && kept >= FIT_LAYER;  // whole-layer fit: x0, Os and the self-attention's lse kept
        if (keep_l && !L.rc) L.rc = keep_rows(kp.x0, p.xq, 4, "layer_keep", s);
        const CsAttnParams a = attn_params(p.dqkv, 3 * C, p.dqkv + C, p.dqkv + 2 * C, 3 * C, p.dob, p.Np, p.Np, c.dec_heads, keep_l ? kp.lse_s : nullptr);
        L.attn(a, dec_dh, B);
        if (keep_l && !L.rc) L.rc = keep_rows(kp.Os, p.dob, 2, "layer_keep", s);
        have_q = dec_close(L, p.dob, D.sa_Wo, D.sa_bo, shortcut, D.n1g, D.n1b, "norm1", next_of(D.ca_Wq, D.ca_bq, p.dq, 0));
      }
      if (kv_side && l == 0 && !L.rc && hipStreamWaitEvent(s, h->ev_kv1, 0) != hipSuccess) L.rc = CS_ERR_HIP;
      if (!have_q) L.gemm(gp(p.q_bf, C, D.ca_Wq, C, M, C, C, D.ca_bq, p.dq, C), CS_EPI_BIAS_F16);
      const bool want_w = attn_out && last_l;  // only the last layer's weights are returned (transformer.py:266-268)
      const bool want_use = last_l && use.any();  // reference use: the same layer, the same lse
      const bool want_fit = last_l && kept >= FIT_CROSS;  // cross-attention fit: lse for the backward, x1 kept below
      const CsAttnParams a = attn_params(p.dq, C, p.kv + (size_t)l * 2 * C, p.kv + (size_t)l * 2 * C + C, KV, p.dob, p.Np, N * p.Np, c.dec_heads, want_w || want_use || want_fit ? p.lse : nullptr);
      L.attn(a, dec_dh, B);
      if (want_w) L.small("attn_weights", [&] { return cs_attn_weights_launch(&a, dec_dh, B, head_id, attn_out, s); });
      if (want_use) reference_use(L, a, dec_dh);
      if (want_fit && !L.rc) L.rc = keep_rows(kp.x1, p.xq, 4, "cross_keep", s);
      if (!dec_close(L, p.dob, D.ca_Wo, D.ca_bo, shortcut, D.n2g, D.n2b, "norm2", next_of(D.l1W, D.l1b, p.dhid, 1)))
        L.gemm(gp(p.q_bf, C, D.l1W, C, M, C, C, D.l1b, p.dhid, C), CS_EPI_BIAS_RELU_F16);
      if (last_l && kept >= FIT_TAIL && !L.rc) L.rc = keep_rows(kp.x2, p.xq, 4, "tail_keep", s);
      if (last_l && kept >= FIT_TAIL && !L.rc) L.rc = keep_rows(kp.H, p.dhid, 2, "tail_keep", s);
      // behind norm3: the head's first linear (its hidden rows replace linear1's in dhid: a workgroup writes exactly the 64 rows it staged into
      // LDS at its start), or -- without self-attention -- the next layer's Q projection
      NextLinear next{};
      if (last_l) next = next_of(h->Wh0, h->bh0, p.dhid, 2);
      else if (!c.do_self_attn) next = next_of(h->dec[l + 1].ca_Wq, h->dec[l + 1].ca_bq, p.dq, 0);
      const bool rode = dec_close(L, p.dhid, D.l2W, D.l2b, p.xq, D.n3g, D.n3b, "norm3", next);
      have_q = rode && !last_l;
      have_head0 = rode && last_l;
      // tap: decoder layer l's output (transformer.py:157-173)
      if (h->capture && !L.rc)
        L.rc = tap_copy(h, "dec" + std::to_string(l) + "_out", p.xq, 0, (size_t)M * C * 4, (size_t)B * p.Np * C * 4, 0, {B, p.Np, C}, s);
    }
    // head + RegressionLayer + jigsaw (cross_reference.py:45-50,82-87)
    if (!have_head0) L.gemm(gp(p.q_bf, C, h->Wh0, C, M, C, C, h->bh0, p.dhid, C), CS_EPI_BIAS_LEAKY_F16);
    CsGemmParams g = gp(p.dhid, C, h->Wh2, C, M, P * P, C, h->bh2, score_out, 4);
    g.Np = p.Np; g.gw = p.gw; g.P = P; g.act = c.act; g.powp = c.pow_p;
    if (mean_out) { g.mean_part = p.mean_part; g.mean_cnt = p.mean_cnt; g.mean_out = mean_out; }
    L.gemm(g, CS_EPI_HEAD_SCORE);
    if (h->capture && !L.rc) {
      // tap: the head's second linear before the activation (cross_reference.py:45-50).  The score epilogue applies the activation in
      // registers, so the pre-activation is produced by one more launch of the same GEMM with a plain fp32 store (capture mode only).
      void* pre = nullptr;
      L.rc = tap_buffer(h, "head_pre_activation", (size_t)B * p.Np * P * P * 4, 0, {B, p.Np, (int64_t)P * P}, &pre);
      if (!L.rc) L.gemm(gp(p.dhid, C, h->Wh2, C, M, P * P, C, h->bh2, pre, P * P), CS_EPI_RESID_F32);
    }
  }

  // The forward as the sequence it is.  Every step enqueues on st or on a lane forked from and joined to it; nothing is waited for.
  int body() {
    if (int r = validate()) return r;
    if (int r = ensure_workspace()) return r;
    if (int r = ensure_tables(h, p.gh, p.gw, H == W, st)) return r;
    // the head launch's arrival counters (per-image mean in the same launch) start from zero; its finisher waves leave them at zero again, but the
    // workspace may have been carved differently by the previous call
    if (mean_out && mode != 2) HIPCHK(hipMemsetAsync(p.mean_cnt, 0, (size_t)B * sizeof(unsigned), st));
    if (int r = stage_select_triples()) return r;
    if (int r = stage_u8_descriptors()) return r;
    if (int r = ensure_lanes()) return r;
    Launcher LL[CS_MAX_LANES] = {Launcher{h, lst[0]}, Launcher{h, lst[1]}, Launcher{h, lst[2]}, Launcher{h, lst[3]}};
    // encoder lanes share the GPU: their GEMMs oversubscribe the CUs so that blocks are short and slots change hands often
    // (cfg-2, same box: 9.03 -> 8.84 ms with 3..16 blocks per CU; alone on the GPU two per CU is best: 9.27 vs 9.38..9.73 ms)
    if (NL >= 2) for (Launcher& L : LL) L.bpc = 4;
    if (int r = fork_lanes()) return r;
    if (int r = encoder_rounds(LL)) return r;
    if (int r = join_lanes()) return r;
    for (const Launcher& L : LL) if (L.rc) return L.rc;
    Launcher LD{h, st};  // every image's tokens are in place (join above) before the decoder starts
    if (mode == 3) {
      select_references(LD);
      if (LD.rc) return LD.rc;
    }
    if (int r = tap_featmaps()) return r;
    if (mode == 2) return 0;
    decoder(LD);
    if (LD.rc) return LD.rc;
    if (!h->cfg.skip_finite_check)
      LD.misc("score_check", -1, 0, 0, [&] { return cs_score_check_launch(score_out, (size_t)B * p.gh * h->cfg.patch * p.gw * h->cfg.patch, h->nonfinite, st); });
    return LD.rc;
  }
};

// Wraps EVERY exit of the body: the cross-stream wait before it; the census, the table hold, the timing and the completion event around it.
int forward_impl(Fwd f) {
  // The workspace is shared by every call on this handle: a call on a different stream than the previous one first waits for that
  // one to finish (calls on one stream are ordered anyway).
  cs_model* h = f.h;
  if (!h) return fail(CS_ERR_BAD_ARG, "null handle");
  if (f.mode != 2) { f.use = h->ref_use; h->ref_use = cs_model::RefUse{}; }  // one-shot: gone whatever this call returns
  if (int r = call_enter(h, f.st)) return r;
  h->census.clear();
  const auto t0 = std::chrono::steady_clock::now();
  if (f.u8) cs_preprocess_tables_hold(1);  // (the filter tables its descriptors point at stay put until everything is queued: preprocess.hip)
  const int rc = f.body();
  if (f.u8) cs_preprocess_tables_hold(0);
  // what cs_head_backward works on: the tokens behind the last norm3 and the head's hidden rows of THIS call (f.p: the plan body() carved)
  h->last_fwd = cs_model::LastForward{rc == 0, f.mode, f.B, f.H, f.W, f.p.xq, f.p.dhid, f.kept};
  if (f.kept >= FIT_CROSS) {  // (the decoder ran: the plan is carved and the handle has a last layer)
    cs_model::LastForward& lf = h->last_fwd;
    const int C = h->cfg.hidden, L = h->cfg.dec_layers;
    lf.N = f.N; lf.dq = f.p.dq; lf.k = f.p.kv + (size_t)(L - 1) * 2 * C; lf.ldkv = 2 * C * L; lf.dob = f.p.dob; lf.lse = f.p.lse;
    lf.mem = f.mode == 1 ? f.ref_tokens : f.p.mem_bf;
    lf.dqkv = f.p.dqkv;
  }
  h->host_enqueue_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (int r = call_leave(h, f.st)) return r;
  return rc;
}

// The four cs_forward_select* entry points: mode 3 over fp32 (`query`) or uint8 (`u8`) queries, `s` plain or grouped
int forward_select(cs_handle h, const float* query, const U8In* u8, const uint16_t* bank_tokens, const SelectIn& s, int B, int N, int H, int W,
                   float* score_out, float* attn_out, int head_id, float* mean_out, cs_stream stream) {
  Fwd f{h, 3, query, nullptr, bank_tokens, nullptr, B, N, H, W, score_out, attn_out, head_id, mean_out, (hipStream_t)stream, u8};
  f.sel = &s;
  return forward_impl(f);
}

}  // namespace

extern "C" {

size_t cs_workspace_bytes(cs_handle h, int B, int N, int H, int W) {
  if (!h || B <= 0 || N <= 0 || H < h->cfg.patch || W < h->cfg.patch) return 0;
  return make_plan(h, B, N, N, H, W, nullptr).total;
}

int cs_forward(cs_handle h, const float* query, const float* refs, int B, int N, int H, int W, float* score_out, float* attn_out,
               int head_id, float* mean_out, cs_stream stream) {
  return forward_impl(Fwd{h, 0, query, refs, nullptr, nullptr, B, N, H, W, score_out, attn_out, head_id, mean_out, (hipStream_t)stream, nullptr});
}

int cs_request_reference_use(cs_handle h, float* share, float* peak_prob, int32_t* peak_index, float* entropy) {
  if (!h) return fail(CS_ERR_BAD_ARG, "null handle");
  h->ref_use = cs_model::RefUse{share, peak_prob, peak_index, entropy};
  return 0;
}

int cs_encode_references(cs_handle h, const float* imgs, int R, int H, int W, uint16_t* tokens_out, cs_stream stream) {
  return forward_impl(Fwd{h, 2, imgs, nullptr, nullptr, tokens_out, R, 0, H, W, nullptr, nullptr, 0, nullptr, (hipStream_t)stream, nullptr});
}

int cs_forward_cached(cs_handle h, const float* query, const uint16_t* ref_tokens, int B, int N, int H, int W, float* score_out,
                      float* attn_out, int head_id, float* mean_out, cs_stream stream) {
  return forward_impl(Fwd{h, 1, query, nullptr, ref_tokens, nullptr, B, N, H, W, score_out, attn_out, head_id, mean_out, (hipStream_t)stream, nullptr});
}

// The three forwards fed from decoded uint8 images (SURVEY.md 8f-4 as worded: uint8 in, tokens out; include/crossscore_hip.h)
int cs_forward_u8(cs_handle h, const cs_u8_image* query, const cs_u8_image* refs, int B, int N, int H, int W, const float* mean3, const float* std3,
                  float* score_out, float* attn_out, int head_id, float* mean_out, cs_stream stream) {
  const U8In u{query, refs, mean3, std3};
  return forward_impl(Fwd{h, 0, nullptr, nullptr, nullptr, nullptr, B, N, H, W, score_out, attn_out, head_id, mean_out, (hipStream_t)stream, &u});
}

int cs_encode_references_u8(cs_handle h, const cs_u8_image* imgs, int R, int H, int W, const float* mean3, const float* std3, uint16_t* tokens_out,
                            cs_stream stream) {
  const U8In u{imgs, nullptr, mean3, std3};
  return forward_impl(Fwd{h, 2, nullptr, nullptr, nullptr, tokens_out, R, 0, H, W, nullptr, nullptr, 0, nullptr, (hipStream_t)stream, &u});
}

int cs_forward_cached_u8(cs_handle h, const cs_u8_image* query, const uint16_t* ref_tokens, int B, int N, int H, int W, const float* mean3,
                         const float* std3, float* score_out, float* attn_out, int head_id, float* mean_out, cs_stream stream) {
  const U8In u{query, nullptr, mean3, std3};
  return forward_impl(Fwd{h, 1, nullptr, nullptr, ref_tokens, nullptr, B, N, H, W, score_out, attn_out, head_id, mean_out, (hipStream_t)stream, &u});
}

int cs_forward_select(cs_handle h, const float* query, const uint16_t* bank_tokens, const float* bank_unit, const float* centre, int R,
                      const int32_t* exclude, int B, int N, int H, int W, float* score_out, float* attn_out, int head_id, float* mean_out,
                      int32_t* index_out, float* sim_out, cs_stream stream) {
  const SelectIn s{bank_unit, centre, R, exclude, index_out, sim_out};
  return forward_select(h, query, nullptr, bank_tokens, s, B, N, H, W, score_out, attn_out, head_id, mean_out, stream);
}

int cs_forward_select_u8(cs_handle h, const cs_u8_image* query, const uint16_t* bank_tokens, const float* bank_unit, const float* centre, int R,
                         const int32_t* exclude, int B, int N, int H, int W, const float* mean3, const float* std3, float* score_out,
                         float* attn_out, int head_id, float* mean_out, int32_t* index_out, float* sim_out, cs_stream stream) {
  const U8In u{query, nullptr, mean3, std3};
  const SelectIn s{bank_unit, centre, R, exclude, index_out, sim_out};
  return forward_select(h, nullptr, &u, bank_tokens, s, B, N, H, W, score_out, attn_out, head_id, mean_out, stream);
}

int cs_forward_select_grouped(cs_handle h, const float* query, const uint16_t* bank_tokens, const float* bank_unit, const float* centre, int R,
                              const int32_t* offsets, int G, const int32_t* query_group, int blank_row, const int32_t* exclude, int B, int N, int H,
                              int W, float* score_out, float* attn_out, int head_id, float* mean_out, int32_t* index_out, float* sim_out,
                              cs_stream stream) {
  if (!offsets) return fail(CS_ERR_BAD_ARG, "cs_forward_select_grouped: offsets missing");
  const SelectIn s{bank_unit, centre, R, exclude, index_out, sim_out, offsets, G, query_group, blank_row};
  return forward_select(h, query, nullptr, bank_tokens, s, B, N, H, W, score_out, attn_out, head_id, mean_out, stream);
}

int cs_forward_select_grouped_u8(cs_handle h, const cs_u8_image* query, const uint16_t* bank_tokens, const float* bank_unit, const float* centre,
                                 int R, const int32_t* offsets, int G, const int32_t* query_group, int blank_row, const int32_t* exclude, int B,
                                 int N, int H, int W, const float* mean3, const float* std3, float* score_out, float* attn_out, int head_id,
                                 float* mean_out, int32_t* index_out, float* sim_out, cs_stream stream) {
  if (!offsets) return fail(CS_ERR_BAD_ARG, "cs_forward_select_grouped_u8: offsets missing");
  const U8In u{query, nullptr, mean3, std3};
  const SelectIn s{bank_unit, centre, R, exclude, index_out, sim_out, offsets, G, query_group, blank_row};
  return forward_select(h, nullptr, &u, bank_tokens, s, B, N, H, W, score_out, attn_out, head_id, mean_out, stream);
}

int cs_u8_input_supported(cs_handle h, const cs_u8_image* im, int H, int W) {
  if (!h || !h->finalized || !im) return 0;
  const cs_config& c = h->cfg;
  if (h->lnfold || !h->Wpatch_frag || !cs_patch_fused_supported(H, W, c.patch, c.hidden)) return 0;
  if (im->h <= 0 || im->w <= 0 || im->rs_h <= 0 || im->rs_w <= 0 || im->crop_y < 0 || im->crop_x < 0 || im->crop_y + H > im->rs_h || im->crop_x + W > im->rs_w) return 0;
  CsU8Tables t{};
  int span = 0;
  if (cs_preprocess_tables(im->h, im->w, im->rs_h, im->rs_w, im->crop_y, H / c.patch, c.patch, &t, &span, nullptr) != hipSuccess) return 0;
  return cs_patch_u8_runs(W, span) > 0 ? 1 : 0;
}

}  // extern "C"
