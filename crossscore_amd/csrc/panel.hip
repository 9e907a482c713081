// Encoder token-panel kernel for gfx950 (ViT-S: C = 384, MLP 4C = 1536): everything a DINOv2 layer does between its attention
// and the next layer's QKV projection, in ONE launch, with the 4C hidden activations never leaving the CU.
//
//   x   += attn_o Wo'^T + bo'                       Dinov2SelfOutput + layer_scale1 + residual   (HF modeling_dinov2.py:249-252,365-370)
//   x   += GELU(LN2(x) W1'^T + b1') W2'^T + b2'     norm2 + Dinov2MLP + layer_scale2 + residual  (HF:373-378, 293-297)
//   u    = f16((x - mean(x)) * rstd(x))             norm1 of the next layer (its gamma/beta live in that layer's packed Wqkv / bias)
//
// Replaces five launches of round 1 (out-proj GEMM, LayerNorm, fc1+GELU GEMM, fc2 GEMM, LayerNorm) and their HBM round trips.
//
// Structure: a workgroup = 8 waves = 128 token rows = 4 wave PAIRS; the two waves of a pair sit on the same SIMD (waves w and w+4)
// and share 32 rows, with different roles:
//   * the A wave (waves 0-3) owns fc1: it keeps norm2(x) of its 32 rows as 24 MFMA B fragments in registers, multiplies one
//     32-wide hidden slice per "tick" (24 weight fragments, 48 MFMAs) and runs the GELU of the PREVIOUS slice's first 16 rows on the
//     VALU between those MFMAs; the activated half goes to its partner through a 1-KiB LDS slot as a ready-made B fragment, the
//     pre-activations of the other 16 rows as they are;
//   * the B wave (waves 4-7) owns the residual rows: 32 x 384 fp32 accumulators (192 registers).  It does the attention output
//     projection onto them, LayerNorm (hands norm2(x) to the A wave through LDS), then one fc2 slice per tick (24 fragments, 48 MFMAs),
//     two ticks behind the A wave, and finally writes x and the next layer's normalised rows.
// So every SIMD has one VALU-heavy and one MFMA/LDS-only instruction stream feeding the same matrix pipe (the one-wave-per-SIMD
// version of this kernel was issue-bound: MFMA issue + GELU + LDS-DMA issue of ONE wave exceeded the MFMA pipe time 1.6x).
// MFMA v_mfma_f32_16x16x32_f16 (the shape the chip sustains the higher clock on at the power cap: DESIGN.md 4), WEIGHT fragment = A
// operand (16 output features x 32 k), activation fragment = B operand (32 k x 16 token rows), D[feature][row].  With
// li = lane & 15, g = lane >> 4: lane (li, g) of an A fragment holds feature row li, contraction slots 8g .. 8g+7 (16 B); of a B
// fragment token li, slots 8g .. 8g+7; of a D tile token li, features 4g .. 4g+3 (4 registers).  A pair's 32 rows are two ROW TILES
// rt = 0, 1 (rows 16 rt + li): every weight fragment is read from LDS once and feeds two MFMAs, one per row tile, back to back on
// independent accumulators -- the fragment count, the LDS bytes per FLOP and the MFMA cycles are those of the 32x32x16 form.
// Two D tiles of one row tile, feature tiles f0 and f1, rounded to 16 bits are the B fragment of the next product with contraction
// slot 8g + e = feature 16 f(e >> 2) + 4g + (e & 3), which the packed weights carry, so LN output -> fc1 (k-step ks = feature tiles
// 2ks, 2ks+1 of the residual accumulators) and GELU output -> fc2 (one k-step = the slice's two feature tiles) need no cross-lane
// movement; D row i of feature tile T is feature 16 T + i, no permutation of the output features.
// Weights stream L2 -> LDS by global_load_lds_dwordx4 as 24-KiB chunks (= 24 fragments of 1 KiB, stored in the order and the
// lane-linear layout they are read in: every ds_read_b128 / LDS-DMA piece is 64 lanes x 16 contiguous bytes, no swizzle needed)
// through a 3-slot ring, two chunks in flight, counted s_waitcnt vmcnt + one raw s_barrier per chunk.  A chunk is one half tick:
// [12 fragments for the A waves (k-steps 0..5 or 6..11 of an fc1 slice x its 2 feature tiles) | 12 for the B waves (12 of the 24 output
// tiles of an fc2 slice)].
#include "cs_common.h"
#include "panel_shared.h"
#include <atomic>
#include <stdlib.h>
#include <type_traits>
#include <utility>

namespace {

constexpr int PC = 384;               // hidden size
constexpr int PF = 1536;              // MLP hidden
constexpr int NT = PC / 16;           // 24 output (feature) tiles of 16 features
constexpr int KS = PC / 32;           // 12 k-steps over C
constexpr int NXF = 2 * KS;           // 24 norm2(x) fragments of a pair: (k-step, row tile) at index 2 ks + rt
constexpr int NSL = PF / 32;          // 48 hidden slices of 32 (two feature tiles for fc1, one k-step for fc2)
constexpr int FRAG = 1024;            // bytes of one MFMA operand fragment (64 lanes x 16 B)
constexpr int CHUNK = 24 * FRAG;      // out-projection unit: one k-step x 24 tiles
constexpr int TICK = 48 * FRAG;       // MLP unit: one tick = [24 fragments of an fc1 slice (A waves) | 24 of an fc2 slice (B waves)]
constexpr int OUT_CHUNKS = KS;        // 12 out-projection units
constexpr int LAGT = 2;               // ticks the fc2 side runs behind the fc1 side
constexpr int NTICK = NSL + LAGT;     // 50 MLP units
constexpr int PAD_TICKS = 1;          // fetched by the last transition, never read
constexpr int PANEL_ROWS = 128;
// LDS map.  Out-projection phase: 3 ring slots of 24 KiB, the residual-row tiles and attention-output fragments that travel with them.
// MLP phase: 2 ring slots of 48 KiB (one barrier per tick) over the ring and the start of the then-idle tile region, activation slots.
constexpr int LDS_RING = 0;
constexpr int LDS_X = 3 * CHUNK;                     // 72 K: 3 slots x 4 pairs x one 6-KiB record [4 residual tiles of 1 KiB | 2 attention-output fragments]
constexpr int XREC = 6 * FRAG;                       //       (one record, one address register on the B side: r4)
constexpr int LDS_OF = LDS_X + 3 * 4 * 4 * FRAG;     // 120 K (the MLP phase's hand-off areas start here; the out-projection records end at 144 K)
constexpr int LDS_XF = 2 * TICK;                     // 96 K: norm2(x) hand-off, 4 pairs x 12 fragments at a time (48 KiB; ends at 144 K)
// 120 K, MLP phase: the pairs' hand-off areas of 6 KiB each (one base register, everything else immediates):
//   [fc2 activation fragment of row tile 0, slot 0 | slot 1 (1 KiB each: written by the A wave) | row tile 1's 8 pre-activations per lane, slot 0 |
//    slot 1 (2 KiB each: packed halves in the first KiB in fp16 mode, fp32 in bf16 mode; the B wave activates them)]
constexpr int LDS_HB = LDS_OF;
constexpr int HB_PAIR = 6 * FRAG;
constexpr int HB_RAW = 2 * FRAG;
constexpr int LDS_B1 = LDS_OF + 3 * 4 * 2 * FRAG;    // 144 K: fc1 bias, fp32
constexpr int LDS_BV = LDS_B1 + PF * 4;              // bo | b2, fp32
constexpr int LDS_BYTES = LDS_BV + 2 * PC * 4;       // 153 KiB
// epilogue staging (over the ring, idle by then): per pair 32 rows x 768 B (half a residual row, or a whole normalised f16 row), rows
// padded to 784 B.  A ds_write_b128 is served in groups of 8 consecutive lanes on 32 banks: a B wave's group is 8 consecutive rows (lanes
// li .. li+7 of one lane group g) at one column, and 784 B = 196 dwords = 4 (mod 32) puts their 4-dword pieces on 8 disjoint bank quads --
// conflict-free (any pitch = 4 (mod 8) dwords that is a multiple of 16 B does; 784 is the smallest above 768).  The A waves' reads are
// row-contiguous (16 lanes x 16 B of one row).  The 8-byte writes of the normalised rows (16 rows of a lane group, 2 dwords each) are 2-way
// on this pitch: 48 writes per lane and launch, not worth a second pitch.
constexpr int ST_ROW = 784;
constexpr int ST_PAIR = 32 * ST_ROW;

typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
template <int OFF>
__device__ __forceinline__ void lds_write8(unsigned addr, u32x2_t v) {
  asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory");
}

#ifdef CS_PANEL_ABLATE
// diagnostic builds only: per (block < 64, wave) six s_memtime stamps + s_memrealtime at both ends (tools/panel_ablate.py)
__device__ unsigned long long g_panel_dbg[64 * 8 * 16];
#define CS_STAMP(k) do { if (blockIdx.x < 64 && lane == 0) { \
    __builtin_amdgcn_sched_barrier(0); g_panel_dbg[(blockIdx.x * 8 + wv) * 16 + (k)] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } } while (0)
#define CS_STAMP_RT(k) do { if (blockIdx.x < 64 && lane == 0) g_panel_dbg[(blockIdx.x * 8 + wv) * 16 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
// arrival / release times at the MLP phase's unit boundaries v = 40 .. 55 (ticks 20 .. 27) of blocks 0 .. 3: who is late at the barriers?
__device__ unsigned long long g_panel_bar[4 * 8 * 16 * 2];
#define CS_BAR_STAMP(v, k) do { if (blockIdx.x < 4 && (v) >= 40 && (v) < 56 && (threadIdx.x & 63) == 0) { \
    __builtin_amdgcn_sched_barrier(0); g_panel_bar[((blockIdx.x * 8 + wv) * 16 + ((v) - 40)) * 2 + (k)] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } } while (0)
#else
#define CS_STAMP(k) do { } while (0)
#define CS_STAMP_RT(k) do { } while (0)
#define CS_BAR_STAMP(v, k) do { } while (0)
#endif

// ABL: timing-only ablations (tools/panel_ablate.py builds them with -DCS_PANEL_ABLATE; results are wrong by design):
//   1 no GELU arithmetic, 2 no weight LDS-DMA after the first two MLP units, 16 no s_barrier per unit, 64 transition-time accounting
template <bool OUTPROJ, int ABL = 0, bool BF = false>
__global__ __launch_bounds__(512, 2) void cs_panel_kernel(CsPanelParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool is_a = wv < 4;
  const int pair = wv & 3;
  const int li = lane & 15, g = lane >> 4;
  const int row0 = blockIdx.x * PANEL_ROWS + pair * 32;
  const unsigned rowt[2] = {(unsigned)min(row0 + li, p.M - 1), (unsigned)min(row0 + 16 + li, p.M - 1)};  // this lane's row of row tile 0 / 1
  constexpr int NOUT = OUTPROJ ? OUT_CHUNKS : 0;
  constexpr size_t IMG_MLP = (size_t)NOUT * CHUNK;  // byte offset of MLP unit 0 in the image
  const unsigned lds0 = (unsigned)(size_t)CS_LDS_PTR(smem);
  const unsigned lane16 = lane * 16;
  // per-lane 32-bit byte offsets (the 64-bit addresses are formed where they are used, from the kernel arguments: no address pair stays live)
  // per row tile: this lane's 4 floats of feature tile 0 of its residual row (M * 1536 < 2^32: cs_panel_check), its 8 halves of k-step 0 of
  // its attention-output row
  const unsigned xoff[2] = {rowt[0] * (PC * 4) + 16 * g, rowt[1] * (PC * 4) + 16 * g};
  const unsigned ooff[2] = {rowt[0] * (PC * 2) + 16 * g, rowt[1] * (PC * 2) + 16 * g};

  // Units: u < NOUT an out-projection chunk (24 KiB, ring slot u % 3, fetched two units ahead); u = NOUT + t MLP tick t (48 KiB, ring slot
  // t % 2, fetched one unit ahead).  The A waves copy the out-projection units (with their pair's residual-row tile and attention-output
  // fragments) and MLP ticks 0 and 1 -- the B waves issue no vector-memory instruction before the MLP phase --, the B waves every later
  // tick, one 1-KiB piece per MFMA gap.
  int u_next = 0;  // next unit to make current
  auto out_unit_issue = [&](int c) {  // A waves: out-projection chunk c with its tile and fragments
    const int slot = c % 3;
    const unsigned dst = lds0 + LDS_RING + slot * CHUNK + pair * 6 * FRAG;
    const char* s6 = reinterpret_cast<const char*>(p.img) + (size_t)c * CHUNK + pair * 6 * FRAG + lane16;
    dma_piece<0>(s6, dst); dma_piece<FRAG>(s6, dst); dma_piece<2 * FRAG>(s6, dst); dma_piece<3 * FRAG>(s6, dst);
    dma_piece<0>(s6 + 4 * FRAG, dst + 4 * FRAG); dma_piece<FRAG>(s6 + 4 * FRAG, dst + 4 * FRAG);
    // residual feature tiles 2c and 2c+1 in the accumulator layout (piece q = tile 2c + (q >> 1) of row tile q & 1: a lane's 4 registers are
    // 16 contiguous bytes of its row) and the two row tiles' B fragments of k-step c (16 contiguous bytes of the attention-output row)
    const unsigned dx = lds0 + LDS_X + (slot * 4 + pair) * XREC;
    const char* sx0 = reinterpret_cast<const char*>(p.x) + (size_t)(xoff[0] + c * 128);
    const char* sx1 = reinterpret_cast<const char*>(p.x) + (size_t)(xoff[1] + c * 128);
    dma_piece<0>(sx0, dx); dma_piece<0>(sx1, dx + FRAG); dma_piece<0>(sx0 + 64, dx + 2 * FRAG); dma_piece<0>(sx1 + 64, dx + 3 * FRAG);
    const unsigned dof = dx + 4 * FRAG;
    dma_piece<0>(reinterpret_cast<const char*>(p.attn_o) + (size_t)(ooff[0] + c * 64), dof);
    dma_piece<0>(reinterpret_cast<const char*>(p.attn_o) + (size_t)(ooff[1] + c * 64), dof + FRAG);
  };
  // MLP weight stream (r4): the image is cut into HALF-tick units v = 2 t + hf of 24 KiB, [12 fragments of the A waves | 12 of the B waves]
  // (fc1 slice t, fragments 12 hf .. 12 hf + 11 = k-steps 6 hf .. 6 hf + 5 x 2 feature tiles | fc2 slice t - 2, feature tiles 12 hf .. 12 hf + 11);
  // unit v lives at ring offset (v & 3) * 24 KiB, i.e.
  // tick t still occupies the 48-KiB half (t & 1) of the ring.  Every A wave copies six 1-KiB pieces of a unit (pair * 6 + K).
  int pend_u = 0;          // unit whose pieces issue_piece() copies
  bool pend = false;       // ... if any
  auto issue_piece = [&](auto K_) {
    constexpr int K = decltype(K_)::value;
    const unsigned dst = lds0 + LDS_RING + (pend_u & 3) * CHUNK + (pair * 6 + (K & ~3)) * FRAG;
    const char* s = reinterpret_cast<const char*>(p.img) + (IMG_MLP + (size_t)pend_u * CHUNK + (pair * 6 + (K & ~3)) * FRAG) + lane16;
    dma_piece<(K & 3) * FRAG>(s, dst);
  };
  auto tick_issue_all = [&](int t) {  // a wave's whole share of tick t at once (outside the tick loops): unit 2t first, then 2t + 1
    sfor<12>([&](auto K_) {
      constexpr int K = decltype(K_)::value % 6, HF = decltype(K_)::value / 6;
      const unsigned dst = lds0 + LDS_RING + (t & 1) * TICK + HF * CHUNK + (pair * 6 + (K & ~3)) * FRAG;
      const char* s = reinterpret_cast<const char*>(p.img) + (IMG_MLP + (size_t)t * TICK + HF * CHUNK + (pair * 6 + (K & ~3)) * FRAG) + lane16;
      dma_piece<(K & 3) * FRAG>(s, dst);
    });
  };
  unsigned long long tw_drain = 0, tw_vm = 0, tw_bar = 0;  // (ABL & 64: where a transition's time goes, summed over the launch)
  // transition into unit u_next: this wave's LDS reads of the current unit are complete (its slot may be refilled right after the barrier)
  // and its own LDS-DMA pieces of unit u_next have landed; barrier (the same holds for every wave); then the next fetch is started (or, with
  // `defer`, left to issue_piece() between the caller's MFMAs).  Returns this lane's LDS address of fragment 0 of unit u_next.
  auto transition = [&](auto ISA_) -> unsigned {
    constexpr bool ISA = decltype(ISA_)::value;
    CS_SB();
    unsigned long long ta = 0, tb = 0, tc = 0, td = 0;
    if constexpr (ABL & 64) { asm volatile("s_memtime %0" : "=s"(ta)::"memory"); }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if constexpr (ABL & 64) { asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tb)::"memory"); }
    if constexpr (ISA) {
      if (u_next + 1 < NOUT) CS_VMCNT(12);  // the out-projection unit after u_next may still be in flight
      else CS_VMCNT(0);
    } else {
      CS_VMCNT(0);
    }
    if constexpr (ABL & 64) { asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tc)::"memory"); }
    if constexpr (!(ABL & 16)) __builtin_amdgcn_s_barrier();
    if constexpr (ABL & 64) {
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(td)::"memory");
      tw_drain += tb - ta; tw_vm += tc - tb; tw_bar += td - tc;
    }
    asm volatile("" ::: "memory");
    if (u_next + 2 < NOUT) {
      if constexpr (ISA && OUTPROJ) out_unit_issue(u_next + 2);
    } else if (u_next + 1 >= NOUT) {
      const int t = u_next + 1 - NOUT;  // the tick to fetch now (the image ends with PAD_TICKS: no tail case)
      // MLP ticks 0 and 1 (units 0..3) are fetched here, whole, by the A waves; every later unit at the MLP phase's own unit boundaries
      if constexpr (ISA) {
        if (t < 2) tick_issue_all(t);
      }
    }
    const unsigned base = lds0 + LDS_RING + lane16 + (u_next < NOUT ? (u_next % 3) * CHUNK : ((u_next - NOUT) & 1) * TICK);
    ++u_next;
    CS_SB();  // (register-only MFMAs must not be scheduled above the waits of this statement)
    return base;
  };
  using TA = std::true_type;
  using TB = std::false_type;
  h16x8_t w[6];  // rolling pool of weight fragments: fragment k of a unit lives in w[k % 6], five reads ahead of its MFMA

  if (is_a) {
    // =====================================================================================================================
    // A wave: loader of the out-projection phase, then fc1 + GELU
    // =====================================================================================================================
    CS_STAMP_RT(8); CS_STAMP(0);
    // bias vectors -> LDS once per workgroup: fc1 (LN2 beta folded in), out-projection and fc2 (LayerScale folded in)
    for (int i = tid; i < PF / 4; i += 256)
      reinterpret_cast<f32x4_t*>(smem + LDS_B1)[i] = reinterpret_cast<const f32x4_t*>(p.b1)[i];
    if (tid < PC / 4) {
      reinterpret_cast<f32x4_t*>(smem + LDS_BV)[tid] = OUTPROJ ? reinterpret_cast<const f32x4_t*>(p.bo)[tid] : f32x4_t{0.f, 0.f, 0.f, 0.f};
      reinterpret_cast<f32x4_t*>(smem + LDS_BV + PC * 4)[tid] = reinterpret_cast<const f32x4_t*>(p.b2)[tid];
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    if constexpr (OUTPROJ) { out_unit_issue(0); out_unit_issue(1); }
    else tick_issue_all(0);
    unsigned cur = transition(TA{});              // unit 0
    CS_STAMP(1);
    for (int c = 0; c < NOUT; ++c) cur = transition(TA{});  // the B waves multiply units 0 .. NOUT-1; `cur` ends at MLP tick 0
    CS_STAMP(2);
    // ---- norm2(x) from the partner: two halves of 12 fragments through the hand-off region ----
    h16x8_t xf[NXF];  // fragment 2 ks + rt
    const unsigned r_addr = lds0 + LDS_XF + pair * 12 * FRAG + lane16;
    __builtin_amdgcn_s_barrier();  // H1: first half written
    sfor<12>([&](auto F_) { lds_read1<decltype(F_)::value * FRAG>(r_addr, xf[decltype(F_)::value]); });
    CS_LGKM(0);
    __builtin_amdgcn_s_barrier();  // H2: first half read
    __builtin_amdgcn_s_barrier();  // H3: second half written
    sfor<12>([&](auto F_) { lds_read1<decltype(F_)::value * FRAG>(r_addr, xf[12 + decltype(F_)::value]); });
    CS_LGKM(0);
    CS_STAMP(3);

    // ---- fc1 ticks.  Tick t: acc(t & 1) = b1 + W1[slice t] . xf (24 fragments of the tick's unit, fragment m = k-step m >> 1, feature tile
    //      m & 1, two MFMAs each: row tiles 0 and 1); the GELU of slice t-1 (the other accumulator) rides in the gaps between the fragments
    //      and leaves as the B fragment of row tile 0 in hb slot (t-1) & 1 before the tick's second boundary (gap 18): the partner multiplies
    //      it from tick t+1 on ----
    struct Acc { f32x4_t v[4]; };  // a slice's fc1 tiles: v[2 rt + ft] = D tile (feature tile ft, row tile rt): hidden units 32 t + 16 ft + 4 g + i
    Acc acE, acO;                  // even / odd slices
    const unsigned bias_addr = lds0 + LDS_B1 + 16 * g;
    f32x4_t bb[2];
    auto read_bias = [&](int t) {  // this lane's 2 x 4 hidden units of slice t: 32 t + 16 ft + 4 g + i
      const unsigned a = bias_addr + t * 128;
      lds_read_f4<0>(a, bb[0]); lds_read_f4<64>(a, bb[1]);
    };
    // One tick: per fragment m [counted wait for it; two MFMAs; read of fragment m + 6 (of the next unit from m = 18 on); a GELU block]; the
    // transition to the next unit sits before fragment 18, when all 24 fragments of this unit are in registers or behind it in the LDS queue.
    // hb_write = false for tick 0: its "previous slice" does not exist, and the hand-off areas lie inside the norm2 hand-off region (LDS_XF),
    // which the sibling pairs' A waves may still be reading behind H3 -- nothing may be written there before the first tick's transition
    // GELU split (r4): the VALU work of a slice is shared by the two waves of the pair -- a single wave issues a vector instruction every 4-8
    // cycles, and with all 16 values per lane on the A wave its instruction stream set the tick (2 600 cycles against 1 536 of MFMA) while the
    // B wave idled at the barrier.  The A wave activates the 8 values of ROW TILE 0 (tiles v[0], v[1]: in slot order e = 4 ft + i they are that
    // row tile's fc2 B fragment) and hands the 8 values of row tile 1 (v[2], v[3]) over as they are -- packed halves in fp16 mode (1 KiB per
    // pair), fp32 in bf16 mode (2 KiB; its relu must keep fp32's range) -- in gap 3 of the tick; the B wave activates those.
    // Every fc2 weight fragment feeds both row tiles at once, so the B wave needs BOTH fragments of slice s when its tick s + 2 starts: it
    // reads the raw half behind the boundary of gap 6 of its tick s + 1 -- this wave's lgkmcnt(3) in front of that barrier retires the write of
    // gap 3, and nothing younger than it -- and activates it in the gaps 12..23 of that tick, one block per gap; this wave's own fragment (gap 11)
    // is retired by the counted wait of gap 17 and read by the partner behind the boundary of gap 18.
    // Slot parities.  Slice s uses fragment slot s & 1 and raw slot s & 1.  Raw slot: written in gap 3 of tick s + 1, i.e. behind boundary
    // 2 s + 1; its previous content (slice s - 2) was read by the partner in gaps 6.. of tick s - 1, and the partner's counted waits retired
    // that read before it arrived at boundary 2 s - 1.  Fragment slot: written in gap 11 of tick s + 1, behind boundary 2 s + 2; its
    // previous content (slice s - 2) was read by the partner behind boundary 2 s - 1 (gap 18 of tick s - 1) and retired by its counted waits
    // before it arrived at boundary 2 s.  No slot is rewritten before its reader is done, with at least one whole boundary to spare.
    // Unit boundaries of the MLP phase (r4).  Round 3 had ONE barrier per tick with an LDS drain in front of it (the slot of the tick just
    // read was refilled right behind the barrier): all eight waves stopped issuing MFMAs, emptied their prefetch queues, met, and refilled
    // them -- the matrix pipe idled a quarter of every tick.  Now a unit is HALF a tick and is released LATE: the barrier in front of the first
    // read of unit v + 1 (gap 6 / gap 18) only says "unit v + 1 has landed and everybody is done with unit v - 1" -- which the counted LDS waits
    // of the gaps in between already guarantee -- so nobody drains anything, the reads in flight across the barrier target units v and v + 1,
    // and the loader refills the slot of unit v - 1 with unit v + 3 (one 1-KiB piece per gap, 6 per A wave) two boundaries ahead of its use.
    const unsigned hb_base = lds0 + LDS_HB + pair * HB_PAIR + lane16;
    const unsigned ring = lds0 + LDS_RING + lane16;   // + (t & 1) * TICK: this lane's address of tick t's fragment 0
    unsigned xa[4] = {0u, 0u, 0u, 0u}, xb[4];  // (fp16 mode) the previous slice as packed halves: this wave's pairs, the partner's
    PkGelu pg;
    const PkGeluK kk = pk_gelu_consts();
    auto boundary = [&](auto FC1_, int v) {  // in front of the first read of unit v + 1
      CS_SB();
      if constexpr (!decltype(FC1_)::value) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }  // (last tick: no counted waits retire its hand-off writes)
      CS_BAR_STAMP(v, 0);
      CS_VMCNT(6);  // this wave's pieces of unit v + 1 have landed (those of unit v + 2, issued one boundary ago, may be in flight)
      if constexpr (!(ABL & 16)) __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      CS_BAR_STAMP(v, 1);
      pend_u = v + 3;
      pend = v >= 1 && v + 3 < 2 * NTICK && !(ABL & 2);
      CS_SB();
    };
    auto tick = [&](auto FC1_, Acc& acc, const Acc& act, int hb_slot, int t, int t_next, bool hb_write) {
      constexpr bool FC1 = decltype(FC1_)::value;
      sfor<24>([&](auto M_) {
        constexpr int M = decltype(M_)::value;
        if constexpr (M == 6) {
          // the raw half written in gap 3 (followed by the reads of gaps 3, 4, 5) is in LDS before the partner is told to read it
          if constexpr (FC1) { CS_SB(); asm volatile("s_waitcnt lgkmcnt(3)" ::: "memory"); }
          boundary(FC1_, 2 * t);
        }
        if constexpr (M == 18) {
          boundary(FC1_, 2 * t + 1);
          cur = ring + ((t + 1) & 1) * TICK;
          if constexpr (FC1) read_bias(t_next);  // (never leave an inline-asm read without a consumer: hipcc would reuse its destination
                                                 //  registers at once, and the LDS data would land on top of the new owner)
        }
        if constexpr ((M >= 6 && M < 12) || M >= 18) {
          if (pend) issue_piece(IC<(M >= 18 ? M - 18 : M - 6)>{});
        }
        // `act` was completed by the last MFMAs of the previous tick, and an inline-asm consumer gets none of the wait states hipcc inserts
        // between an MFMA and a reader of its result (8 passes = 32 cycles for 16x16x32; r4 lost k-steps to a ds_write placed in gap 0 of the
        // 32x32x16 form).  Every reader of `act` in gaps 1 and 2 is a compiler-visible conversion, so hipcc places those wait states itself;
        // the only inline-asm readers are bf16 mode's raw stores of gap 3 and its GELU block 5 (gap 6 or later): at least six MFMAs of this
        // tick (8 passes of matrix pipe each, issued in order behind the MFMAs that completed `act`) lie in between.  The MFMA-free last
        // tick waits explicitly.
        if constexpr (M == 1) {
          if constexpr (!FC1) asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
          for (int i = 0; i < 4; ++i) xa[i] = pack_h16x2(act.v[i >> 1][2 * (i & 1)], act.v[i >> 1][2 * (i & 1) + 1]);
        }
        if constexpr (!BF) {
          if constexpr (M == 2) {
#pragma unroll
            for (int i = 0; i < 4; ++i) xb[i] = pack_h16x2(act.v[2 + (i >> 1)][2 * (i & 1)], act.v[2 + (i >> 1)][2 * (i & 1) + 1]);
          }
          if constexpr (M == 3) {
            if (hb_write) lds_write16<HB_RAW>(hb_base + hb_slot * (2 * FRAG), u32x4_t{xb[0], xb[1], xb[2], xb[3]});
          }
        } else {
          if constexpr (M == 3) {
            if (hb_write) {
              lds_write16<HB_RAW>(hb_base + hb_slot * (2 * FRAG), __builtin_bit_cast(u32x4_t, act.v[2]));
              lds_write16<HB_RAW + FRAG>(hb_base + hb_slot * (2 * FRAG), __builtin_bit_cast(u32x4_t, act.v[3]));
            }
          }
        }
        if constexpr (FC1) {
          CS_LGKM(5);
          constexpr int FT = M & 1, KSTEP = M >> 1;
          if constexpr (M < 2) {  // k-step 0: the accumulators start at the bias
            if constexpr (ABL & 4) { acc.v[FT] = bb[FT]; acc.v[2 + FT] = bb[FT]; }
            else {
              acc.v[FT] = mfma_16x16x32<BF>(w[M], xf[0], bb[FT]);
              acc.v[2 + FT] = mfma_16x16x32<BF>(w[M], xf[1], bb[FT]);
            }
          } else if constexpr (!(ABL & 4)) {
            acc.v[FT] = mfma_16x16x32<BF>(w[M % 6], xf[2 * KSTEP], acc.v[FT]);
            acc.v[2 + FT] = mfma_16x16x32<BF>(w[M % 6], xf[2 * KSTEP + 1], acc.v[2 + FT]);
          }
          CS_SB();
          constexpr int F = (M + 6) % 24;  // the fragment read now: of this tick up to gap 17, of the next one (cur has moved) from gap 18 on
          if constexpr (!(ABL & 32)) lds_read1<((F / 12) * 24 + F % 12) * FRAG>(cur, w[M % 6]);
        }
        // GELU of row tile 0 of the previous slice; the fragment leaves in gap 11, so that the counted wait of gap 17 has retired the write
        // before the barrier of gap 18 tells the partner to read it
        // packed-half GELU of this wave's four pairs: twelve blocks in gaps 2..11 (two in gaps 2 and 7); the pairs turn into the B fragment in place
        if constexpr (M >= 2 && M < 12 && !(ABL & 1)) {
          constexpr int B0 = M < 3 ? 0 : (M < 8 ? M - 1 : M);  // first block of this gap: 0, 2, 3, 4, 5, 6, 8, 9, 10, 11
          const float a8[8] = {act.v[0][0], act.v[0][1], act.v[0][2], act.v[0][3], act.v[1][0], act.v[1][1], act.v[1][2], act.v[1][3]};
          pk_gelu_op<B0, BF>(pg, xa, kk, a8);
          if constexpr (M == 2 || M == 7) pk_gelu_op<B0 + 1, BF>(pg, xa, kk, a8);
        }
        if constexpr (M == 11) { if (hb_write) lds_write16<0>(hb_base + hb_slot * FRAG, u32x4_t{xa[0], xa[1], xa[2], xa[3]}); }
        CS_SB();
      });
    };
    read_bias(0);  // (before the fragments: the counted waits retire LDS reads in order)
    sfor<6>([&](auto F_) { lds_read1<decltype(F_)::value * FRAG>(cur, w[decltype(F_)::value]); });
#pragma unroll
    for (int i = 0; i < 4; ++i) acO.v[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};  // tick 0 "activates" this (slice -1: never read by the partner)
    for (int t = 0; t < NSL; t += 2) {
      tick(std::true_type{}, acE, acO, 1, t, t + 1, t > 0);
      tick(std::true_type{}, acO, acE, 0, t + 1, min(t + 2, NSL - 1), true);
    }
    CS_STAMP(4);
    // tick NSL: only the GELU of the last slice (odd), and the boundaries the B waves' tick NSL needs
    CS_LGKM(0);
    tick(std::false_type{}, acE, acO, 1, NSL, 0, true);
    CS_VMCNT(0);  // every LDS-DMA has landed before the workgroup can end ...
    if constexpr (!(ABL & 16)) __builtin_amdgcn_s_barrier();  // ... and the B waves' last boundary (tick NSL + 1, gap 6: unit 2 NTICK - 1)
    CS_STAMP(5);
    // ---- epilogue, A side: the partner stages its rows in LDS (three rounds: residual halves, normalised rows), this wave writes them to
    //      memory as whole 128-byte lines: a store instruction covers 4 rows x 256 contiguous bytes (16 lanes x 16 B per row) ----
    {
      const unsigned st_addr = lds0 + pair * ST_PAIR + (lane >> 4) * ST_ROW + (lane & 15) * 16;
      const int r_in = lane >> 4;
      auto drain = [&](char* gbase, size_t row_bytes) {  // gbase: row0's first byte of this round's 768-byte column range
#pragma unroll
        for (int rg = 0; rg < 8; ++rg) {
          f32x4_t v[3];
          lds_read_f4<0>(st_addr + rg * 4 * ST_ROW, v[0]);
          lds_read_f4<256>(st_addr + rg * 4 * ST_ROW, v[1]);
          lds_read_f4<512>(st_addr + rg * 4 * ST_ROW, v[2]);
          CS_LGKM(0);
          const int r = rg * 4 + r_in;
          if (row0 + r < p.M) {
            char* g = gbase + (size_t)r * row_bytes + (lane & 15) * 16;
            *reinterpret_cast<f32x4_t*>(g) = v[0];
            *reinterpret_cast<f32x4_t*>(g + 256) = v[1];
            *reinterpret_cast<f32x4_t*>(g + 512) = v[2];
          }
        }
      };
      char* xg = reinterpret_cast<char*>(p.x + (size_t)row0 * PC);
      __builtin_amdgcn_s_barrier();  // E0: every wave's LDS-DMA has landed (the staging area lies over the ring)
      __builtin_amdgcn_s_barrier();  // E1: residual columns 0..191 staged
      drain(xg, PC * 4);
      __builtin_amdgcn_s_barrier();  // E2: read
      __builtin_amdgcn_s_barrier();  // E3: residual columns 192..383 staged
      drain(xg + 768, PC * 4);
      __builtin_amdgcn_s_barrier();  // E4: read
      if (p.u_out) {
        __builtin_amdgcn_s_barrier();  // E5: normalised rows staged
        drain(reinterpret_cast<char*>(p.u_out + (size_t)row0 * PC), PC * 2);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    CS_STAMP_RT(9);
#ifdef CS_PANEL_ABLATE
    if (blockIdx.x < 64 && lane == 0) { unsigned long long* d = g_panel_dbg + (blockIdx.x * 8 + wv) * 16; d[10] = tw_drain; d[11] = tw_vm; d[12] = tw_bar; }
#endif
    return;
  }

  // =======================================================================================================================
  // B wave: residual rows; out-projection, LayerNorm hand-off, fc2, epilogue.  acc2[T][rt][i] = x[row 16 rt + li][16 T + 4 g + i]
  // =======================================================================================================================
  CS_STAMP_RT(8); CS_STAMP(0);
  f32x4_t acc2[NT][2];
  const unsigned bv_addr = lds0 + LDS_BV + 16 * (fresh_lane() >> 4);
  unsigned cur = transition(TB{});  // unit 0 (and: the bias vectors are in LDS)
  CS_STAMP(1);
  auto add_bias = [&](auto T_, auto INIT_, int which) {  // acc2[T][rt] (+)= bias[16 T + 4 g + i]
    constexpr int T = decltype(T_)::value;
    f32x4_t b4;
    const unsigned a = bv_addr + which * (PC * 4);
    lds_read_f4<T * 64>(a, b4);
    CS_LGKM(0);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc2[T][rt][i] = (decltype(INIT_)::value ? 0.f : acc2[T][rt][i]) + b4[i];
  };
  if constexpr (OUTPROJ) {
    // ---- attention output projection.  Unit c = k-step c x 24 output tiles (fragment T).  Its B fragments (this lane's 16 B of its
    //      attention-output row, one per row tile) and the residual tiles 2c, 2c+1 arrive in LDS with the unit (copied by the partner). ----
    sfor<NT>([&](auto T_) { add_bias(T_, std::true_type{}, 0); });
    const unsigned xs_addr = lds0 + LDS_X + pair * XREC + lane16;  // this pair's record of slot 0 (+ slot * 4 * XREC)
    h16x8_t of[2];  // [row tile]
    lds_read1<4 * FRAG>(xs_addr, of[0]);
    lds_read1<5 * FRAG>(xs_addr, of[1]);
    sfor<6>([&](auto F_) { lds_read1<decltype(F_)::value * FRAG>(cur, w[decltype(F_)::value]); });
    int slot_x = 0;  // ring slot of the current unit (its residual tiles / attention-output fragments share the index)
    // The twelve unrolled units sit in a loop that runs ONCE (its trip count is opaque to hipcc).  Unrolled, every MFMA result is a short
    // live range of its own, which hipcc assigns in program order, while the results of the last unit live on through the LayerNorm code
    // and get their registers first, wherever it likes: the last two units then spilled 40-60 accumulator registers to permute them into
    // place.  As loop-carried values the first and the last link of every accumulator's chain are one register.
    int once;
    asm volatile("s_mov_b32 %0, 1" : "=s"(once));
    for (int rep = 0; rep < once; ++rep)
    sfor<OUT_CHUNKS>([&](auto C_) {
      constexpr int C = decltype(C_)::value;
      f32x4_t xs;
      sfor<24>([&](auto M_) {
        constexpr int M = decltype(M_)::value;
        // the unit's four residual tiles (piece q = feature tile 2C + (q >> 1), row tile q & 1), ONE at a time: piece q is read at the start
        // of gap 12 + q and added in gap 13 + q (its LDS slot is refilled after the transition below).  The only LDS read issued after it is
        // weight fragment M + 5, so lgkmcnt(1) retires it; the phase is bound by the A waves' memory stream, not by this wave's LDS latency.
        // (Two pieces at a time with their transient registers pushed the 32x32x16 form of this loop over 256 VGPRs, r2.)
        // Both row tiles of a feature tile must take their residual on the SAME side of the unit's MFMAs on that tile (gap T = 2C + (q >> 1)),
        // or a row's fp32 sum would depend on the row tile it sits in.  A piece added at the top of gap 13 + q comes before those MFMAs iff
        // 13 + q <= T; the two row tiles (q, q + 1) disagree for T = 15 only (C = 7, q = 2: gap 15 against gap 16) -- that piece is added
        // behind the MFMAs of gap 15 instead.
        constexpr bool LATE = (C == 7);
        if constexpr (M >= 13 && M <= 16) {
          constexpr int Q = M - 13;
          CS_LGKM(1);
          if constexpr (!(LATE && Q == 2)) acc2[2 * C + (Q >> 1)][Q & 1] += xs;
          CS_SB();
        }
        f32x4_t xs_late;
        if constexpr (LATE && M == 15) xs_late = xs;
        if constexpr (M >= 12 && M <= 15) lds_read_f4<(M - 12) * FRAG>(xs_addr + slot_x * (4 * XREC), xs);
        if constexpr (M == 18) {
          cur = transition(TB{});
          slot_x = slot_x + 1 >= 3 ? 0 : slot_x + 1;
        }
        if constexpr (M == 0 && C > 0) CS_LGKM(0);  // (the unit's B fragments were the last reads issued)
        else CS_LGKM(5);
        acc2[M][0] = mfma_16x16x32<BF>(w[M % 6], of[0], acc2[M][0]);
        acc2[M][1] = mfma_16x16x32<BF>(w[M % 6], of[1], acc2[M][1]);
        if constexpr (LATE && M == 15) acc2[15][0] += xs_late;
        CS_SB();  // (the read below reuses the fragment's registers: not between the two MFMAs)
        // (no read without a consumer: behind the last unit's transition, which drained the LDS queue, nothing more is read)
        if constexpr (M < 18) lds_read1<(M + 6) * FRAG>(cur, w[M % 6]);
        else if constexpr (C + 1 < OUT_CHUNKS) lds_read1<(M - 18) * FRAG>(cur, w[M % 6]);
        // the next unit's B fragments (it landed before the transition of gap 18): both of this unit's are in use up to here, and a second
        // pair of registers does not fit beside the 192 accumulators -- the next gap 0 waits for them (one LDS latency per unit, in a
        // phase that is bound by the A waves' memory stream)
        if constexpr (M == 23 && C + 1 < OUT_CHUNKS) {
          lds_read1<4 * FRAG>(xs_addr + slot_x * (4 * XREC), of[0]);
          lds_read1<5 * FRAG>(xs_addr + slot_x * (4 * XREC), of[1]);
        }
        CS_SB();
      });
    });
    CS_LGKM(0);
  } else {
    // no out-projection (tests): x straight from memory
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const float* xr = p.x + (size_t)rowt[rt] * PC + 4 * g;
#pragma unroll
      for (int T = 0; T < NT; ++T) acc2[T][rt] = *reinterpret_cast<const f32x4_t*>(xr + 16 * T);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  CS_STAMP(2);

  // ---- LayerNorm statistics of the rows held in acc2 (two-pass, fp32, in registers; row 16 rt + li lives in the four lanes li + 16 g) ----
  auto add_row_lanes = [&](float x) {  // the sum over the four lane groups, the same value in all four lanes
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return add_other_half(__uint_as_float(r[0]) + __uint_as_float(r[1]));
  };
  auto row_stats = [&](auto RT_, float& mean, float& rstd) {
    constexpr int RT = decltype(RT_)::value;
    float s = 0.f;
#pragma unroll
    for (int T = 0; T < NT; ++T) s += (acc2[T][RT][0] + acc2[T][RT][1]) + (acc2[T][RT][2] + acc2[T][RT][3]);
    s = add_row_lanes(s);
    mean = s * (1.0f / PC);
    float q = 0.f;
#pragma unroll
    for (int T = 0; T < NT; ++T)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float d = acc2[T][RT][i] - mean;
        q = fmaf(d, d, q);
      }
    q = add_row_lanes(q);
    rstd = 1.0f / sqrtf(q * (1.0f / PC) + p.eps);
  };
  {
    // norm2 -> the partner's fc1 B fragments: k-step KSTEP of row tile RT is the tiles 2 KSTEP and 2 KSTEP + 1 of that row tile (slot e = 4 ft + i)
    float mean[2], rstd[2];
    row_stats(IC<0>{}, mean[0], rstd[0]);
    row_stats(IC<1>{}, mean[1], rstd[1]);
    const float nb[2] = {-mean[0] * rstd[0], -mean[1] * rstd[1]};
    const unsigned r_addr = lds0 + LDS_XF + pair * 12 * FRAG + lane16;
    auto put = [&](auto K_, auto RT_) {
      constexpr int KSTEP = decltype(K_)::value, RT = decltype(RT_)::value;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = fmaf(acc2[2 * KSTEP + (e >> 2)][RT][e & 3], rstd[RT], nb[RT]);  // (not (x - mean) * rstd: the differences of the variance pass would be kept alive)
      lds_write16<((2 * KSTEP + RT) % 12) * FRAG>(r_addr, pack8<BF>(v));
    };
    sfor<6>([&](auto T_) { put(T_, IC<0>{}); put(T_, IC<1>{}); });
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // H1
    __builtin_amdgcn_s_barrier();  // H2
    sfor<6>([&](auto T_) { put(IC<6 + decltype(T_)::value>{}, IC<0>{}); put(IC<6 + decltype(T_)::value>{}, IC<1>{}); });
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // H3
  }
  // the fc2 accumulators start at residual + bias: the residual add and the bias add are free
  sfor<NT>([&](auto T_) { add_bias(T_, std::false_type{}, 1); });
  CS_STAMP(3);

  // ---- fc2, LAGT ticks behind fc1.  Tick t >= LAGT: fragments 24 .. 47 of its unit = feature tiles 0 .. 23 of hidden slice t - LAGT (one
  //      k-step), each multiplied with BOTH row tiles' activation fragments: row tile 0's comes ready from the partner (hb slot
  //      (t - LAGT) & 1, read behind the boundary of gap 18 of the previous tick), row tile 1's is activated here from the partner's raw
  //      values (read behind the boundary of gap 6 of the previous tick, one GELU block in each of its gaps 12 .. 23).  Both fragments are
  //      in use up to the tick's last fragment.  Row tile 1's has two register sets by slice parity (the next one is being activated).  Row
  //      tile 0's has ONE (a second set does not fit beside the 192 accumulators): gap 23 multiplies row tile 0 first and reads the next
  //      slice's fragment behind that MFMA, gap 0 multiplies row tile 1 first, so two MFMAs of this wave (and the partner's share of the
  //      matrix pipe) cover the read's latency before the counted wait in front of gap 0's second MFMA. ----
  const unsigned hb_base = lds0 + LDS_HB + pair * HB_PAIR + lane16;
  int cur_step = TICK;  // this lane's address of tick T's fragment 0 is lds0 + LDS_RING + lane16 + (T & 1) * TICK: `cur` alternates (no base register kept)
  h16x8_t hbA;           // B fragment of row tile 0 (activated by the partner)
  unsigned hbB[2][4];    // [slice parity] B fragment of row tile 1: the partner's raw values as packed halves, activated in place
  f32x4_t rw[2];         // (bf16 mode) those raw values in fp32 (tiles v[2], v[3] of the partner's fc1 accumulator of the slice)
  u32x4_t xr;            // (fp16 mode) those values as 4 packed pairs, rounded by the partner
  PkGelu pg;
  const PkGeluK kk = pk_gelu_consts();
  auto read_raw = [&](int slot) {
    if constexpr (BF) {
      lds_read_f4<HB_RAW>(hb_base + slot * (2 * FRAG), rw[0]);
      lds_read_f4<HB_RAW + FRAG>(hb_base + slot * (2 * FRAG), rw[1]);
    } else {
      lds_read_u4<HB_RAW>(hb_base + slot * (2 * FRAG), xr);
    }
  };
  auto raw_to_halves = [&](auto I0_, unsigned (&hx)[4]) {  // pairs I0, I0 + 1 (blocks 0..5 use pairs 0 and 1, blocks 6..11 pairs 2 and 3)
#pragma unroll
    for (int i = decltype(I0_)::value; i < decltype(I0_)::value + 2; ++i) {
      if constexpr (BF) hx[i] = pack_h16x2(rw[i >> 1][2 * (i & 1)], rw[i >> 1][2 * (i & 1) + 1]);
      else hx[i] = xr[i];
    }
  };
  // the A waves' first LAGT ticks: two unit boundaries each, nothing to multiply yet.  Slice 0's raw half is in LDS behind the third of them
  // (gap 6 of tick 1) and is activated here, outside any MFMA loop; its ready fragment is in LDS behind the fourth.
  for (int b = 0; b < 2 * LAGT - 1; ++b) { if constexpr (!(ABL & 16)) __builtin_amdgcn_s_barrier(); }
  asm volatile("" ::: "memory");
  read_raw(0);
  CS_LGKM(0);
  raw_to_halves(IC<0>{}, hbB[0]);
  raw_to_halves(IC<2>{}, hbB[0]);
  if constexpr (!(ABL & 1)) {
    const float a8[8] = {rw[0][0], rw[0][1], rw[0][2], rw[0][3], rw[1][0], rw[1][1], rw[1][2], rw[1][3]};
    sfor<12>([&](auto N_) { pk_gelu_op<decltype(N_)::value, BF>(pg, hbB[0], kk, a8); });
  }
  CS_SB();
  if constexpr (!(ABL & 16)) __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  // fc2 tick T = slice + LAGT (same parity): unit boundaries in front of gaps 6 and 18 as on the A side, but a B wave has nothing to wait for
  // except the barrier itself (it issues no LDS-DMA, and its own reads of the released unit were retired by the counted waits long before)
  // PAR = slice & 1; MORE: a next slice exists (its fragments are fetched and activated during this tick)
  auto fc2_tick = [&](auto PAR_, auto MORE_, int slice) {
    constexpr int PAR = decltype(PAR_)::value;
    constexpr bool MORE = decltype(MORE_)::value;
    sfor<24>([&](auto M_) {
      constexpr int M = decltype(M_)::value;
      if constexpr (M == 6) {
        CS_SB(); CS_BAR_STAMP(2 * (slice + LAGT), 0); if constexpr (!(ABL & 16)) __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); CS_BAR_STAMP(2 * (slice + LAGT), 1);
        if constexpr (MORE) read_raw(PAR ^ 1);  // the partner wrote it in its gap 3 and retired the write in front of this barrier
        CS_SB();
      }
      if constexpr (M == 18 && MORE) {
        CS_SB();
        CS_BAR_STAMP(2 * (slice + LAGT) + 1, 0);
        if constexpr (!(ABL & 16)) __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        CS_BAR_STAMP(2 * (slice + LAGT) + 1, 1);
        cur += cur_step;
        cur_step = -cur_step;
        CS_SB();
      }
      // the last tick reads nothing behind its fragment 23 (no read without a consumer), so its last waits count down: fragment M, read in gap
      // M - 6, is followed by the reads of gaps M - 5 .. 17
      if constexpr (!MORE && M >= 18) CS_LGKM(23 - M);
      else CS_LGKM(5);
      if constexpr (ABL & 8) { if constexpr (M == 12) asm volatile("" ::"v"(hbB[PAR][0])); }
      else {
        const h16x8_t hb1 = __builtin_bit_cast(h16x8_t, u32x4_t{hbB[PAR][0], hbB[PAR][1], hbB[PAR][2], hbB[PAR][3]});
        if constexpr (M == 0) {
          acc2[M][1] = mfma_16x16x32<BF>(w[M % 6], hb1, acc2[M][1]);
          CS_LGKM(1);  // hbA was read in gap 23 of the previous tick (or ahead of the first tick), in front of that gap's weight fragment
          acc2[M][0] = mfma_16x16x32<BF>(w[M % 6], hbA, acc2[M][0]);
        } else {
          acc2[M][0] = mfma_16x16x32<BF>(w[M % 6], hbA, acc2[M][0]);
          if constexpr (M == 23 && MORE) {
            CS_SB();
            lds_read1<0>(hb_base + (PAR ^ 1) * FRAG, hbA);  // the next slice's: the partner wrote it before the barrier of gap 18
            CS_SB();
          }
          acc2[M][1] = mfma_16x16x32<BF>(w[M % 6], hb1, acc2[M][1]);
        }
      }
      CS_SB();
      constexpr int F = (M + 6) % 24;
      if constexpr (!(ABL & 32) && (MORE || M < 18)) lds_read1<((F / 12) * 24 + 12 + F % 12) * FRAG>(cur, w[M % 6]);
      // packed-half GELU of row tile 1 of the NEXT slice: one block per gap in gaps 12..23, in place in the other parity's registers (fp16
      // mode: the partner rounded the values; bf16 mode: its fp32 accumulators arrive and are rounded here for the correction term, their
      // relu stays fp32).  The raw values were read in gap 6: the counted wait of gap 11 has retired them.
      if constexpr (MORE) {
        if constexpr (M == 12) raw_to_halves(IC<0>{}, hbB[PAR ^ 1]);
        if constexpr (M == 18) raw_to_halves(IC<2>{}, hbB[PAR ^ 1]);
        if constexpr (M >= 12 && !(ABL & 1)) {
          const float a8[8] = {rw[0][0], rw[0][1], rw[0][2], rw[0][3], rw[1][0], rw[1][1], rw[1][2], rw[1][3]};
          pk_gelu_op<M - 12, BF>(pg, hbB[PAR ^ 1], kk, a8);
        }
      }
      CS_SB();
    });
  };
  cur = lds0 + LDS_RING + lane16;  // tick LAGT (even): slice 0
  lds_read1<0>(hb_base, hbA);
  sfor<6>([&](auto F_) { lds_read1<(12 + decltype(F_)::value) * FRAG>(cur, w[decltype(F_)::value]); });
  for (int sl = 0; sl < NSL - 2; sl += 2) {
    fc2_tick(IC<0>{}, std::true_type{}, sl);
    fc2_tick(IC<1>{}, std::true_type{}, sl + 1);
  }
  fc2_tick(IC<0>{}, std::true_type{}, NSL - 2);
  fc2_tick(IC<1>{}, std::false_type{}, NSL - 1);
  CS_LGKM(0);
  CS_VMCNT(0);  // every LDS-DMA has landed before the workgroup can end
  CS_STAMP(4);

  // ---- epilogue, B side: rows go to memory through LDS and the partner (a lane holds 16 B of a row per tile: stored directly, every store
  //      instruction would touch 16 rows) ----
  {
    const unsigned le = fresh_lane();
    const unsigned st_addr = (unsigned)(size_t)CS_LDS_PTR(smem) + pair * ST_PAIR + (le & 15) * ST_ROW + 16 * (le >> 4);
    auto stage_x = [&](auto HALF_) {
      constexpr int HALF = decltype(HALF_)::value;
      sfor<12>([&](auto T_) {
        constexpr int T = 12 * HALF + decltype(T_)::value;
        sfor<2>([&](auto RT_) {
          constexpr int RT = decltype(RT_)::value;
          lds_write16<RT * 16 * ST_ROW + decltype(T_)::value * 64>(st_addr, __builtin_bit_cast(u32x4_t, acc2[T][RT]));
        });
      });
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    __builtin_amdgcn_s_barrier();  // E0
    stage_x(IC<0>{});
    __builtin_amdgcn_s_barrier();  // E1
    float mean[2] = {0.f, 0.f}, rstd[2] = {0.f, 0.f};
    if (p.u_out) {  // (under the partner's stores)
      row_stats(IC<0>{}, mean[0], rstd[0]);
      row_stats(IC<1>{}, mean[1], rstd[1]);
    }
    __builtin_amdgcn_s_barrier();  // E2
    stage_x(IC<1>{});
    __builtin_amdgcn_s_barrier();  // E3
    __builtin_amdgcn_s_barrier();  // E4
    if (p.u_out) {
      const float nb[2] = {-mean[0] * rstd[0], -mean[1] * rstd[1]};
      const unsigned su = (unsigned)(size_t)CS_LDS_PTR(smem) + pair * ST_PAIR + (le & 15) * ST_ROW + 8 * (le >> 4);
      sfor<NT>([&](auto T_) {
        constexpr int T = decltype(T_)::value;
        sfor<2>([&](auto RT_) {
          constexpr int RT = decltype(RT_)::value;
          const unsigned lo = pack_o16x2<BF>(fmaf(acc2[T][RT][0], rstd[RT], nb[RT]), fmaf(acc2[T][RT][1], rstd[RT], nb[RT]));
          const unsigned hi = pack_o16x2<BF>(fmaf(acc2[T][RT][2], rstd[RT], nb[RT]), fmaf(acc2[T][RT][3], rstd[RT], nb[RT]));
          lds_write8<RT * 16 * ST_ROW + T * 32>(su, u32x2_t{lo, hi});
        });
      });
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // E5
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  CS_STAMP(5); CS_STAMP_RT(9);
#ifdef CS_PANEL_ABLATE
  if (blockIdx.x < 64 && lane == 0) { unsigned long long* d = g_panel_dbg + (blockIdx.x * 8 + wv) * 16; d[10] = tw_drain; d[11] = tw_vm; d[12] = tw_bar; }
#endif
}

// ---- weight image.  One thread per 16-byte fragment element (8 f16): [unit][fragment][lane 0..63].  Lane (i = lane & 15, g = lane >> 4) of
//      an A-operand fragment holds MFMA row i of its 16-feature tile T -- output feature 16 T + i, no permutation -- and the 8 contraction
//      slots 8g .. 8g+7 of its 32-wide k-step ks.
//      Contraction index of slot 8g + e:  natural  32 ks + 8 g + e                        (out-projection: B fragments come from memory)
//                                         tiled    32 ks + 16 (e >> 2) + 4 g + (e & 3)    (fc1 / fc2: B fragments are two accumulator tiles)
//      Units: [12 out-projection chunks c of 24 fragments: fragment T = (k-step c, tile T)]
//             [50 MLP ticks t of 48 fragments: fragments 0..23  = fc1 slice t, (k-step f >> 1, feature tile f & 1: hidden 32 t + 16 (f & 1) + i)  (t < 48)
//                                              fragments 24..47 = fc2 slice t - 2 (its one k-step), tile f'                                   (t >= 2)]
//             [1 padding tick] ----
template <bool BF>
__global__ __launch_bounds__(256) void cs_panel_pack_kernel(const float* __restrict__ wo, const float* __restrict__ ls1,
                                                            const float* __restrict__ w1, const float* __restrict__ g2,
                                                            const float* __restrict__ w2, const float* __restrict__ ls2,
                                                            h16_t* __restrict__ img) {
  const int nout = wo ? OUT_CHUNKS : 0;
  const long long n_out16 = (long long)nout * (CHUNK / 16);
  const long long total16 = n_out16 + (long long)(NTICK + PAD_TICKS) * (TICK / 16);
  const long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gi >= total16) return;
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (gi < n_out16) {
    const int c = (int)(gi / (CHUNK / 16));
    const int within = (int)(gi - (long long)c * (CHUNK / 16));
    const int T = within >> 6, lane = within & 63, i = lane & 15, g = lane >> 4;
    const int rowi = 16 * T + i;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = wo[(size_t)rowi * PC + 32 * c + 8 * g + e] * (ls1 ? ls1[rowi] : 1.f);
  } else {
    const long long g2i = gi - n_out16;
    const int t = (int)(g2i / (TICK / 16));
    const int within = (int)(g2i - (long long)t * (TICK / 16));
    // position in the tick: [half 0: 12 A | 12 B][half 1: 12 A | 12 B]  ->  f = role * 24 + (fragment of that role, 0..23)
    const int fpos = within >> 6, lane = within & 63, i = lane & 15, g = lane >> 4;
    const int f = ((fpos % 24) / 12) * 24 + (fpos / 24) * 12 + fpos % 12;
    if (t < NTICK) {
      if (f < 24) {
        if (t < NSL) {
          const int ks = f >> 1;
          const int rowi = 32 * t + 16 * (f & 1) + i;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int col = 32 * ks + 16 * (e >> 2) + 4 * g + (e & 3);
            v[e] = w1[(size_t)rowi * PC + col] * (g2 ? g2[col] : 1.f);
          }
        }
      } else if (t >= LAGT) {
        const int tt = t - LAGT, T = f - 24;
        const int rowi = 16 * T + i;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int col = 32 * tt + 16 * (e >> 2) + 4 * g + (e & 3);
          v[e] = w2[(size_t)rowi * PF + col] * (ls2 ? ls2[rowi] : 1.f);
        }
      }
    }
  }
  const uint4 o = {pack_o16x2<BF>(v[0], v[1]), pack_o16x2<BF>(v[2], v[3]), pack_o16x2<BF>(v[4], v[5]), pack_o16x2<BF>(v[6], v[7])};
  reinterpret_cast<uint4*>(img)[gi] = o;
}

template <bool OUTPROJ, bool BF>
hipError_t panel_launch_t(const CsPanelParams* p, hipStream_t st) {
  static std::atomic<bool> attr_done[16];  // (zero-initialised; hipFuncSetAttribute is idempotent, a racing second caller only repeats it)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return hipErrorInvalidDevice;
  if (!attr_done[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cs_panel_kernel<OUTPROJ, 0, BF>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    if (e != hipSuccess) return e;
    attr_done[dev] = true;
  }
  const int grid = (p->M + PANEL_ROWS - 1) / PANEL_ROWS;
  hipLaunchKernelGGL((cs_panel_kernel<OUTPROJ, 0, BF>), dim3(grid), dim3(512), LDS_BYTES, st, *p);
  return hipGetLastError();
}

}  // namespace

extern "C" {

#ifdef CS_PANEL_ABLATE
int cs_panel_debug_read(unsigned long long* dst) { return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_panel_dbg), sizeof(g_panel_dbg)); }
int cs_panel_bar_read(unsigned long long* dst) { return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_panel_bar), sizeof(g_panel_bar)); }
#endif

int cs_panel_supported(int C, int mlp_ratio) { return C == PC && mlp_ratio * C == PF; }
size_t cs_panel8_image_bytes(int with_outproj) { return (size_t)(with_outproj ? OUT_CHUNKS : 0) * CHUNK + (size_t)(NTICK + PAD_TICKS) * TICK; }

hipError_t cs_panel_pack_launch(const float* wo, const float* ls1, const float* w1, const float* g2, const float* w2, const float* ls2,
                                h16_t* img, int bf16, hipStream_t st) {
  const int total = (int)(cs_panel8_image_bytes(wo ? 1 : 0) / 16);
  if (bf16) hipLaunchKernelGGL(cs_panel_pack_kernel<true>, dim3((total + 255) / 256), dim3(256), 0, st, wo, ls1, w1, g2, w2, ls2, img);
  else hipLaunchKernelGGL(cs_panel_pack_kernel<false>, dim3((total + 255) / 256), dim3(256), 0, st, wo, ls1, w1, g2, w2, ls2, img);
  return hipGetLastError();
}

const char* cs_panel_check(const CsPanelParams* p) {
  if (!p->x || !p->img || !p->b1 || !p->b2) return "panel: null operand";
  if (p->attn_o && !p->bo) return "panel: the out-projection needs its bias";
  if (p->M <= 0) return "panel: empty shape";
  if ((long long)p->M * PC * 4 >= (1ll << 32)) return "panel: too many rows for 32-bit byte offsets";
  if (((uintptr_t)p->x | (uintptr_t)p->img | (uintptr_t)p->b1 | (uintptr_t)p->b2 | (uintptr_t)p->attn_o | (uintptr_t)p->u_out | (uintptr_t)p->bo) & 15)
    return "panel: operands must be 16-byte aligned";
  return nullptr;
}

hipError_t cs_panel_launch(const CsPanelParams* p, hipStream_t st) {
#ifdef CS_PANEL_ABLATE
  if (const char* e = getenv("CS_PANEL_ABL")) {
    const int abl = atoi(e);
    const int grid = (p->M + PANEL_ROWS - 1) / PANEL_ROWS;
#define CS_ABL_CASE(N) if (abl == N) { \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cs_panel_kernel<true, N>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES); \
      hipLaunchKernelGGL((cs_panel_kernel<true, N>), dim3(grid), dim3(512), LDS_BYTES, st, *p); return hipGetLastError(); }
    CS_ABL_CASE(1) CS_ABL_CASE(2) CS_ABL_CASE(3) CS_ABL_CASE(4) CS_ABL_CASE(8) CS_ABL_CASE(12) CS_ABL_CASE(16) CS_ABL_CASE(18) CS_ABL_CASE(32) CS_ABL_CASE(34) CS_ABL_CASE(50) CS_ABL_CASE(64)
#undef CS_ABL_CASE
  }
#endif
  if (p->attn_o) return p->bf16 ? panel_launch_t<true, true>(p, st) : panel_launch_t<true, false>(p, st);
  return p->bf16 ? panel_launch_t<false, true>(p, st) : panel_launch_t<false, false>(p, st);
}

}  // extern "C"
