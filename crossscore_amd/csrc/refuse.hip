// Reference use of the last decoder layer's cross-attention: which reference view each query patch's attention went to,
// where in that view it looked, and whether it found anything -- all heads in one launch, no attention matrix in memory.
//
// Keys are N segments of Np rows (key k = n Np + j is patch j of reference n).  With the base-2 logits s = q.k the attention kernel sees
// (Q pre-scaled, 16-bit operands, fp32 accumulation) and the lse it wrote, e = s - lse, p = 2^e, pm = (1 / heads) sum_hd p:
//   share[b][n][q]      = sum_j pm[b][q][n Np + j]                      peak_prob[b][n][q] = max_j pm, peak_index its j (lowest on ties)
//   entropy[b][q]       = (1 / heads) sum_hd sum_k -p e                 (bits)
// lse is used as written, nothing is renormalised: p has the value need_attn_weights returns for that head.
//
// Structure (wave64, MFMA 16x16x32 in the swapped form of the attention tile loop): a workgroup = 4 waves = 64 query rows of one batch item, a
// wave 16 rows.  The workgroup walks the references, inside each the 64-key tiles of [0, Np) -- no tile straddles two references, the ragged
// last one is masked, its rows clamped to the reference's last row when staged -- and inside each tile the heads.  A K row of the kv buffer holds
// all heads side by side, so one step = (reference, tile, group of HG heads) stages the group's HG dh contiguous columns of the tile's 64 rows
// HBM -> VGPR -> LDS (issue early / write late, double buffered, one barrier per step; HG = 8 up to dh 64: 66 KB per buffer at dh 48, all heads
// of the ViT-S decoder at once -- staged per head the launch took 1067 us at the cfg-2 shape, its loads' latency exposed in every step), each head
// in a slot of 32 ceil(dh / 32) columns whose columns behind dh are zero like the matching Q elements.  S^T = K Q^T gives lane (li, g) the query column li
// and the keys 16 kt + 4 g .. + 3 of the tile, the same (query, key) pairs for every head: p is added into a per-pair head sum and -p e into the
// row's entropy partial with no lane traffic.  Behind the last head the pair sums join the lane's segment sum and its running (best, lowest
// index); the four lanes of a row are reduced once per reference, the entropy once at the end.  Stores are coalesced over q in (B, N, Np).
// Every branch is wave-uniform.
#include "cs_common.h"
#include <atomic>
#include <math.h>

namespace {

template <int DH>
struct RefUseCfg {
  static constexpr int KS2 = (DH + 31) / 32;  // QK^T k-steps (MFMA K = 32; dh = 16, 48: the last one is half zeros)
  static constexpr int CH = DH / 8;           // 16-byte chunks per K row of one head
  static constexpr int SLOT = KS2 * 64;       // bytes of one head's slot in an LDS row
  static constexpr int HG = SLOT <= 128 ? 8 : (SLOT <= 256 ? 4 : 2);  // heads staged per step: two buffers of 64 rows stay below 136 KB
  // K row pitch, bytes: the 16x16x32 rule of the attention kernel (2 * odd 16-byte chunks: a ds_read_b128 of 16 rows x 4 lane groups is conflict free)
  static constexpr int KROW = HG * SLOT + 32;
  static_assert((KROW / 16) % 4 == 2, "K row pitch");
  static constexpr int TILE = 64 * KROW;
  static constexpr int RC = HG * CH;                 // 16-byte chunks per staged row
  static constexpr int NIT = 64 * RC / 256;          // 16-byte chunks per thread per step
  static_assert((64 * RC) % 256 == 0, "whole passes");
  static constexpr bool PAD = DH % 32 != 0;          // 16 zero columns behind each head's dh (2 chunks per slot)
};

template <int DH, bool BF>
__global__ __launch_bounds__(256) void cs_refuse_kernel(CsRefUseParams p) {
  using Cfg = RefUseCfg<DH>;
  constexpr int KS2 = Cfg::KS2, CH = Cfg::CH, NIT = Cfg::NIT, HG = Cfg::HG, RC = Cfg::RC;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, g = lane >> 4;
  const int QB = (p.Lq + 63) / 64;
  const int bat = blockIdx.x / QB, qb = blockIdx.x - bat * QB;
  const int q0 = qb * 64 + wv * 16;
  const bool live = q0 < p.Lq;  // wave-uniform: a wave beyond Lq stages, writes and meets the barriers and does nothing else

  const h16_t* Qb = p.Q + (size_t)bat * p.q_bs;
  const h16_t* Kb = p.K + (size_t)bat * p.k_bs;

  if constexpr (Cfg::PAD) {  // the zero columns of every slot of both LDS images: the last k-step reads them, the staging never writes them
    for (int z = tid; z < 2 * 64 * HG * 2; z += 256) {  // (buffer, row, slot, chunk)
      const int chunk = z & 1, slot = (z >> 1) % HG, row = (z >> 1) / HG % 64, buf = (z >> 1) / (HG * 64);
      *reinterpret_cast<uint4*>(smem + buf * Cfg::TILE + row * Cfg::KROW + slot * Cfg::SLOT + DH * 2 + 16 * chunk) = make_uint4(0, 0, 0, 0);
    }
  }

  // ---- staging map: chunk c = tid + it*256 -> (key = c / RC, r = c % RC); r counts the group's contiguous 16-byte chunks of the K row, chunk
  //      r % CH of head r / CH of the group.  A group at the end of the heads may hold fewer than HG: the chunks of absent heads are skipped ----
  int skey[NIT], sr[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int c = tid + it * 256;
    skey[it] = c / RC;
    sr[it] = c - skey[it] * RC;
  }
  uint4 kreg[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) kreg[it] = make_uint4(0, 0, 0, 0);
  const int ngrp = (p.heads + HG - 1) / HG;
  // rows of the ragged tile beyond Np are read from the reference's last row (inside the buffer whatever follows it) and masked below
#define CS_REFUSE_LOAD(N_, T_, G_)                                                                               \
  {                                                                                                              \
    const int live_ = (p.heads - (G_) * HG < HG ? p.heads - (G_) * HG : HG) * CH;                                \
    _Pragma("unroll") for (int it = 0; it < NIT; ++it) {                                                         \
      if (sr[it] < live_) {                                                                                      \
        int row_ = (T_) * 64 + skey[it];                                                                         \
        row_ = row_ < p.Np ? row_ : p.Np - 1;                                                                    \
        kreg[it] = *reinterpret_cast<const uint4*>(Kb + ((size_t)(N_) * p.Np + row_) * p.ldk + (G_) * HG * DH + sr[it] * 8); \
      }                                                                                                          \
    }                                                                                                            \
  }
#define CS_REFUSE_WRITE(BUF, G_)                                                                                 \
  {                                                                                                              \
    const int live_ = (p.heads - (G_) * HG < HG ? p.heads - (G_) * HG : HG) * CH;                                \
    _Pragma("unroll") for (int it = 0; it < NIT; ++it) {                                                         \
      if (sr[it] < live_)                                                                                        \
        *reinterpret_cast<uint4*>(smem + (BUF) * Cfg::TILE + skey[it] * Cfg::KROW + (sr[it] / CH) * Cfg::SLOT + (sr[it] % CH) * 16) = kreg[it]; \
    }                                                                                                            \
  }

  // ---- this lane's query row (clamped: rows beyond Lq compute on the last row and store nothing) ----
  int qr = q0 + li;
  qr = qr < p.Lq ? qr : p.Lq - 1;
  const h16_t* qp = Qb + (size_t)qr * p.ldq + 8 * g;
  const float* lsep = p.lse + (size_t)bat * p.heads * p.Lq + qr;
  const float sc = p.scale_log2e;
  const float inv_heads = 1.0f / (float)p.heads;
  const int koff = li * Cfg::KROW + g * 16;  // + slot*SLOT + kt*16*KROW + s*64

  const int ntile = (p.Np + 63) / 64;
  const int nsteps = p.N * ntile * ngrp;

  f32x4_t pm[4];          // head sums of p for this lane's 16 (query, key) pairs of the tile
  float ent = 0.f;        // -sum p e over this lane's pairs, all heads, all keys
  float seg = 0.f;        // this lane's part of the reference's share
  float best = -1.0f;     // running peak of the reference among this lane's keys (a real pm is >= 0)
  int bidx = 0x7fffffff;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int j = 0; j < 4; ++j) pm[kt][j] = 0.f;

  // ---- Q^T fragments and lse of a head group, in registers: lane (li, g) holds Q[q][hd dh + 32 s + 8 g .. + 7], zeros beyond dh, pre-multiplied
  //      like cs_attn_kernel's.  With one group (heads <= HG: the decoder's eight heads) they are loaded once, else again at every step; read
  //      per head inside the loop instead, each head waited for its own loads: 911 us at the cfg-2 shape ----
  h16x8_t qf[HG][KS2];
  float lse_r[HG];
#define CS_REFUSE_LOAD_Q(G_)                                                                                     \
  _Pragma("unroll") for (int hh = 0; hh < HG; ++hh) {                                                            \
    const int hd_ = (G_) * HG + hh;                                                                              \
    lse_r[hh] = 0.f;                                                                                             \
    _Pragma("unroll") for (int s = 0; s < KS2; ++s) {                                                            \
      _Pragma("unroll") for (int j = 0; j < 8; ++j) qf[hh][s][j] = (_Float16)0.f;                                \
    }                                                                                                            \
    if (hd_ < p.heads) {                                                                                         \
      lse_r[hh] = lsep[(size_t)hd_ * p.Lq];                                                                      \
      _Pragma("unroll") for (int s = 0; s < KS2; ++s) {                                                          \
        if (32 * s + 32 <= DH || 32 * s + 8 * g < DH) qf[hh][s] = *reinterpret_cast<const h16x8_t*>(qp + hd_ * DH + 32 * s); \
        if (sc != 1.0f) {                                                                                        \
          _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                                        \
            const _Float16 e_ = qf[hh][s][j]; /* (a scalar copy first, as in attention.hip) */                   \
            qf[hh][s][j] = __builtin_bit_cast(_Float16, f2o<BF>(o2f<BF>(__builtin_bit_cast(h16_t, e_)) * sc));   \
          }                                                                                                      \
        }                                                                                                        \
      }                                                                                                          \
    }                                                                                                            \
  }

  CS_REFUSE_LOAD(0, 0, 0)
  CS_REFUSE_LOAD_Q(0)
  CS_REFUSE_WRITE(0, 0)
  __syncthreads();

  int n = 0, t = 0, grp = 0;
  for (int step = 0; step < nsteps; ++step) {
    int n2 = n, t2 = t, grp2 = grp + 1;
    if (grp2 == ngrp) {
      grp2 = 0;
      if (++t2 == ntile) { t2 = 0; ++n2; }
    }
    const bool more = step + 1 < nsteps;
    if (more) { CS_REFUSE_LOAD(n2, t2, grp2) }
    if (ngrp > 1 && step > 0 && live) { CS_REFUSE_LOAD_Q(grp) }
    const int hd_n = live ? (p.heads - grp * HG < HG ? p.heads - grp * HG : HG) : 0;  // heads of this group (none for a dead wave)
#pragma unroll
    for (int hh = 0; hh < HG; ++hh) {
      if (hh >= hd_n) break;  // (wave-uniform)
      const int hd = grp * HG + hh;
      const char* kb = smem + (step & 1) * Cfg::TILE + hh * Cfg::SLOT;
      const float lse = lse_r[hh];
      const int left = p.Np - t * 64;  // keys of this reference from the tile's first on
      const int nkt = left >= 64 ? 4 : (left + 15) >> 4;
      if (hd == 0) {
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int j = 0; j < 4; ++j) pm[kt][j] = 0.f;
      }
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        if (kt < nkt) {
          f32x4_t st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < KS2; ++s) {
            const h16x8_t kf = *reinterpret_cast<const h16x8_t*>(kb + koff + kt * 16 * Cfg::KROW + s * 64);
            st = mfma_16x16x32<BF>(kf, qf[hh][s], st);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bool ok = 16 * kt + 4 * g + j < left;  // a key of the ragged tail contributes nothing
            const float e = st[j] - lse;
            const float pr = ok ? __builtin_amdgcn_exp2f(e) : 0.f;
            pm[kt][j] += pr;
            ent -= ok ? pr * e : 0.f;
          }
        }
      }
      if (hd == p.heads - 1) {
        // ---- the head mean, then this lane's segment sum and peak (keys in ascending order, strictly greater wins: the lowest index stays) ----
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          if (kt < nkt) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int key = 16 * kt + 4 * g + j;
              if (key < left) {
                const float v = pm[kt][j] * inv_heads;
                seg += v;
                if (v > best) { best = v; bidx = t * 64 + key; }
              }
            }
          }
        }
        if (t == ntile - 1) {
          // ---- the reference is complete: the row's four lanes li + 16 g -> sum, and max with the lowest index on equal values ----
          float sum = seg + __shfl_xor(seg, 16, 64);
          sum += __shfl_xor(sum, 32, 64);
#pragma unroll
          for (int off = 16; off <= 32; off <<= 1) {
            const float ob = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bidx, off, 64);
            if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
          }
          if (g == 0 && q0 + li < p.Lq) {
            const size_t o = ((size_t)bat * p.N + n) * p.Lq + q0 + li;
            if (p.share) p.share[o] = sum;
            if (p.peak_prob) p.peak_prob[o] = best;
            if (p.peak_index) p.peak_index[o] = bidx;
          }
          seg = 0.f; best = -1.0f; bidx = 0x7fffffff;
        }
      }
    }
    if (more) { CS_REFUSE_WRITE((step + 1) & 1, grp2) }
    __syncthreads();
    n = n2; t = t2; grp = grp2;
  }

  if (live) {
    float es = ent + __shfl_xor(ent, 16, 64);
    es += __shfl_xor(es, 32, 64);
    if (p.entropy && g == 0 && q0 + li < p.Lq) p.entropy[(size_t)bat * p.Lq + q0 + li] = es * inv_heads;
  }
#undef CS_REFUSE_LOAD
#undef CS_REFUSE_LOAD_Q
#undef CS_REFUSE_WRITE
}

template <int DH, bool BF>
hipError_t launch(const CsRefUseParams& p, hipStream_t stream) {
  const int lds = 2 * RefUseCfg<DH>::TILE;
  if (lds > 48 * 1024) {  // (every instantiation: 68 KiB at dh = 16, 132 KiB at dh = 48 .. 128, 100 KiB at dh = 192)
    static std::atomic<bool> attr_done[16];  // (zero-initialised; hipFuncSetAttribute is idempotent, a racing second caller only repeats it)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return hipErrorInvalidDevice;
    if (!attr_done[dev]) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cs_refuse_kernel<DH, BF>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      if (e != hipSuccess) return e;
      attr_done[dev] = true;
    }
  }
  dim3 grid((unsigned)p.nbatch * (unsigned)((p.Lq + 63) / 64));
  hipLaunchKernelGGL((cs_refuse_kernel<DH, BF>), grid, dim3(256), lds, stream, p);
  return hipGetLastError();
}

}  // namespace

extern "C" const char* cs_refuse_check(const CsRefUseParams* p, int dh) {
  if (dh != 16 && dh != 48 && dh != 64 && dh != 96 && dh != 128 && dh != 192) return "reference_use: head dim must be 16, 48, 64, 96, 128 or 192";
  if (p->Lq <= 0 || p->N <= 0 || p->Np <= 0 || p->heads <= 0 || p->nbatch <= 0) return "reference_use: empty shape";
  if ((long long)p->nbatch * ((p->Lq + 63) / 64) > (1ll << 30)) return "reference_use: grid too large";
  if ((long long)p->N * p->Np * p->heads > (1ll << 30)) return "reference_use: too many keys";
  // Q and K rows are read in 16-byte chunks and a key row is addressed like cs_attn_kernel's: what cs_attn_check refuses for Q and K is refused here
  if (p->ldq % 8 || p->ldk % 8) return "reference_use: row strides must keep 16-byte rows";
  if (p->q_bs % 8 || p->k_bs % 8) return "reference_use: batch strides must keep 16-byte rows";
  if (!p->Q || !p->K || !p->lse) return "reference_use: null operand";
  if ((long long)p->N * p->Np * p->ldk >= (1ll << 30)) return "reference_use: Lk * row stride must stay below 2^30 elements";
  return nullptr;
}

extern "C" hipError_t cs_refuse_launch(const CsRefUseParams* p, int dh, hipStream_t stream) {
  switch (dh) {
    case 16: return p->bf16 ? launch<16, true>(*p, stream) : launch<16, false>(*p, stream);
    case 48: return p->bf16 ? launch<48, true>(*p, stream) : launch<48, false>(*p, stream);
    case 64: return p->bf16 ? launch<64, true>(*p, stream) : launch<64, false>(*p, stream);
    case 96: return p->bf16 ? launch<96, true>(*p, stream) : launch<96, false>(*p, stream);
    case 128: return p->bf16 ? launch<128, true>(*p, stream) : launch<128, false>(*p, stream);
    case 192: return p->bf16 ? launch<192, true>(*p, stream) : launch<192, false>(*p, stream);
  }
  return hipErrorInvalidValue;
}
