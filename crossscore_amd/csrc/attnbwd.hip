// Flash-style attention backward for gfx950: from Q, K, V, O, dO and the base-2 lse cs_attn_kernel wrote,
//   S2 = Q' K^T (Q' = Q, or Q * q_scale rounded once as the forward rounds it),  P = 2^(S2 - lse),  D[q] = sum_d dO[q][d] O[q][d],
//   dP = dO V^T,  dz = P (dP - D),  dV = Ph^T dO,  dKu = dzh^T Q',  dQu = dzh K        (Ph, dzh: P and dz rounded once to the operand type)
// dKu and dQu are left unscaled: d loss / dK = ln2 dKu and d loss / dQ' = ln2 dQu (the consumer's fp32 reduction carries the scalars).
// P is recomputed from lse and never stored.  Three launches, no atomics, every sum in a fixed order:
//   attnbwd_d_kernel      D (batch, heads, Lq) fp32 into the workspace, one thread per row, d in index order
//   attnbwd_kernel<KEYS>  a workgroup owns 64 keys of one (batch, head), streams all queries in 64-row tiles, keeps dV^T and dKu^T in registers
//   attnbwd_kernel<!KEYS> a workgroup owns 64 queries, streams all keys in 64-row tiles, keeps dQu^T in registers
// The two tile kernels are one template: a wave owns 16 "stationary" rows (the columns of its score tiles, lane index li), whose two operands
// (K and V, or Q and dO) stay in registers as MFMA B fragments; the "streamed" rows (Q and dO, or K and V) pass through LDS.  All five products
// run on v_mfma_f32_16x16x32 (dh = 16 and 48: the last k-step is zero padded, as in the forward's dh = 48 loop):
//   scores   st[kt] = streamed1 (A: rows 16 kt + li, d = 32 s + 8 g ..) x stationary1^T (B)  -> lane (li, g) holds streamed rows 16 kt + 4 g + j of column li
//   dP       the same with streamed2 / stationary2
//   outputs  acc^T[d][column] += streamed^T (A: transposed LDS reads) x {Ph | dzh} (B: the score tiles of two kt packed to 16 bits, exactly the
//            forward's P V step: contraction slot 8 g + j is streamed row 32 s + 4 g + j (j < 4) or 32 s + 16 + 4 g + (j - 4))
// LDS row pitch: 32 bytes x odd (96 / 160 / 224 for dh 16 / 48 / 96), the forward's 16x16x32 rule for both the ds_read_b128 of the A rows
// and the transposed reads.  Streamed rows past the end are zeros (the buffer descriptor's range check) and their P is forced to 0;
// stationary rows past the end are computed on zeros and never stored.
#include "cs_common.h"

#include <initializer_list>

namespace {

template <int DH>
struct BwdCfg {
  static constexpr int KS2 = (DH + 31) / 32;    // k-steps of the score products (the last one zero padded for dh = 16, 48)
  static constexpr int DT16 = DH / 16;          // 16-wide d tiles of the transposed outputs
  static constexpr int CH = DH / 8;             // 16-byte chunks per streamed row
  static constexpr int ROW = KS2 * 64 + 32;     // LDS row pitch, bytes
  static_assert((ROW / 16) % 4 == 2 && (ROW / 4) % 16 == 8 && DH % 16 == 0, "row pitch");
  static constexpr int MAT = 64 * ROW;          // one streamed matrix tile
  static constexpr int LDS = 2 * MAT + 512;     // + lse and D of the tile's 64 rows (key-stationary kernel)
  static constexpr int NIT = (64 * CH + 255) / 256;
};

__global__ __launch_bounds__(256) void attnbwd_d_kernel(CsAttnBwdParams p, int dh) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n = (long long)p.nbatch * p.heads * p.Lq;
  if (i >= n) return;
  const int q = (int)(i % p.Lq);
  const int head = (int)((i / p.Lq) % p.heads);
  const int bat = (int)(i / ((long long)p.Lq * p.heads));
  const h16_t* o = p.O + (size_t)bat * p.o_bs + (size_t)q * p.ldo + head * dh;
  const h16_t* g = p.dO + (size_t)bat * p.do_bs + (size_t)q * p.lddo + head * dh;
  float acc = 0.f;
  for (int c = 0; c < dh; c += 8) {
    const uint4 a = *reinterpret_cast<const uint4*>(o + c), b = *reinterpret_cast<const uint4*>(g + c);
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      acc += o2f((h16_t)(bw[k] & 0xffffu), p.bf16) * o2f((h16_t)(aw[k] & 0xffffu), p.bf16);
      acc += o2f((h16_t)(bw[k] >> 16), p.bf16) * o2f((h16_t)(aw[k] >> 16), p.bf16);
    }
  }
  p.D[i] = acc;
}

template <bool BF>
__device__ __forceinline__ uint4 scale_chunk(uint4 v, float sc) {
  uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    w[k] = pack_o16x2<BF>(o2f<BF>((h16_t)(w[k] & 0xffffu)) * sc, o2f<BF>((h16_t)(w[k] >> 16)) * sc);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// KEYS: stationary = keys (K, V), streamed = queries (Q', dO), outputs dV and dKu.  !KEYS: stationary = queries (Q', dO), streamed = keys
// (K, V), output dQu.
template <int DH, bool BF, bool KEYS>
__global__ __launch_bounds__(256) void attnbwd_kernel(CsAttnBwdParams p) {
  using Cfg = BwdCfg<DH>;
  constexpr int KS2 = Cfg::KS2, DT16 = Cfg::DT16, CH = Cfg::CH, NIT = Cfg::NIT, ROW = Cfg::ROW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, g = lane >> 4;
  const int Ls = KEYS ? p.Lk : p.Lq;  // stationary rows
  const int Lt = KEYS ? p.Lq : p.Lk;  // streamed rows
  const int SB = (Ls + 63) / 64;
  const int grp = blockIdx.x / SB, sb = blockIdx.x - grp * SB;
  const int head = grp % p.heads, bat = grp / p.heads;
  const int c0 = sb * 64 + wv * 16;  // this wave's first stationary row
  const int c = c0 + li;
  const bool live = c0 < Ls;         // wave-uniform

  const h16_t* Qb = p.Q + (size_t)bat * p.q_bs + head * DH;
  const h16_t* Kb = p.K + (size_t)bat * p.k_bs + head * DH;
  const h16_t* Vb = p.V + (size_t)bat * p.v_bs + head * DH;
  const h16_t* Gb = p.dO + (size_t)bat * p.do_bs + head * DH;
  const h16_t* s1 = KEYS ? Kb : Qb;  const int lds1 = KEYS ? p.ldk : p.ldq;   // stationary operands
  const h16_t* s2 = KEYS ? Vb : Gb;  const int lds2 = KEYS ? p.ldv : p.lddo;
  const h16_t* t1 = KEYS ? Qb : Kb;  const int ldt1 = KEYS ? p.ldq : p.ldk;   // streamed operands
  const h16_t* t2 = KEYS ? Gb : Vb;  const int ldt2 = KEYS ? p.lddo : p.ldv;
  const float sc = p.scale_log2e;
  const float* lse_g = p.lse + ((size_t)bat * p.heads + head) * p.Lq;
  const float* D_g = p.D + ((size_t)bat * p.heads + head) * p.Lq;

  // ---- the LDS image starts as zeros: the padded columns [DH, 32 KS2) of every row are read by the last k-step and never staged ----
  for (int i = tid; i < Cfg::LDS / 16; i += 256) *reinterpret_cast<uint4*>(smem + i * 16) = make_uint4(0, 0, 0, 0);

  // ---- stationary B fragments: lane (li, g) holds row c, d = 32 s + 8 g .. + 7 (zeros beyond dh and beyond the last row) ----
  h16x8_t f1[KS2], f2[KS2];
#pragma unroll
  for (int s = 0; s < KS2; ++s) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { f1[s][j] = (_Float16)0.f; f2[s][j] = (_Float16)0.f; }
    if (c < Ls && 32 * s + 8 * g < DH) {
      f1[s] = *reinterpret_cast<const h16x8_t*>(s1 + (size_t)c * lds1 + 32 * s + 8 * g);
      f2[s] = *reinterpret_cast<const h16x8_t*>(s2 + (size_t)c * lds2 + 32 * s + 8 * g);
    }
  }
  float lse_c = 0.f, D_c = 0.f;  // !KEYS: the statistics of this lane's query
  if constexpr (!KEYS) {
    if (c < Ls) { lse_c = lse_g[c]; D_c = D_g[c]; }
    if (sc != 1.0f) {  // Q' = Q * q_scale, rounded once, as cs_attn_kernel forms it
#pragma unroll
      for (int s = 0; s < KS2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const _Float16 e = f1[s][j];  // (a scalar copy first, as in attention.hip)
          f1[s][j] = __builtin_bit_cast(_Float16, f2o<BF>(o2f<BF>(__builtin_bit_cast(h16_t, e)) * sc));
        }
    }
  }

  // ---- staging of a streamed tile: chunk = tid + it * 256 -> (row = chunk / CH, ch = chunk % CH); buffer loads, so rows past Lt read zeros ----
  constexpr bool kFullLast = (64 * CH) % 256 == 0;
  int srow[NIT], sch[NIT];
  unsigned go1[NIT], go2[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int ck = tid + it * 256;
    srow[it] = ck / CH;
    sch[it] = ck - srow[it] * CH;
    go1[it] = ((unsigned)srow[it] * (unsigned)ldt1 + (unsigned)sch[it] * 8u) * 2u;
    go2[it] = ((unsigned)srow[it] * (unsigned)ldt2 + (unsigned)sch[it] * 8u) * 2u;
  }
  uint4 r1[NIT], r2[NIT];
  float rstat = 0.f;  // KEYS: tid < 64 carries lse of streamed row tid, tid in [64, 128) D of row tid - 64
  const unsigned bytes1 = (unsigned)(((size_t)(Lt - 1) * ldt1 + DH) * 2), bytes2 = (unsigned)(((size_t)(Lt - 1) * ldt2 + DH) * 2);
  auto load_tile = [&](const int t) __attribute__((always_inline)) {
    // a descriptor per tile: the range check covers the VGPR offset only, so the tile's position goes into the base (attention.hip)
    const unsigned o1 = (unsigned)t * 64u * (unsigned)ldt1 * 2u, o2 = (unsigned)t * 64u * (unsigned)ldt2 * 2u;
    const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(t1)) + o1, 0, (int)(bytes1 - o1), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(t2)) + o2, 0, (int)(bytes2 - o2), 0x00020000);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      if (kFullLast || it + 1 < NIT || tid + it * 256 < 64 * CH) {
        r1[it] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs1, go1[it], 0, 0));
        r2[it] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs2, go2[it], 0, 0));
      }
    }
    if constexpr (KEYS) {
      rstat = 0.f;
      if (tid < 128) {
        const int q = t * 64 + (tid & 63);
        if (q < Lt) rstat = (tid < 64 ? lse_g : D_g)[q];
      }
    }
  };
  auto write_tile = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      if (kFullLast || it + 1 < NIT || tid + it * 256 < 64 * CH) {
        uint4 a = r1[it];
        if constexpr (KEYS) { if (sc != 1.0f) a = scale_chunk<BF>(a, sc); }  // streamed1 = Q'
        *reinterpret_cast<uint4*>(smem + srow[it] * ROW + sch[it] * 16) = a;
        *reinterpret_cast<uint4*>(smem + Cfg::MAT + srow[it] * ROW + sch[it] * 16) = r2[it];
      }
    }
    if constexpr (KEYS) { if (tid < 128) *reinterpret_cast<float*>(smem + 2 * Cfg::MAT + tid * 4) = rstat; }
  };

  f32x4_t acc1[DT16], acc2[DT16];  // KEYS: dV^T, dKu^T;  !KEYS: dQu^T (acc2 unused)
#pragma unroll
  for (int d = 0; d < DT16; ++d)
#pragma unroll
    for (int e = 0; e < 4; ++e) { acc1[d][e] = 0.f; acc2[d][e] = 0.f; }

  const int aoff = li * ROW + g * 16;                          // + kt * 16 * ROW + s * 64
  const int toff = (4 * g + (li >> 2)) * ROW + (li & 3) * 8;   // + (32 s2 [+ 16]) * ROW + d * 32
  const int nt = (Lt + 63) / 64;

  load_tile(0);
  __syncthreads();  // the zero fill is complete
  write_tile();
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) load_tile(t + 1);
    if (live) {
      const bool ragged = t * 64 + 64 > Lt;  // wave-uniform
      const char* m1 = smem;
      const char* m2 = smem + Cfg::MAT;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        h16x8_t ph, dzh;
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          const int kt = 2 * s2 + k2;
          f32x4_t st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < KS2; ++s) {
            const h16x8_t a1 = *reinterpret_cast<const h16x8_t*>(m1 + aoff + kt * 16 * ROW + s * 64);
            const h16x8_t a2 = *reinterpret_cast<const h16x8_t*>(m2 + aoff + kt * 16 * ROW + s * 64);
            st = mfma_16x16x32<BF>(a1, f1[s], st);
            dp = mfma_16x16x32<BF>(a2, f2[s], dp);
          }
          float ls[4], ds[4];
          if constexpr (KEYS) {
            const float4 l4 = *reinterpret_cast<const float4*>(smem + 2 * Cfg::MAT + (16 * kt + 4 * g) * 4);
            const float4 d4 = *reinterpret_cast<const float4*>(smem + 2 * Cfg::MAT + 256 + (16 * kt + 4 * g) * 4);
            ls[0] = l4.x; ls[1] = l4.y; ls[2] = l4.z; ls[3] = l4.w;
            ds[0] = d4.x; ds[1] = d4.y; ds[2] = d4.z; ds[3] = d4.w;
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) { ls[j] = lse_c; ds[j] = D_c; }
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float pj = __builtin_amdgcn_exp2f(st[j] - ls[j]);
            float zj = pj * (dp[j] - ds[j]);
            if (ragged && t * 64 + 16 * kt + 4 * g + j >= Lt) { pj = 0.f; zj = 0.f; }  // a row that does not exist: exact zeros, not 2^(0 - lse)
            ph[4 * k2 + j] = __builtin_bit_cast(_Float16, f2o<BF>(pj));
            dzh[4 * k2 + j] = __builtin_bit_cast(_Float16, f2o<BF>(zj));
          }
        }
        // ---- outputs: acc^T += streamed^T x {Ph | dzh}; the A fragments are transposed reads of the row-major LDS image ----
        const char* tr1 = m1 + toff + 32 * s2 * ROW;
        const char* tr2 = m2 + toff + 32 * s2 * ROW;
#pragma unroll
        for (int d = 0; d < DT16; ++d) {
          {
            const short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4_t*)(tr1 + d * 32));
            const short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4_t*)(tr1 + 16 * ROW + d * 32));
            const short8_t a8 = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            if constexpr (KEYS) acc2[d] = mfma_16x16x32<BF>(__builtin_bit_cast(h16x8_t, a8), dzh, acc2[d]);  // dKu^T += Q'^T dzh
            else acc1[d] = mfma_16x16x32<BF>(__builtin_bit_cast(h16x8_t, a8), dzh, acc1[d]);               // dQu^T += K^T dzh^T
          }
          if constexpr (KEYS) {
            const short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4_t*)(tr2 + d * 32));
            const short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4_t*)(tr2 + 16 * ROW + d * 32));
            const short8_t a8 = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            acc1[d] = mfma_16x16x32<BF>(__builtin_bit_cast(h16x8_t, a8), ph, acc1[d]);                     // dV^T += dO^T Ph
          }
        }
      }
    }
    __syncthreads();  // every wave is done with tile t
    if (t + 1 < nt) write_tile();
    __syncthreads();
  }

  // ---- epilogue: lane (li, g) holds d = 16 dt + 4 g .. + 3 of stationary row c ----
  if (c < Ls) {
    if constexpr (KEYS) {
      h16_t* ov = p.dV + (size_t)bat * p.dv_bs + (size_t)c * p.lddv + head * DH + 4 * g;
      h16_t* ok = p.dK + (size_t)bat * p.dk_bs + (size_t)c * p.lddk + head * DH + 4 * g;
#pragma unroll
      for (int d = 0; d < DT16; ++d) {
        uint2 o;
        o.x = pack_o16x2<BF>(acc1[d][0], acc1[d][1]); o.y = pack_o16x2<BF>(acc1[d][2], acc1[d][3]);
        *reinterpret_cast<uint2*>(ov + 16 * d) = o;
        o.x = pack_o16x2<BF>(acc2[d][0], acc2[d][1]); o.y = pack_o16x2<BF>(acc2[d][2], acc2[d][3]);
        *reinterpret_cast<uint2*>(ok + 16 * d) = o;
      }
    } else {
      h16_t* oq = p.dQ + (size_t)bat * p.dq_bs + (size_t)c * p.lddq + head * DH + 4 * g;
#pragma unroll
      for (int d = 0; d < DT16; ++d) {
        uint2 o;
        o.x = pack_o16x2<BF>(acc1[d][0], acc1[d][1]); o.y = pack_o16x2<BF>(acc1[d][2], acc1[d][3]);
        *reinterpret_cast<uint2*>(oq + 16 * d) = o;
      }
    }
  }
}

template <int DH, bool BF>
hipError_t launch(const CsAttnBwdParams& p, hipStream_t st) {
  const long long groups = (long long)p.nbatch * p.heads;
  const long long rows = groups * p.Lq;
  hipLaunchKernelGGL(attnbwd_d_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, p, DH);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((attnbwd_kernel<DH, BF, true>), dim3((unsigned)(groups * ((p.Lk + 63) / 64))), dim3(256), BwdCfg<DH>::LDS, st, p);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((attnbwd_kernel<DH, BF, false>), dim3((unsigned)(groups * ((p.Lq + 63) / 64))), dim3(256), BwdCfg<DH>::LDS, st, p);
  return hipGetLastError();
}

}  // namespace

extern "C" {

int cs_attnbwd_supported(int dh) { return dh == 16 || dh == 48 || dh == 96; }

size_t cs_attnbwd_workspace(int batch, int heads, int Lq) { return (((size_t)batch * heads * Lq * sizeof(float)) + 255) & ~(size_t)255; }

const char* cs_attnbwd_check(const CsAttnBwdParams* p) {
  if (p->Lq <= 0 || p->Lk <= 0 || p->heads <= 0 || p->nbatch <= 0) return "attention_backward: empty shape";
  if (!p->Q || !p->K || !p->V || !p->O || !p->dO || !p->lse || !p->dQ || !p->dK || !p->dV || !p->D) return "attention_backward: null pointer";
  for (const void* q : {(const void*)p->Q, (const void*)p->K, (const void*)p->V, (const void*)p->O, (const void*)p->dO, (const void*)p->dQ, (const void*)p->dK,
                        (const void*)p->dV})
    if (reinterpret_cast<uintptr_t>(q) & 15) return "attention_backward: the 16-bit operands must be 16-byte aligned";
  if ((reinterpret_cast<uintptr_t>(p->lse) & 3) || (reinterpret_cast<uintptr_t>(p->D) & 255)) return "attention_backward: lse must be 4-byte and the workspace 256-byte aligned";
  for (int ld : {p->ldq, p->ldk, p->ldv, p->ldo, p->lddo, p->lddq, p->lddk, p->lddv})
    if (ld <= 0 || ld % 8) return "attention_backward: row strides must be positive multiples of 8 elements";
  for (long long bs : {p->q_bs, p->k_bs, p->v_bs, p->o_bs, p->do_bs, p->dq_bs, p->dk_bs, p->dv_bs})
    if (bs < 0 || bs % 8) return "attention_backward: batch strides must be multiples of 8 elements";
  for (long long e : {(long long)p->Lk * p->ldk, (long long)p->Lk * p->ldv, (long long)p->Lq * p->ldq, (long long)p->Lq * p->lddo})
    if (e >= (1ll << 30)) return "attention_backward: rows * row stride must stay below 2^30 elements (32-bit tile offsets)";
  const long long groups = (long long)p->nbatch * p->heads;
  if (groups * ((p->Lk + 63) / 64) >= (1ll << 31) || groups * ((p->Lq + 63) / 64) >= (1ll << 31) || groups * p->Lq >= (1ll << 38))
    return "attention_backward: grid too large";
  return nullptr;
}

hipError_t cs_attnbwd_launch(const CsAttnBwdParams* p, int dh, hipStream_t st) {
  switch (dh) {
    case 16: return p->bf16 ? launch<16, true>(*p, st) : launch<16, false>(*p, st);
    case 48: return p->bf16 ? launch<48, true>(*p, st) : launch<48, false>(*p, st);
    case 96: return p->bf16 ? launch<96, true>(*p, st) : launch<96, false>(*p, st);
  }
  return hipErrorInvalidValue;
}

}  // extern "C"
