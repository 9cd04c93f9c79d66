// bf16 MFMA streaming-softmax attention for the full-width binaural head dims (gfx950):
//   (dqk, dv) in {(16,128), (32,256), (64,512)}  = channels C/8 and C of attention levels 2..5 at base 64,
//   N a multiple of the query block.  Everything else falls back to the generic kernels of attn.hip.
//
// Forward, one workgroup (4 waves) per block of 64*QT queries, 64 keys per iteration:
//   S^T = K Q^T        v_mfma_f32_16x16x16_bf16, A = K rows (8-byte global loads), B = Q rows held in VGPRs.
//                      Computing the TRANSPOSE puts, for every lane, 4 consecutive keys of ONE query into the
//                      accumulator registers -- which is exactly the A-operand register layout of the next MFMA,
//                      so the probabilities never move between lanes.
//   P = exp2(S^T * scale*log2e - m)   online max / sum per query (2 xor-shuffles across the 4 lane groups)
//   O += P V           v_mfma_f32_16x16x32_bf16, A = P (VGPRs), B = V tile staged in LDS by LDS-DMA
//                      (global_load_lds, double buffered) and read with ds_read_b64_tr_b16 (hardware
//                      transpose: V is [key][channel] in memory, the MFMA wants channel-major k-slots).
// LDS V tile: DV/128 panels of [64 keys][128 ch] bf16, 32-byte granules XOR-swizzled by (key & 7) so that the
// 8 rows a half-wave transposes at once hit 8 different granules (all 64 banks).
#include "adn_common.h"

namespace {

typedef short s16x8_t __attribute__((ext_vector_type(8)));
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
typedef __attribute__((address_space(3))) s16x4_t* ltr_t;

struct FParams {
  const uint16_t* q; const uint16_t* k; const uint16_t* v;
  uint16_t* o; float* lse;
  int B2, N, shift;
  int ld_q, ld_k, ld_v, ld_o;
  float sc2;        // scale * log2(e)
};

__device__ __forceinline__ int vswz(int row) { return row & 7; }

__device__ __forceinline__ bf16x8_t pack8(const f32x4_t& a, const f32x4_t& b) {
  s16x8_t v8;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    v8[r] = (short)f32_to_bf16_bits(a[r]);
    v8[4 + r] = (short)f32_to_bf16_bits(b[r]);
  }
  return *reinterpret_cast<bf16x8_t*>(&v8);
}

__device__ __forceinline__ bf16x8_t tr_pair(const char* lo_addr, const char* hi_addr) {
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ltr_t)lo_addr);
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ltr_t)hi_addr);
  s16x8_t v8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return *reinterpret_cast<bf16x8_t*>(&v8);
}

// xor-16 / xor-32 butterflies on the VALU (gfx950 v_permlane16_swap / v_permlane32_swap) instead of LDS permutes:
// with both operands = x the swap leaves {rows 0,0,2,2} / {rows 1,1,3,3} (resp. lower / upper half twice)
__device__ __forceinline__ float xor16_max(float x) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xor32_max(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xor16_sum(float x) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float xor32_sum(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

template <int DQK, int DV, int QT, int NW>
__global__ __launch_bounds__(64 * NW) void attn_fwd_mfma_kernel(FParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int NP = DV / 128;            // 128-channel panels of the V tile
  constexpr int PANEL = 64 * 256;         // bytes: 64 keys x 128 ch bf16
  constexpr int TILE = NP * PANEL;
  constexpr int KS = DQK / 16;            // k-steps of the score MFMA
  constexpr int CB = DV / 16;             // 16-channel output blocks
  extern __shared__ __attribute__((aligned(16))) char smem[];      // [2][TILE]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int b = blockIdx.y;
  const int kb = (b + p.shift) % p.B2;
  const int qbase = blockIdx.x * (16 * QT * NW) + wave * (16 * QT);
  const uint16_t* Q = p.q + (int64_t)b * p.N * p.ld_q;
  const uint16_t* Kp = p.k + (int64_t)kb * p.N * p.ld_k;
  const uint16_t* Vp = p.v + (int64_t)kb * p.N * p.ld_v;

  s16x4_t qf[QT][KS];
#pragma unroll
  for (int t = 0; t < QT; ++t)
#pragma unroll
    for (int s = 0; s < KS; ++s)
      qf[t][s] = *reinterpret_cast<const s16x4_t*>(Q + (int64_t)(qbase + 16 * t + li) * p.ld_q + 16 * s + 4 * g);

  float m[QT], l[QT];
  f32x4_t oacc[QT][CB];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    m[t] = -INFINITY;
    l[t] = 0.f;
#pragma unroll
    for (int c = 0; c < CB; ++c) oacc[t][c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  // V tile staging: per panel 16 wave-writes of 1 KiB (4 rows); wave w, pass j -> rows 4 NW j + 4w .. +3
  const int vrow = lane >> 4, vpc = lane & 15;
  auto issue_v = [&](int kt, int buf) {
#pragma unroll
    for (int pn = 0; pn < NP; ++pn)
#pragma unroll
      for (int j = 0; j < 16 / NW; ++j) {
        const int r = 4 * NW * j + 4 * wave + vrow;
        const int lg = (vpc >> 1) ^ vswz(r);
        const uint16_t* src = Vp + (int64_t)(kt * 64 + r) * p.ld_v + pn * 128 + (lg * 2 + (vpc & 1)) * 8;
        char* dst = smem + buf * TILE + pn * PANEL + (4 * NW * j + 4 * wave) * 256;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
      }
  };
  s16x4_t kf[4][KS];
  auto load_k = [&](int kt) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int s = 0; s < KS; ++s)
        kf[u][s] = *reinterpret_cast<const s16x4_t*>(Kp + (int64_t)(kt * 64 + 16 * u + li) * p.ld_k + 16 * s + 4 * g);
  };

  const int nkt = p.N / 64;
  const int q4 = li >> 2, pp = li & 3;

  // S^T = K Q^T : st[t][u][r] = score(query 16t + li, key 16u + 4g + r); the first MFMA of a chain takes literal 0
  auto scores = [&](f32x4_t (&st)[QT][4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int t = 0; t < QT; ++t) {
        st[t][u] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(kf[u][0], qf[t][0], f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
        for (int s = 1; s < KS; ++s)
          st[t][u] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(kf[u][s], qf[t][s], st[t][u], 0, 0, 0);
      }
  };
  // online softmax of one 64-key tile: running max / sum, the probabilities packed as the A operand of the PV
  // MFMA and the factor alpha the accumulator has to be rescaled by before this tile is added
  auto softmax_tile = [&](f32x4_t (&st)[QT][4], bf16x8_t (&pa)[QT][2], float (&al)[QT]) {
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      float mx = -INFINITY;           // scale > 0 (adn_attn_mfma_qt): take the maximum of the raw scores, scale it once
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, st[t][u][r]);
      mx = xor16_max(mx);
      mx = xor32_max(mx);
      const float mn = fmaxf(m[t], mx * p.sc2);
      al[t] = __builtin_amdgcn_exp2f(m[t] - mn);
      m[t] = mn;
      float rs4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(st[t][u][r], p.sc2, -mn));
          st[t][u][r] = pv;
          rs4[r] += pv;
        }
      float rs = (rs4[0] + rs4[1]) + (rs4[2] + rs4[3]);
      rs = xor16_sum(rs);
      rs = xor32_sum(rs);
      l[t] = l[t] * al[t] + rs;
#pragma unroll
      for (int h = 0; h < 2; ++h) pa[t][h] = pack8(st[t][2 * h], st[t][2 * h + 1]);
    }
  };
  // accumulator rows are queries 4g + r; their alpha lives in the lanes with li == 4g + r.  Once the running
  // maxima have settled alpha is 1 for the whole wave and the rescale (and its shuffles) is skipped
  auto rescale = [&](const float (&al)[QT]) {
#pragma unroll
    for (int t = 0; t < QT; ++t)
      if (__builtin_amdgcn_ballot_w64(al[t] != 1.f) != 0) {
        float ar[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ar[r] = __shfl(al[t], 4 * g + r, 64);
#pragma unroll
        for (int c = 0; c < CB; ++c)
#pragma unroll
          for (int r = 0; r < 4; ++r) oacc[t][c][r] *= ar[r];
      }
  };
  // O += P V : k-slot j of lane group g is key 32h + 4g + j (j < 4) / 32h + 16 + 4g + (j - 4)
  auto pv_tile = [&](const char* Vb, const bf16x8_t (&pa)[QT][2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row_lo = 32 * h + 4 * g + q4, row_hi = row_lo + 16;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const int pn = cb >> 3, cw = cb & 7;
        const bf16x8_t bfr = tr_pair(Vb + pn * PANEL + row_lo * 256 + ((cw ^ vswz(row_lo)) << 5) + pp * 8,
                                     Vb + pn * PANEL + row_hi * 256 + ((cw ^ vswz(row_hi)) << 5) + pp * 8);
#pragma unroll
        for (int t = 0; t < QT; ++t)
          oacc[t][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa[t][h], bfr, oacc[t][cb], 0, 0, 0);
      }
    }
  };

  // (A software-pipelined form - softmax of tile kt + 1 under the P V MFMAs of tile kt - needs 196 registers; the
  //  third resident wave per SIMD that 160 registers allow is worth more: 7.5 vs 8.3 ms at B2 = 64, N = 16384.)
  issue_v(0, 0);
  load_k(0);
  for (int kt = 0; kt < nkt; ++kt) {
    f32x4_t st[QT][4];
    bf16x8_t pa[QT][2];
    float al[QT];
    scores(st);
    softmax_tile(st, pa, al);
    rescale(al);
    __syncthreads();        // V tile kt has landed (vmcnt(0) in front of the barrier); tile kt-1 is no longer read
    if (kt + 1 < nkt) {
      issue_v(kt + 1, (kt + 1) & 1);
      load_k(kt + 1);
    }
    pv_tile(smem + (kt & 1) * TILE, pa);
  }

  // ---- epilogue: O / l, lse
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const float inv = 1.f / l[t];
    float ir[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ir[r] = __shfl(inv, 4 * g + r, 64);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      uint16_t* orow = p.o + ((int64_t)b * p.N + qbase + 16 * t + 4 * g + r) * p.ld_o + li;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) orow[16 * cb] = f32_to_bf16_bits(oacc[t][cb][r] * ir[r]);
    }
    if (g == 0)
      p.lse[(int64_t)b * p.N + qbase + 16 * t + li] = (m[t] + __log2f(l[t])) * 0.6931471805599453f;
  }
#endif
}

template <int DQK, int DV, int QT, int NW>
void launch_fwd(const FParams& p, hipStream_t st) {
  constexpr int lds = 2 * (DV / 128) * 64 * 256;
  ADN_SET_LDS_ONCE(lds, &attn_fwd_mfma_kernel<DQK, DV, QT, NW>);
  hipLaunchKernelGGL((attn_fwd_mfma_kernel<DQK, DV, QT, NW>), dim3(p.N / (16 * QT * NW), p.B2), dim3(64 * NW), lds, st, p);
}

bool aligned16(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }


// ---------------------------------------------------------------------------------------------------------
// Backward.  Two kernels, no atomics (deterministic):
//   dQ  kernel: one workgroup per block of queries, loop over 64-key tiles (structure of the forward):
//               S^T = K Q^T, dP^T = V dO^T (A = V rows from LDS, B = dO rows in VGPRs), dS^T = P (dP - D) scale,
//               dQ += dS K (A = dS registers, B = K tile by transpose reads from LDS)
//   dKV kernel: one workgroup per block of keys, loop over 64-query tiles:
//               S = Q K^T, dP = dO V^T (A = dO rows from LDS, B = V rows in VGPRs), dV += P^T dO, dK += dS^T Q
//               (A = P / dS registers, B = dO / Q tiles by transpose reads from LDS)
// Again each product is oriented so that the accumulator layout of one MFMA is the A-operand layout of the
// next; the price is that dP is computed in both kernels (1.5x the minimal backward FLOPs for dv >> dqk).
struct BParams {
  const uint16_t* q; const uint16_t* k; const uint16_t* v; const uint16_t* dout;
  const float* lse; const float* dsum;
  uint16_t* dq; uint16_t* dk; uint16_t* dv;
  int B2, N, shift;
  int ld_q, ld_k, ld_v, ld_do, ld_dq, ld_dk, ld_dv;
  float sc2, scale;
};

// swizzle of the small [64][DQK] tiles (32-byte granules, DQK/16 granules per row)
template <int DQK>
__device__ __forceinline__ int sswz(int row) {
  return DQK == 16 ? 0 : (DQK == 32 ? ((row >> 2) & 1) : ((row >> 1) & 3));
}

// stage a [64 rows][DV] bf16 tile (row stride ld elements) into LDS panels with the vswz granule swizzle
template <int DV>
__device__ __forceinline__ void stage_wide(const uint16_t* base, int ld, int row0, char* dst_tile, int wave, int lane) {
  constexpr int NP = DV / 128;
  constexpr int PANEL = 64 * 256;
  const int vrow = lane >> 4, vpc = lane & 15;
#pragma unroll
  for (int pn = 0; pn < NP; ++pn)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = 16 * j + 4 * wave + vrow;
      const int lg = (vpc >> 1) ^ vswz(r);
      const uint16_t* src = base + (int64_t)(row0 + r) * ld + pn * 128 + (lg * 2 + (vpc & 1)) * 8;
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(dst_tile + pn * PANEL + (16 * j + 4 * wave) * 256), 16, 0, 0);
    }
}

// stage a [64 rows][DQK] bf16 tile: 64 * DQK * 2 bytes = 2 / 4 / 8 KiB, 1 KiB per wave-write
template <int DQK>
__device__ __forceinline__ void stage_narrow(const uint16_t* base, int ld, int row0, char* dst_tile, int wave, int lane) {
  constexpr int RB = DQK * 2;             // bytes per row
  constexpr int CPR = RB / 16;            // 16-byte chunks per row
  constexpr int RPW = 1024 / RB;          // rows per wave-write
  constexpr int WRITES = 64 / RPW;        // wave-writes per tile: 2 / 4 / 8
#pragma unroll
  for (int j = 0; j < (WRITES + 3) / 4; ++j) {
    const int wi = 4 * j + wave;
    if (wi < WRITES) {
      const int r = wi * RPW + lane / CPR, pc = lane % CPR;
      const int lg = (pc >> 1) ^ sswz<DQK>(r);
      const uint16_t* src = base + (int64_t)(row0 + r) * ld + (lg * 2 + (pc & 1)) * 8;
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(dst_tile + wi * 1024), 16, 0, 0);
    }
  }
}

template <int DQK, int DV, int QT>
__global__ __launch_bounds__(256, DQK == 16 ? 3 : 1) void attn_bwd_dq_mfma_kernel(BParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int NP = DV / 128, PANEL = 64 * 256, VT = NP * PANEL, KTB = 64 * DQK * 2;
  constexpr int KS = DQK / 16, CK = DV / 32, DB = DQK / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];      // [2][VT] V tiles, then [2][KTB] K tiles
  char* vs = smem;
  char* ksm = smem + 2 * VT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15, q4 = li >> 2, pp = li & 3;
  const int b = blockIdx.y;
  const int kb = (b + p.shift) % p.B2;
  const int qbase = blockIdx.x * (64 * QT) + wave * (16 * QT);
  const uint16_t* Q = p.q + (int64_t)b * p.N * p.ld_q;
  const uint16_t* DO = p.dout + (int64_t)b * p.N * p.ld_do;
  const uint16_t* Kp = p.k + (int64_t)kb * p.N * p.ld_k;
  const uint16_t* Vp = p.v + (int64_t)kb * p.N * p.ld_v;

  s16x4_t qf[QT][KS];
  bf16x8_t dof[QT][CK];
  // Row constants ride in as the initial accumulators: S' = S - lse / scale makes P = exp2(sc2 S') and
  // dP' = dP - delta makes dS = P dP' (the factor `scale` is applied once, to dQ, at the end)
  const float inv_scale = 1.f / p.scale;
  f32x4_t s0[QT], d0[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int64_t row = qbase + 16 * t + li;
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[t][s] = *reinterpret_cast<const s16x4_t*>(Q + row * p.ld_q + 16 * s + 4 * g);
#pragma unroll
    for (int c = 0; c < CK; ++c) dof[t][c] = *reinterpret_cast<const bf16x8_t*>(DO + row * p.ld_do + 32 * c + 8 * g);
    const float ls = -p.lse[(int64_t)b * p.N + row] * inv_scale, ds = -p.dsum[(int64_t)b * p.N + row];
    s0[t] = f32x4_t{ls, ls, ls, ls};
    d0[t] = f32x4_t{ds, ds, ds, ds};
  }
  f32x4_t dqa[QT][DB];
#pragma unroll
  for (int t = 0; t < QT; ++t)
#pragma unroll
    for (int d = 0; d < DB; ++d) dqa[t][d] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  s16x4_t kf[4][KS];
  auto load_k = [&](int kt) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int s = 0; s < KS; ++s)
        kf[u][s] = *reinterpret_cast<const s16x4_t*>(Kp + (int64_t)(kt * 64 + 16 * u + li) * p.ld_k + 16 * s + 4 * g);
  };
  const int nkt = p.N / 64;
  stage_wide<DV>(Vp, p.ld_v, 0, vs, wave, lane);
  stage_narrow<DQK>(Kp, p.ld_k, 0, ksm, wave, lane);
  load_k(0);
  for (int kt = 0; kt < nkt; ++kt) {
    f32x4_t st[QT][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int t = 0; t < QT; ++t) {
        st[t][u] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(kf[u][0], qf[t][0], s0[t], 0, 0, 0);
#pragma unroll
        for (int s = 1; s < KS; ++s)
          st[t][u] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(kf[u][s], qf[t][s], st[t][u], 0, 0, 0);
      }
    __syncthreads();
    if (kt + 1 < nkt) {
      stage_wide<DV>(Vp, p.ld_v, (kt + 1) * 64, vs + ((kt + 1) & 1) * VT, wave, lane);
      stage_narrow<DQK>(Kp, p.ld_k, (kt + 1) * 64, ksm + ((kt + 1) & 1) * KTB, wave, lane);
      load_k(kt + 1);
    }
    const char* Vb = vs + (kt & 1) * VT;
    const char* Kb = ksm + (kt & 1) * KTB;
    // dP^T = V dO^T : A = V[key 16u + li][32c + 8g ..+7] (16-byte LDS reads), B = dO fragments; then
    // dS^T = P dP' packed as the A operand (k-slots = keys) and dQ += dS K (B[k = key][col = d] by transpose reads
    // of the K tile).  Two halves of 32 keys keep only half of dP' live.
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4_t dp[QT][2];
#pragma unroll
      for (int uu = 0; uu < 2; ++uu) {
        const int row = 32 * h + 16 * uu + li;
#pragma unroll
        for (int c = 0; c < CK; ++c) {
          const int pn = c >> 2, gi = 2 * (c & 3) + (g >> 1);
          const bf16x8_t vf = *reinterpret_cast<const bf16x8_t*>(Vb + pn * PANEL + row * 256 + ((gi ^ vswz(row)) << 5) + (g & 1) * 16);
#pragma unroll
          for (int t = 0; t < QT; ++t)
            dp[t][uu] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, dof[t][c], c == 0 ? d0[t] : dp[t][uu], 0, 0, 0);
        }
      }
      bf16x8_t dsa[QT];
#pragma unroll
      for (int t = 0; t < QT; ++t) {
#pragma unroll
        for (int uu = 0; uu < 2; ++uu)
#pragma unroll
          for (int r = 0; r < 4; ++r) dp[t][uu][r] *= __builtin_amdgcn_exp2f(st[t][2 * h + uu][r] * p.sc2);
        dsa[t] = pack8(dp[t][0], dp[t][1]);
      }
      const int row_lo = 32 * h + 4 * g + q4, row_hi = row_lo + 16;
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        const bf16x8_t kfr = tr_pair(Kb + row_lo * (DQK * 2) + ((d ^ sswz<DQK>(row_lo)) << 5) + pp * 8,
                                     Kb + row_hi * (DQK * 2) + ((d ^ sswz<DQK>(row_hi)) << 5) + pp * 8);
#pragma unroll
        for (int t = 0; t < QT; ++t) dqa[t][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsa[t], kfr, dqa[t][d], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < QT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      uint16_t* row = p.dq + ((int64_t)b * p.N + qbase + 16 * t + 4 * g + r) * p.ld_dq + li;
#pragma unroll
      for (int d = 0; d < DB; ++d) row[16 * d] = f32_to_bf16_bits(dqa[t][d][r] * p.scale);
    }
#endif
}

template <int DQK, int DV, int KT>
__global__ __launch_bounds__(256, DQK == 16 ? 2 : 1) void attn_bwd_dkv_mfma_kernel(BParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int NP = DV / 128, PANEL = 64 * 256, VT = NP * PANEL, QTB = 64 * DQK * 2;
  constexpr int KS = DQK / 16, CK = DV / 32, CB = DV / 16, DB = DQK / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];      // [2][VT] dO tiles, then [2][QTB] Q tiles
  char* dos = smem;
  char* qsm = smem + 2 * VT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15, q4 = li >> 2, pp = li & 3;
  const int kb = blockIdx.y;                                     // batch entry of this key block
  const int qb = (kb - p.shift + p.B2) % p.B2;                   // the queries attending to it
  const int kbase = blockIdx.x * (64 * KT) + wave * (16 * KT);
  const uint16_t* Q = p.q + (int64_t)qb * p.N * p.ld_q;
  const uint16_t* DO = p.dout + (int64_t)qb * p.N * p.ld_do;
  const uint16_t* Kp = p.k + (int64_t)kb * p.N * p.ld_k;
  const uint16_t* Vp = p.v + (int64_t)kb * p.N * p.ld_v;
  const float* lse = p.lse + (int64_t)qb * p.N;
  const float* dsum = p.dsum + (int64_t)qb * p.N;

  s16x4_t kfr[KT][KS];        // B operand of S = Q K^T : K[key = li][d = 16s + 4g ..]
  bf16x8_t vfr[KT][CK];       // B operand of dP = dO V^T : V[key = li][c = 32c + 8g ..]
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    const int64_t row = kbase + 16 * t + li;
#pragma unroll
    for (int s = 0; s < KS; ++s) kfr[t][s] = *reinterpret_cast<const s16x4_t*>(Kp + row * p.ld_k + 16 * s + 4 * g);
#pragma unroll
    for (int c = 0; c < CK; ++c) vfr[t][c] = *reinterpret_cast<const bf16x8_t*>(Vp + row * p.ld_v + 32 * c + 8 * g);
  }
  f32x4_t dva[KT][CB], dka[KT][DB];
#pragma unroll
  for (int t = 0; t < KT; ++t) {
#pragma unroll
    for (int c = 0; c < CB; ++c) dva[t][c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < DB; ++d) dka[t][d] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  // log-sum-exp and delta of the 64 queries of a tile: 16 + 16 floats per lane (rows 16u + 4g + r), reloaded for the
  // next tile as soon as the half that used them is done, so only one copy is ever live.  They ride into the MFMA
  // chains as initial accumulators: S' = S - lse / scale makes P = exp2(sc2 S'), dP' = dP - delta makes dS = P dP'
  // (the factor `scale` is applied once, to dK, at the end)
  const float neg_inv_scale = -1.f / p.scale;
  f32x4_t lq[4], dq4[4];
  auto load_ld = [&](int qt, int u) {
    lq[u] = *reinterpret_cast<const f32x4_t*>(lse + qt * 64 + 16 * u + 4 * g);
    dq4[u] = *reinterpret_cast<const f32x4_t*>(dsum + qt * 64 + 16 * u + 4 * g);
  };
  const int nqt = p.N / 64;
  stage_wide<DV>(DO, p.ld_do, 0, dos, wave, lane);
  stage_narrow<DQK>(Q, p.ld_q, 0, qsm, wave, lane);
#pragma unroll
  for (int u = 0; u < 4; ++u) load_ld(0, u);
  for (int qt = 0; qt < nqt; ++qt) {
    __syncthreads();          // tile qt has landed (vmcnt(0) in front of the barrier); tile qt-1 is no longer read
    const bool more = qt + 1 < nqt;
    if (more) {
      stage_wide<DV>(DO, p.ld_do, (qt + 1) * 64, dos + ((qt + 1) & 1) * VT, wave, lane);
      stage_narrow<DQK>(Q, p.ld_q, (qt + 1) * 64, qsm + ((qt + 1) & 1) * QTB, wave, lane);
    }
    const char* Db = dos + (qt & 1) * VT;
    const char* Qb = qsm + (qt & 1) * QTB;
    // the tile is processed in two halves of 32 queries (= one K step of the dV / dK products), so that only the
    // scores of one half are live and the exp / dS math of a half overlaps the MFMAs of the other
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // S = Q K^T, dP = dO V^T : st[t][uu][r] = score(query 32h + 16uu + 4g + r, key 16t + li)
      f32x4_t st[KT][2], dp[KT][2];
#pragma unroll
      for (int uu = 0; uu < 2; ++uu) {
        const int row = 32 * h + 16 * uu + li;
        const f32x4_t s0 = lq[2 * h + uu] * neg_inv_scale, d0 = -dq4[2 * h + uu];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const s16x4_t qv = *reinterpret_cast<const s16x4_t*>(Qb + row * (DQK * 2) + ((s ^ sswz<DQK>(row)) << 5) + 8 * g);
#pragma unroll
          for (int t = 0; t < KT; ++t)
            st[t][uu] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(qv, kfr[t][s], s == 0 ? s0 : st[t][uu], 0, 0, 0);
        }
#pragma unroll
        for (int c = 0; c < CK; ++c) {
          const int pn = c >> 2, gi = 2 * (c & 3) + (g >> 1);
          const bf16x8_t df = *reinterpret_cast<const bf16x8_t*>(Db + pn * PANEL + row * 256 + ((gi ^ vswz(row)) << 5) + (g & 1) * 16);
#pragma unroll
          for (int t = 0; t < KT; ++t)
            dp[t][uu] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df, vfr[t][c], c == 0 ? d0 : dp[t][uu], 0, 0, 0);
        }
      }
      bf16x8_t pa[KT], dsa[KT];
#pragma unroll
      for (int t = 0; t < KT; ++t) {
#pragma unroll
        for (int uu = 0; uu < 2; ++uu)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float pv = __builtin_amdgcn_exp2f(st[t][uu][r] * p.sc2);
            st[t][uu][r] = pv;
            dp[t][uu][r] *= pv;
          }
        pa[t] = pack8(st[t][0], st[t][1]);
        dsa[t] = pack8(dp[t][0], dp[t][1]);
      }
      if (more) {
        load_ld(qt + 1, 2 * h);
        load_ld(qt + 1, 2 * h + 1);
      }
      // dV += P^T dO, dK += dS^T Q : k-slots are queries 32h + 4g + j / 32h + 16 + 4g + (j - 4)
      const int row_lo = 32 * h + 4 * g + q4, row_hi = row_lo + 16;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const int pn = cb >> 3, cw = cb & 7;
        const bf16x8_t bfr = tr_pair(Db + pn * PANEL + row_lo * 256 + ((cw ^ vswz(row_lo)) << 5) + pp * 8,
                                     Db + pn * PANEL + row_hi * 256 + ((cw ^ vswz(row_hi)) << 5) + pp * 8);
#pragma unroll
        for (int t = 0; t < KT; ++t) dva[t][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa[t], bfr, dva[t][cb], 0, 0, 0);
      }
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        const bf16x8_t qfr = tr_pair(Qb + row_lo * (DQK * 2) + ((d ^ sswz<DQK>(row_lo)) << 5) + pp * 8,
                                     Qb + row_hi * (DQK * 2) + ((d ^ sswz<DQK>(row_hi)) << 5) + pp * 8);
#pragma unroll
        for (int t = 0; t < KT; ++t) dka[t][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsa[t], qfr, dka[t][d], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < KT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = (int64_t)kb * p.N + kbase + 16 * t + 4 * g + r;
      uint16_t* vrow = p.dv + row * p.ld_dv + li;
#pragma unroll
      for (int c = 0; c < CB; ++c) vrow[16 * c] = f32_to_bf16_bits(dva[t][c][r]);
      uint16_t* krow = p.dk + row * p.ld_dk + li;
#pragma unroll
      for (int d = 0; d < DB; ++d) krow[16 * d] = f32_to_bf16_bits(dka[t][d][r] * p.scale);
    }
#endif
}

template <int DQK, int DV, int QT>
void launch_bwd(const BParams& p, hipStream_t st) {
  constexpr int lds = 2 * (DV / 128) * 64 * 256 + 2 * 64 * DQK * 2;
  ADN_SET_LDS_ONCE(lds, &attn_bwd_dq_mfma_kernel<DQK, DV, QT>);
  ADN_SET_LDS_ONCE(lds, &attn_bwd_dkv_mfma_kernel<DQK, DV, QT>);
  const dim3 grid(p.N / (64 * QT), p.B2);
  hipLaunchKernelGGL((attn_bwd_dq_mfma_kernel<DQK, DV, QT>), grid, dim3(256), lds, st, p);
  hipLaunchKernelGGL((attn_bwd_dkv_mfma_kernel<DQK, DV, QT>), grid, dim3(256), lds, st, p);
}

}  // namespace

static bool attn_generic_forced() {   // ADN_ATTN_GENERIC: test knob, read once
  static const bool forced = getenv("ADN_ATTN_GENERIC") != nullptr;
  return forced;
}

// The one eligibility test of the MFMA kernels, shared by both launches and by adn_attn_form (attn.hip): the query-block
// factor QT of the kernel that takes this descriptor, 0 when it has to run on the generic kernels.  The softmax takes the
// maximum of the RAW scores and scales it once, which is the maximum of the scaled scores only for a positive scale; the
// backward divides by the scale.  A non-positive scale is therefore generic.
int adn_attn_mfma_qt(const AdnAttnDesc* d, bool bwd) {
  if (d->dtype != ADN_BF16) return 0;
  if (attn_generic_forced()) return 0;
  if (!(d->scale > 0.f)) return 0;
  int qt;
  if (d->dqk == 16 && d->dv == 128) qt = 2;
  else if (d->dqk == 32 && d->dv == 256) qt = 2;
  else if (d->dqk == 64 && d->dv == 512) qt = 1;
  else return 0;
  if (d->N % (64 * qt) != 0) return 0;
  if ((d->ld_q | d->ld_k | d->ld_v) & 7) return 0;                      // 16-byte rows for the DMA / 8-byte frags
  if (!aligned16(d->q) || !aligned16(d->k) || !aligned16(d->v)) return 0;
  if (bwd && ((d->ld_do & 7) || !aligned16(d->dout))) return 0;
  return qt;
}

// returns 1 when the MFMA kernel took the launch, 0 when the caller must use the generic path
int adn_attn_mfma_fwd(const AdnAttnDesc* d, hipStream_t st) {
  if (adn_attn_mfma_qt(d, false) == 0) return 0;
  FParams p;
  p.q = reinterpret_cast<const uint16_t*>(d->q);
  p.k = reinterpret_cast<const uint16_t*>(d->k);
  p.v = reinterpret_cast<const uint16_t*>(d->v);
  p.o = reinterpret_cast<uint16_t*>(d->o);
  p.lse = d->lse;
  p.B2 = d->B2; p.N = d->N; p.shift = d->kv_shift;
  p.ld_q = d->ld_q; p.ld_k = d->ld_k; p.ld_v = d->ld_v; p.ld_o = d->ld_o;
  p.sc2 = d->scale * 1.4426950408889634f;
  // (NW = 8 waves / 256 queries per workgroup halves the K / V re-streaming but measured slower: 1299 vs 1189 us at L2)
  if (d->dqk == 16) launch_fwd<16, 128, 2, 4>(p, st);
  else if (d->dqk == 32) launch_fwd<32, 256, 2, 4>(p, st);
  else launch_fwd<64, 512, 1, 4>(p, st);
  return 1;
}


// d->workspace already holds D = rowsum(dO * O) (attn.hip computes it before calling)
int adn_attn_mfma_bwd(const AdnAttnDesc* d, hipStream_t st) {
  if (adn_attn_mfma_qt(d, true) == 0) return 0;
  BParams p;
  p.q = reinterpret_cast<const uint16_t*>(d->q);
  p.k = reinterpret_cast<const uint16_t*>(d->k);
  p.v = reinterpret_cast<const uint16_t*>(d->v);
  p.dout = reinterpret_cast<const uint16_t*>(d->dout);
  p.lse = d->lse;
  p.dsum = reinterpret_cast<const float*>(d->workspace);
  p.dq = reinterpret_cast<uint16_t*>(d->dq);
  p.dk = reinterpret_cast<uint16_t*>(d->dk);
  p.dv = reinterpret_cast<uint16_t*>(d->dvp);
  p.B2 = d->B2; p.N = d->N; p.shift = d->kv_shift;
  p.ld_q = d->ld_q; p.ld_k = d->ld_k; p.ld_v = d->ld_v; p.ld_do = d->ld_do;
  p.ld_dq = d->ld_dq; p.ld_dk = d->ld_dk; p.ld_dv = d->ld_dv;
  p.sc2 = d->scale * 1.4426950408889634f;
  p.scale = d->scale;
  if (d->dqk == 16) launch_bwd<16, 128, 2>(p, st);
  else if (d->dqk == 32) launch_bwd<32, 256, 2>(p, st);
  else launch_bwd<64, 512, 1>(p, st);
  return 1;
}
