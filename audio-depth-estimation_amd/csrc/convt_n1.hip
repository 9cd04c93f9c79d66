// Outermost ConvTranspose2d(k4,s2,p1) with a single output channel (the depth map), forward.
//
// With Cout = 1 the 4-phase implicit GEMM degenerates to N = 1.  Instead: every input pixel m first
// produces its 16 kernel-tap products P[m][kh*4+kw] = sum_c in[m][c] * W[c][kh][kw] -- a pointwise GEMM
// [M x Cin] x [Cin x 16] that fits one MFMA N-tile with the weights resident in LDS and the activations
// streamed straight from HBM into the A fragments (no LDS staging: each element is used once) -- and
// a second pass adds, per output pixel, the four (input pixel, tap) products that land on it (col2im),
// plus bias and the final ReLU / Sigmoid.  The one-launch form keeps P of a row tile in LDS (2*Cin bytes per input pixel
// in, 16 bytes of output, a halo row per tile side read twice); the two-launch form (ADN_N1_TWO_LAUNCH) passes P
// through the workspace: 64 + 64 more bytes per input pixel.
#include <stdlib.h>

#include "epilogue.h"

namespace {

// ReLU of a 16-byte operand chunk on its raw bits: an element whose sign bit is set (negative values and -0) becomes +0,
// every other element is untouched -- what fmaxf(v, 0.f) stores.  bf16: signed 16-bit max with 0, two elements per dword.
template <typename T>
__device__ __forceinline__ u32x4_t relu_chunk(const u32x4_t& a) {
  if constexpr (sizeof(T) == 2) {
    typedef __attribute__((ext_vector_type(8))) short s16x8_t;
    const s16x8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
    const s16x8_t v = __builtin_elementwise_max(*reinterpret_cast<const s16x8_t*>(&a), z);
    return *reinterpret_cast<const u32x4_t*>(&v);
  } else {
    typedef __attribute__((ext_vector_type(4))) int s32x4_t;
    const s32x4_t z = {0, 0, 0, 0};
    const s32x4_t v = __builtin_elementwise_max(*reinterpret_cast<const s32x4_t*>(&a), z);
    return *reinterpret_cast<const u32x4_t*>(&v);
  }
}

// B operand of the tap GEMM in LDS: lane (tap = fr, k-group fq) of step s holds W[c = s*KS + fq*EPC + j][tap]
template <typename T>
__device__ __forceinline__ void load_tap_weights(const float* w, int nk, u32x4_t* wl) {
  constexpr int EPC = 16 / (int)sizeof(T);
  constexpr int KS = 4 * EPC;
  for (int e = threadIdx.x; e < nk * 64; e += blockDim.x) {
    const int s = e >> 6, l = e & 63;
    const int tap = l & 15, q = l >> 4;
    float f[EPC];
#pragma unroll
    for (int j = 0; j < EPC; ++j) f[j] = w[(int64_t)(s * KS + q * EPC + j) * 16 + tap];
    wl[e] = Chunk<T>::pack(f);
  }
}

// BN1 (bf16): in1 holds the raw conv output z of a train-mode BatchNorm + ReLU layer; the kernel computes the activation
// the materialised tensor would hold (bn_relu_chunk, epilogue.h) on every chunk after its load.  The scale / shift rows
// [2][C1] sit in LDS behind the tap weights and are read per chunk (runtime channel index: not registers).
__device__ __forceinline__ void load_bn_coef(const float* sc1, const float* sh1, int C1, float* cf) {
  for (int e = threadIdx.x; e < C1; e += blockDim.x) {
    cf[e] = sc1[e];
    cf[C1 + e] = sh1[e];
  }
}

// Two-launch form, first pass.  RELU0: in0 holds the values before the ReLU (see relu_chunk).
template <typename T, bool RELU0, bool BN1>
__global__ __launch_bounds__(256) void convt_n1_partial_kernel(const T* in0, int C0, const T* in1, int C1,
                                                               const float* w, int64_t M, float* P, const float* sc1,
                                                               const float* sh1) {
  static_assert(!BN1 || sizeof(T) == 2, "BN1 is a bf16 form");
  constexpr int EPC = 16 / (int)sizeof(T);
  constexpr int KS = 4 * EPC;                       // channels per MFMA step group (32 bf16 / 16 f32)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u32x4_t* wl = reinterpret_cast<u32x4_t*>(smem);   // [nk][64 lanes]
  const int Cin = C0 + C1;
  const int nk = Cin / KS;
  const float* cf = reinterpret_cast<const float*>(smem + nk * 1024);       // BN1: [2][C1]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  load_tap_weights<T>(w, nk, wl);
  if constexpr (BN1) load_bn_coef(sc1, sh1, C1, reinterpret_cast<float*>(smem + nk * 1024));
  __syncthreads();
  const int64_t groups = (M + 15) >> 4;
  const int nk0 = C0 / KS;
  for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < groups; g += (int64_t)gridDim.x * 4) {
    const int64_t m = g * 16 + fr;
    const bool ok = m < M;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < nk; ++s) {
      u32x4_t a = {0u, 0u, 0u, 0u};
      if (ok) {
        if (s < nk0) {
          a = *reinterpret_cast<const u32x4_t*>(in0 + m * C0 + s * KS + fq * EPC);
          if constexpr (RELU0) a = relu_chunk<T>(a);
        } else {
          a = *reinterpret_cast<const u32x4_t*>(in1 + m * C1 + (s - nk0) * KS + fq * EPC);
          if constexpr (BN1) a = bn_relu_chunk(a, cf + (s - nk0) * KS + fq * EPC, cf + C1 + (s - nk0) * KS + fq * EPC);
        }
      }
      const u32x4_t b = wl[s * 64 + lane];
      mma_tile<T>(a, b, acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t mm = g * 16 + 4 * fq + r;
      if (mm < M) P[mm * 16 + fr] = acc[r];
    }
  }
}

__global__ __launch_bounds__(256) void convt_n1_gather_kernel(const float* P, int B, int Hs, int Ws,
                                                              const float* bias, int final_act, float* out) {
  const int Hl = 2 * Hs, Wl = 2 * Ws;
  const int64_t n = (int64_t)B * Hl * Wl;
  const float bv = bias ? bias[0] : 0.f;
  // (32-bit index arithmetic: the host checks n < 2^31; a 64-bit division is a several-hundred-instruction routine)
  for (unsigned e = blockIdx.x * 256 + threadIdx.x; e < (unsigned)n; e += gridDim.x * 256) {
    const unsigned rowi = e / (unsigned)Wl;
    const int ox = (int)(e - rowi * (unsigned)Wl);
    const int b = (int)(rowi / (unsigned)Hl);
    const int oy = (int)(rowi - (unsigned)b * Hl);
    const int ph = oy & 1, pw = ox & 1, i = oy >> 1, j = ox >> 1;
    float v = bv;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int iy = i + adn_t2_dy(ph, t >> 1), ix = j + adn_t2_dy(pw, t & 1);
      if ((unsigned)iy < (unsigned)Hs && (unsigned)ix < (unsigned)Ws)
        v += P[(((int64_t)b * Hs + iy) * Ws + ix) * 16 + adn_t2_kh(ph, t >> 1) * 4 + adn_t2_kh(pw, t & 1)];
    }
    out[e] = adn_final_act(v, final_act);
  }
}

// One-launch form.  A workgroup owns TH input rows (full width) of one image: it computes the 16 tap products of those
// rows and of one halo row above and below -- the same MFMA sequence per pixel as convt_n1_partial_kernel, an MFMA row
// depends on its own pixel only, so the products are the same bits -- into LDS, then writes the 2 TH output rows with
// the addition order of convt_n1_gather_kernel (bias, t = 0..3), four outputs = 16 bytes per thread.  The rows of a tile
// are one contiguous run of pixels (NHWC, full width), so the first phase is a plain stream.
constexpr int kFusedThreads = 1024;
constexpr int kFusedLds = 160 * 1024;               // LDS of a CU (gfx950); a tile that does not fit halves TH
constexpr int kPStride = 17;                        // dwords per pixel in LDS: 16 taps + 1 (the gather walks every other
                                                    // pixel: 34-dword lane stride = 2-way bank conflicts, not 64-way)

template <typename T, bool RELU0, bool BN1>
__global__ __launch_bounds__(kFusedThreads) void convt_n1_fused_kernel(const T* in0, int C0, const T* in1, int C1,
                                                                        const float* w, int Hs, int Ws, int TH,
                                                                        const float* bias, int final_act, float* out,
                                                                        const float* sc1, const float* sh1) {
  static_assert(!BN1 || sizeof(T) == 2, "BN1 is a bf16 form");
  constexpr int EPC = 16 / (int)sizeof(T);
  constexpr int KS = 4 * EPC;
  constexpr int NW = kFusedThreads / 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u32x4_t* wl = reinterpret_cast<u32x4_t*>(smem);   // [nk][64 lanes]
  const int nk = (C0 + C1) / KS, nk0 = C0 / KS;
  const float* cf = reinterpret_cast<const float*>(smem + nk * 1024);       // BN1: [2][C1] (see load_bn_coef)
  float* Pl = reinterpret_cast<float*>(smem + nk * 1024 + (BN1 ? 2 * C1 * 4 : 0));       // [tile pixels][kPStride]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  load_tap_weights<T>(w, nk, wl);
  if constexpr (BN1) load_bn_coef(sc1, sh1, C1, reinterpret_cast<float*>(smem + nk * 1024));
  const int tpi = (Hs + TH - 1) / TH;               // tiles per image
  const int b = (int)blockIdx.x / tpi;
  const int r0 = ((int)blockIdx.x - b * tpi) * TH;
  const int rows = min(TH, Hs - r0);
  const int rlo = max(r0 - 1, 0), rhi = min(r0 + rows + 1, Hs);
  const int m_lo = (b * Hs + rlo) * Ws;             // (32-bit: the host checks 4 M < 2^31)
  const int npix = (rhi - rlo) * Ws;
  const int ngroups = (npix + 15) >> 4;
  __syncthreads();
  // phase 1: two 16-pixel groups per wave and trip, up to 4 K-steps of both requested before the first MFMA
  // (8 x 16 bytes per lane in flight: one workgroup per CU has to cover the HBM latency on its own)
  for (int g = wave; g < ngroups; g += 2 * NW) {
    const int ml[2] = {g * 16 + fr, (g + NW) * 16 + fr};
    f32x4_t acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int s0 = 0; s0 < nk; s0 += 4) {
      u32x4_t a[2][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int s = s0 + u;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          a[h][u] = u32x4_t{0u, 0u, 0u, 0u};
          if (s < nk && ml[h] < npix) {
            const int64_t m = m_lo + ml[h];
            if (s < nk0) {
              a[h][u] = *reinterpret_cast<const u32x4_t*>(in0 + m * C0 + s * KS + fq * EPC);
              if constexpr (RELU0) a[h][u] = relu_chunk<T>(a[h][u]);
            } else {
              a[h][u] = *reinterpret_cast<const u32x4_t*>(in1 + m * C1 + (s - nk0) * KS + fq * EPC);
              if constexpr (BN1)
                a[h][u] = bn_relu_chunk(a[h][u], cf + (s - nk0) * KS + fq * EPC, cf + C1 + (s - nk0) * KS + fq * EPC);
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (s0 + u < nk) {
          const u32x4_t bw = wl[(s0 + u) * 64 + lane];
          mma_tile<T>(a[0][u], bw, acc[0]);
          mma_tile<T>(a[1][u], bw, acc[1]);
        }
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int mm = (g + h * NW) * 16 + 4 * fq + r;
        if (mm < npix) Pl[mm * kPStride + fr] = acc[h][r];
      }
  }
  __syncthreads();
  // phase 2: col2im of the tile's 2 * rows output rows
  const int Hl = 2 * Hs, Wl = 2 * Ws;
  const int qpr = (Wl + 3) >> 2;                    // 4-output pieces per output row
  const int nq = 2 * rows * qpr;
  const bool vec = (Wl & 3) == 0;
  const float bv = bias ? bias[0] : 0.f;
  for (int e = tid; e < nq; e += kFusedThreads) {
    const int orow = e / qpr;
    const int ox0 = (e - orow * qpr) * 4;
    const int oy = 2 * r0 + orow;
    const int ph = oy & 1, i = oy >> 1;
    f32x4_t o;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int ox = ox0 + x;
      const int pw = x & 1, j = ox >> 1;
      float v = bv;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int iy = i + adn_t2_dy(ph, t >> 1), ix = j + adn_t2_dy(pw, t & 1);
        if ((unsigned)iy < (unsigned)Hs && (unsigned)ix < (unsigned)Ws)
          v += Pl[((iy - rlo) * Ws + ix) * kPStride + adn_t2_kh(ph, t >> 1) * 4 + adn_t2_kh(pw, t & 1)];
      }
      o[x] = adn_final_act(v, final_act);
    }
    float* op = out + ((int64_t)b * Hl + oy) * Wl + ox0;
    if (vec) {
      *reinterpret_cast<f32x4_t*>(op) = o;
    } else {
#pragma unroll
      for (int x = 0; x < 4; ++x)
        if (ox0 + x < Wl) op[x] = o[x];
    }
  }
}

// Tile height of the one-launch form (0: the shape does not fit, take the two-launch form).  16 rows re-read 2 of 18
// rows; smaller batches take shorter tiles so that every CU still gets one, and a tile has to fit the LDS.
inline int fused_tile_rows(int B, int Hs, int Ws, int wbytes) {
  static const int forced = getenv("ADN_CONVT_N1_TH") ? atoi(getenv("ADN_CONVT_N1_TH")) : 0;
  int th = forced > 0 ? forced : 16;
  if (forced <= 0)
    while (th > 4 && (int64_t)B * adn_cdiv(Hs, th) < 256) th >>= 1;
  while (th > 1 && (int64_t)(th + 2) * Ws * kPStride * 4 + wbytes > kFusedLds) th >>= 1;
  return (int64_t)(th + 2) * Ws * kPStride * 4 + wbytes <= kFusedLds ? th : 0;
}

template <typename T, bool RELU0, bool BN1>
int launch_n1(int B, int Hs, int Ws, const void* in0, int C0, const void* in1, int C1, const float* w,
              const float* bias, int final_act, float* out, float* P, bool two_launch, const float* sc1,
              const float* sh1, hipStream_t st) {
  const int64_t M = (int64_t)B * Hs * Ws;
  const int nk = (C0 + C1) / (64 / (int)sizeof(T));
  const int wbytes = nk * 64 * 16 + (BN1 ? 2 * C1 * 4 : 0);        // tap weights (+ the scale / shift rows of in1)
  const T* a0 = reinterpret_cast<const T*>(in0);
  const T* a1 = reinterpret_cast<const T*>(in1);
  const int th = two_launch ? 0 : fused_tile_rows(B, Hs, Ws, wbytes);
  if (th > 0) {
    const int rows = th < Hs ? th : Hs;
    const int lds = wbytes + (rows + 2) * Ws * kPStride * 4;
    ADN_SET_LDS_ONCE(kFusedLds, &convt_n1_fused_kernel<T, RELU0, BN1>);
    hipLaunchKernelGGL((convt_n1_fused_kernel<T, RELU0, BN1>), dim3((unsigned)(B * adn_cdiv(Hs, th))),
                       dim3(kFusedThreads), lds, st, a0, C0, a1, C1, w, Hs, Ws, th, bias, final_act, out, sc1, sh1);
    ADN_CHECK_LAUNCH();
    return ADN_OK;
  }
  int64_t blocks = adn_cdiv(adn_cdiv(M, 16), 4);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL((convt_n1_partial_kernel<T, RELU0, BN1>), dim3((unsigned)blocks), dim3(256), wbytes, st, a0, C0, a1,
                     C1, w, M, P, sc1, sh1);
  ADN_CHECK_LAUNCH();
  int64_t gb = adn_cdiv(M * 4, 256);
  if (gb > 4096) gb = 4096;
  hipLaunchKernelGGL(convt_n1_gather_kernel, dim3((unsigned)gb), dim3(256), 0, st, P, B, Hs, Ws, bias, final_act, out);
  ADN_CHECK_LAUNCH();
  return ADN_OK;
}

}  // namespace

extern "C" int64_t adn_convt_n1_workspace_bytes(int32_t B, int32_t Hs, int32_t Ws) {
  if (B <= 0 || Hs <= 0 || Ws <= 0) return -1;
  return (int64_t)B * Hs * Ws * 16 * 4;
}

extern "C" int adn_convt_n1_forward_bn(int32_t dtype, int32_t B, int32_t Hs, int32_t Ws, const void* in0, int32_t C0,
                                       const void* in1, int32_t C1, const float* w, const float* bias,
                                       int32_t final_act, float* out, void* workspace, int64_t workspace_bytes,
                                       int32_t flags, const float* scale1, const float* shift1, void* stream) {
  ADN_CHECK_DTYPE("adn_convt_n1_forward", dtype);
  ADN_CHECK_ARG(!scale1 == !shift1, "adn_convt_n1_forward: scale1 and shift1 come together");
  ADN_CHECK_ARG(!scale1 || (dtype == ADN_BF16 && C1 > 0 && in1),
                "adn_convt_n1_forward: scale1 / shift1 need a bf16 in1 (the raw output of a BatchNorm + ReLU layer)");
  ADN_CHECK_ARG(B > 0 && Hs > 0 && Ws > 0 && C0 > 0 && C1 >= 0, "adn_convt_n1_forward: bad shape");
  ADN_CHECK_ARG(in0 && (C1 == 0 || in1) && w && out && workspace, "adn_convt_n1_forward: null operand");
  ADN_CHECK_ARG((flags & ~(ADN_N1_RELU_IN0 | ADN_N1_TWO_LAUNCH)) == 0, "adn_convt_n1_forward: bad flags %d", flags);
  const int ks = dtype == ADN_BF16 ? 32 : 16;
  ADN_CHECK_ARG(C0 % ks == 0 && C1 % ks == 0, "adn_convt_n1_forward: channels must be multiples of %d (got %d+%d)",
                ks, C0, C1);
  const int64_t M = (int64_t)B * Hs * Ws;
  ADN_CHECK_ARG(workspace_bytes >= M * 64, "adn_convt_n1_forward: workspace too small");
  ADN_CHECK_ARG(M * 4 < (1ll << 31), "adn_convt_n1_forward: tensor too large");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* P = reinterpret_cast<float*>(workspace);
  const bool two = (flags & ADN_N1_TWO_LAUNCH) != 0;
  const bool relu0 = (flags & ADN_N1_RELU_IN0) != 0;
  if (scale1)
    return relu0 ? launch_n1<uint16_t, true, true>(B, Hs, Ws, in0, C0, in1, C1, w, bias, final_act, out, P, two, scale1,
                                                   shift1, st)
                 : launch_n1<uint16_t, false, true>(B, Hs, Ws, in0, C0, in1, C1, w, bias, final_act, out, P, two, scale1,
                                                    shift1, st);
  return adn_by_dtype("adn_convt_n1_forward", dtype, [&](auto t) {
    using T = decltype(t);
    return relu0 ? launch_n1<T, true, false>(B, Hs, Ws, in0, C0, in1, C1, w, bias, final_act, out, P, two, nullptr,
                                             nullptr, st)
                 : launch_n1<T, false, false>(B, Hs, Ws, in0, C0, in1, C1, w, bias, final_act, out, P, two, nullptr,
                                              nullptr, st);
  });
}

extern "C" int adn_convt_n1_forward_ex(int32_t dtype, int32_t B, int32_t Hs, int32_t Ws, const void* in0, int32_t C0,
                                       const void* in1, int32_t C1, const float* w, const float* bias,
                                       int32_t final_act, float* out, void* workspace, int64_t workspace_bytes,
                                       int32_t flags, void* stream) {
  return adn_convt_n1_forward_bn(dtype, B, Hs, Ws, in0, C0, in1, C1, w, bias, final_act, out, workspace,
                                 workspace_bytes, flags, nullptr, nullptr, stream);
}

extern "C" int adn_convt_n1_forward(int32_t dtype, int32_t B, int32_t Hs, int32_t Ws, const void* in0, int32_t C0,
                                    const void* in1, int32_t C1, const float* w, const float* bias,
                                    int32_t final_act, float* out, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
  return adn_convt_n1_forward_ex(dtype, B, Hs, Ws, in0, C0, in1, C1, w, bias, final_act, out, workspace,
                                 workspace_bytes, 0, stream);
}
