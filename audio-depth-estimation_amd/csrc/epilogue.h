// Epilogue of the implicit-GEMM family, shared by the fused MFMA path (8 channels per thread,
// 16-byte accesses) and the split-K / generic reduce path (1 element per call, or its arithmetic on 8 registers).
#pragma once
#include "adn_common.h"

// kind 0 ReLU, 1 Sigmoid, 2 identity (the cVAE head with depth_norm)
__device__ __forceinline__ float adn_final_act(float y, int kind) {
  return kind == 1 ? 1.0f / (1.0f + __expf(-y)) : (kind == 2 ? y : fmaxf(y, 0.0f));
}

// ---- scalar form ---------------------------------------------------------------------------------
// v: GEMM result for output pixel `op`, channel `nl` of segment `sg`.  s1/s2 accumulate stats.
template <typename T>
__device__ __forceinline__ void epi_scalar(int epi, const AdnEpiSeg& sg, int64_t op, int nl, float v,
                                           float& s1, float& s2) {
  const int64_t idx = op * sg.channels + nl;
  if (epi == ADN_EPI_RAW) {
    reinterpret_cast<float*>(sg.out0)[idx] = v;
  } else if (epi == ADN_EPI_Z_STATS) {
    if (sg.bias) v += sg.bias[nl];
    ElemTraits<T>::store(reinterpret_cast<T*>(sg.out0) + idx, v);
    s1 += v;
    s2 += v * v;
  } else if (epi == ADN_EPI_ACT) {
    float y = v;
    if (sg.scale) y = y * sg.scale[nl];
    if (sg.shift) y += sg.shift[nl];
    if (sg.bias) y += sg.bias[nl];
    if (sg.out0) ElemTraits<T>::store(reinterpret_cast<T*>(sg.out0) + idx, y > 0.f ? y : y * sg.slope);
    if (sg.out1) ElemTraits<T>::store(reinterpret_cast<T*>(sg.out1) + idx, fmaxf(y, 0.f));
  } else if (epi == ADN_EPI_BWD) {
    const float r = ElemTraits<T>::load(reinterpret_cast<const T*>(sg.ref) + idx);
    float g = v * (r > 0.f ? 1.0f : sg.slope);
    if (sg.accumulate) g += ElemTraits<T>::load(reinterpret_cast<const T*>(sg.out0) + idx);
    ElemTraits<T>::store(reinterpret_cast<T*>(sg.out0) + idx, g);
    if (sg.partials) {
      const float z = ElemTraits<T>::load(reinterpret_cast<const T*>(sg.z) + idx);
      s1 += g;
      s2 += g * ((z - sg.mean[nl]) * sg.istd[nl]);
    }
  } else if (epi == ADN_EPI_ADD) {
    float g = v;
    if (sg.bias) g += sg.bias[nl];
    if (sg.scale) g *= sg.final_act ? sg.scale[0] : sg.scale[nl];
    if (sg.ref) g += ElemTraits<T>::load(reinterpret_cast<const T*>(sg.ref) + idx);
    if (sg.accumulate) g += ElemTraits<T>::load(reinterpret_cast<const T*>(sg.out0) + idx);
    ElemTraits<T>::store(reinterpret_cast<T*>(sg.out0) + idx, g);
  } else {  // ADN_EPI_FINAL
    float y = v;
    if (sg.bias) y += sg.bias[nl];
    reinterpret_cast<float*>(sg.out0)[idx] = adn_final_act(y, sg.final_act);
  }
}

// ---- 8-channel vector form -------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void load8(const void* base, int64_t idx, float* f) {
  if constexpr (sizeof(T) == 2) {
    u32x4_t c = *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const uint16_t*>(base) + idx);
    Chunk<uint16_t>::unpack(c, f);
  } else {
    const u32x4_t* p = reinterpret_cast<const u32x4_t*>(reinterpret_cast<const float*>(base) + idx);
    u32x4_t c0 = p[0], c1 = p[1];
    Chunk<float>::unpack(c0, f);
    Chunk<float>::unpack(c1, f + 4);
  }
}
template <typename T>
__device__ __forceinline__ void store8(void* base, int64_t idx, const float* f) {
  if constexpr (sizeof(T) == 2) {
    *reinterpret_cast<u32x4_t*>(reinterpret_cast<uint16_t*>(base) + idx) = Chunk<uint16_t>::pack(f);
  } else {
    u32x4_t* p = reinterpret_cast<u32x4_t*>(reinterpret_cast<float*>(base) + idx);
    p[0] = Chunk<float>::pack(f);
    p[1] = Chunk<float>::pack(f + 4);
  }
}

// ---- BatchNorm apply, one element --------------------------------------------------------------------
// Forward: the affine value bn_act_kernel activates, and the bf16 bits its ReLU copy holds for z.  The kernels that read
// a BatchNorm + ReLU activation "virtually" (from z, scale and shift: convt_n1, thin_wgrad, d0_dgrad's mask) call the
// same two functions, so the product and the sum are contracted the same way everywhere.
__device__ __forceinline__ float bn_affine1(float z, float scale, float shift) { return z * scale + shift; }
__device__ __forceinline__ uint32_t bn_relu_bf16_bits(float z, float scale, float shift) {
  return f32_to_bf16_bits(fmaxf(bn_affine1(z, scale, shift), 0.f));
}
// bn_relu_bf16_bits over a 16-byte chunk of bf16 z (8 consecutive channels, coefficients sc[0..7] / sh[0..7])
__device__ __forceinline__ u32x4_t bn_relu_chunk(const u32x4_t& zc, const float* sc, const float* sh) {
  float z[8];
  Chunk<uint16_t>::unpack(zc, z);
  u32x4_t c;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    c[i] = bn_relu_bf16_bits(z[2 * i], sc[2 * i], sh[2 * i]) | (bn_relu_bf16_bits(z[2 * i + 1], sc[2 * i + 1], sh[2 * i + 1]) << 16);
  return c;
}

// Per-thread constants of an 8-channel column group (hoisted out of the row loop).
struct EpiCols {
  float a[8], b[8];  // ACT: scale, shift(+bias); BWD: mean, istd; FINAL: bias in b
};

template <typename T>
__device__ __forceinline__ void epi_cols_init(int epi, const AdnEpiSeg& sg, int nl, EpiCols& c) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    c.a[e] = 1.0f;
    c.b[e] = 0.0f;
  }
  if (epi == ADN_EPI_ACT) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (sg.scale) c.a[e] = sg.scale[nl + e];
      if (sg.shift) c.b[e] = sg.shift[nl + e];
      if (sg.bias) c.b[e] += sg.bias[nl + e];
    }
  } else if (epi == ADN_EPI_BWD && sg.partials) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      c.a[e] = sg.mean[nl + e];
      c.b[e] = sg.istd[nl + e];
    }
  } else if ((epi == ADN_EPI_FINAL || epi == ADN_EPI_Z_STATS) && sg.bias) {
#pragma unroll
    for (int e = 0; e < 8; ++e) c.b[e] = sg.bias[nl + e];
  } else if (epi == ADN_EPI_ADD) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (sg.scale) c.a[e] = sg.final_act ? sg.scale[0] : sg.scale[nl + e];
      if (sg.bias) c.b[e] = sg.bias[nl + e];
    }
  }
}

template <typename T>
__device__ __forceinline__ void epi_vec8(int epi, const AdnEpiSeg& sg, const EpiCols& c, int64_t op, int nl,
                                         const float* v, float* s1, float* s2) {
  const int64_t idx = op * sg.channels + nl;
  if (epi == ADN_EPI_RAW) {
    store8<float>(sg.out0, idx, v);
  } else if (epi == ADN_EPI_Z_STATS) {
    float zb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) zb[e] = v[e] + c.b[e];       // c.b = bias (0 when the conv has none)
    store8<T>(sg.out0, idx, zb);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s1[e] += zb[e];
      s2[e] += zb[e] * zb[e];
    }
  } else if (epi == ADN_EPI_ACT) {
    float y[8], o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = v[e] * c.a[e] + c.b[e];
    if (sg.out0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = y[e] > 0.f ? y[e] : y[e] * sg.slope;
      store8<T>(sg.out0, idx, o);
    }
    if (sg.out1) {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = fmaxf(y[e], 0.f);
      store8<T>(sg.out1, idx, o);
    }
  } else if (epi == ADN_EPI_BWD) {
    float r[8], g[8];
    load8<T>(sg.ref, idx, r);
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = v[e] * (r[e] > 0.f ? 1.0f : sg.slope);
    if (sg.accumulate) {
      float old[8];
      load8<T>(sg.out0, idx, old);
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] += old[e];
    }
    store8<T>(sg.out0, idx, g);
    if (sg.partials) {
      float z[8];
      load8<T>(sg.z, idx, z);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s1[e] += g[e];
        s2[e] += g[e] * ((z[e] - c.a[e]) * c.b[e]);
      }
    }
  } else if (epi == ADN_EPI_ADD) {
    float g[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = (v[e] + c.b[e]) * c.a[e];       // a = 1, b = 0 when not given
    if (sg.ref) {
      float r[8];
      load8<T>(sg.ref, idx, r);
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] += r[e];
    }
    if (sg.accumulate) {
      float old[8];
      load8<T>(sg.out0, idx, old);
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] += old[e];
    }
    store8<T>(sg.out0, idx, g);
  } else {  // FINAL
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = adn_final_act(v[e] + c.b[e], sg.final_act);
    store8<float>(sg.out0, idx, o);
  }
}

// BWD epilogue (bf16) on operand chunks that were loaded ahead of the K loop: same arithmetic as the ADN_EPI_BWD branch
// of epi_vec8.
__device__ __forceinline__ void epi_bwd_pre8(const AdnEpiSeg& sg, const EpiCols& c, int64_t op, int nl, const float* v,
                                             const u32x4_t& ref_raw, const u32x4_t& old_raw, const u32x4_t& z_raw,
                                             float* s1, float* s2) {
  const int64_t idx = op * sg.channels + nl;
  float r[8], g[8];
  Chunk<uint16_t>::unpack(ref_raw, r);
#pragma unroll
  for (int e = 0; e < 8; ++e) g[e] = v[e] * (r[e] > 0.f ? 1.0f : sg.slope);
  if (sg.accumulate) {
    float old[8];
    Chunk<uint16_t>::unpack(old_raw, old);
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] += old[e];
  }
  store8<uint16_t>(sg.out0, idx, g);
  if (sg.partials) {
    float z[8];
    Chunk<uint16_t>::unpack(z_raw, z);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s1[e] += g[e];
      s2[e] += g[e] * ((z[e] - c.a[e]) * c.b[e]);
    }
  }
}

// ---- epi_scalar on 8 registers (the vector form of the split-K / direct reduce kernel) -------------
// The arithmetic of epi_scalar, element for element and bit for bit -- NOT that of epi_vec8, which adds a zero bias
// (-0 becomes +0) and folds shift + bias ahead of the multiply-add in ACT.  epi_scalar compiles without a single fused
// multiply-add: its mul -> add pairs sit in different basic blocks, and the two statistics adds are paired into one
// v_pk_add_f32.  In straight-line code over 8 registers the compiler would contract them (-ffp-contract=fast), so every
// product that feeds an add goes through epi_unfused().
__device__ __forceinline__ float epi_unfused(float x) {
  asm("" : "+v"(x));
  return x;
}

// The bf16 / f32 operand chunks of 8 channels, requested ahead of the arithmetic and unpacked behind it.
template <typename T>
struct EpiRaw8 {
  u32x4_t c[sizeof(T) == 2 ? 1 : 2];
};
template <typename T>
__device__ __forceinline__ void raw8_load(const void* base, int64_t idx, EpiRaw8<T>& r) {
  const u32x4_t* p = reinterpret_cast<const u32x4_t*>(reinterpret_cast<const T*>(base) + idx);
  r.c[0] = p[0];
  if constexpr (sizeof(T) == 4) r.c[1] = p[1];
}
template <typename T>
__device__ __forceinline__ void raw8_unpack(const EpiRaw8<T>& r, float* f) {
  Chunk<T>::unpack(r.c[0], f);
  if constexpr (sizeof(T) == 4) Chunk<T>::unpack(r.c[1], f + 4);
}

// Per-channel vectors of the 8 channels, as epi_scalar reads them (a: scale / mean, b: shift / istd, c: bias)
struct EpiVecs8 {
  float a[8], b[8], c[8];
};
template <int EPI>
__device__ __forceinline__ void epi_scalar8_vecs(const AdnEpiSeg& sg, int nl, EpiVecs8& k) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if constexpr (EPI == ADN_EPI_ACT) {
      if (sg.scale) k.a[e] = sg.scale[nl + e];
      if (sg.shift) k.b[e] = sg.shift[nl + e];
    } else if constexpr (EPI == ADN_EPI_BWD) {
      if (sg.partials) {
        k.a[e] = sg.mean[nl + e];
        k.b[e] = sg.istd[nl + e];
      }
    } else if constexpr (EPI == ADN_EPI_ADD) {
      if (sg.scale) k.a[e] = sg.final_act ? sg.scale[0] : sg.scale[nl + e];
    }
    if constexpr (EPI != ADN_EPI_RAW && EPI != ADN_EPI_BWD) {
      if (sg.bias) k.c[e] = sg.bias[nl + e];
    }
  }
}

// The tensors an element's epilogue reads besides the GEMM result: ref (BWD, ADD), old out0 (accumulate), z (BWD stats)
template <typename T>
struct EpiOps8 {
  EpiRaw8<T> ref, old, z;
};
template <typename T, int EPI>
__device__ __forceinline__ void epi_scalar8_request(const AdnEpiSeg& sg, int64_t op, int nl, EpiOps8<T>& o) {
  const int64_t idx = op * sg.channels + nl;
  if constexpr (EPI == ADN_EPI_BWD) {
    raw8_load<T>(sg.ref, idx, o.ref);
    if (sg.accumulate) raw8_load<T>(sg.out0, idx, o.old);
    if (sg.partials) raw8_load<T>(sg.z, idx, o.z);
  } else if constexpr (EPI == ADN_EPI_ADD) {
    if (sg.ref) raw8_load<T>(sg.ref, idx, o.ref);
    if (sg.accumulate) raw8_load<T>(sg.out0, idx, o.old);
  }
}

// v: the GEMM results of output pixel `op`, channels nl .. nl+7 of segment `sg`.  t1 / t2: the element's statistics terms
// (Z_STATS: t1 = z; BWD: t1 = g, t2 = (z - mean) * istd); the caller folds them in row order:
// s1 += t1, s2 += epi_unfused(t1 * t1) resp. epi_unfused(t1 * t2).
template <typename T, int EPI>
__device__ __forceinline__ void epi_scalar8(const AdnEpiSeg& sg, const EpiVecs8& k, const EpiOps8<T>& o, int64_t op, int nl,
                                            const float* v, float* t1, float* t2) {
  const int64_t idx = op * sg.channels + nl;
  if constexpr (EPI == ADN_EPI_RAW) {
    store8<float>(sg.out0, idx, v);
  } else if constexpr (EPI == ADN_EPI_Z_STATS) {
#pragma unroll
    for (int e = 0; e < 8; ++e) t1[e] = sg.bias ? v[e] + k.c[e] : v[e];
    store8<T>(sg.out0, idx, t1);
  } else if constexpr (EPI == ADN_EPI_ACT) {
    float y[8], w[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      y[e] = v[e];
      if (sg.scale) y[e] = epi_unfused(y[e] * k.a[e]);
      if (sg.shift) y[e] += k.b[e];
      if (sg.bias) y[e] += k.c[e];
    }
    if (sg.out0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] = y[e] > 0.f ? y[e] : y[e] * sg.slope;
      store8<T>(sg.out0, idx, w);
    }
    if (sg.out1) {
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] = fmaxf(y[e], 0.f);
      store8<T>(sg.out1, idx, w);
    }
  } else if constexpr (EPI == ADN_EPI_BWD) {
    float r[8], g[8];
    raw8_unpack<T>(o.ref, r);
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = epi_unfused(v[e] * (r[e] > 0.f ? 1.0f : sg.slope));
    if (sg.accumulate) {
      float old[8];
      raw8_unpack<T>(o.old, old);
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] += old[e];
    }
    store8<T>(sg.out0, idx, g);
    if (sg.partials) {
      float z[8];
      raw8_unpack<T>(o.z, z);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        t1[e] = g[e];
        t2[e] = (z[e] - k.a[e]) * k.b[e];
      }
    }
  } else if constexpr (EPI == ADN_EPI_ADD) {
    float g[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      g[e] = v[e];
      if (sg.bias) g[e] += k.c[e];
      if (sg.scale) g[e] = epi_unfused(g[e] * k.a[e]);
    }
    if (sg.ref) {
      float r[8];
      raw8_unpack<T>(o.ref, r);
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] += r[e];
    }
    if (sg.accumulate) {
      float old[8];
      raw8_unpack<T>(o.old, old);
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] += old[e];
    }
    store8<T>(sg.out0, idx, g);
  } else {  // ADN_EPI_FINAL
    float y[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = adn_final_act(sg.bias ? v[e] + k.c[e] : v[e], sg.final_act);
    store8<float>(sg.out0, idx, y);
  }
}
