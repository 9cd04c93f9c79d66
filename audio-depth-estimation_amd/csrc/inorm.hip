// InstanceNorm2d(affine=False, track_running_stats=False) + activation (+ dropout) of a raw conv output, and its
// backward (get_norm_layer('instance'), unetbaseline_model.py:70-71,190-229; nn.Dropout(0.5) :227).
//
// Activations are NHWC [B][HW][C]; statistics are per (sample, channel) over the HW rows.  A workgroup of 256 threads owns
// `cg` consecutive channels of up to kSlabRows rows of ONE sample: thread t handles the item (VEC channels) at channel
// group t % ng of the rows t / ng, t / ng + 256 / ng, ... (ng = cg / VEC items per row), so a thread stays on the same
// channels and every reduction is over threads with equal t % ng, in a fixed order (wave butterflies, then the four
// waves in order): no atomics, the same bits every run.
//
//   resident form  (HW <= kSlabRows): the slice is copied to LDS while it is summed (each thread re-reads only what it
//                  wrote itself), the variance is taken about the mean from LDS and the outputs are written from LDS:
//                  z (backward: g and z) is read from memory once.
//   streaming form (HW  > kSlabRows): one workgroup per slab of kSlabRows rows.  Forward: the slab is made resident as
//                  above and leaves (mean, M2) in the workspace; the apply pass merges the slabs of its sample with
//                  Chan's formula in slab order, then reads z again.  Backward: plain slab sums, merged in slab order.
//   VEC = 8 (C % 8 == 0): 16-byte accesses.  VEC = 1: any C, one element per access, channels past C masked.
#include "adn_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSlabRows = 1024;            // rows of one sample per workgroup; also the resident / streaming switch
constexpr int kSliceBytes = 64 * 1024;     // LDS for the resident slice(s) of a workgroup (two workgroups per CU)
constexpr int kRedBytes = 4 * 2 * 32 * 4;  // reduction scratch in front of the slices (group_sum)

template <typename T, int VEC> struct Item;
template <typename T> struct Item<T, 8> {
  static constexpr int NCH = 8 * (int)sizeof(T) / 16;
  struct Raw { u32x4_t c[NCH]; };
  __device__ static __forceinline__ Raw load(const T* p) {
    Raw r;
#pragma unroll
    for (int i = 0; i < NCH; ++i) r.c[i] = reinterpret_cast<const u32x4_t*>(p)[i];
    return r;
  }
  __device__ static __forceinline__ void store(T* p, const Raw& r) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) reinterpret_cast<u32x4_t*>(p)[i] = r.c[i];
  }
  __device__ static __forceinline__ void unpack(const Raw& r, float* f) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) Chunk<T>::unpack(r.c[i], f + i * Chunk<T>::N);
  }
  __device__ static __forceinline__ Raw pack(const float* f) {
    Raw r;
#pragma unroll
    for (int i = 0; i < NCH; ++i) r.c[i] = Chunk<T>::pack(f + i * Chunk<T>::N);
    return r;
  }
  __device__ static __forceinline__ void load_keep(const uint8_t* p, float scale, float* k) {
    const uint2 m = *reinterpret_cast<const uint2*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      k[i] = ((m.x >> (8 * i)) & 0xffu) ? scale : 0.f;
      k[4 + i] = ((m.y >> (8 * i)) & 0xffu) ? scale : 0.f;
    }
  }
};
template <typename T> struct Item<T, 1> {
  struct Raw { T c; };
  __device__ static __forceinline__ Raw load(const T* p) { return Raw{*p}; }
  __device__ static __forceinline__ void store(T* p, const Raw& r) { *p = r.c; }
  __device__ static __forceinline__ void unpack(const Raw& r, float* f) { f[0] = ElemTraits<T>::load(&r.c); }
  __device__ static __forceinline__ Raw pack(const float* f) {
    Raw r;
    ElemTraits<T>::store(&r.c, f[0]);
    return r;
  }
  __device__ static __forceinline__ void load_keep(const uint8_t* p, float scale, float* k) { k[0] = *p ? scale : 0.f; }
};

// Sum of NV values per thread over the threads with the same t % ng (ng a power of two <= 32); every thread gets the
// total.  red: 4 * NV * ng floats (<= 4 * 2 * 32).
template <int NV>
__device__ __forceinline__ void group_sum(float* v, int ng, float* red) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = t % ng;
#pragma unroll
  for (int k = 0; k < NV; ++k)
    for (int o = 32; o >= ng; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
  __syncthreads();                                   // red may still be read from the previous reduction
  if (lane < ng) {
#pragma unroll
    for (int k = 0; k < NV; ++k) red[(wave * ng + g) * NV + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k)
    v[k] = ((red[(0 * ng + g) * NV + k] + red[(1 * ng + g) * NV + k]) + red[(2 * ng + g) * NV + k]) +
           red[(3 * ng + g) * NV + k];
}

template <typename T, int VEC>
__device__ __forceinline__ void emit(const float* xhat, int64_t e, float slope, T* out_leaky, T* out_relu,
                                     const uint8_t* keep, float kscale) {
  using I = Item<T, VEC>;
  float ks[VEC], o[VEC];
  if (keep) I::load_keep(keep + e, kscale, ks);
  if (out_leaky) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      o[k] = xhat[k] > 0.f ? xhat[k] : xhat[k] * slope;
      if (keep) o[k] *= ks[k];
    }
    I::store(out_leaky + e, I::pack(o));
  }
  if (out_relu) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      o[k] = fmaxf(xhat[k], 0.f);
      if (keep) o[k] *= ks[k];
    }
    I::store(out_relu + e, I::pack(o));
  }
}

enum { kResident = 0, kSlabStats = 1, kApply = 2 };

struct Geo {
  int HW, C, cg, S;      // S slabs of kSlabRows rows per sample
};

// grid (channel groups, S, B).  ws: [B][S][2][C] f32.
template <typename T, int VEC, int MODE>
__global__ __launch_bounds__(kThreads) void inorm_fwd_kernel(const T* z, Geo geo, float eps, float slope, float* mean,
                                                             float* istd, T* out_leaky, T* out_relu,
                                                             const uint8_t* keep, float kscale, float* ws) {
  using I = Item<T, VEC>;
  extern __shared__ __attribute__((aligned(16))) unsigned char inorm_smem[];
  float* red = reinterpret_cast<float*>(inorm_smem);
  T* slice = reinterpret_cast<T*>(inorm_smem + kRedBytes);
  const int t = threadIdx.x, HW = geo.HW, C = geo.C;
  const int ng = geo.cg / VEC, g = t % ng, prow = t / ng, pstride = kThreads / ng;
  const int b = blockIdx.z, s = blockIdx.y, c = blockIdx.x * geo.cg + g * VEC;
  const int r0 = s * kSlabRows, nrows = min(kSlabRows, HW - r0);
  const bool cvalid = c < C;                        // VEC 8: always (C % cg == 0)
  const int64_t base = ((int64_t)b * HW + r0) * C + c;
  float mu[VEC], is[VEC];

  if constexpr (MODE != kApply) {
    // pass 1: copy to LDS, sum about the slab's first row (the mean then carries no cancellation of a large offset)
    float k0[VEC], acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) k0[k] = acc[k] = 0.f;
    if (cvalid) {
      I::unpack(I::load(z + base), k0);
      int it = t;
      for (int r = prow; r < nrows; r += pstride, it += kThreads) {
        const typename I::Raw raw = I::load(z + base + (int64_t)r * C);
        I::store(slice + (int64_t)it * VEC, raw);
        float v[VEC];
        I::unpack(raw, v);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] += v[k] - k0[k];
      }
    }
    group_sum<VEC>(acc, ng, red);
#pragma unroll
    for (int k = 0; k < VEC; ++k) mu[k] = k0[k] + acc[k] / (float)nrows;
    // pass 2: M2 about the mean, from LDS (each thread reads back its own items)
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    if (cvalid) {
      int it = t;
      for (int r = prow; r < nrows; r += pstride, it += kThreads) {
        float v[VEC];
        I::unpack(I::load(slice + (int64_t)it * VEC), v);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float d = v[k] - mu[k];
          acc[k] += d * d;
        }
      }
    }
    group_sum<VEC>(acc, ng, red);
    if constexpr (MODE == kSlabStats) {
      if (t < ng && cvalid) {
        float* row = ws + ((int64_t)b * geo.S + s) * 2 * C + c;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          row[k] = mu[k];
          row[C + k] = acc[k];
        }
      }
      return;
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) is[k] = 1.0f / sqrtf(acc[k] / (float)nrows + eps);
  } else {
    // merge the slabs of this sample in slab order (Chan et al.): the same order in every workgroup -> the same bits
    float m2[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) mu[k] = m2[k] = 0.f;
    if (cvalid) {
      float na = 0.f;
      for (int q = 0; q < geo.S; ++q) {
        const float* row = ws + ((int64_t)b * geo.S + q) * 2 * C + c;
        const float nb = (float)min(kSlabRows, HW - q * kSlabRows), n = na + nb;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float d = row[k] - mu[k];
          mu[k] += d * (nb / n);
          m2[k] += row[C + k] + d * d * (na * nb / n);
        }
        na = n;
      }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) is[k] = 1.0f / sqrtf(m2[k] / (float)HW + eps);
  }
  if (t < ng && cvalid && s == 0) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      mean[(int64_t)b * C + c + k] = mu[k];
      istd[(int64_t)b * C + c + k] = is[k];
    }
  }
  if (!cvalid) return;
  int it = t;
  for (int r = prow; r < nrows; r += pstride, it += kThreads) {
    const int64_t e = base + (int64_t)r * C;
    float v[VEC];
    if constexpr (MODE == kApply) I::unpack(I::load(z + e), v);
    else I::unpack(I::load(slice + (int64_t)it * VEC), v);
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = (v[k] - mu[k]) * is[k];
    emit<T, VEC>(v, e, slope, out_leaky, out_relu, keep, kscale);
  }
}

// g <- istd * (g' - mean_hw(g') - xhat * mean_hw(g' * xhat)), g' = gscale * g.  lds_items: items per tensor slice.
template <typename T, int VEC, int MODE>
__global__ __launch_bounds__(kThreads) void inorm_bwd_kernel(T* gbuf, const T* z, Geo geo, const float* mean,
                                                             const float* istd, float gscale, float* ws,
                                                             int lds_items) {
  using I = Item<T, VEC>;
  extern __shared__ __attribute__((aligned(16))) unsigned char inorm_smem[];
  float* red = reinterpret_cast<float*>(inorm_smem);
  T* slice_g = reinterpret_cast<T*>(inorm_smem + kRedBytes);
  T* slice_z = slice_g + (int64_t)lds_items * VEC;
  const int t = threadIdx.x, HW = geo.HW, C = geo.C;
  const int ng = geo.cg / VEC, g = t % ng, prow = t / ng, pstride = kThreads / ng;
  const int b = blockIdx.z, s = blockIdx.y, c = blockIdx.x * geo.cg + g * VEC;
  const int r0 = s * kSlabRows, nrows = min(kSlabRows, HW - r0);
  const bool cvalid = c < C;
  const int64_t base = ((int64_t)b * HW + r0) * C + c;
  float mu[VEC], is[VEC], sums[2 * VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) mu[k] = is[k] = sums[k] = sums[VEC + k] = 0.f;
  if (cvalid) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      mu[k] = mean[(int64_t)b * C + c + k];
      is[k] = istd[(int64_t)b * C + c + k];
    }
  }
  if constexpr (MODE != kApply) {
    if (cvalid) {
      int it = t;
      for (int r = prow; r < nrows; r += pstride, it += kThreads) {
        const int64_t e = base + (int64_t)r * C;
        const typename I::Raw rg = I::load(gbuf + e), rz = I::load(z + e);
        if constexpr (MODE == kResident) {
          I::store(slice_g + (int64_t)it * VEC, rg);
          I::store(slice_z + (int64_t)it * VEC, rz);
        }
        float gv[VEC], zv[VEC];
        I::unpack(rg, gv);
        I::unpack(rz, zv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float gp = gv[k] * gscale;
          sums[k] += gp;
          sums[VEC + k] += gp * ((zv[k] - mu[k]) * is[k]);
        }
      }
    }
    group_sum<2 * VEC>(sums, ng, red);
    if constexpr (MODE == kSlabStats) {
      if (t < ng && cvalid) {
        float* row = ws + ((int64_t)b * geo.S + s) * 2 * C + c;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          row[k] = sums[k];
          row[C + k] = sums[VEC + k];
        }
      }
      return;
    }
  } else if (cvalid) {
    for (int q = 0; q < geo.S; ++q) {                // slab order, the same in every workgroup
      const float* row = ws + ((int64_t)b * geo.S + q) * 2 * C + c;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        sums[k] += row[k];
        sums[VEC + k] += row[C + k];
      }
    }
  }
  if (!cvalid) return;
  const float inv = 1.0f / (float)HW;
  int it = t;
  for (int r = prow; r < nrows; r += pstride, it += kThreads) {
    const int64_t e = base + (int64_t)r * C;
    float gv[VEC], zv[VEC];
    if constexpr (MODE == kApply) {
      I::unpack(I::load(gbuf + e), gv);
      I::unpack(I::load(z + e), zv);
    } else {
      I::unpack(I::load(slice_g + (int64_t)it * VEC), gv);
      I::unpack(I::load(slice_z + (int64_t)it * VEC), zv);
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float xh = (zv[k] - mu[k]) * is[k];
      gv[k] = is[k] * (gv[k] * gscale - sums[k] * inv - xh * (sums[VEC + k] * inv));
    }
    I::store(gbuf + e, I::pack(gv));
  }
}

// x <- x * (keep ? scale : 0) in place (keep == nullptr: x * scale): nn.Dropout around a BatchNorm or no norm.
template <typename T, int VEC>
__global__ __launch_bounds__(kThreads) void dropout_apply_kernel(T* x, const uint8_t* keep, int64_t n, float scale) {
  using I = Item<T, VEC>;
  const int64_t items = n / VEC;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < items; i += (int64_t)gridDim.x * kThreads) {
    const int64_t e = i * VEC;
    float v[VEC], ks[VEC];
    I::unpack(I::load(x + e), v);
    if (keep) I::load_keep(keep + e, scale, ks);
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] *= keep ? ks[k] : scale;
    I::store(x + e, I::pack(v));
  }
}

// ---- host side: one rule for the form, the channel width of a workgroup and its LDS ------------------------------------
struct Plan {
  int vec, cg, S, resident;
  int lds_items;          // items of one tensor slice in LDS
  int lds_bytes;
};

int pow2_ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

// tensors: slices a workgroup keeps in LDS (forward 1, resident backward 2, streaming backward 0)
bool make_plan(int HW, int C, int dtype, bool bwd, Plan* p) {
  const int esz = adn_dtype_bytes(dtype);
  p->vec = (C % 8 == 0) ? 8 : 1;
  p->resident = HW <= kSlabRows;
  p->S = (int)adn_cdiv(HW, kSlabRows);
  const int rows = p->resident ? HW : kSlabRows;
  const int tensors = bwd ? (p->resident ? 2 : 0) : 1;
  for (int cg = 32; cg >= p->vec; cg >>= 1) {
    if (p->vec == 8 ? (C % cg != 0) : (cg > pow2_ceil(C))) continue;
    const int pstride = kThreads / (cg / p->vec);
    const int64_t items = adn_cdiv(rows, pstride) * kThreads;
    const int64_t bytes = (int64_t)tensors * items * p->vec * esz;
    if (bytes > kSliceBytes) continue;
    p->cg = cg;
    p->lds_items = (int)items;
    p->lds_bytes = (int)bytes;
    return true;
  }
  return false;
}

bool aligned(const void* ptr, int bytes) { return (reinterpret_cast<uintptr_t>(ptr) & (uintptr_t)(bytes - 1)) == 0; }

int check_common(const char* who, int32_t B, int32_t HW, int32_t C, int32_t dtype, const void* workspace,
                 int64_t workspace_bytes, Plan* p, bool bwd) {
  ADN_CHECK_DTYPE(who, dtype);
  ADN_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && (int64_t)B * C < (1ll << 31), "%s: bad shape B=%d C=%d", who, B, C);
  ADN_CHECK_ARG(HW >= 2, "%s: HW=%d: instance statistics need more than 1 spatial element", who, HW);
  ADN_CHECK_ARG(HW <= 65535 * kSlabRows, "%s: HW=%d too large", who, HW);
  ADN_CHECK_ARG(make_plan(HW, C, dtype, bwd, p), "%s: no plan for HW=%d C=%d", who, HW, C);
  const int64_t need = adn_inorm_workspace_bytes(B, HW, C);
  ADN_CHECK_ARG(workspace && aligned(workspace, 4) && workspace_bytes >= need,
                "%s: workspace of %lld bytes, adn_inorm_workspace_bytes says %lld", who, (long long)workspace_bytes,
                (long long)need);
  return ADN_OK;
}

template <typename T, int VEC>
int launch_fwd(const Plan& p, const T* z, int B, int HW, int C, float eps, float slope, float* mean, float* istd,
               T* out_leaky, T* out_relu, const uint8_t* keep, float kscale, float* ws, hipStream_t st) {
  const Geo geo{HW, C, p.cg, p.S};
  const dim3 grid((unsigned)adn_cdiv(C, p.cg), (unsigned)p.S, (unsigned)B);
  if (p.resident) {
    ADN_SET_LDS_ONCE(kSliceBytes + kRedBytes, &inorm_fwd_kernel<T, VEC, kResident>);
    hipLaunchKernelGGL((inorm_fwd_kernel<T, VEC, kResident>), grid, dim3(kThreads), p.lds_bytes + kRedBytes, st, z, geo, eps, slope,
                       mean, istd, out_leaky, out_relu, keep, kscale, ws);
    ADN_CHECK_LAUNCH();
    return ADN_OK;
  }
  ADN_SET_LDS_ONCE(kSliceBytes + kRedBytes, &inorm_fwd_kernel<T, VEC, kSlabStats>);
  hipLaunchKernelGGL((inorm_fwd_kernel<T, VEC, kSlabStats>), grid, dim3(kThreads), p.lds_bytes + kRedBytes, st, z, geo, eps, slope,
                     mean, istd, out_leaky, out_relu, keep, kscale, ws);
  ADN_CHECK_LAUNCH();
  hipLaunchKernelGGL((inorm_fwd_kernel<T, VEC, kApply>), grid, dim3(kThreads), 0, st, z, geo, eps, slope, mean, istd,
                     out_leaky, out_relu, keep, kscale, ws);
  ADN_CHECK_LAUNCH();
  return ADN_OK;
}

template <typename T, int VEC>
int launch_bwd(const Plan& p, T* g, const T* z, int B, int HW, int C, const float* mean, const float* istd,
               float gscale, float* ws, hipStream_t st) {
  const Geo geo{HW, C, p.cg, p.S};
  const dim3 grid((unsigned)adn_cdiv(C, p.cg), (unsigned)p.S, (unsigned)B);
  if (p.resident) {
    ADN_SET_LDS_ONCE(kSliceBytes + kRedBytes, &inorm_bwd_kernel<T, VEC, kResident>);
    hipLaunchKernelGGL((inorm_bwd_kernel<T, VEC, kResident>), grid, dim3(kThreads), p.lds_bytes + kRedBytes, st, g, z, geo, mean,
                       istd, gscale, ws, p.lds_items);
    ADN_CHECK_LAUNCH();
    return ADN_OK;
  }
  hipLaunchKernelGGL((inorm_bwd_kernel<T, VEC, kSlabStats>), grid, dim3(kThreads), kRedBytes, st, g, z, geo, mean, istd, gscale,
                     ws, 0);
  ADN_CHECK_LAUNCH();
  hipLaunchKernelGGL((inorm_bwd_kernel<T, VEC, kApply>), grid, dim3(kThreads), 0, st, g, z, geo, mean, istd, gscale, ws,
                     0);
  ADN_CHECK_LAUNCH();
  return ADN_OK;
}

}  // namespace

extern "C" int64_t adn_inorm_workspace_bytes(int32_t B, int32_t HW, int32_t C) {
  if (B <= 0 || HW < 2 || C <= 0) {
    adn_set_error("adn_inorm_workspace_bytes: bad shape B=%d HW=%d C=%d", B, HW, C);
    return -1;
  }
  return (int64_t)B * adn_cdiv(HW, kSlabRows) * 2 * C * (int64_t)sizeof(float);
}

extern "C" int adn_dropout_apply(void* x, const uint8_t* keep, int64_t n, int32_t dtype, float scale, void* stream) {
  ADN_CHECK_ARG(x && n > 0, "adn_dropout_apply: null tensor or n=%lld", (long long)n);
  ADN_CHECK_DTYPE("adn_dropout_apply", dtype);
  const bool vec = n % 8 == 0 && aligned(x, 16) && aligned(keep, 8);
  ADN_CHECK_ARG(aligned(x, adn_dtype_bytes(dtype)), "adn_dropout_apply: misaligned tensor");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)adn_grid_blocks(vec ? n / 8 : n, kThreads, 4096));
  return adn_by_dtype_v("adn_dropout_apply", dtype, vec, [&](auto t, auto v) {
    using T = decltype(t);
    constexpr int VEC = decltype(v)::value;
    hipLaunchKernelGGL((dropout_apply_kernel<T, VEC>), grid, dim3(kThreads), 0, st, adn_as<T>(x), keep, n, scale);
    ADN_CHECK_LAUNCH();
    return ADN_OK;
  });
}

extern "C" int adn_inorm_form(int32_t HW, int32_t C, int32_t dtype) {
  Plan p;
  ADN_CHECK_DTYPE("adn_inorm_form", dtype);
  ADN_CHECK_ARG(HW >= 2 && C > 0, "adn_inorm_form: bad shape HW=%d C=%d", HW, C);
  ADN_CHECK_ARG(make_plan(HW, C, dtype, false, &p) && make_plan(HW, C, dtype, true, &p),
                "adn_inorm_form: no plan for HW=%d C=%d", HW, C);
  return (p.resident ? 1 : 2) + (p.vec == 8 ? 0 : 2);
}

extern "C" int adn_inorm_fwd(const void* z, int32_t B, int32_t HW, int32_t C, int32_t dtype, float eps, float slope,
                             float* mean, float* istd, void* out_leaky, void* out_relu, const uint8_t* keep,
                             float keep_scale, void* workspace, int64_t workspace_bytes, void* stream) {
  Plan p;
  const int rc = check_common("adn_inorm_fwd", B, HW, C, dtype, workspace, workspace_bytes, &p, false);
  if (rc != ADN_OK) return rc;
  ADN_CHECK_ARG(z && mean && istd && (out_leaky || out_relu) && eps > 0.f, "adn_inorm_fwd: null argument or eps <= 0");
  const int al = p.vec == 8 ? 16 : adn_dtype_bytes(dtype);
  ADN_CHECK_ARG(aligned(z, al) && aligned(out_leaky, al) && aligned(out_relu, al) && aligned(mean, 4) &&
                    aligned(istd, 4) && aligned(keep, p.vec == 8 ? 8 : 1),
                "adn_inorm_fwd: misaligned pointer (activations need %d bytes)", al);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* ws = reinterpret_cast<float*>(workspace);
  return adn_by_dtype_v("adn_inorm_fwd", dtype, p.vec == 8, [&](auto t, auto v) {
    using T = decltype(t);
    return launch_fwd<T, decltype(v)::value>(p, adn_as<T>(z), B, HW, C, eps, slope, mean, istd, adn_as<T>(out_leaky),
                                             adn_as<T>(out_relu), keep, keep_scale, ws, st);
  });
}

extern "C" int adn_inorm_bwd(void* g, const void* z, const float* mean, const float* istd, int32_t B, int32_t HW,
                             int32_t C, int32_t dtype, float gscale, void* workspace, int64_t workspace_bytes,
                             void* stream) {
  Plan p;
  const int rc = check_common("adn_inorm_bwd", B, HW, C, dtype, workspace, workspace_bytes, &p, true);
  if (rc != ADN_OK) return rc;
  ADN_CHECK_ARG(g && z && mean && istd, "adn_inorm_bwd: null argument");
  const int al = p.vec == 8 ? 16 : adn_dtype_bytes(dtype);
  ADN_CHECK_ARG(aligned(g, al) && aligned(z, al) && aligned(mean, 4) && aligned(istd, 4),
                "adn_inorm_bwd: misaligned pointer (activations need %d bytes)", al);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* ws = reinterpret_cast<float*>(workspace);
  return adn_by_dtype_v("adn_inorm_bwd", dtype, p.vec == 8, [&](auto t, auto v) {
    using T = decltype(t);
    return launch_bwd<T, decltype(v)::value>(p, adn_as<T>(g), adn_as<T>(z), B, HW, C, mean, istd, gscale, ws, st);
  });
}
