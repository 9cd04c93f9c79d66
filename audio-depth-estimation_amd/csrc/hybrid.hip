// Hybrid coarse-depth family (CoarseWithOffsetModel / CoarseOffsetLoss, coarse_depth_model.py:591-850,
// train_coarse_depth.py:336-343): the loss tail behind the class head and the offset head.  Memory-bound; conventions of
// coarse.hip / dualreg.hip: f32 arithmetic, f64 final reductions, no atomics, bit-reproducible run to run (fixed grid per
// pixel count, fixed reduction order).
//   hybrid_loss      ONE pass over the logits: final = coarse + offset, label-smoothed cross-entropy, L1 / L2 of final,
//                    |offset|, the monitoring |coarse - gt|, and the gradients towards the logits and the offset plane.
//                    The coarse depth is an INPUT (what the forward-only adn_coarse_loss pass wrote before the offset
//                    branch ran), so the softmax expectation is not accumulated again.  No valid mask anywhere.
//   hybrid_finish    per-block f64 partials -> sums -> (ce, regression, offset_reg, coarse_l1, total)
// The chunk / lane-group helpers of coarse.hip are not shared: this file keeps its own small copies, coarse.hip is untouched.
#include "adn_common.h"

namespace {

constexpr int kMaxNb = 512;          // 8 x 64 lanes of one wave (generic kernel) / 64 lanes x one 16-byte chunk (vector kernel)
constexpr int kMaxBlocks = 2048;
constexpr int kSums = 4;             // ce, regression, |offset|, |coarse - gt|

struct HybridP {
  const void* logits; const float* centers; const float* coarse; const float* offset; const int32_t* bins; const float* gt;
  float* final_; void* dlogits; float* doffset; double* partial;
  int64_t pixels;
  int nb, ld, reg_mode;
  float ce_coef, reg_coef, off_coef;      // the three weights / global pixel count
  float keep, smooth, inv_nb;             // 1 - eps, eps / nb, 1 / nb
  float eps;
};

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }      // torch's abs backward

// What one pixel contributes once its reductions are known.  se = sum exp(x - max), sd = sum (x - max), A = x_t - max.
struct PixTerms {
  float inv, coarse, final_, ce, reg, aoff, cl1, r, doff;
};
__device__ __forceinline__ PixTerms pixel_terms(const HybridP& p, float se, float sd, float A, float c, float o, float gtv) {
  PixTerms t;
  t.inv = 1.f / se;
  const float logz = __logf(se);
  t.ce = p.keep * (logz - A) + p.eps * (logz - sd * p.inv_nb);
  t.coarse = c;
  t.final_ = c + o;
  const float e = t.final_ - gtv;
  if (p.reg_mode == 0) {
    t.reg = fabsf(e);
    t.r = p.reg_coef * sgn(e);
  } else {
    t.reg = e * e;
    t.r = p.reg_coef * 2.f * e;
  }
  t.aoff = fabsf(o);
  t.cl1 = fabsf(c - gtv);
  t.doff = t.r + p.off_coef * sgn(o);
  return t;
}

__device__ __forceinline__ float grad_elem(const HybridP& p, const PixTerms& t, float pk, bool is_t, float ck) {
  return p.ce_coef * (pk - (is_t ? p.keep : 0.f) - p.smooth) + t.r * pk * (ck - t.coarse);
}

__device__ __forceinline__ void block_partials(double (&a)[kSums], double* out) {      // 256 threads
  __shared__ double sm[kSums][4];
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
    a[k] = wave_sum_d(a[k]);
    if ((threadIdx.x & 63) == 0) sm[k][threadIdx.x >> 6] = a[k];
  }
  __syncthreads();
  if (threadIdx.x < kSums) out[threadIdx.x] = sm[threadIdx.x][0] + sm[threadIdx.x][1] + sm[threadIdx.x][2] + sm[threadIdx.x][3];
}

// bf16, ld == nb = 8 LPP, LPP a power of two <= 64 (coarse_loss_vec_kernel's layout): a pixel's bins are LPP lanes x one
// 16-byte load each, 64 / LPP pixels per wave-iteration, reductions across those lanes only; the gradient leaves as one
// 16-byte store
template <int LPP>
__global__ __launch_bounds__(256) void hybrid_loss_vec_kernel(HybridP p) {
  constexpr int NB = LPP * 8, PPW = 64 / LPP;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int li = lane % LPP, pw = lane / LPP;
  const uint16_t* lg = reinterpret_cast<const uint16_t*>(p.logits);
  uint16_t* dl = reinterpret_cast<uint16_t*>(p.dlogits);
  float cv[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) cv[k] = p.centers[li * 8 + k];
  double acc[kSums] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t p0 = ((int64_t)blockIdx.x * 4 + wave) * PPW; p0 < p.pixels; p0 += (int64_t)gridDim.x * 4 * PPW) {
    const int64_t pix = p0 + pw;
    const bool live = pix < p.pixels;
    float d[8];
    float mx = -INFINITY;
    int t = 0;
    float c = 0.f, o = 0.f, gtv = 0.f;
    if (live) {
      const u32x4_t ch = *reinterpret_cast<const u32x4_t*>(lg + pix * NB + li * 8);
      t = p.bins[pix];
      c = p.coarse[pix];
      o = p.offset[pix];
      gtv = p.gt[pix];
      Chunk<uint16_t>::unpack(ch, d);
#pragma unroll
      for (int k = 0; k < 8; ++k) mx = fmaxf(mx, d[k]);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) d[k] = 0.f;
      mx = 0.f;
    }
#pragma unroll
    for (int off = 1; off < LPP; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    float e[8];
    float se = 0.f, sd = 0.f, A = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      d[k] -= mx;
      e[k] = __expf(d[k]);
      se += e[k];
      sd += d[k];
      A += (li * 8 + k) == t ? d[k] : 0.f;
    }
#pragma unroll
    for (int off = 1; off < LPP; off <<= 1) {
      se += __shfl_xor(se, off, 64);
      sd += __shfl_xor(sd, off, 64);
      A += __shfl_xor(A, off, 64);
    }
    if (live) {                                        // the shuffles above need every lane; what follows does not
      const PixTerms pt = pixel_terms(p, se, sd, A, c, o, gtv);
      if (li == 0) {
        p.final_[pix] = pt.final_;
        p.doffset[pix] = pt.doff;
        acc[0] += (double)pt.ce;
        acc[1] += (double)pt.reg;
        acc[2] += (double)pt.aoff;
        acc[3] += (double)pt.cl1;
      }
      float gr[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) gr[k] = grad_elem(p, pt, e[k] * pt.inv, li * 8 + k == t, cv[k]);
      *reinterpret_cast<u32x4_t*>(dl + pix * NB + li * 8) = Chunk<uint16_t>::pack(gr);
    }
  }
  block_partials(acc, p.partial + (int64_t)blockIdx.x * kSums);
}

// every other (dtype, nb, ld): one wave per pixel, lane l holds bins l, l + 64, ... (nb <= 512), row stride ld >= nb
template <typename T>
__global__ __launch_bounds__(256) void hybrid_loss_kernel(HybridP p) {
  constexpr int U = kMaxNb / 64;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const T* lg = reinterpret_cast<const T*>(p.logits);
  T* dl = reinterpret_cast<T*>(p.dlogits);
  const int nb = p.nb;
  float cv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) cv[u] = (lane + 64 * u) < nb ? p.centers[lane + 64 * u] : 0.f;
  double acc[kSums] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t pix = (int64_t)blockIdx.x * 4 + wave; pix < p.pixels; pix += (int64_t)gridDim.x * 4) {
    const T* row = lg + pix * p.ld;
    float d[U], mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = lane + 64 * u;
      d[u] = k < nb ? ElemTraits<T>::load(row + k) : -INFINITY;
      mx = fmaxf(mx, d[u]);
    }
    const int t = p.bins[pix];
    const float c = p.coarse[pix], o = p.offset[pix], gtv = p.gt[pix];
    mx = wave_max(mx);
    float e[U];
    float se = 0.f, sd = 0.f, A = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = lane + 64 * u;
      e[u] = 0.f;
      if (k < nb) {
        d[u] -= mx;
        e[u] = __expf(d[u]);
        se += e[u];
        sd += d[u];
        A += k == t ? d[u] : 0.f;
      }
    }
    se = wave_sum(se);
    sd = wave_sum(sd);
    A = wave_sum(A);
    const PixTerms pt = pixel_terms(p, se, sd, A, c, o, gtv);
    if (lane == 0) {
      p.final_[pix] = pt.final_;
      p.doffset[pix] = pt.doff;
      acc[0] += (double)pt.ce;
      acc[1] += (double)pt.reg;
      acc[2] += (double)pt.aoff;
      acc[3] += (double)pt.cl1;
    }
    T* drow = dl + pix * p.ld;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = lane + 64 * u;
      if (k < nb) ElemTraits<T>::store(drow + k, grad_elem(p, pt, e[u] * pt.inv, k == t, cv[u]));
    }
    for (int k = nb + lane; k < p.ld; k += 64) ElemTraits<T>::store(drow + k, 0.f);      // the tape's padding columns
  }
  block_partials(acc, p.partial + (int64_t)blockIdx.x * kSums);
}

// one block: partial [rows][4] -> sums[4] (skipped when partial is NULL: the sums were all-reduced by the caller), then
// terms = (ce, regression, offset_reg, coarse_l1, total)
__global__ __launch_bounds__(256) void hybrid_finish_kernel(const double* partial, int rows, double* sums, double pixels_global,
                                                            float ce_weight, float reg_weight, float off_weight, float* terms) {
  __shared__ double sm[kSums][4];
  if (partial) {
    double a[kSums] = {0.0, 0.0, 0.0, 0.0};
    for (int r = threadIdx.x; r < rows; r += 256)
      for (int k = 0; k < kSums; ++k) a[k] += partial[(int64_t)r * kSums + k];
    for (int k = 0; k < kSums; ++k) {
      a[k] = wave_sum_d(a[k]);
      if ((threadIdx.x & 63) == 0) sm[k][threadIdx.x >> 6] = a[k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double s[kSums];
    for (int k = 0; k < kSums; ++k) {
      if (partial) {
        s[k] = sm[k][0] + sm[k][1] + sm[k][2] + sm[k][3];
        sums[k] = s[k];
      } else {
        s[k] = sums[k];
      }
    }
    if (terms) {
      const float ce = (float)(s[0] / pixels_global), reg = (float)(s[1] / pixels_global);
      const float off = (float)(s[2] / pixels_global);
      terms[0] = ce;
      terms[1] = reg;
      terms[2] = off;
      terms[3] = (float)(s[3] / pixels_global);
      terms[4] = ce_weight * ce + reg_weight * reg + off_weight * off;
    }
  }
}

inline int loss_blocks(int64_t pixels) {      // coarse.hip's grid: 16 pixels per block of the wave-per-pixel form
  int64_t b = adn_cdiv(pixels, 16);
  if (b > kMaxBlocks) b = kMaxBlocks;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

extern "C" int64_t adn_hybrid_loss_workspace_bytes(int64_t pixels) {
  if (pixels <= 0) return -1;
  return (int64_t)loss_blocks(pixels) * kSums * 8;
}

extern "C" int adn_hybrid_loss(const AdnHybridLoss* d, void* stream) {
  ADN_CHECK_ARG(d && d->logits && d->centers && d->coarse && d->offset && d->bins && d->gt && d->final_depth && d->dlogits &&
                    d->doffset && d->workspace && d->pixels > 0,
                "adn_hybrid_loss: null operand or no pixels");
  ADN_CHECK_ARG(d->dtype == ADN_F32 || d->dtype == ADN_BF16, "adn_hybrid_loss: bad dtype %d", d->dtype);
  ADN_CHECK_ARG(d->nb >= 2 && d->nb <= kMaxNb, "adn_hybrid_loss: n_bins %d outside the supported range [2, %d]", d->nb, kMaxNb);
  ADN_CHECK_ARG(d->ld >= d->nb, "adn_hybrid_loss: row stride %d < n_bins %d", d->ld, d->nb);
  ADN_CHECK_ARG(d->workspace_bytes >= adn_hybrid_loss_workspace_bytes(d->pixels),
                "adn_hybrid_loss: the workspace is smaller than adn_hybrid_loss_workspace_bytes()");
  ADN_CHECK_ARG(d->reg_mode == 0 || d->reg_mode == 1, "adn_hybrid_loss: reg_mode %d (0 L1, 1 L2)", d->reg_mode);
  ADN_CHECK_ARG(d->label_smoothing >= 0.f && d->label_smoothing <= 1.f, "adn_hybrid_loss: label_smoothing %g outside [0, 1]",
                (double)d->label_smoothing);
  ADN_CHECK_ARG(d->pixels_global >= d->pixels, "adn_hybrid_loss: global pixel count %lld < local %lld",
                (long long)d->pixels_global, (long long)d->pixels);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HybridP p;
  p.logits = d->logits; p.centers = d->centers; p.coarse = d->coarse; p.offset = d->offset; p.bins = d->bins; p.gt = d->gt;
  p.final_ = d->final_depth; p.dlogits = d->dlogits; p.doffset = d->doffset;
  p.partial = reinterpret_cast<double*>(d->workspace);
  p.pixels = d->pixels; p.nb = d->nb; p.ld = d->ld; p.reg_mode = d->reg_mode;
  const double P = (double)d->pixels_global;
  p.ce_coef = (float)((double)d->ce_weight / P);
  p.reg_coef = (float)((double)d->reg_weight / P);
  p.off_coef = (float)((double)d->offset_reg_weight / P);
  p.eps = d->label_smoothing;
  p.keep = 1.f - d->label_smoothing;
  p.inv_nb = 1.f / (float)d->nb;
  p.smooth = d->label_smoothing / (float)d->nb;
  const dim3 grid(loss_blocks(d->pixels));
  const int lpp = d->nb / 8;
  const bool vec = d->dtype == ADN_BF16 && d->ld == d->nb && d->nb % 8 == 0 && (lpp & (lpp - 1)) == 0 &&
                   (reinterpret_cast<uintptr_t>(d->logits) & 15) == 0 && (reinterpret_cast<uintptr_t>(d->dlogits) & 15) == 0;
  if (vec) {
    switch (lpp) {
#define ADN_HYBRID_VEC(L) case L: hipLaunchKernelGGL((hybrid_loss_vec_kernel<L>), grid, dim3(256), 0, st, p); break;
      ADN_HYBRID_VEC(1) ADN_HYBRID_VEC(2) ADN_HYBRID_VEC(4) ADN_HYBRID_VEC(8) ADN_HYBRID_VEC(16) ADN_HYBRID_VEC(32) ADN_HYBRID_VEC(64)
#undef ADN_HYBRID_VEC
    }
  } else if (d->dtype == ADN_BF16) {
    hipLaunchKernelGGL((hybrid_loss_kernel<uint16_t>), grid, dim3(256), 0, st, p);
  } else {
    hipLaunchKernelGGL((hybrid_loss_kernel<float>), grid, dim3(256), 0, st, p);
  }
  ADN_CHECK_LAUNCH();
  return ADN_OK;
}

extern "C" int adn_hybrid_loss_finish(const void* workspace, int64_t pixels, double* sums, int64_t pixels_global,
                                      float ce_weight, float reg_weight, float offset_reg_weight, float* terms, void* stream) {
  ADN_CHECK_ARG(sums && pixels > 0, "adn_hybrid_loss_finish: bad arguments");
  ADN_CHECK_ARG(!terms || pixels_global >= pixels, "adn_hybrid_loss_finish: global pixel count %lld < local %lld",
                (long long)pixels_global, (long long)pixels);
  hipLaunchKernelGGL(hybrid_finish_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const double*>(workspace), loss_blocks(pixels), sums, (double)pixels_global, ce_weight,
                     reg_weight, offset_reg_weight, terms);
  ADN_CHECK_LAUNCH();
  return ADN_OK;
}
