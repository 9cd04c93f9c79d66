// Coarse-depth classification family (coarse_depth_model.py:324-468, train_coarse_depth.py:446-463): the loss head behind
// the 1x1 class conv.  Memory-bound; conventions of adabins.hip: f32 arithmetic, f64 final reductions, no atomics,
// bit-reproducible run to run (fixed grid per pixel count, fixed reduction order).
//   coarse_targets   depth -> bin index (torch.bucketize(depth, interior edges), right=False) and the valid-pixel count
//   coarse_loss      ONE pass over the logits: softmax expectation (depth), optional argmax, classification loss
//                    (soft CE / focal / plain CE) + masked L1 of the expectation, and the gradient of their weighted sum
//   coarse_finish    per-block f64 partials -> sums -> (ce, regression, total)
#include "adn_common.h"

namespace {

constexpr int kMaxNb = 512;          // 8 x 64 lanes of one wave (generic kernel) / 64 lanes x one 16-byte chunk (vector kernel)
constexpr int kMaxBlocks = 2048;
constexpr int kTargetBlocks = 1024;

struct CoarseP {
  const void* logits; const float* centers; const int32_t* bins; const float* gt; const double* n_valid;
  float* depth; int32_t* argmax; void* dlogits; double* partial;
  int64_t pixels;
  int nb, ld, ce_mode;
  float inv_2s2, gamma, ce_coef, reg_weight;      // 1 / (2 sigma^2);  ce_coef = ce_weight / global pixel count
};

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// What one pixel contributes once its reductions are known.  se = sum exp(x - max), sc = sum exp(x - max) c,
// S = sum of the unnormalised soft labels g_k, A = sum g_k (x_k - max)  (modes 1, 2: A = x_t - max).
struct PixTerms {
  float inv, depth, ys, Y, w, r, loss, l1;
};
__device__ __forceinline__ PixTerms pixel_terms(const CoarseP& p, float se, float sc, float S, float A, bool have_loss,
                                                float gtv, float inv_nv) {
  PixTerms t;
  t.inv = 1.f / se;
  t.depth = sc * t.inv;
  t.ys = t.Y = t.loss = t.l1 = t.r = 0.f;
  t.w = 1.f;
  if (!have_loss) return t;
  const float logz = __logf(se);
  if (p.ce_mode == 0) {
    // labels y_k = g_k / (S + 1e-8): their sum Y is not exactly 1 and stays in the gradient (p_j Y - y_j)
    t.ys = 1.f / (S + 1e-8f);
    t.Y = S * t.ys;
    t.loss = logz * t.Y - A * t.ys;
  } else {
    const float ce = logz - A;                       // -log p_t >= 0
    if (p.ce_mode == 1) {                            // focal: (1 - pt)^gamma ce, pt = exp(-ce)
      const float pt = __expf(-ce), om = 1.f - pt;
      const float f = powf(om, p.gamma);
      t.loss = f * ce;
      t.w = f + p.gamma * powf(om, p.gamma - 1.f) * pt * ce;      // d loss / d ce
    } else {
      t.loss = ce;
    }
  }
  if (gtv > 0.f) {
    const float d = t.depth - gtv;
    t.l1 = fabsf(d);
    t.r = p.reg_weight * sgn(d) * inv_nv;
  }
  return t;
}

__device__ __forceinline__ float grad_elem(const CoarseP& p, const PixTerms& t, float pk, float gk, bool is_t, float ck) {
  const float ce = p.ce_mode == 0 ? pk * t.Y - gk * t.ys : t.w * (pk - (is_t ? 1.f : 0.f));
  return p.ce_coef * ce + t.r * pk * (ck - t.depth);
}

__device__ __forceinline__ void block_partials(double a, double b, double* out) {      // 256 threads
  __shared__ double sm[2][4];
  a = wave_sum_d(a);
  b = wave_sum_d(b);
  if ((threadIdx.x & 63) == 0) {
    sm[0][threadIdx.x >> 6] = a;
    sm[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x < 2) out[threadIdx.x] = sm[threadIdx.x][0] + sm[threadIdx.x][1] + sm[threadIdx.x][2] + sm[threadIdx.x][3];
}

// bf16, ld == nb = 8 LPP, LPP a power of two <= 64 (bins_fwd_vec_kernel's layout): a pixel's bins are LPP lanes x one 16-byte
// load each, 64 / LPP pixels per wave-iteration, reductions across those lanes only; the gradient leaves as one 16-byte store
template <int LPP>
__global__ __launch_bounds__(256) void coarse_loss_vec_kernel(CoarseP p) {
  constexpr int NB = LPP * 8, PPW = 64 / LPP;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int li = lane % LPP, pw = lane / LPP;
  const uint16_t* lg = reinterpret_cast<const uint16_t*>(p.logits);
  uint16_t* dl = reinterpret_cast<uint16_t*>(p.dlogits);
  const bool have_loss = p.bins != nullptr;
  float cv[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) cv[k] = p.centers[li * 8 + k];
  float inv_nv = 0.f;
  if (have_loss) {
    const double nv = p.n_valid[0];
    inv_nv = nv > 0.0 ? (float)(1.0 / nv) : 0.f;
  }
  double acc_ce = 0.0, acc_l1 = 0.0;
  for (int64_t p0 = ((int64_t)blockIdx.x * 4 + wave) * PPW; p0 < p.pixels; p0 += (int64_t)gridDim.x * 4 * PPW) {
    const int64_t pix = p0 + pw;
    const bool live = pix < p.pixels;
    float d[8];
    float mx = -INFINITY;
    if (live) {
      const u32x4_t c = *reinterpret_cast<const u32x4_t*>(lg + pix * NB + li * 8);
      Chunk<uint16_t>::unpack(c, d);
#pragma unroll
      for (int k = 0; k < 8; ++k) mx = fmaxf(mx, d[k]);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) d[k] = 0.f;
      mx = 0.f;
    }
#pragma unroll
    for (int o = 1; o < LPP; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (p.argmax) {                                   // first maximum, as torch.argmax picks it
      int cand = 0x7fffffff;
#pragma unroll
      for (int k = 7; k >= 0; --k)
        if (d[k] == mx) cand = li * 8 + k;
#pragma unroll
      for (int o = 1; o < LPP; o <<= 1) cand = min(cand, __shfl_xor(cand, o, 64));
      if (live && li == 0) p.argmax[pix] = cand;
    }
    const int t = (live && have_loss) ? p.bins[pix] : 0;
    float e[8], g[8];
    float se = 0.f, sc = 0.f, S = 0.f, A = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      d[k] -= mx;
      e[k] = __expf(d[k]);
      se += e[k];
      sc += e[k] * cv[k];
      const int kk = li * 8 + k;
      g[k] = 0.f;
      if (!have_loss) continue;                       // forward only: no labels, S and A stay 0 (wave-uniform)
      if (p.ce_mode == 0) {
        const float dk = (float)(kk - t);
        g[k] = __expf(-dk * dk * p.inv_2s2);
        S += g[k];
        A += g[k] * d[k];
      } else {
        A += kk == t ? d[k] : 0.f;
      }
    }
#pragma unroll
    for (int o = 1; o < LPP; o <<= 1) {
      se += __shfl_xor(se, o, 64);
      sc += __shfl_xor(sc, o, 64);
      S += __shfl_xor(S, o, 64);
      A += __shfl_xor(A, o, 64);
    }
    const float gtv = (live && have_loss) ? p.gt[pix] : 0.f;
    const PixTerms pt = pixel_terms(p, se, sc, S, A, have_loss, gtv, inv_nv);
    if (live && li == 0) {
      p.depth[pix] = pt.depth;
      acc_ce += (double)pt.loss;
      acc_l1 += (double)pt.l1;
    }
    if (dl && live) {
      float gr[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) gr[k] = grad_elem(p, pt, e[k] * pt.inv, g[k], li * 8 + k == t, cv[k]);
      *reinterpret_cast<u32x4_t*>(dl + pix * NB + li * 8) = Chunk<uint16_t>::pack(gr);
    }
  }
  if (have_loss) block_partials(acc_ce, acc_l1, p.partial + (int64_t)blockIdx.x * 2);
}

// every other (dtype, nb, ld): one wave per pixel, lane l holds bins l, l + 64, ... (nb <= 512), row stride ld >= nb
template <typename T>
__global__ __launch_bounds__(256) void coarse_loss_kernel(CoarseP p) {
  constexpr int U = kMaxNb / 64;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const T* lg = reinterpret_cast<const T*>(p.logits);
  T* dl = reinterpret_cast<T*>(p.dlogits);
  const bool have_loss = p.bins != nullptr;
  const int nb = p.nb;
  float cv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) cv[u] = (lane + 64 * u) < nb ? p.centers[lane + 64 * u] : 0.f;
  float inv_nv = 0.f;
  if (have_loss) {
    const double nv = p.n_valid[0];
    inv_nv = nv > 0.0 ? (float)(1.0 / nv) : 0.f;
  }
  double acc_ce = 0.0, acc_l1 = 0.0;
  for (int64_t pix = (int64_t)blockIdx.x * 4 + wave; pix < p.pixels; pix += (int64_t)gridDim.x * 4) {
    const T* row = lg + pix * p.ld;
    float d[U], mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = lane + 64 * u;
      d[u] = k < nb ? ElemTraits<T>::load(row + k) : -INFINITY;
      mx = fmaxf(mx, d[u]);
    }
    mx = wave_max(mx);
    if (p.argmax) {
      int cand = 0x7fffffff;
#pragma unroll
      for (int u = U - 1; u >= 0; --u)
        if ((lane + 64 * u) < nb && d[u] == mx) cand = lane + 64 * u;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
      if (lane == 0) p.argmax[pix] = cand;
    }
    const int t = have_loss ? p.bins[pix] : 0;
    float e[U], g[U];
    float se = 0.f, sc = 0.f, S = 0.f, A = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = lane + 64 * u;
      e[u] = g[u] = 0.f;
      if (k < nb) {
        d[u] -= mx;
        e[u] = __expf(d[u]);
        se += e[u];
        sc += e[u] * cv[u];
        if (!have_loss) continue;
        if (p.ce_mode == 0) {
          const float dk = (float)(k - t);
          g[u] = __expf(-dk * dk * p.inv_2s2);
          S += g[u];
          A += g[u] * d[u];
        } else {
          A += k == t ? d[u] : 0.f;
        }
      }
    }
    se = wave_sum(se);
    sc = wave_sum(sc);
    S = wave_sum(S);
    A = wave_sum(A);
    const float gtv = have_loss ? p.gt[pix] : 0.f;
    const PixTerms pt = pixel_terms(p, se, sc, S, A, have_loss, gtv, inv_nv);
    if (lane == 0) {
      p.depth[pix] = pt.depth;
      acc_ce += (double)pt.loss;
      acc_l1 += (double)pt.l1;
    }
    if (dl) {
      T* drow = dl + pix * p.ld;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = lane + 64 * u;
        if (k < nb) ElemTraits<T>::store(drow + k, grad_elem(p, pt, e[u] * pt.inv, g[u], k == t, cv[u]));
      }
      for (int k = nb + lane; k < p.ld; k += 64) ElemTraits<T>::store(drow + k, 0.f);      // the tape's padding columns
    }
  }
  if (have_loss) block_partials(acc_ce, acc_l1, p.partial + (int64_t)blockIdx.x * 2);
}

// one block: partial [rows][2] -> sums[2] (skipped when partial is NULL: the sums were all-reduced by the caller), then
// terms = (ce, regression, total); regression is NaN without a valid pixel (the reference's mean over an empty selection)
__global__ __launch_bounds__(256) void coarse_finish_kernel(const double* partial, int rows, double* sums, const double* n_valid,
                                                            double pixels_global, float ce_weight, float reg_weight,
                                                            float* terms) {
  __shared__ double sm[2][4];
  if (partial) {
    double a = 0.0, b = 0.0;
    for (int r = threadIdx.x; r < rows; r += 256) {
      a += partial[(int64_t)r * 2];
      b += partial[(int64_t)r * 2 + 1];
    }
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    if ((threadIdx.x & 63) == 0) {
      sm[0][threadIdx.x >> 6] = a;
      sm[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double s0, s1;
    if (partial) {
      s0 = sm[0][0] + sm[0][1] + sm[0][2] + sm[0][3];
      s1 = sm[1][0] + sm[1][1] + sm[1][2] + sm[1][3];
      sums[0] = s0;
      sums[1] = s1;
    } else {
      s0 = sums[0];
      s1 = sums[1];
    }
    if (terms) {
      const double nv = n_valid[0];
      const float ce = (float)(s0 / pixels_global);
      const float reg = nv > 0.0 ? (float)(s1 / nv) : NAN;
      terms[0] = ce;
      terms[1] = reg;
      terms[2] = ce_weight * ce + reg_weight * reg;
    }
  }
}

// bins[e] = number of interior edges strictly below depth[e] (bucketize, right=False; already inside [0, nb - 1]);
// partial[block] = count of depth > 0
__global__ __launch_bounds__(256) void coarse_targets_kernel(const float* depth, int64_t n, const float* edges, int ne,
                                                             int32_t* bins, double* partial) {
  __shared__ float es[kMaxNb];
  __shared__ double sm[4];
  if (bins)
    for (int i = threadIdx.x; i < ne; i += 256) es[i] = edges[i];
  __syncthreads();
  int64_t cnt = 0;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const float v = depth[e];
    cnt += v > 0.f ? 1 : 0;
    if (bins) {
      int lo = 0, hi = ne;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (!(es[mid] >= v)) lo = mid + 1;          // e < v, and NaN sorts behind every edge as in torch
        else hi = mid;
      }
      bins[e] = lo;
    }
  }
  const double c = wave_sum_d((double)cnt);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
}

__global__ __launch_bounds__(64) void coarse_count_kernel(const double* partial, int rows, double* stats) {
  double s = 0.0;
  for (int r = threadIdx.x; r < rows; r += 64) s += partial[r];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) stats[0] = s;
}

inline int loss_blocks(int64_t pixels) {
  int64_t b = adn_cdiv(pixels, 16);
  if (b > kMaxBlocks) b = kMaxBlocks;
  if (b < 1) b = 1;
  return (int)b;
}
inline int target_blocks(int64_t n) {
  int64_t b = adn_cdiv(n, 1024);
  if (b > kTargetBlocks) b = kTargetBlocks;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

extern "C" int64_t adn_coarse_targets_workspace_bytes(int64_t n) {
  if (n <= 0) return -1;
  return (int64_t)target_blocks(n) * 8;
}

extern "C" int adn_coarse_targets(const float* depth, int64_t n, const float* edges, int32_t nb, int32_t* bins,
                                  double* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  ADN_CHECK_ARG(depth && stats && n > 0, "adn_coarse_targets: bad arguments");
  ADN_CHECK_ARG(!bins || (edges && nb >= 2 && nb <= kMaxNb), "adn_coarse_targets: binning needs the %d interior edges, 2 <= nb <= %d (nb = %d)",
                nb - 1, kMaxNb, nb);
  ADN_CHECK_ARG(workspace && workspace_bytes >= adn_coarse_targets_workspace_bytes(n), "adn_coarse_targets: workspace too small");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nbk = target_blocks(n);
  double* part = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(coarse_targets_kernel, dim3(nbk), dim3(256), 0, st, depth, n, edges, bins ? nb - 1 : 0, bins, part);
  ADN_CHECK_LAUNCH();
  hipLaunchKernelGGL(coarse_count_kernel, dim3(1), dim3(64), 0, st, part, nbk, stats);
  ADN_CHECK_LAUNCH();
  return ADN_OK;
}

extern "C" int64_t adn_coarse_loss_workspace_bytes(int64_t pixels) {
  if (pixels <= 0) return -1;
  return (int64_t)loss_blocks(pixels) * 2 * 8;
}

extern "C" int adn_coarse_loss(const AdnCoarseLoss* d, void* stream) {
  ADN_CHECK_ARG(d && d->logits && d->centers && d->depth && d->pixels > 0, "adn_coarse_loss: null operand or no pixels");
  ADN_CHECK_ARG(d->dtype == ADN_F32 || d->dtype == ADN_BF16, "adn_coarse_loss: bad dtype %d", d->dtype);
  ADN_CHECK_ARG(d->nb >= 2 && d->nb <= kMaxNb, "adn_coarse_loss: n_bins %d outside the supported range [2, %d]", d->nb, kMaxNb);
  ADN_CHECK_ARG(d->ld >= d->nb, "adn_coarse_loss: row stride %d < n_bins %d", d->ld, d->nb);
  ADN_CHECK_ARG(!d->dlogits || d->bins, "adn_coarse_loss: a gradient needs the target bins");
  ADN_CHECK_ARG(!d->bins || (d->gt && d->n_valid && d->workspace && d->workspace_bytes >= adn_coarse_loss_workspace_bytes(d->pixels)),
                "adn_coarse_loss: the loss needs gt, n_valid and a workspace of adn_coarse_loss_workspace_bytes()");
  ADN_CHECK_ARG(d->ce_mode >= 0 && d->ce_mode <= 2, "adn_coarse_loss: ce_mode %d (0 soft, 1 focal, 2 plain)", d->ce_mode);
  ADN_CHECK_ARG(!d->bins || d->ce_mode != 0 || d->sigma > 0.f, "adn_coarse_loss: soft cross-entropy needs sigma > 0");
  ADN_CHECK_ARG(!d->bins || d->pixels_global >= d->pixels, "adn_coarse_loss: global pixel count %lld < local %lld",
                (long long)d->pixels_global, (long long)d->pixels);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  CoarseP p;
  p.logits = d->logits; p.centers = d->centers; p.bins = d->bins; p.gt = d->gt; p.n_valid = d->n_valid;
  p.depth = d->depth; p.argmax = d->argmax; p.dlogits = d->dlogits; p.partial = reinterpret_cast<double*>(d->workspace);
  p.pixels = d->pixels; p.nb = d->nb; p.ld = d->ld; p.ce_mode = d->ce_mode;
  p.inv_2s2 = d->sigma > 0.f ? 0.5f / (d->sigma * d->sigma) : 0.f;
  p.gamma = d->gamma;
  p.ce_coef = d->bins ? (float)((double)d->ce_weight / (double)d->pixels_global) : 0.f;
  p.reg_weight = d->reg_weight;
  const dim3 grid(loss_blocks(d->pixels));
  const int lpp = d->nb / 8;
  const bool vec = d->dtype == ADN_BF16 && d->ld == d->nb && d->nb % 8 == 0 && (lpp & (lpp - 1)) == 0 &&
                   (reinterpret_cast<uintptr_t>(d->logits) & 15) == 0 && (reinterpret_cast<uintptr_t>(d->dlogits) & 15) == 0;
  if (vec) {
    switch (lpp) {
#define ADN_COARSE_VEC(L) case L: hipLaunchKernelGGL((coarse_loss_vec_kernel<L>), grid, dim3(256), 0, st, p); break;
      ADN_COARSE_VEC(1) ADN_COARSE_VEC(2) ADN_COARSE_VEC(4) ADN_COARSE_VEC(8) ADN_COARSE_VEC(16) ADN_COARSE_VEC(32) ADN_COARSE_VEC(64)
#undef ADN_COARSE_VEC
    }
  } else if (d->dtype == ADN_BF16) {
    hipLaunchKernelGGL((coarse_loss_kernel<uint16_t>), grid, dim3(256), 0, st, p);
  } else {
    hipLaunchKernelGGL((coarse_loss_kernel<float>), grid, dim3(256), 0, st, p);
  }
  ADN_CHECK_LAUNCH();
  return ADN_OK;
}

extern "C" int adn_coarse_loss_finish(const void* workspace, int64_t pixels, double* sums, const double* n_valid,
                                      int64_t pixels_global, float ce_weight, float reg_weight, float* terms, void* stream) {
  ADN_CHECK_ARG(sums && pixels > 0, "adn_coarse_loss_finish: bad arguments");
  ADN_CHECK_ARG(!terms || (n_valid && pixels_global >= pixels), "adn_coarse_loss_finish: the terms need n_valid and the global pixel count");
  hipLaunchKernelGGL(coarse_finish_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const double*>(workspace), loss_blocks(pixels), sums, n_valid, (double)pixels_global,
                     ce_weight, reg_weight, terms);
  ADN_CHECK_LAUNCH();
  return ADN_OK;
}
