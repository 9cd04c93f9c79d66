// Coarse-depth classification family (coarse_depth_model.py:324-468, train_coarse_depth.py:446-463): the loss head behind
// the 1x1 class conv.  Memory-bound; conventions of adabins.hip: f32 arithmetic, f64 final reductions, no atomics,
// bit-reproducible run to run (fixed grid per pixel count, fixed reduction order).
//   coarse_targets   depth -> bin index (torch.bucketize(depth, interior edges), right=False) and the valid-pixel count
//   coarse_loss      ONE pass over the logits: softmax expectation (depth), optional argmax, classification loss
//                    (soft CE / focal / plain CE) + masked L1 of the expectation, and the gradient of their weighted sum
//   coarse_finish    per-block f64 partials -> sums -> (ce, regression, total)
#include "loss_tail.h"

namespace {

constexpr int kTargetBlocks = 1024;

struct CoarseP {
  const void* logits; const float* centers; const int32_t* bins; const float* gt; const double* n_valid;
  float* depth; int32_t* argmax; void* dlogits; double* partial;
  int64_t pixels;
  int nb, ld, ce_mode;
  float inv_2s2, gamma, ce_coef, reg_weight;      // 1 / (2 sigma^2);  ce_coef = ce_weight / global pixel count
};

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
    t.r = p.reg_weight * adn_sgn(d) * inv_nv;
  }
  return t;
}

__device__ __forceinline__ float grad_elem(const CoarseP& p, const PixTerms& t, float pk, float gk, bool is_t, float ck) {
  const float ce = p.ce_mode == 0 ? pk * t.Y - gk * t.ys : t.w * (pk - (is_t ? 1.f : 0.f));
  return p.ce_coef * ce + t.r * pk * (ck - t.depth);
}

// one body over either layout of loss_tail.h (VecRow<LPP>: bins_fwd_vec_kernel's layout; WaveRow<T>)
template <typename Row>
__global__ __launch_bounds__(256) void coarse_loss_kernel(CoarseP p) {
  constexpr int U = Row::U;
  const Row row(p.nb, p.ld);
  const bool have_loss = p.bins != nullptr;
  float cv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) cv[u] = row.has(u) ? p.centers[row.bin(u)] : 0.f;
  float inv_nv = 0.f;
  if (have_loss) {
    const double nv = p.n_valid[0];
    inv_nv = nv > 0.0 ? (float)(1.0 / nv) : 0.f;
  }
  double acc[2] = {0.0, 0.0};                         // ce, l1
  for (int64_t p0 = row.first(); p0 < p.pixels; p0 += row.stride()) {
    const int64_t pix = row.pixel(p0);
    const bool live = row.live(pix, p.pixels);
    float d[U];
    const float mx = row.group_max(row.load(p.logits, pix, live, d));
    if (p.argmax) {                                   // first maximum, as torch.argmax picks it
      int cand = 0x7fffffff;
#pragma unroll
      for (int u = U - 1; u >= 0; --u)
        if (row.has(u) && d[u] == mx) cand = row.bin(u);
      cand = row.group_min(cand);
      if (live && row.leader()) p.argmax[pix] = cand;
    }
    const int t = (live && have_loss) ? p.bins[pix] : 0;
    float e[U], g[U];
    float se = 0.f, sc = 0.f, S = 0.f, A = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      e[u] = g[u] = 0.f;
      if (!row.has(u)) continue;
      d[u] -= mx;
      e[u] = __expf(d[u]);
      se += e[u];
      sc += e[u] * cv[u];
      const int k = row.bin(u);
      if (!have_loss) continue;                       // forward only: no labels, S and A stay 0 (wave-uniform)
      if (p.ce_mode == 0) {
        const float dk = (float)(k - t);
        g[u] = __expf(-dk * dk * p.inv_2s2);
        S += g[u];
        A += g[u] * d[u];
      } else {
        A += k == t ? d[u] : 0.f;
      }
    }
    se = row.group_sum(se);
    sc = row.group_sum(sc);
    S = row.group_sum(S);
    A = row.group_sum(A);
    const float gtv = (live && have_loss) ? p.gt[pix] : 0.f;
    const PixTerms pt = pixel_terms(p, se, sc, S, A, have_loss, gtv, inv_nv);
    if (live && row.leader()) {
      p.depth[pix] = pt.depth;
      acc[0] += (double)pt.loss;
      acc[1] += (double)pt.l1;
    }
    if (p.dlogits && live) {
      float gr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) gr[u] = row.has(u) ? grad_elem(p, pt, e[u] * pt.inv, g[u], row.bin(u) == t, cv[u]) : 0.f;
      row.store(p.dlogits, pix, gr);
    }
  }
  if (have_loss) block_partial_row(acc, p.partial + (int64_t)blockIdx.x * 2);
}

// one block: partial [rows][2] -> sums[2] (skipped when partial is NULL: the sums were all-reduced by the caller), then
// terms = (ce, regression, total); regression is NaN without a valid pixel (the reference's mean over an empty selection)
__global__ __launch_bounds__(256) void coarse_finish_kernel(const double* partial, int rows, double* sums, const double* n_valid,
                                                            double pixels_global, float ce_weight, float reg_weight,
                                                            float* terms) {
  sum_partial_rows<2>(partial, rows, sums, [&](const double (&s)[2]) {
    if (!terms) return;
    const double nv = n_valid[0];
    const float ce = (float)(s[0] / pixels_global);
    const float reg = nv > 0.0 ? (float)(s[1] / nv) : NAN;
    terms[0] = ce;
    terms[1] = reg;
    terms[2] = ce_weight * ce + reg_weight * reg;
  });
}

// bins[e] = number of interior edges strictly below depth[e] (bucketize, right=False; already inside [0, nb - 1]);
// partial[block] = count of depth > 0
__global__ __launch_bounds__(256) void coarse_targets_kernel(const float* depth, int64_t n, const float* edges, int ne,
                                                             int32_t* bins, double* partial) {
  __shared__ float es[kMaxNb];
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
  double c[1] = {(double)cnt};
  block_partial_row(c, partial + blockIdx.x);
}

__global__ __launch_bounds__(64) void coarse_count_kernel(const double* partial, int rows, double* stats) {
  double s[1];
  sum_partial_rows_wave(partial, rows, s);
  if (threadIdx.x == 0) stats[0] = s[0];
}

inline int loss_blocks(int64_t pixels) { return adn_grid_blocks(pixels, 16, kLossBlocks); }      // both layouts
inline int target_blocks(int64_t n) { return adn_grid_blocks(n, 1024, kTargetBlocks); }

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
  ADN_CHECK_DTYPE("adn_coarse_loss", d->dtype);
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
  const int rc = launch_bin_rows("adn_coarse_loss", d->dtype, d->nb, d->ld, d->logits, d->dlogits, [&](auto row) {
    hipLaunchKernelGGL((coarse_loss_kernel<typename decltype(row)::type>), grid, dim3(256), 0, st, p);
  });
  if (rc != ADN_OK) return rc;
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
