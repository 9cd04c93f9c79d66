// Hybrid coarse-depth family (CoarseWithOffsetModel / CoarseOffsetLoss, coarse_depth_model.py:591-850,
// train_coarse_depth.py:336-343): the loss tail behind the class head and the offset head.  Memory-bound; conventions of
// coarse.hip / dualreg.hip: f32 arithmetic, f64 final reductions, no atomics, bit-reproducible run to run (fixed grid per
// pixel count, fixed reduction order).
//   hybrid_loss      ONE pass over the logits: final = coarse + offset, label-smoothed cross-entropy, L1 / L2 of final,
//                    |offset|, the monitoring |coarse - gt|, and the gradients towards the logits and the offset plane.
//                    The coarse depth is an INPUT (what the forward-only adn_coarse_loss pass wrote before the offset
//                    branch ran), so the softmax expectation is not accumulated again.  No valid mask anywhere.
//   hybrid_finish    per-block f64 partials -> sums -> (ce, regression, offset_reg, coarse_l1, total)
#include "loss_tail.h"

namespace {

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
    t.r = p.reg_coef * adn_sgn(e);
  } else {
    t.reg = e * e;
    t.r = p.reg_coef * 2.f * e;
  }
  t.aoff = fabsf(o);
  t.cl1 = fabsf(c - gtv);
  t.doff = t.r + p.off_coef * adn_sgn(o);
  return t;
}

__device__ __forceinline__ float grad_elem(const HybridP& p, const PixTerms& t, float pk, bool is_t, float ck) {
  return p.ce_coef * (pk - (is_t ? p.keep : 0.f) - p.smooth) + t.r * pk * (ck - t.coarse);
}

// one body over either layout of loss_tail.h (VecRow<LPP>, WaveRow<T>): the walk of coarse_loss_kernel
template <typename Row>
__global__ __launch_bounds__(256) void hybrid_loss_kernel(HybridP p) {
  constexpr int U = Row::U;
  const Row row(p.nb, p.ld);
  float cv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) cv[u] = row.has(u) ? p.centers[row.bin(u)] : 0.f;
  double acc[kSums] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t p0 = row.first(); p0 < p.pixels; p0 += row.stride()) {
    const int64_t pix = row.pixel(p0);
    const bool live = row.live(pix, p.pixels);
    int t = 0;
    float c = 0.f, o = 0.f, gtv = 0.f;
    if (live) {                                        // issued ahead of the row, so that all five loads are in flight at once
      t = p.bins[pix];
      c = p.coarse[pix];
      o = p.offset[pix];
      gtv = p.gt[pix];
    }
    float d[U];
    const float mx = row.group_max(row.load(p.logits, pix, live, d));
    float e[U];
    float se = 0.f, sd = 0.f, A = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      e[u] = 0.f;
      if (!row.has(u)) continue;
      d[u] -= mx;
      e[u] = __expf(d[u]);
      se += e[u];
      sd += d[u];
      A += row.bin(u) == t ? d[u] : 0.f;
    }
    row.group_sums(se, sd, A);
    if (live) {                                        // the reductions above need every lane; what follows does not
      const PixTerms pt = pixel_terms(p, se, sd, A, c, o, gtv);
      if (row.leader()) {
        p.final_[pix] = pt.final_;
        p.doffset[pix] = pt.doff;
        acc[0] += (double)pt.ce;
        acc[1] += (double)pt.reg;
        acc[2] += (double)pt.aoff;
        acc[3] += (double)pt.cl1;
      }
      float gr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) gr[u] = row.has(u) ? grad_elem(p, pt, e[u] * pt.inv, row.bin(u) == t, cv[u]) : 0.f;
      row.store(p.dlogits, pix, gr);
    }
  }
  block_partial_row(acc, p.partial + (int64_t)blockIdx.x * kSums);
}

// one block: partial [rows][4] -> sums[4] (skipped when partial is NULL: the sums were all-reduced by the caller), then
// terms = (ce, regression, offset_reg, coarse_l1, total)
__global__ __launch_bounds__(256) void hybrid_finish_kernel(const double* partial, int rows, double* sums, double pixels_global,
                                                            float ce_weight, float reg_weight, float off_weight, float* terms) {
  sum_partial_rows<kSums>(partial, rows, sums, [&](const double (&s)[kSums]) {
    if (!terms) return;
    const float ce = (float)(s[0] / pixels_global), reg = (float)(s[1] / pixels_global);
    const float off = (float)(s[2] / pixels_global);
    terms[0] = ce;
    terms[1] = reg;
    terms[2] = off;
    terms[3] = (float)(s[3] / pixels_global);
    terms[4] = ce_weight * ce + reg_weight * reg + off_weight * off;
  });
}

inline int loss_blocks(int64_t pixels) { return adn_grid_blocks(pixels, 16, kLossBlocks); }      // coarse.hip's grid

}  // namespace

extern "C" int64_t adn_hybrid_loss_workspace_bytes(int64_t pixels) {
  if (pixels <= 0) return -1;
  return (int64_t)loss_blocks(pixels) * kSums * 8;
}

extern "C" int adn_hybrid_loss(const AdnHybridLoss* d, void* stream) {
  ADN_CHECK_ARG(d && d->logits && d->centers && d->coarse && d->offset && d->bins && d->gt && d->final_depth && d->dlogits &&
                    d->doffset && d->workspace && d->pixels > 0,
                "adn_hybrid_loss: null operand or no pixels");
  ADN_CHECK_DTYPE("adn_hybrid_loss", d->dtype);
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
  const int rc = launch_bin_rows("adn_hybrid_loss", d->dtype, d->nb, d->ld, d->logits, d->dlogits, [&](auto row) {
    hipLaunchKernelGGL((hybrid_loss_kernel<typename decltype(row)::type>), grid, dim3(256), 0, st, p);
  });
  if (rc != ADN_OK) return rc;
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
