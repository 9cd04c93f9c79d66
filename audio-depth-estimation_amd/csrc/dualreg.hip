// Dual-regression coarse-depth family (coarse_depth_model.py:857-1056, train_coarse_depth.py:422-432): the loss tail
// behind the two 1x1 heads.  Memory-bound; conventions of coarse.hip: f32 arithmetic, f64 final reductions, no atomics,
// bit-reproducible run to run (fixed grid per pixel count, fixed reduction order).
//   dualreg_loss     ONE pass over the pixels: final = coarse + offset, and with a target the three L1 sums
//                    (masked |coarse - gt|, masked |final - gt|, |offset|) and the gradients of their weighted means
//   dualreg_finish   per-block f64 partials -> sums -> (coarse, final, offset_reg, total)
#include "loss_tail.h"

namespace {

struct DualRegP {
  const float* coarse; const float* offset; const float* gt; const double* n_valid;
  float* final_; float* dcoarse; float* doffset; double* partial;
  int64_t pixels;
  double pixels_global;
  float cw, fw, rw;
};

__global__ __launch_bounds__(256) void dualreg_loss_kernel(DualRegP p) {
  const bool have_loss = p.gt != nullptr;
  // no valid pixel in the global batch: DualRegressionLoss takes the unmasked mean (its valid_mask.any() else-branch)
  bool all = false;
  float inv_n = 0.f, inv_pix = 0.f;
  if (have_loss) {
    const double nv = p.n_valid[0];
    all = !(nv > 0.0);
    inv_n = (float)(1.0 / (all ? p.pixels_global : nv));
    inv_pix = (float)(1.0 / p.pixels_global);
  }
  const float rcoef = p.rw * inv_pix;
  double a[3] = {0.0, 0.0, 0.0};
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < p.pixels; e += (int64_t)gridDim.x * 256) {
    const float c = p.coarse[e], o = p.offset[e];
    const float f = c + o;
    p.final_[e] = f;
    if (!have_loss) continue;
    const float g = p.gt[e];
    const float m = (all || g > 0.f) ? 1.f : 0.f;
    const float dc = c - g, df = f - g;
    a[0] += (double)(m * fabsf(dc));
    a[1] += (double)(m * fabsf(df));
    a[2] += (double)fabsf(o);
    const float gf = p.fw * adn_sgn(df) * m * inv_n;
    p.dcoarse[e] = p.cw * adn_sgn(dc) * m * inv_n + gf;
    p.doffset[e] = gf + rcoef * adn_sgn(o);
  }
  if (have_loss) block_partial_row(a, p.partial + (int64_t)blockIdx.x * 3);
}

// one block: partial [rows][3] -> sums[3] (skipped when partial is NULL: the sums were all-reduced by the caller), then
// terms = (coarse, final, offset_reg, total)
__global__ __launch_bounds__(256) void dualreg_finish_kernel(const double* partial, int rows, double* sums, const double* n_valid,
                                                             double pixels_global, float cw, float fw, float rw, float* terms) {
  sum_partial_rows<3>(partial, rows, sums, [&](const double (&s)[3]) {
    if (!terms) return;
    const double nv = n_valid[0];
    const double n = nv > 0.0 ? nv : pixels_global;
    const float lc = (float)(s[0] / n), lf = (float)(s[1] / n), lo = (float)(s[2] / pixels_global);
    terms[0] = lc;
    terms[1] = lf;
    terms[2] = lo;
    terms[3] = cw * lc + fw * lf + rw * lo;
  });
}

inline int loss_blocks(int64_t pixels) { return adn_grid_blocks(pixels, 256, kLossBlocks); }

}  // namespace

extern "C" int64_t adn_dualreg_loss_workspace_bytes(int64_t pixels) {
  if (pixels <= 0) return -1;
  return (int64_t)loss_blocks(pixels) * 3 * 8;
}

extern "C" int adn_dualreg_loss(const AdnDualRegLoss* d, void* stream) {
  ADN_CHECK_ARG(d && d->coarse && d->offset && d->final_depth && d->pixels > 0, "adn_dualreg_loss: null plane or no pixels");
  ADN_CHECK_ARG(!d->gt || (d->dcoarse && d->doffset && d->n_valid && d->workspace &&
                           d->workspace_bytes >= adn_dualreg_loss_workspace_bytes(d->pixels)),
                "adn_dualreg_loss: the loss needs dcoarse, doffset, n_valid and a workspace of adn_dualreg_loss_workspace_bytes()");
  ADN_CHECK_ARG(!d->gt || d->pixels_global >= d->pixels, "adn_dualreg_loss: global pixel count %lld < local %lld",
                (long long)d->pixels_global, (long long)d->pixels);
  DualRegP p;
  p.coarse = d->coarse; p.offset = d->offset; p.gt = d->gt; p.n_valid = d->n_valid;
  p.final_ = d->final_depth; p.dcoarse = d->dcoarse; p.doffset = d->doffset;
  p.partial = reinterpret_cast<double*>(d->workspace);
  p.pixels = d->pixels;
  p.pixels_global = (double)d->pixels_global;
  p.cw = d->coarse_weight; p.fw = d->final_weight; p.rw = d->offset_reg_weight;
  hipLaunchKernelGGL(dualreg_loss_kernel, dim3(loss_blocks(d->pixels)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
  ADN_CHECK_LAUNCH();
  return ADN_OK;
}

extern "C" int adn_dualreg_loss_finish(const void* workspace, int64_t pixels, double* sums, const double* n_valid,
                                       int64_t pixels_global, float coarse_weight, float final_weight,
                                       float offset_reg_weight, float* terms, void* stream) {
  ADN_CHECK_ARG(sums && pixels > 0, "adn_dualreg_loss_finish: bad arguments");
  ADN_CHECK_ARG(!terms || (n_valid && pixels_global >= pixels), "adn_dualreg_loss_finish: the terms need n_valid and the global pixel count");
  hipLaunchKernelGGL(dualreg_finish_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const double*>(workspace), loss_blocks(pixels), sums, n_valid, (double)pixels_global,
                     coarse_weight, final_weight, offset_reg_weight, terms);
  ADN_CHECK_LAUNCH();
  return ADN_OK;
}
