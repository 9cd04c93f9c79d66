// Coarse-depth classification family, evaluation side: what the class head's per-pixel distribution says beyond its
// expectation.  Memory-bound; conventions of coarse.hip: f32 arithmetic, f64 final reductions, no atomics, bit-reproducible
// run to run (fixed grid per pixel count, fixed reduction order).
//   coarse_decode       ONE pass over the logits: expectation, first-maximum bin and its centre, standard deviation,
//                       entropy and confidence of softmax(x) over the bin centres
//   coarse_eval_stats   one pass over those planes, the target bins and gt: per-block f64 partials of the classification,
//                       spread and calibration sums over gt > 0
//   coarse_eval_finish  partials -> sums -> (n, top-1, within-1, ..., std / error correlation, ECE, reliability table)
#include "loss_tail.h"

namespace {

struct DecodeP {
  const void* logits; const float* centers;
  float *mean, *hard, *stdev, *entropy, *confidence; int32_t* argmax;
  int64_t pixels;
  int nb, ld;
};

// one body over either layout of loss_tail.h; the max / exp / sum se / sum sc chain is coarse_loss_kernel's, statement by
// statement, so mean and argmax carry the bits of the forward-only adn_coarse_loss
template <typename Row>
__global__ __launch_bounds__(256) void coarse_decode_kernel(DecodeP p) {
  constexpr int U = Row::U;
  const Row row(p.nb, p.ld);
  const bool want_idx = p.argmax || p.hard;
  float cv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) cv[u] = row.has(u) ? p.centers[row.bin(u)] : 0.f;
  for (int64_t p0 = row.first(); p0 < p.pixels; p0 += row.stride()) {
    const int64_t pix = row.pixel(p0);
    const bool live = row.live(pix, p.pixels);
    float d[U];
    const float mx = row.group_max(row.load(p.logits, pix, live, d));
    int cand = 0x7fffffff;
    if (want_idx) {                                   // first maximum, as torch.argmax picks it
#pragma unroll
      for (int u = U - 1; u >= 0; --u)
        if (row.has(u) && d[u] == mx) cand = row.bin(u);
      cand = row.group_min(cand);
    }
    float e[U];
    float se = 0.f, sc = 0.f, sd = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      e[u] = 0.f;
      if (!row.has(u)) continue;
      d[u] -= mx;
      e[u] = __expf(d[u]);
      se += e[u];
      sc += e[u] * cv[u];
      sd += e[u] * fmaxf(d[u], -3.0e38f);             // one max + one fma; 0 where exp underflowed, also at d = -inf
    }
    se = row.group_sum(se);
    sc = row.group_sum(sc);
    sd = row.group_sum(sd);
    const float inv = 1.f / se;
    const float mean = sc * inv;
    float m2 = 0.f;                                   // second moment about the mean from the e and c in registers:
    if (p.stdev) {                                    // no sum p c^2 - mean^2 cancellation, no second read of the logits
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float dc = cv[u] - mean;
        m2 += e[u] * (dc * dc);
      }
      m2 = row.group_sum(m2);
    }
    if (live && row.leader()) {
      if (p.mean) p.mean[pix] = mean;
      if (p.argmax) p.argmax[pix] = cand;
      if (p.hard) p.hard[pix] = p.centers[min(cand, p.nb - 1)];     // (a row of NaNs has no maximum: stay inside centers)
      if (p.stdev) p.stdev[pix] = sqrtf(m2 * inv);
      if (p.entropy) p.entropy[pix] = __logf(se) - sd * inv;       // ln Z + sum p_k (-d_k): both terms >= 0
      if (p.confidence) p.confidence[pix] = inv;                    // the maximum's e is exp(0) = 1
    }
  }
}

// sums of one evaluation, over gt > 0
enum {
  kN = 0, kTop1, kWithin1, kBinErr, kStd, kEnt, kConf,       // n, [argmax == t], [|argmax - t| <= 1], |argmax - t|, s, H, conf
  kErr, kStd2, kErr2, kStdErr,                               // a = |mean - gt|: a, s^2, a^2, s a  (with kStd: Pearson)
  kTable,                                                    // 10 confidence bins x (count, sum confidence, sum correct)
  kRelBins = 10, kEvalSums = kTable + 3 * kRelBins,
  kEvalHead = 9, kEvalOut = kEvalHead + 3 * kRelBins
};

struct EvalP {
  const int32_t *argmax, *bins;
  const float *confidence, *stdev, *entropy, *mean, *gt;
  double* partial;
  int64_t pixels;
};

__global__ __launch_bounds__(256) void coarse_eval_stats_kernel(EvalP p) {
  double acc[kEvalSums];
#pragma unroll
  for (int k = 0; k < kEvalSums; ++k) acc[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.pixels; i += (int64_t)gridDim.x * 256) {
    const float gtv = p.gt[i];
    if (!(gtv > 0.f)) continue;
    const int db = abs(p.argmax[i] - p.bins[i]);
    const float cf = p.confidence[i];
    const double s = (double)p.stdev[i], a = fabs((double)p.mean[i] - (double)gtv), c = (double)cf;
    const double hit = db == 0 ? 1.0 : 0.0;
    acc[kN] += 1.0;
    acc[kTop1] += hit;
    acc[kWithin1] += db <= 1 ? 1.0 : 0.0;
    acc[kBinErr] += (double)db;
    acc[kStd] += s;
    acc[kEnt] += (double)p.entropy[i];
    acc[kConf] += c;
    acc[kErr] += a;
    acc[kStd2] += s * s;
    acc[kErr2] += a * a;
    acc[kStdErr] += s * a;
    const int rb = min(kRelBins - 1, max(0, (int)floorf(cf * 10.f)));
#pragma unroll
    for (int b = 0; b < kRelBins; ++b) {              // predicated: a run-time index would put acc into scratch
      const bool in = rb == b;
      acc[kTable + 3 * b] += in ? 1.0 : 0.0;
      acc[kTable + 3 * b + 1] += in ? c : 0.0;
      acc[kTable + 3 * b + 2] += in ? hit : 0.0;
    }
  }
  block_partial_row(acc, p.partial + (int64_t)blockIdx.x * kEvalSums);
}

// one block: partial [rows][kEvalSums] -> sums (skipped when partial is NULL: the caller added up the sums of several
// batches), then out = (n, top1, within1, mean bin error, mean std, mean entropy, mean confidence, corr(std, |mean - gt|),
// ECE, the 30 table entries); every ratio is NaN without a valid pixel
__global__ __launch_bounds__(256) void coarse_eval_finish_kernel(const double* partial, int rows, double* sums, double* out) {
  sum_partial_rows<kEvalSums>(partial, rows, sums, [&](const double (&s)[kEvalSums]) {
    if (!out) return;
    const double n = s[kN];
    const double rn = n > 0.0 ? 1.0 / n : NAN;
    out[0] = n;
#pragma unroll
    for (int k = kTop1; k <= kConf; ++k) out[k] = n > 0.0 ? s[k] / n : NAN;
    double corr = NAN, ece = NAN;
    if (n > 0.0) {
      const double vs = s[kStd2] - s[kStd] * s[kStd] * rn, va = s[kErr2] - s[kErr] * s[kErr] * rn;
      if (vs > 0.0 && va > 0.0) corr = (s[kStdErr] - s[kStd] * s[kErr] * rn) / sqrt(vs * va);
      ece = 0.0;
      for (int b = 0; b < kRelBins; ++b) {
        const double nb = s[kTable + 3 * b];
        if (nb > 0.0) ece += nb * rn * fabs(s[kTable + 3 * b + 2] / nb - s[kTable + 3 * b + 1] / nb);
      }
    }
    out[7] = corr;
    out[8] = ece;
    for (int k = 0; k < 3 * kRelBins; ++k) out[kEvalHead + k] = s[kTable + k];
  });
}

inline int decode_blocks(int64_t pixels) { return adn_grid_blocks(pixels, 16, kLossBlocks); }     // adn_coarse_loss's grid
inline int eval_blocks(int64_t pixels) { return adn_grid_blocks(pixels, 1024, kLossBlocks); }

}  // namespace

extern "C" int adn_coarse_decode(const AdnCoarseDecode* d, void* stream) {
  ADN_CHECK_ARG(d, "adn_coarse_decode: null descriptor");
  ADN_CHECK_ARG(d->logits && d->centers && d->pixels > 0, "adn_coarse_decode: null operand or no pixels");
  ADN_CHECK_DTYPE("adn_coarse_decode", d->dtype);
  ADN_CHECK_ARG(d->nb >= 2 && d->nb <= kMaxNb, "adn_coarse_decode: n_bins %d outside the supported range [2, %d]", d->nb, kMaxNb);
  ADN_CHECK_ARG(d->ld >= d->nb, "adn_coarse_decode: row stride %d < n_bins %d", d->ld, d->nb);
  ADN_CHECK_ARG(d->mean || d->hard || d->stdev || d->entropy || d->confidence || d->argmax,
                "adn_coarse_decode: every output is NULL");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  DecodeP p;
  p.logits = d->logits; p.centers = d->centers;
  p.mean = d->mean; p.hard = d->hard; p.stdev = d->stdev; p.entropy = d->entropy; p.confidence = d->confidence;
  p.argmax = d->argmax;
  p.pixels = d->pixels; p.nb = d->nb; p.ld = d->ld;
  const dim3 grid(decode_blocks(d->pixels));
  const int rc = launch_bin_rows("adn_coarse_decode", d->dtype, d->nb, d->ld, d->logits, nullptr, [&](auto row) {
    hipLaunchKernelGGL((coarse_decode_kernel<typename decltype(row)::type>), grid, dim3(256), 0, st, p);
  });
  if (rc != ADN_OK) return rc;
  ADN_CHECK_LAUNCH();
  return ADN_OK;
}

extern "C" int64_t adn_coarse_eval_stats_workspace_bytes(int64_t pixels) {
  if (pixels <= 0) return -1;
  return (int64_t)eval_blocks(pixels) * kEvalSums * 8;
}

extern "C" int adn_coarse_eval_stats(const AdnCoarseEvalStats* d, void* stream) {
  ADN_CHECK_ARG(d, "adn_coarse_eval_stats: null descriptor");
  ADN_CHECK_ARG(d->argmax && d->bins && d->confidence && d->stdev && d->entropy && d->mean && d->gt && d->pixels > 0,
                "adn_coarse_eval_stats: null operand or no pixels");
  ADN_CHECK_ARG(d->workspace && d->workspace_bytes >= adn_coarse_eval_stats_workspace_bytes(d->pixels),
                "adn_coarse_eval_stats: workspace smaller than adn_coarse_eval_stats_workspace_bytes()");
  EvalP p;
  p.argmax = d->argmax; p.bins = d->bins; p.confidence = d->confidence; p.stdev = d->stdev; p.entropy = d->entropy;
  p.mean = d->mean; p.gt = d->gt; p.partial = reinterpret_cast<double*>(d->workspace); p.pixels = d->pixels;
  hipLaunchKernelGGL(coarse_eval_stats_kernel, dim3(eval_blocks(d->pixels)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), p);
  ADN_CHECK_LAUNCH();
  return ADN_OK;
}

extern "C" int adn_coarse_eval_finish(const void* workspace, int64_t pixels, double* sums, double* out, void* stream) {
  ADN_CHECK_ARG(sums && (!workspace || pixels > 0), "adn_coarse_eval_finish: bad arguments");
  hipLaunchKernelGGL(coarse_eval_finish_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const double*>(workspace), workspace ? eval_blocks(pixels) : 0, sums, out);
  ADN_CHECK_LAUNCH();
  return ADN_OK;
}
