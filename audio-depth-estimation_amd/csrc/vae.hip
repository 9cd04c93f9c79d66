// VAE bottleneck of the U-Net cVAE family (models/unet_cvae_model.py: VAEBottleneck on the 1x1 innermost level).
//
// h [B][C] f32 (the innermost down conv's raw output) -> mu, logvar = Linear(C, L)(h); z = mu + eps * exp(logvar / 2);
// h_recon = Linear(L, C)(z); per-image KL = -1/2 sum_j (1 + logvar - mu^2 - exp(logvar)) and its mean over B.
// The GEMMs are tiny (B = 32, C = 512, L = 128: ~12 MFLOP, 0.8 MB of f32 weights): everything here is latency bound,
// so the kernels are plain wave dot products sized for few launches and L2 residency, not MFMA tiles.  Two launches
// forward, two backward; phases hand data over at launch boundaries only (the XCDs' L2s are not coherent), no atomics,
// every sum in a fixed order: results are bit-reproducible run to run.
#include "adn_common.h"

namespace {

constexpr int kVB = 8;             // images per wave in the dot-product kernels

// Counter-based standard normal: splitmix64 of (seed, element) -> two 24-bit uniforms -> Box-Muller (cosine branch).
__device__ __forceinline__ float vae_gauss(uint64_t seed, int64_t idx) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(idx + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const float u1 = ((float)(z >> 40) + 1.0f) * (1.0f / 16777216.0f);               // (0, 1]
  const float u2 = (float)((z >> 16) & 0xFFFFFFull) * (1.0f / 16777216.0f);        // [0, 1)
  return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958648f * u2);
}

// Row j of fc_mu / fc_logvar against images b0 .. b0 + nb - 1 (one wave, lanes stride over C): lane k < nb ends up with
// image b0 + k's two dot products (no bias yet).  Shared by the training forward and the multi-draw sampler.
__device__ __forceinline__ void vae_mu_logvar_dots(const float* __restrict__ h, int C, const float* __restrict__ w_mu,
                                                   const float* __restrict__ w_lv, int j, int b0, int nb, int lane,
                                                   float& m, float& l) {
  float am[kVB], al[kVB];
#pragma unroll
  for (int k = 0; k < kVB; ++k) am[k] = al[k] = 0.f;
  const float* wm = w_mu + (int64_t)j * C;
  const float* wl = w_lv + (int64_t)j * C;
  for (int c = lane; c < C; c += 64) {
    const float xm = wm[c], xl = wl[c];
#pragma unroll
    for (int k = 0; k < kVB; ++k) {
      if (k < nb) {
        const float hv = h[(int64_t)(b0 + k) * C + c];
        am[k] = fmaf(xm, hv, am[k]);
        al[k] = fmaf(xl, hv, al[k]);
      }
    }
  }
  m = l = 0.f;
#pragma unroll
  for (int k = 0; k < kVB; ++k) {
    const float sm = wave_sum(am[k]), sl = wave_sum(al[k]);
    if (lane == k) {
      m = sm;
      l = sl;
    }
  }
}

// mu / logvar / eps / z: one wave per (latent row j, group of kVB images); lanes stride over C.
__global__ __launch_bounds__(256) void vae_encode_kernel(const float* __restrict__ h, int B, int C, int L,
                                                         const float* __restrict__ w_mu, const float* __restrict__ b_mu,
                                                         const float* __restrict__ w_lv, const float* __restrict__ b_lv,
                                                         uint64_t seed, const double* counter,
                                                         const float* __restrict__ eps_in, float* mu, float* logvar,
                                                         float* eps, float* z) {
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int nbg = (B + kVB - 1) / kVB;
  if (wave >= L * nbg) return;                                  // wave-uniform
  if (counter) seed += 0xD1B54A32D192ED03ull * (uint64_t)(counter[0] + 1.0);     // device step count: replay safe
  const int j = wave % L, b0 = (wave / L) * kVB;
  const int nb = min(kVB, B - b0);
  float m, l;
  vae_mu_logvar_dots(h, C, w_mu, w_lv, j, b0, nb, lane, m, l);
  if (lane < nb) {
    const int64_t idx = (int64_t)(b0 + lane) * L + j;
    m += b_mu[j];
    l += b_lv[j];
    const float e = eps_in ? eps_in[idx] : vae_gauss(seed, idx);
    const float sd = expf(0.5f * l);
    mu[idx] = m;
    logvar[idx] = l;
    eps[idx] = e;
    z[idx] = m + e * sd;
  }
}

// The sampler's form of the kernel above: mu / logvar once, then K draws z[k][b][j] = mu + eps[k][b][j] * exp(logvar / 2).
// The drawn eps of draw k is element k * B * L + b * L + j of the stream of ``seed``: every (k, b, j) has a counter of
// its own (no two draws share one), draw k does not depend on K, and draw 0 is what vae_encode_kernel draws for the seed.
// draw == 0 (mean decode): eps = 0, z = mu.
__global__ __launch_bounds__(256) void vae_sample_encode_kernel(const float* __restrict__ h, int B, int C, int L, int K,
                                                                int draw, const float* __restrict__ w_mu,
                                                                const float* __restrict__ b_mu,
                                                                const float* __restrict__ w_lv,
                                                                const float* __restrict__ b_lv, uint64_t seed,
                                                                const float* __restrict__ eps_in, float* mu,
                                                                float* logvar, float* eps, float* z) {
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int nbg = (B + kVB - 1) / kVB;
  if (wave >= L * nbg) return;                                  // wave-uniform
  const int j = wave % L, b0 = (wave / L) * kVB;
  const int nb = min(kVB, B - b0);
  float m, l;
  vae_mu_logvar_dots(h, C, w_mu, w_lv, j, b0, nb, lane, m, l);
  if (lane < nb) {
    const int64_t idx = (int64_t)(b0 + lane) * L + j, BL = (int64_t)B * L;
    m += b_mu[j];
    l += b_lv[j];
    const float sd = expf(0.5f * l);
    mu[idx] = m;
    logvar[idx] = l;
    for (int k = 0; k < K; ++k) {
      const int64_t kidx = (int64_t)k * BL + idx;
      const float e = !draw ? 0.f : (eps_in ? eps_in[kidx] : vae_gauss(seed, kidx));
      eps[kidx] = e;
      z[kidx] = m + e * sd;
    }
  }
}

// ReLU(fc_dec(z)) in the compute dtype: one wave per (output channel c, group of kVB images); lanes stride over L.
// The last block computes the per-image KL and its batch mean (fixed order: wave w sums images w, w+4, ...) over the
// Bkl rows of mu / logvar: B in the training forward, B / K in the sampler, whose K draws share one mu / logvar.
template <typename T>
__global__ __launch_bounds__(256) void vae_decode_kernel(const float* __restrict__ z, int B, int Bkl, int C, int L,
                                                         const float* __restrict__ w_dec, const float* __restrict__ b_dec,
                                                         const float* __restrict__ mu, const float* __restrict__ logvar,
                                                         float* kl_img, float* kl, T* out) {
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (blockIdx.x == gridDim.x - 1) {
    __shared__ float part[4];
    float acc = 0.f;
    for (int b = wid; b < Bkl; b += 4) {
      float s = 0.f;
      for (int j = lane; j < L; j += 64) {
        const float l = logvar[(int64_t)b * L + j], m = mu[(int64_t)b * L + j];
        s += 1.0f + l - m * m - expf(l);
      }
      const float kb = -0.5f * wave_sum(s);
      if (lane == 0) kl_img[b] = kb;
      acc += kb;
    }
    if (lane == 0) part[wid] = acc;
    __syncthreads();
    if (threadIdx.x == 0) kl[0] = (((part[0] + part[1]) + part[2]) + part[3]) / (float)Bkl;
    return;
  }
  const int wave = blockIdx.x * 4 + wid;
  const int nbg = (B + kVB - 1) / kVB;
  if (wave >= C * nbg) return;
  const int c = wave % C, b0 = (wave / C) * kVB;
  const int nb = min(kVB, B - b0);
  float acc[kVB];
#pragma unroll
  for (int k = 0; k < kVB; ++k) acc[k] = 0.f;
  const float* wr = w_dec + (int64_t)c * L;
  for (int j = lane; j < L; j += 64) {
    const float w = wr[j];
#pragma unroll
    for (int k = 0; k < kVB; ++k)
      if (k < nb) acc[k] = fmaf(w, z[(int64_t)(b0 + k) * L + j], acc[k]);
  }
  float v = 0.f;
#pragma unroll
  for (int k = 0; k < kVB; ++k) {
    const float s = wave_sum(acc[k]);
    if (lane == k) v = s;
  }
  if (lane < nb) ElemTraits<T>::store(out + (int64_t)(b0 + lane) * C + c, fmaxf(v + b_dec[c], 0.f));
}

// Backward phase 1.
//   blocks [0, B * ceil(L/64)): dz[b][j] = sum_c g[b][c] W_dec[c][j] (4 waves split c, LDS sum in fixed order), then
//     dmu = dz + g_kl mu / B,  dlv = dz eps std / 2 + g_kl (exp(logvar) - 1) / (2B)  -> dmu_dlv [2][B][L]
//   blocks [.., + C): row c of dW_dec = sum_b g[b][c] z[b][:], db_dec[c] = sum_b g[b][c]
//   block 0 also adds g_kl * kl to the caller's loss (the fused trainer's total loss), when asked.
template <typename T>
__global__ __launch_bounds__(256) void vae_bwd_dec_kernel(const T* __restrict__ g, int B, int C, int L,
                                                          const float* __restrict__ mu, const float* __restrict__ logvar,
                                                          const float* __restrict__ eps, const float* __restrict__ z,
                                                          const float* __restrict__ w_dec, const float* g_kl,
                                                          float* dw_dec, float* db_dec, float* dmu_dlv, const float* kl,
                                                          float* loss) {
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int njc = (L + 63) / 64;
  const int nA = B * njc;
  if (blockIdx.x == 0 && threadIdx.x == 0 && loss) loss[0] += g_kl[0] * kl[0];
  if ((int)blockIdx.x < nA) {
    __shared__ float red[4][64];
    const int b = blockIdx.x / njc, j = (blockIdx.x % njc) * 64 + lane;
    float s = 0.f;
    if (j < L) {
      const T* gb = g + (int64_t)b * C;
      for (int c = wid; c < C; c += 4) s = fmaf(ElemTraits<T>::load(gb + c), w_dec[(int64_t)c * L + j], s);
    }
    red[wid][lane] = s;
    __syncthreads();
    if (wid == 0 && j < L) {
      const float dz = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
      const int64_t idx = (int64_t)b * L + j;
      const float gk = g_kl[0], invB = 1.0f / (float)B;
      const float m = mu[idx], l = logvar[idx];
      dmu_dlv[idx] = dz + gk * m * invB;
      dmu_dlv[(int64_t)B * L + idx] = dz * eps[idx] * 0.5f * expf(0.5f * l) + gk * 0.5f * (expf(l) - 1.0f) * invB;
    }
    return;
  }
  const int c = blockIdx.x - nA;
  for (int j = threadIdx.x; j < L; j += 256) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s = fmaf(ElemTraits<T>::load(g + (int64_t)b * C + c), z[(int64_t)b * L + j], s);
    dw_dec[(int64_t)c * L + j] = s;
  }
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += ElemTraits<T>::load(g + (int64_t)b * C + c);
    db_dec[c] = s;
  }
}

// Backward phase 2.
//   blocks [0, 2L): row j of dW_mu (r < L) / dW_lv (r >= L) = sum_b d[b][j] h[b][:], and the bias entry sum_b d[b][j]
//   blocks [2L, 2L + B * ceil(C/64)): dh[b][c] = sum_j W_mu[j][c] dmu[b][j] + W_lv[j][c] dlv[b][j] (4 waves split j)
template <typename T>
__global__ __launch_bounds__(256) void vae_bwd_enc_kernel(const float* __restrict__ h, int B, int C, int L,
                                                          const float* __restrict__ w_mu, const float* __restrict__ w_lv,
                                                          const float* __restrict__ dmu_dlv, float* dw_mu, float* db_mu,
                                                          float* dw_lv, float* db_lv, T* dh) {
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* dmu = dmu_dlv;
  const float* dlv = dmu_dlv + (int64_t)B * L;
  if ((int)blockIdx.x < 2 * L) {
    const int which = blockIdx.x / L, j = blockIdx.x % L;
    const float* d = which ? dlv : dmu;
    float* dw = which ? dw_lv : dw_mu;
    for (int c = threadIdx.x; c < C; c += 256) {
      float s = 0.f;
      for (int b = 0; b < B; ++b) s = fmaf(d[(int64_t)b * L + j], h[(int64_t)b * C + c], s);
      dw[(int64_t)j * C + c] = s;
    }
    if (threadIdx.x == 0) {
      float s = 0.f;
      for (int b = 0; b < B; ++b) s += d[(int64_t)b * L + j];
      (which ? db_lv : db_mu)[j] = s;
    }
    return;
  }
  __shared__ float red[4][64];
  const int ncc = (C + 63) / 64;
  const int blk = blockIdx.x - 2 * L;
  const int b = blk / ncc, c = (blk % ncc) * 64 + lane;
  float s = 0.f;
  if (c < C) {
    for (int j = wid; j < L; j += 4) {
      s = fmaf(w_mu[(int64_t)j * C + c], dmu[(int64_t)b * L + j], s);
      s = fmaf(w_lv[(int64_t)j * C + c], dlv[(int64_t)b * L + j], s);
    }
  }
  red[wid][lane] = s;
  __syncthreads();
  if (wid == 0 && c < C)
    ElemTraits<T>::store(dh + (int64_t)b * C + c, ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]);
}

int vae_check(int32_t B, int32_t C, int32_t L, int32_t dtype, const char* who) {
  ADN_CHECK_ARG(B >= 1 && C >= 8 && C % 8 == 0 && L >= 1 && L <= 1024,
                "%s: B %d, C %d, L %d (need B >= 1, C %% 8 == 0, 1 <= L <= 1024)", who, B, C, L);
  ADN_CHECK_DTYPE(who, dtype);
  return ADN_OK;
}

}  // namespace

extern "C" int adn_vae_fwd(const float* h, int32_t B, int32_t C, int32_t L, const float* w_mu, const float* b_mu,
                           const float* w_lv, const float* b_lv, const float* w_dec, const float* b_dec, uint64_t seed,
                           const double* counter, const float* eps_in, float* mu, float* logvar, float* eps, float* z,
                           float* kl_img, float* kl, int32_t dtype, void* out_relu, void* stream) {
  if (int rc = vae_check(B, C, L, dtype, "adn_vae_fwd")) return rc;
  ADN_CHECK_ARG(h && w_mu && b_mu && w_lv && b_lv && w_dec && b_dec && mu && logvar && eps && z && kl_img && kl && out_relu,
                "adn_vae_fwd: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nbg = (B + kVB - 1) / kVB;
  hipLaunchKernelGGL(vae_encode_kernel, dim3((unsigned)adn_cdiv((int64_t)L * nbg, 4)), dim3(256), 0, st, h, B, C, L,
                     w_mu, b_mu, w_lv, b_lv, seed, counter, eps_in, mu, logvar, eps, z);
  ADN_CHECK_LAUNCH();
  const unsigned nb = (unsigned)adn_cdiv((int64_t)C * nbg, 4) + 1;
  return adn_by_dtype("adn_vae_fwd", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((vae_decode_kernel<T>), dim3(nb), dim3(256), 0, st, z, B, B, C, L, w_dec, b_dec, mu, logvar, kl_img,
                       kl, adn_as<T>(out_relu));
    ADN_CHECK_LAUNCH();
    return ADN_OK;
  });
}

extern "C" int adn_vae_sample(const float* h, int32_t B, int32_t C, int32_t L, int32_t K, int32_t mode,
                              const float* w_mu, const float* b_mu, const float* w_lv, const float* b_lv,
                              const float* w_dec, const float* b_dec, uint64_t seed, const float* eps_in, float* mu,
                              float* logvar, float* eps, float* z, float* kl_img, float* kl, int32_t dtype,
                              void* out_relu, void* stream) {
  if (int rc = vae_check(B, C, L, dtype, "adn_vae_sample")) return rc;
  ADN_CHECK_ARG(mode == ADN_VAE_DRAW || mode == ADN_VAE_MEAN, "adn_vae_sample: bad mode %d", mode);
  ADN_CHECK_ARG(K >= 1 && (mode == ADN_VAE_DRAW || K == 1), "adn_vae_sample: K %d (need K >= 1, and K == 1 for the mean decode)",
                K);
  // the decode grid has one wave per (channel, group of kVB rows) of the K * B rows
  const int64_t rows = (int64_t)K * B, nbg = adn_cdiv(rows, (int64_t)kVB);
  ADN_CHECK_ARG(rows <= INT32_MAX && (int64_t)C * nbg <= INT32_MAX - 4,
                "adn_vae_sample: K %d x B %d rows of %d channels exceed the decode grid", K, B, C);
  ADN_CHECK_ARG(h && w_mu && b_mu && w_lv && b_lv && w_dec && b_dec && mu && logvar && eps && z && kl_img && kl && out_relu,
                "adn_vae_sample: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vae_sample_encode_kernel, dim3((unsigned)adn_cdiv((int64_t)L * adn_cdiv(B, kVB), 4)), dim3(256), 0, st,
                     h, B, C, L, K, mode == ADN_VAE_DRAW ? 1 : 0, w_mu, b_mu, w_lv, b_lv, seed, eps_in, mu, logvar, eps, z);
  ADN_CHECK_LAUNCH();
  const unsigned nb = (unsigned)adn_cdiv((int64_t)C * nbg, 4) + 1;
  return adn_by_dtype("adn_vae_sample", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((vae_decode_kernel<T>), dim3(nb), dim3(256), 0, st, z, (int)rows, B, C, L, w_dec, b_dec, mu, logvar,
                       kl_img, kl, adn_as<T>(out_relu));
    ADN_CHECK_LAUNCH();
    return ADN_OK;
  });
}

extern "C" int64_t adn_vae_bwd_workspace_bytes(int32_t B, int32_t L) {
  if (B < 1 || L < 1) return -1;
  return (int64_t)2 * B * L * (int64_t)sizeof(float);
}

extern "C" int adn_vae_bwd(const void* g_rec, int32_t dtype, int32_t B, int32_t C, int32_t L, const float* h,
                           const float* mu, const float* logvar, const float* eps, const float* z, const float* w_mu,
                           const float* w_lv, const float* w_dec, const float* g_kl, float* dw_mu, float* db_mu,
                           float* dw_lv, float* db_lv, float* dw_dec, float* db_dec, const float* kl, float* loss,
                           void* dh, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = vae_check(B, C, L, dtype, "adn_vae_bwd")) return rc;
  ADN_CHECK_ARG(g_rec && h && mu && logvar && eps && z && w_mu && w_lv && w_dec && g_kl && dw_mu && db_mu && dw_lv &&
                    db_lv && dw_dec && db_dec && dh && workspace,
                "adn_vae_bwd: null pointer");
  ADN_CHECK_ARG(!loss || kl, "adn_vae_bwd: a loss accumulator needs the KL scalar");
  ADN_CHECK_ARG(workspace_bytes >= adn_vae_bwd_workspace_bytes(B, L), "adn_vae_bwd: workspace too small");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* dmu_dlv = reinterpret_cast<float*>(workspace);
  const unsigned na = (unsigned)((int64_t)B * adn_cdiv(L, 64) + C);
  const unsigned nb = (unsigned)(2 * (int64_t)L + (int64_t)B * adn_cdiv(C, 64));
  return adn_by_dtype("adn_vae_bwd", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((vae_bwd_dec_kernel<T>), dim3(na), dim3(256), 0, st, adn_as<T>(g_rec), B, C, L, mu, logvar, eps, z,
                       w_dec, g_kl, dw_dec, db_dec, dmu_dlv, kl, loss);
    ADN_CHECK_LAUNCH();
    hipLaunchKernelGGL((vae_bwd_enc_kernel<T>), dim3(nb), dim3(256), 0, st, h, B, C, L, w_mu, w_lv, dmu_dlv, dw_mu, db_mu,
                       dw_lv, db_lv, adn_as<T>(dh));
    ADN_CHECK_LAUNCH();
    return ADN_OK;
  });
}
