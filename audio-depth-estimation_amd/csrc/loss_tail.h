// What the loss tails share (coarse / hybrid / dualreg, the statistics kernels of baseres / adabins / dcnet): the f64
// partial-row reductions and the two layouts of a pixel's row of bin logits.  Every order of additions here fixes output
// bits: per-thread accumulation over k ascending, the xor butterfly of a wave, then the four wave values left to right.
#pragma once
#include "adn_common.h"

constexpr int kMaxNb = 512;          // 8 x 64 lanes of one wave (WaveRow) / 64 lanes x one 16-byte chunk (VecRow)
constexpr int kLossBlocks = 2048;    // cap of the loss grids: one partial row per block

// 256 threads: K per-thread f64 accumulators -> out[K], one partial row of this block
template <int K>
__device__ __forceinline__ void block_partial_row(double (&acc)[K], double* out) {
  __shared__ double sm[K][4];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = wave_sum_d(acc[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) sm[k][threadIdx.x >> 6] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < K) out[threadIdx.x] = sm[threadIdx.x][0] + sm[threadIdx.x][1] + sm[threadIdx.x][2] + sm[threadIdx.x][3];
}

// one block of 256 threads: partial [rows][K] -> sums[K], then thread 0 runs finish(s) on them.  partial == NULL: the
// sums were all-reduced by the caller and are read as given.
template <int K, typename Finish>
__device__ __forceinline__ void sum_partial_rows(const double* partial, int rows, double* sums, Finish&& finish) {
  __shared__ double sm[K][4];
  if (partial) {
    double a[K];
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = 0.0;
    for (int r = threadIdx.x; r < rows; r += 256)
#pragma unroll
      for (int k = 0; k < K; ++k) a[k] += partial[(int64_t)r * K + k];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      a[k] = wave_sum_d(a[k]);
      if ((threadIdx.x & 63) == 0) sm[k][threadIdx.x >> 6] = a[k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (partial) {
        s[k] = sm[k][0] + sm[k][1] + sm[k][2] + sm[k][3];
        sums[k] = s[k];
      } else {
        s[k] = sums[k];
      }
    }
    finish(s);
  }
}

// the same in one wave of 64 threads (another order of additions: stride 64, then the butterfly); every lane gets s
template <int K>
__device__ __forceinline__ void sum_partial_rows_wave(const double* partial, int rows, double (&s)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double a = 0.0;
    for (int r = threadIdx.x; r < rows; r += 64) a += partial[(int64_t)r * K + k];
    s[k] = wave_sum_d(a);
  }
}

// ---- a pixel's row of nb bin logits, held in U = 8 registers per lane --------------------------------------------------
// A loss kernel (256 threads) walks  for (p0 = row.first(); p0 < pixels; p0 += row.stride())  and serves pixel
// row.pixel(p0), which may lie past the last one (row.live): such lanes still take part in every group reduction.

// bf16, ld == nb = 8 LPP, LPP a power of two <= 64: a row is LPP lanes x one 16-byte chunk, 64 / LPP pixels per
// wave-iteration, reductions across those lanes only (xor offsets ascending); the gradient leaves as one 16-byte store.
// Dead lanes hold d = 0, mx = 0 and read no per-pixel operand.
template <int LPP>
struct VecRow {
  static constexpr int U = 8, NB = LPP * 8, PPW = 64 / LPP;
  int li, pw;
  __device__ __forceinline__ VecRow(int, int) : li((threadIdx.x & 63) % LPP), pw((threadIdx.x & 63) / LPP) {}
  __device__ __forceinline__ int64_t first() const { return ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * PPW; }
  __device__ __forceinline__ int64_t stride() const { return (int64_t)gridDim.x * 4 * PPW; }
  __device__ __forceinline__ int64_t pixel(int64_t p0) const { return p0 + pw; }
  __device__ __forceinline__ bool live(int64_t pix, int64_t pixels) const { return pix < pixels; }
  __device__ __forceinline__ int bin(int u) const { return li * 8 + u; }
  __device__ __forceinline__ bool has(int) const { return true; }
  __device__ __forceinline__ bool leader() const { return li == 0; }
  // d = the lane's logits, returns their maximum
  __device__ __forceinline__ float load(const void* logits, int64_t pix, bool live, float (&d)[U]) const {
    float mx = -INFINITY;
    if (live) {
      const u32x4_t c = *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const uint16_t*>(logits) + pix * NB + li * 8);
      Chunk<uint16_t>::unpack(c, d);
#pragma unroll
      for (int k = 0; k < 8; ++k) mx = fmaxf(mx, d[k]);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) d[k] = 0.f;
      mx = 0.f;
    }
    return mx;
  }
  __device__ __forceinline__ float group_max(float v) const {
#pragma unroll
    for (int o = 1; o < LPP; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
  }
  __device__ __forceinline__ float group_sum(float v) const {
#pragma unroll
    for (int o = 1; o < LPP; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
  }
  // several sums sharing each butterfly step.  Same sums; but under -ffp-contract=fast the order in which a loss's sums
  // become ready decides which product of its pixel terms fuses with the add, so each loss keeps the form its parent
  // kernel compiled to (coarse: one by one, hybrid: together; pinned by tools/loss_tail_dump.py).
  template <typename... F>
  __device__ __forceinline__ void group_sums(F&... v) const {
#pragma unroll
    for (int o = 1; o < LPP; o <<= 1) ((v += __shfl_xor(v, o, 64)), ...);
  }
  __device__ __forceinline__ int group_min(int v) const {
#pragma unroll
    for (int o = 1; o < LPP; o <<= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
  }
  __device__ __forceinline__ void store(void* dlogits, int64_t pix, const float (&g)[U]) const {
    *reinterpret_cast<u32x4_t*>(reinterpret_cast<uint16_t*>(dlogits) + pix * NB + li * 8) = Chunk<uint16_t>::pack(g);
  }
};

// every other (dtype, nb, ld): one wave per pixel, lane l holds bins l, l + 64, ... (nb <= 512), row stride ld >= nb.
// Absent bins load -INFINITY; the store also zeroes the tape's padding columns nb .. ld - 1.
template <typename T>
struct WaveRow {
  static constexpr int U = kMaxNb / 64;
  int lane, nb, ld;
  __device__ __forceinline__ WaveRow(int nb_, int ld_) : lane(threadIdx.x & 63), nb(nb_), ld(ld_) {}
  __device__ __forceinline__ int64_t first() const { return (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); }
  __device__ __forceinline__ int64_t stride() const { return (int64_t)gridDim.x * 4; }
  __device__ __forceinline__ int64_t pixel(int64_t p0) const { return p0; }
  __device__ __forceinline__ bool live(int64_t, int64_t) const { return true; }
  __device__ __forceinline__ int bin(int u) const { return lane + 64 * u; }
  __device__ __forceinline__ bool has(int u) const { return bin(u) < nb; }
  __device__ __forceinline__ bool leader() const { return lane == 0; }
  __device__ __forceinline__ float load(const void* logits, int64_t pix, bool, float (&d)[U]) const {
    const T* row = reinterpret_cast<const T*>(logits) + pix * ld;
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      d[u] = has(u) ? ElemTraits<T>::load(row + bin(u)) : -INFINITY;
      mx = fmaxf(mx, d[u]);
    }
    return mx;
  }
  __device__ __forceinline__ float group_max(float v) const { return wave_max(v); }
  __device__ __forceinline__ float group_sum(float v) const { return wave_sum(v); }
  template <typename... F>
  __device__ __forceinline__ void group_sums(F&... v) const { ((v = wave_sum(v)), ...); }
  __device__ __forceinline__ int group_min(int v) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
  }
  __device__ __forceinline__ void store(void* dlogits, int64_t pix, const float (&g)[U]) const {
    T* drow = reinterpret_cast<T*>(dlogits) + pix * ld;
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (has(u)) ElemTraits<T>::store(drow + bin(u), g[u]);
    for (int k = nb + lane; k < ld; k += 64) ElemTraits<T>::store(drow + k, 0.f);
  }
};

// Picks the layout of one launch and calls launch(RowTag<Row>()): the vector form needs bf16, unpadded rows of 8 LPP
// bins, LPP a power of two, and 16-byte aligned logits and gradient (a NULL gradient counts as aligned).  Returns
// ADN_OK, or ADN_ERR_ARG ("<who>: bad dtype <n>", nothing launched) for a dtype code it does not know.
template <typename Row> struct RowTag { typedef Row type; };
template <typename Launch>
inline int launch_bin_rows(const char* who, int dtype, int nb, int ld, const void* logits, const void* dlogits, Launch&& launch) {
  const int lpp = nb / 8;
  const bool vec = dtype == ADN_BF16 && ld == nb && nb % 8 == 0 && (lpp & (lpp - 1)) == 0 &&
                   (reinterpret_cast<uintptr_t>(logits) & 15) == 0 && (reinterpret_cast<uintptr_t>(dlogits) & 15) == 0;
  if (vec) {
    switch (lpp) {
#define ADN_VEC_ROW(L) case L: launch(RowTag<VecRow<L>>()); break;
      ADN_VEC_ROW(1) ADN_VEC_ROW(2) ADN_VEC_ROW(4) ADN_VEC_ROW(8) ADN_VEC_ROW(16) ADN_VEC_ROW(32) ADN_VEC_ROW(64)
#undef ADN_VEC_ROW
    }
    return ADN_OK;
  }
  return adn_by_dtype(who, dtype, [&](auto t) {
    launch(RowTag<WaveRow<decltype(t)>>());
    return ADN_OK;
  });
}
