// Pseudo-label / guidance quality counts of the semi-supervised step (monitor.py): ONE streaming pass over the step's label
// maps adds 13 per-class rows, two confidence histograms and the pixel count into an int64 table (layout: semivl_hip.h).
// Shape of iou_hist_kernel (pixel_loss.hip): block-private 32-bit counters in LDS, flushed with 64-bit integer atomics --
// integer sums do not depend on the order, so two runs agree bit for bit.
//
// Label maps are spatially coherent: the 64 lanes of a wave usually carry ONE class, and 64 LDS atomics on one address
// serialise.  So a wave aggregates before it touches LDS: it ballots on the class of its first pending lane, and one lane
// per row adds the popcount of that row's flag ballot (one ds_add, distinct addresses).  That is repeated for at most PLS_PEEL
// distinct classes; lanes still pending after that (a noisy map: many classes per wave, so little contention each) add 1 per
// row themselves.
#include "svl_common.h"

namespace {

constexpr int PLS_ROWS = 13;
constexpr int PLS_MAX_GRID = 2048;   // 256 CUs x 8 blocks, the rest is grid-strided
constexpr int PLS_PEEL = 4;

typedef long long i64x2 __attribute__((ext_vector_type(2)));

// Lane counts in row ((rows >> 4 j) & 15) of `tab` ([row][stride]) at column `key` when bit j of `f` is set; f == 0: not at
// all.  Must be reached by all 64 lanes of the wave (ballots).
template <int NR>
__device__ __forceinline__ void wave_count(unsigned int* tab, int stride, unsigned long long rows, int key, unsigned int f) {
  const int lane = threadIdx.x & 63;
  unsigned long long B[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) B[j] = __ballot((f >> j) & 1u);
  unsigned long long rem = __ballot(f != 0u);
  const int my_row = (int)((rows >> (4 * (lane & 15))) & 15ull);
  for (int it = 0; it < PLS_PEEL && rem; ++it) {
    const int c = __builtin_amdgcn_readlane(key, __ffsll((long long)rem) - 1);
    const unsigned long long same = __ballot(f != 0u && key == c);
    unsigned int cnt = 0;
#pragma unroll
    for (int j = 0; j < NR; ++j)
      if (lane == j) cnt = (unsigned int)__popcll(same & B[j]);
    if (lane < NR && cnt) atomicAdd(&tab[my_row * stride + c], cnt);
    rem &= ~same;
  }
  if ((rem >> lane) & 1ull) {
#pragma unroll
    for (int j = 0; j < NR; ++j)
      if ((f >> j) & 1u) atomicAdd(&tab[(int)((rows >> (4 * j)) & 15ull) * stride + key], 1u);
  }
}

// rows keyed by the pseudo-label, the guidance and the annotation (bit j of the flag word <-> nibble j), and the histograms
constexpr unsigned long long ROWS_P = 0x9865310ull;   // 0 pl_area, 1 plc_area, 3 agree, 5 pl_inter, 6 pl_area_gt, 8 plc_inter, 9 plc_area_gt
constexpr unsigned long long ROWS_MC = 0xCB2ull;      // 2 mc_area, 11 mc_inter, 12 mc_area_gt
constexpr unsigned long long ROWS_GT = 0xA74ull;      // 4 gt_area, 7 plc_gt_area, 10 mc_gt_area
constexpr unsigned long long ROWS_H = 0x10ull;        // conf_hist, conf_hist_correct

// V = 2: every thread reads two neighbouring pixels, the int64 maps with 16-byte loads (pointers 16-byte aligned, conf 8).
template <int V>
__global__ __launch_bounds__(256) void pl_stats_kernel(const int64_t* __restrict__ mask_w, const float* __restrict__ conf,
                                                       const int64_t* __restrict__ ign, const int64_t* __restrict__ mc,
                                                       const int64_t* __restrict__ gt, long n, int N, int bins,
                                                       float thresh, unsigned long long* __restrict__ stats) {
  extern __shared__ unsigned int sh[];  // [13 N + 2 bins]
  const int T = PLS_ROWS * N + 2 * bins;
  for (int i = threadIdx.x; i < T; i += 256) sh[i] = 0;
  __syncthreads();
  unsigned int* hist = sh + PLS_ROWS * N;
  const long nq = (n + V - 1) / V;
  // (q0 is the same in every thread of the block: all 64 lanes of a wave make the same trips and reach every ballot)
  for (long q0 = (long)blockIdx.x * 256; q0 < nq; q0 += (long)gridDim.x * 256) {
    const long i0 = (q0 + threadIdx.x) * V;
    long p_[V], ig_[V], mc_[V], gt_[V];
    float cf_[V];
    bool in_[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      in_[e] = i0 + e < n;
      p_[e] = -1; ig_[e] = 255; mc_[e] = 255; gt_[e] = 255; cf_[e] = 0.f;
    }
    if (V == 2 && i0 + 1 < n) {
      const i64x2 a = *reinterpret_cast<const i64x2*>(mask_w + i0);
      const i64x2 b = *reinterpret_cast<const i64x2*>(ign + i0);
      const float2 c = *reinterpret_cast<const float2*>(conf + i0);
      p_[0] = a.x; p_[V - 1] = a.y; ig_[0] = b.x; ig_[V - 1] = b.y; cf_[0] = c.x; cf_[V - 1] = c.y;
      if (mc) { const i64x2 d = *reinterpret_cast<const i64x2*>(mc + i0); mc_[0] = d.x; mc_[V - 1] = d.y; }
      if (gt) { const i64x2 d = *reinterpret_cast<const i64x2*>(gt + i0); gt_[0] = d.x; gt_[V - 1] = d.y; }
    } else if (in_[0]) {   // V == 1, or the last pixel of an odd n
      p_[0] = mask_w[i0]; ig_[0] = ign[i0]; cf_[0] = conf[i0];
      if (mc) mc_[0] = mc[i0];
      if (gt) gt_[0] = gt[i0];
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const long p = p_[e], mcv = mc_[e], gtv = gt_[e];
      const float cf = cf_[e];
      const bool v = in_[e] && ig_[e] != 255;
      const bool k = v && cf >= thresh;                 // the cross-entropy kernels' fp32 comparison; NaN is not confident
      const bool m = v && mcv >= 0 && mcv < N;
      const bool g = v && gtv >= 0 && gtv < N;
      const bool pv = p >= 0 && p < N;
      const bool pg = g && p == gtv;
      unsigned int f = 0;
      if (pv) f = (v ? 1u : 0u) | (k ? 2u : 0u) | (m && mcv == p ? 4u : 0u) | (pg ? 8u : 0u) | (g ? 16u : 0u) |
                  (k && pg ? 32u : 0u) | (k && g ? 64u : 0u);
      wave_count<7>(sh, N, ROWS_P, pv ? (int)p : 0, f);
      if (mc) {
        f = (m ? 1u : 0u) | (m && g && gtv == mcv ? 2u : 0u) | (m && g ? 4u : 0u);
        wave_count<3>(sh, N, ROWS_MC, m ? (int)mcv : 0, f);
      }
      if (gt) {
        f = (g ? 1u : 0u) | (k && g ? 2u : 0u) | (m && g ? 4u : 0u);
        wave_count<3>(sh, N, ROWS_GT, g ? (int)gtv : 0, f);
      }
      // bin = min((int)(conf * bins), bins - 1) in fp32; a conf that is not >= 0 (negative, NaN) goes to bin 0
      const float t = cf * (float)bins;
      const int bin = !(cf >= 0.f) ? 0 : (t >= (float)bins ? bins - 1 : (int)t);
      f = (v ? 1u : 0u) | (pg ? 2u : 0u);
      wave_count<2>(hist, bins, ROWS_H, bin, f);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < T; i += 256)
    if (sh[i]) atomicAdd(&stats[i], (unsigned long long)sh[i]);
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&stats[T], (unsigned long long)n);
}

// sum[i] += losses[i] (i < k), steps[0] += 1: the meter's per-step bookkeeping, stream-ordered, no atomics
__global__ void pl_add_losses_kernel(const float* __restrict__ losses, int k, double* __restrict__ sum,
                                     int64_t* __restrict__ steps) {
  const int i = threadIdx.x;
  if (i < k) sum[i] += (double)losses[i];
  if (i == 0) steps[0] += 1;
}

}  // namespace

extern "C" int64_t svl_pl_stats_pass_pixels(void) { return (int64_t)PLS_MAX_GRID * 256 * 2; }

extern "C" int svl_pl_stats_i64(const int64_t* mask_w, const float* conf, const int64_t* ign, const int64_t* mc,
                                const int64_t* gt, int64_t n, int N, int bins, float thresh, int64_t* stats,
                                svl_stream_t stream) {
  SVL_CHECK_ARG(mask_w && conf && ign && stats, "svl_pl_stats_i64: null pointer (mask_w, conf, ign and stats are required)");
  SVL_CHECK_ARG(n >= 1, "svl_pl_stats_i64: n = %lld < 1", (long long)n);
  SVL_CHECK_ARG(N >= 1, "svl_pl_stats_i64: N = %d < 1", N);
  SVL_CHECK_ARG(bins >= 1, "svl_pl_stats_i64: bins = %d < 1", bins);
  const long T = (long)PLS_ROWS * N + 2L * bins;
  SVL_CHECK_ARG(T * (long)sizeof(unsigned int) <= 64L * 1024,
                "svl_pl_stats_i64: table of 13 x %d + 2 x %d counters does not fit 64 KB of LDS", N, bins);
  const bool vec = (((uintptr_t)mask_w | (uintptr_t)ign | (uintptr_t)mc | (uintptr_t)gt) % 16 == 0) && ((uintptr_t)conf % 8 == 0);
  const int V = vec ? 2 : 1;
  const long nq = (n + V - 1) / V;
  long grid = (nq + 255) / 256;
  if (grid > PLS_MAX_GRID) grid = PLS_MAX_GRID;
  // the block-private counters are 32 bits wide: a block makes ceil(nq / (grid * 256)) trips of 256 * V pixels
  const long trips = (nq + grid * 256 - 1) / (grid * 256);
  SVL_CHECK_ARG(trips < (1L << 32) / (256 * V),
                "svl_pl_stats_i64: n = %lld too large: a block of the capped grid would see 2^32 pixels", (long long)n);
  auto* out = reinterpret_cast<unsigned long long*>(stats);
  const size_t lds = (size_t)T * sizeof(unsigned int);
  if (vec)
    hipLaunchKernelGGL(pl_stats_kernel<2>, dim3((unsigned)grid), dim3(256), lds, (hipStream_t)stream, mask_w, conf, ign, mc,
                       gt, (long)n, N, bins, thresh, out);
  else
    hipLaunchKernelGGL(pl_stats_kernel<1>, dim3((unsigned)grid), dim3(256), lds, (hipStream_t)stream, mask_w, conf, ign, mc,
                       gt, (long)n, N, bins, thresh, out);
  SVL_LAUNCH_CHECK("svl_pl_stats_i64");
  return SVL_OK;
}

extern "C" int svl_pl_add_losses(const float* losses, int k, double* sum, int64_t* steps, svl_stream_t stream) {
  SVL_CHECK_ARG(losses && sum && steps && k >= 1 && k <= 64, "svl_pl_add_losses: bad args");
  hipLaunchKernelGGL(pl_add_losses_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, losses, k, sum, steps);
  SVL_LAUNCH_CHECK("svl_pl_add_losses");
  return SVL_OK;
}
