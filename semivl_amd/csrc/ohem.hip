// OHEM pixel selection (third_party/unimatch/util/ohem.py: ProbOhemCrossEntropy2d), without a host synchronisation.
//
// The criterion keeps a labelled pixel when its target-class probability p is <= a threshold: the k-th smallest p over
// ALL B*H*W pixels (invalid ones count as 1.0) when that exceeds `thresh`, else `thresh`.  Three kernels:
//   target_prob_kernel   p [B, H, W] from full-resolution logits (the head-resolution form is in pixel_loss_up.hip);
//   radix select         the exact k-th smallest p: p lies in [0, 1], so its fp32 bit patterns order like uint32.  Three
//                        digit passes (bits 31..21, 20..10, 9..0) each count the elements that match the digits chosen
//                        so far into an LDS histogram, flushed to global memory with one integer atomic per non-empty bin
//                        and block; the next pass (and the last, single-block kernel) re-derives the chosen digits from
//                        the finished histograms itself, so no separate selection launch exists.  Integer counts: the
//                        result is exact and does not depend on the order of the atomics;
//   relabel_kernel       target where valid and p <= threshold, else 255, + the kept count.
#include "svl_common.h"

namespace {

constexpr int NT = 256;
constexpr int NBINS = 2048;                    // the widest digit (11 bits)
constexpr int DIG_BITS[3] = {11, 11, 10};
constexpr int DIG_SHIFT[3] = {21, 10, 0};

struct OhemWs {
  unsigned hist[3][NBINS];                     // one histogram per digit pass (zeroed by ohem_init_kernel)
};

__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The digits of passes [0, npass) of the k-th smallest element and its rank among the elements that share them.
// Every thread of the block gets (prefix, rank).  rank is 1-based; the caller guarantees 1 <= k <= n.
__device__ void descend(const OhemWs* ws, int npass, unsigned k, unsigned& prefix, unsigned& rank) {
  __shared__ unsigned wsum[NT / 64];
  __shared__ unsigned sel[2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  prefix = 0;
  rank = k;
  for (int j = 0; j < npass; ++j) {
    const int nb = 1 << DIG_BITS[j], per = nb / NT;   // 8 or 4 consecutive bins per thread
    const unsigned* h = ws->hist[j];
    unsigned mine = 0;
    for (int i = 0; i < per; ++i) mine += h[tid * per + i];
    // inclusive scan of the per-thread sums: inside the wave, then across the four waves
    unsigned inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned v = __shfl_up(inc, o, 64);
      if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    for (int w = 0; w < wv; ++w) inc += wsum[w];
    const unsigned exc = inc - mine;
    if (exc < rank && rank <= inc) {                  // exactly one thread holds the rank
      unsigned c = exc;
      int d = tid * per;
      for (int i = 0; i < per; ++i, ++d) {
        const unsigned hv = h[d];
        if (rank <= c + hv) break;
        c += hv;
      }
      sel[0] = prefix | ((unsigned)d << DIG_SHIFT[j]);
      sel[1] = rank - c;
    }
    __syncthreads();
    prefix = sel[0];
    rank = sel[1];
    __syncthreads();                                  // (wsum / sel are reused by the next pass)
  }
}

__global__ __launch_bounds__(NT) void ohem_init_kernel(OhemWs* ws) {
  unsigned* h = &ws->hist[0][0];
  for (int i = threadIdx.x; i < 3 * NBINS; i += NT) h[i] = 0u;
}

// Digit pass j: histogram of digit j over the elements whose higher digits equal those already chosen.
template <int J>
__global__ __launch_bounds__(NT) void ohem_hist_kernel(const float* __restrict__ p, long n, unsigned k, OhemWs* ws) {
  __shared__ unsigned lh[NBINS];
  constexpr int NB = 1 << DIG_BITS[J], SH = DIG_SHIFT[J];
  constexpr unsigned HI = (SH + DIG_BITS[J] >= 32) ? 0u : ~((1u << (SH + DIG_BITS[J])) - 1u);   // bits already chosen
  for (int i = threadIdx.x; i < NB; i += NT) lh[i] = 0u;
  unsigned prefix = 0, rank = 0;
  if (J > 0) descend(ws, J, k, prefix, rank);
  __syncthreads();
  const unsigned* u = reinterpret_cast<const unsigned*>(p);
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * NT;
  for (long q = (long)blockIdx.x * NT + threadIdx.x; q < n4; q += stride) {
    const uint4 v = reinterpret_cast<const uint4*>(u)[q];
    const unsigned e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if ((e[i] & HI) == prefix) atomicAdd(&lh[(e[i] >> SH) & (NB - 1)], 1u);
  }
  for (long i = (n4 << 2) + (long)blockIdx.x * NT + threadIdx.x; i < n; i += stride) {   // (the n % 4 tail)
    const unsigned e = u[i];
    if ((e & HI) == prefix) atomicAdd(&lh[(e >> SH) & (NB - 1)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NB; i += NT) {
    const unsigned c = lh[i];
    if (c) atomicAdd(&ws->hist[J][i], c);
  }
}

// The effective threshold of ohem.py:39-52 (+inf: every valid pixel is kept).
__global__ __launch_bounds__(NT) void ohem_threshold_kernel(const OhemWs* ws, unsigned k, const int64_t* num_valid,
                                                            long min_kept, float thresh, float* threshold) {
  const long nv = *num_valid;
  unsigned prefix = 0, rank = 0;
  const bool sel = k > 0 && min_kept <= nv && nv > 0;   // (block-uniform)
  if (sel) descend(ws, 3, k, prefix, rank);
  if (threadIdx.x == 0) {
    float t = INFINITY;                          // min_kept > num_valid, num_valid == 0, or min_kept == 0: nothing dropped
    if (sel) {
      const float v = __uint_as_float(prefix);
      t = v > thresh ? v : thresh;
    }
    threshold[0] = t;
  }
}

__global__ __launch_bounds__(256) void target_prob_kernel(const float* __restrict__ logits, int B, int N, long HW,
                                                          const int64_t* __restrict__ target, float* __restrict__ prob) {
  const long total = (long)B * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long t = target[i];
    float pr = 1.f;
    if (t != 255) {
      const long b = i / HW, q = i - b * HW;
      const float* x = logits + b * N * HW + q;
      // ce_fused_kernel's arithmetic (N <= 64: one thread per pixel there): max, then sum of expf(x - max) in class order;
      // p = expf(x_t - max) * (1 / sum) is its gradient's softmax term for the target class
      float m = -INFINITY;
      for (int c = 0; c < N; ++c) m = fmaxf(m, x[(long)c * HW]);
      float s = 0.f;
      for (int c = 0; c < N; ++c) s += expf(x[(long)c * HW] - m);
      pr = (t >= 0 && t < N) ? expf(x[t * HW] - m) * (1.f / s) : 1.f;
    }
    prob[i] = pr;
  }
}

__global__ __launch_bounds__(256) void relabel_kernel(const int64_t* __restrict__ target, const float* __restrict__ prob,
                                                      long n, const float* __restrict__ threshold, int64_t* __restrict__ out,
                                                      unsigned long long* count) {
  __shared__ unsigned red[4];
  const float thr = threshold[0];
  unsigned kept = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long t = target[i];
    const bool keep = t != 255 && prob[i] <= thr;
    out[i] = keep ? t : 255;
    kept += keep ? 1u : 0u;
  }
  if (!count) return;
  kept = wave_sum_u(kept);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = kept;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned tot = red[0] + red[1] + red[2] + red[3];
    if (tot) atomicAdd(count, (unsigned long long)tot);
  }
}

inline unsigned grid_cap(long n, long per_block, unsigned cap) {
  const long g = (n + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace

extern "C" int64_t svl_ohem_ws_bytes(int64_t n) { return n > 0 ? (int64_t)sizeof(OhemWs) : -1; }

extern "C" int svl_target_prob_f32(const float* logits, int B, int N, int64_t HW, const int64_t* target, float* prob,
                                   svl_stream_t stream) {
  SVL_CHECK_ARG(logits && target && prob && B > 0 && N > 0 && HW > 0, "svl_target_prob_f32: bad args");
  hipLaunchKernelGGL(target_prob_kernel, dim3(grid_cap((long)B * HW, 256, 4096)), dim3(256), 0, (hipStream_t)stream, logits,
                     B, N, (long)HW, target, prob);
  SVL_LAUNCH_CHECK("svl_target_prob_f32");
  return SVL_OK;
}

extern "C" int svl_ohem_threshold_f32(const float* prob, int64_t n, int64_t k, const int64_t* num_valid, int64_t min_kept,
                                      float thresh, void* ws, float* threshold, svl_stream_t stream) {
  SVL_CHECK_ARG(prob && num_valid && ws && threshold && n > 0, "svl_ohem_threshold_f32: bad args");
  SVL_CHECK_ARG(n <= 0x7fffffffLL, "svl_ohem_threshold_f32: n = %lld exceeds 2^31 - 1", (long long)n);
  SVL_CHECK_ARG(k >= 0 && k <= n && min_kept >= 0, "svl_ohem_threshold_f32: k = %lld outside [0, n]", (long long)k);
  SVL_CHECK_ARG(((uintptr_t)prob & 15) == 0, "svl_ohem_threshold_f32: prob must be 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  OhemWs* w = reinterpret_cast<OhemWs*>(ws);
  if (k > 0) {
    // ~64 elements per thread: a few hundred blocks, each flushing at most one atomic per non-empty bin
    const unsigned g = grid_cap(n, 256L * 64, 1024);
    hipLaunchKernelGGL(ohem_init_kernel, dim3(1), dim3(NT), 0, st, w);
    hipLaunchKernelGGL(ohem_hist_kernel<0>, dim3(g), dim3(NT), 0, st, prob, (long)n, (unsigned)k, w);
    hipLaunchKernelGGL(ohem_hist_kernel<1>, dim3(g), dim3(NT), 0, st, prob, (long)n, (unsigned)k, w);
    hipLaunchKernelGGL(ohem_hist_kernel<2>, dim3(g), dim3(NT), 0, st, prob, (long)n, (unsigned)k, w);
  }
  hipLaunchKernelGGL(ohem_threshold_kernel, dim3(1), dim3(NT), 0, st, w, (unsigned)k, num_valid, (long)min_kept, thresh,
                     threshold);
  SVL_LAUNCH_CHECK("svl_ohem_threshold_f32");
  return SVL_OK;
}

extern "C" int svl_ohem_relabel_i64(const int64_t* target, const float* prob, int64_t n, const float* threshold,
                                    int64_t* out, int64_t* count, svl_stream_t stream) {
  SVL_CHECK_ARG(target && prob && threshold && out && n > 0, "svl_ohem_relabel_i64: bad args");
  hipLaunchKernelGGL(relabel_kernel, dim3(grid_cap(n, 256L * 8, 2048)), dim3(256), 0, (hipStream_t)stream, target, prob,
                     (long)n, threshold, out, (unsigned long long*)count);
  SVL_LAUNCH_CHECK("svl_ohem_relabel_i64");
  return SVL_OK;
}
