// Confusion table of the evaluation report (semivl_amd/report.py): ONE pass over the prediction and annotation maps adds 1 at
// table[r][c] of an int64 [(K+1) x (K+1)] table for every pixel whose annotation is not the ignore index (semivl_hip.h).
// Shape of pl_stats.hip: block-private 32-bit counters in LDS, flushed with 64-bit integer atomics -- integer sums do not
// depend on the order, so two runs agree bit for bit.  Above svl_confusion_lds_max_classes() classes the table has no LDS
// copy and the same wave aggregation goes straight into 64-bit global atomics.
//
// Label maps are spatially coherent: the 64 lanes of a wave usually carry ONE (annotation, prediction) pair, and 64 atomics
// on one address serialise.  So a wave aggregates on the pair key r (K+1) + c before it touches the table: it ballots on the
// key of its first pending lane and counts the lanes that share it, for at most CF_PEEL distinct keys; lanes still pending
// after that (a noisy map: many keys per wave, so little contention each) add their own ones.  The counted lanes are not
// added at once either: the wave keeps ONE open run (key, count) in scalar registers over its trips and adds it when the key
// changes, so a one-class map costs one atomic per wave and flush, not one per trip.
//
// Both keys are formed (clamped to [0, K]) before anything is indexed with them: a raw label is never an address.
#include "svl_common.h"
#include <atomic>

namespace {

constexpr int CF_MAX_GRID = 2048;    // 256 CUs x 8 blocks, the rest is grid-strided
constexpr int CF_PEEL = 4;
constexpr int CF_MAX_K = 1024;
constexpr int CF_LDS_HW_MAX_K = 201;        // (201 + 1)^2 x 4 B = 163216 B <= 160 KB of LDS; 203^2 x 4 B is beyond it
// Measured (README "Evaluation report", profiles/confusion_times.json): at every K that fits, the LDS form's slowest map (a
// random one) takes 50 - 84 us for 16 x 512^2 pixels where the global form takes 300 - 1600 us; the global form is ahead
// only on piecewise-constant maps from K = 150 on (36 against 58 - 64 us).  So the boundary is the hardware's.
constexpr int CF_LDS_DEFAULT_MAX_K = CF_LDS_HW_MAX_K;
// 32-bit counters (LDS table, the waves' open runs) are flushed every CF_FLUSH_TRIPS trips of a block: a trip is at most
// 256 threads x 2 pixels = 2^9 pixels, so a counter holds at most 2^22 x 2^9 = 2^31 < 2^32 between two flushes.
constexpr long CF_FLUSH_TRIPS = 1L << 22;

typedef long long i64x2 __attribute__((ext_vector_type(2)));

std::atomic<int> g_lds_max_k{CF_LDS_DEFAULT_MAX_K};

template <typename CT>
__device__ __forceinline__ void run_flush(CT* tab, int key, unsigned int cnt) {
  if (cnt && (threadIdx.x & 63) == 0) atomicAdd(&tab[key], (CT)cnt);
}

// Counts the lanes with `valid` at tab[key].  Must be reached by all 64 lanes of the wave (ballots); run_key / run_cnt are
// wave-uniform.
template <typename CT>
__device__ __forceinline__ void wave_count(CT* tab, int key, bool valid, int& run_key, unsigned int& run_cnt) {
  const int lane = threadIdx.x & 63;
  unsigned long long rem = __ballot(valid);
  for (int it = 0; it < CF_PEEL && rem; ++it) {
    const int c = __builtin_amdgcn_readlane(key, __ffsll((long long)rem) - 1);
    const unsigned long long same = __ballot(valid && key == c);
    if (c != run_key) {
      run_flush(tab, run_key, run_cnt);
      run_key = c;
      run_cnt = 0;
    }
    run_cnt += (unsigned int)__popcll(same);
    rem &= ~same;
  }
  if ((rem >> lane) & 1ull) atomicAdd(&tab[key], (CT)1);
}

// CT = unsigned int: the table's block-private copy in LDS; CT = unsigned long long: the global table itself.
// V = 2: every thread reads two neighbouring pixels with 16-byte loads (both pointers 16-byte aligned).
template <int V, typename CT>
__global__ __launch_bounds__(256) void confusion_kernel(const int64_t* __restrict__ pred, const int64_t* __restrict__ tgt,
                                                        long n, int K, long ignore, unsigned long long* table) {
  extern __shared__ unsigned int sh[];  // [(K+1)^2] with CT = unsigned int, nothing otherwise
  constexpr bool LDS = sizeof(CT) == 4;
  const int S = K + 1, T = S * S;
  CT* tab;
  if constexpr (LDS) {
    for (int i = threadIdx.x; i < T; i += 256) sh[i] = 0;
    __syncthreads();
    tab = sh;
  } else {
    tab = table;
  }
  int run_key = 0;
  unsigned int run_cnt = 0;
  long trip = 0;
  const long nq = (n + V - 1) / V;
  // (q0 and trip are the same in every thread of the block: all lanes make the same trips and reach every ballot and barrier)
  for (long q0 = (long)blockIdx.x * 256; q0 < nq; q0 += (long)gridDim.x * 256) {
    const long i0 = (q0 + threadIdx.x) * V;
    long p_[V], t_[V];
    bool in_[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      in_[e] = i0 + e < n;
      p_[e] = 0; t_[e] = 0;
    }
    if (V == 2 && i0 + 1 < n) {
      const i64x2 a = *reinterpret_cast<const i64x2*>(pred + i0);
      const i64x2 b = *reinterpret_cast<const i64x2*>(tgt + i0);
      p_[0] = a.x; p_[V - 1] = a.y; t_[0] = b.x; t_[V - 1] = b.y;
    } else if (in_[0]) {   // V == 1, or the last pixel of an odd n
      p_[0] = pred[i0]; t_[0] = tgt[i0];
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const long p = p_[e], t = t_[e];
      const bool valid = in_[e] && t != ignore;
      const int r = (t >= 0 && t < K) ? (int)t : K;
      const int c = (p >= 0 && p < K) ? (int)p : K;
      wave_count<CT>(tab, valid ? r * S + c : 0, valid, run_key, run_cnt);
    }
    if (++trip == CF_FLUSH_TRIPS) {
      trip = 0;
      run_flush<CT>(tab, run_key, run_cnt);
      run_cnt = 0;
      if constexpr (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < T; i += 256)
          if (sh[i]) { atomicAdd(&table[i], (unsigned long long)sh[i]); sh[i] = 0; }
        __syncthreads();
      }
    }
  }
  run_flush<CT>(tab, run_key, run_cnt);
  if constexpr (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < T; i += 256)
      if (sh[i]) atomicAdd(&table[i], (unsigned long long)sh[i]);
  }
}

// out[i] = (uint8_t)label[i].  VEC: a thread converts 8 labels, four 16-byte loads and one 8-byte store; the n % 8 labels
// of the tail, and everything on unaligned pointers, go one by one.
template <bool VEC>
__global__ __launch_bounds__(256) void label_u8_kernel(const int64_t* __restrict__ label, long n, uint8_t* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
  if (VEC) {
    const long n8 = n / 8;
    for (long g = i; g < n8; g += step) {
      const i64x2* src = reinterpret_cast<const i64x2*>(label + g * 8);
      unsigned long long w = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const i64x2 v = src[j];
        w |= ((unsigned long long)v.x & 0xffull) << (16 * j);
        w |= ((unsigned long long)v.y & 0xffull) << (16 * j + 8);
      }
      *reinterpret_cast<unsigned long long*>(out + g * 8) = w;
    }
    for (long k = n8 * 8 + i; k < n; k += step) out[k] = (uint8_t)label[k];
  } else {
    for (long k = i; k < n; k += step) out[k] = (uint8_t)label[k];
  }
}

}  // namespace

extern "C" int svl_confusion_lds_max_classes(void) { return g_lds_max_k.load(std::memory_order_relaxed); }

extern "C" int svl_set_confusion_lds_max_classes(int K) {
  SVL_CHECK_ARG(K <= CF_LDS_HW_MAX_K, "svl_set_confusion_lds_max_classes: K = %d > %d: (K + 1)^2 counters do not fit 160 KB of LDS",
                K, CF_LDS_HW_MAX_K);
  g_lds_max_k.store(K < 0 ? CF_LDS_DEFAULT_MAX_K : K, std::memory_order_relaxed);
  return SVL_OK;
}

extern "C" int svl_confusion_i64(const int64_t* pred, const int64_t* target, int64_t n, int K, int ignore_index,
                                 int64_t* table, svl_stream_t stream) {
  SVL_CHECK_ARG(pred && target && table, "svl_confusion_i64: null pointer");
  SVL_CHECK_ARG(n >= 1, "svl_confusion_i64: n = %lld < 1", (long long)n);
  SVL_CHECK_ARG(K >= 1 && K <= CF_MAX_K, "svl_confusion_i64: K = %d outside [1, %d]", K, CF_MAX_K);
  SVL_CHECK_ARG(ignore_index < 0 || ignore_index >= K,
                "svl_confusion_i64: ignore_index = %d is a class (K = %d): an ignored class is not counted as a hit", ignore_index, K);
  const bool lds_tab = K <= g_lds_max_k.load(std::memory_order_relaxed);
  const size_t lds = lds_tab ? (size_t)(K + 1) * (K + 1) * sizeof(unsigned int) : 0;
  const bool vec = ((uintptr_t)pred | (uintptr_t)target) % 16 == 0;
  const int V = vec ? 2 : 1;
  const long nq = (n + V - 1) / V;
  // blocks per CU that the LDS table leaves room for (160 KB per CU, 8 at the most); above 64 KB that is one
  long per_cu = lds ? (160L * 1024) / (long)(lds + 256) : 8;
  per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);
  long grid = (nq + 255) / 256;
  if (grid > 256 * per_cu) grid = 256 * per_cu;
  if (grid > CF_MAX_GRID) grid = CF_MAX_GRID;
  auto* out = reinterpret_cast<unsigned long long*>(table);
  auto launch = [&](auto kern) -> int {
    if (lds > 64 * 1024)   // idempotent per-device attribute: set on every call that needs it (cheap host call)
      SVL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, (hipStream_t)stream, pred, target, (long)n, K,
                       (long)ignore_index, out);
    SVL_LAUNCH_CHECK("svl_confusion_i64");
    return SVL_OK;
  };
  if (lds_tab) return vec ? launch(confusion_kernel<2, unsigned int>) : launch(confusion_kernel<1, unsigned int>);
  return vec ? launch(confusion_kernel<2, unsigned long long>) : launch(confusion_kernel<1, unsigned long long>);
}

extern "C" int svl_label_u8_i64(const int64_t* label, int64_t n, uint8_t* out, svl_stream_t stream) {
  SVL_CHECK_ARG(label && out, "svl_label_u8_i64: null pointer");
  SVL_CHECK_ARG(n >= 1, "svl_label_u8_i64: n = %lld < 1", (long long)n);
  const bool vec = (uintptr_t)label % 16 == 0 && (uintptr_t)out % 8 == 0;
  long grid = ((vec ? (n + 7) / 8 : n) + 255) / 256;
  if (grid > CF_MAX_GRID) grid = CF_MAX_GRID;
  if (vec)
    hipLaunchKernelGGL(label_u8_kernel<true>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, label, (long)n, out);
  else
    hipLaunchKernelGGL(label_u8_kernel<false>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, label, (long)n, out);
  SVL_LAUNCH_CHECK("svl_label_u8_i64");
  return SVL_OK;
}
