// Gradient-norm clipping over the flat gradient arena (torch.nn.utils.clip_grad_norm_ semantics, which is what mmcv's
// OptimizerHook(grad_clip=...) calls; semivl.py itself does not clip).  The arena's padding is zero, so the norm over all of
// the optimizer's tensors is ONE read of `g`: 4 B per parameter.  Two launches, no atomics, a fixed order of every addition:
//   stage 1  every block streams its trips of the arena, a lane keeps its squares (L2) in double or its largest magnitude
//            (max norm, with a NaN flag: fmax would drop it); wave by cross-lane shuffles, block through LDS, ONE double per
//            block into `ws`.  Which lane reads which element depends on `total` alone (not on the alignment of g);
//   stage 2  one block folds the partials in a fixed order and writes {norm, coef, gscale * coef, non-finite flag}.
// The step kernels read stats[2] from the device (svl_adamw_step_dscale / svl_sgd_step_dscale, optim.hip): no host sync.
#include <math.h>

#include "svl_common.h"

namespace {

constexpr int GC_THREADS = 256;
constexpr int GC_TRIP = GC_THREADS * 4;   // floats per block and trip: one 16-byte load per lane
constexpr long GC_GRID_CAP = 1024;        // 256 CUs x 4 blocks; longer arenas take further trips
constexpr int GC_FINAL_THREADS = 256;

long gc_grid(long total) {
  long grid = (total + GC_TRIP - 1) / GC_TRIP;
  return grid > GC_GRID_CAP ? GC_GRID_CAP : grid;
}

// MAXN = false: a + b.  MAXN = true: the larger, a NaN on either side wins (fmax alone returns the other operand).
template <bool MAXN>
__device__ __forceinline__ double gc_fold(double a, double b) {
  if (!MAXN) return a + b;
  return (a != a || b != b) ? __builtin_nan("") : fmax(a, b);
}

template <bool MAXN>
__device__ __forceinline__ double gc_wave_fold(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = gc_fold<MAXN>(v, __shfl_xor(v, o, 64));
  return v;
}

// Block-wide fold for 256 threads; the result is valid in thread 0.  `red` holds 4 doubles.
template <bool MAXN>
__device__ __forceinline__ double gc_block_fold(double v, double* red) {
  v = gc_wave_fold<MAXN>(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return gc_fold<MAXN>(gc_fold<MAXN>(red[0], red[1]), gc_fold<MAXN>(red[2], red[3]));
}

template <bool MAXN, bool VEC>
__global__ __launch_bounds__(GC_THREADS) void grad_norm_partial_kernel(const float* __restrict__ g, long total,
                                                                       double* __restrict__ ws) {
  __shared__ double red[4];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;   // L2: one chain per float4 component
  float mx = 0.f;                                  // max norm: |g| is exact in fp32
  bool nan = false;
#pragma unroll 4
  for (long base = (long)blockIdx.x * GC_TRIP; base < total; base += (long)gridDim.x * GC_TRIP) {
    const long i = base + (long)threadIdx.x * 4;
    if (i + 4 <= total) {
      float4 x;
      if (VEC) {
        x = *reinterpret_cast<const float4*>(g + i);
      } else {
        x.x = g[i]; x.y = g[i + 1]; x.z = g[i + 2]; x.w = g[i + 3];
      }
      if (MAXN) {
        nan = nan || x.x != x.x || x.y != x.y || x.z != x.z || x.w != x.w;
        mx = fmaxf(fmaxf(mx, fmaxf(fabsf(x.x), fabsf(x.y))), fmaxf(fabsf(x.z), fabsf(x.w)));
      } else {
        s0 = fma((double)x.x, (double)x.x, s0);
        s1 = fma((double)x.y, (double)x.y, s1);
        s2 = fma((double)x.z, (double)x.z, s2);
        s3 = fma((double)x.w, (double)x.w, s3);
      }
    } else {  // the last total % 4 elements
      for (long j = i; j < total; ++j) {
        const float x = g[j];
        if (MAXN) {
          nan = nan || x != x;
          mx = fmaxf(mx, fabsf(x));
        } else {
          s0 = fma((double)x, (double)x, s0);
        }
      }
    }
  }
  double v = MAXN ? (nan ? __builtin_nan("") : (double)mx) : (s0 + s1) + (s2 + s3);
  v = gc_block_fold<MAXN>(v, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = v;
}

template <bool MAXN>
__global__ __launch_bounds__(GC_FINAL_THREADS) void grad_norm_final_kernel(const double* __restrict__ ws, int parts,
                                                                           float gscale, float max_norm,
                                                                           float* __restrict__ stats) {
  __shared__ double red[4];
  double v = 0.0;
  for (int k = threadIdx.x; k < parts; k += GC_FINAL_THREADS) v = gc_fold<MAXN>(v, ws[k]);
  v = gc_block_fold<MAXN>(v, red);
  if (threadIdx.x == 0) {
    const double norm = (double)gscale * (MAXN ? v : sqrt(v));
    double coef = (double)max_norm / (norm + 1e-6);
    if (coef > 1.0) coef = 1.0;   // torch.clamp(max=1): a NaN stays a NaN
    stats[0] = (float)norm;
    stats[1] = (float)coef;
    stats[2] = (float)((double)gscale * coef);
    // (not `norm - norm == 0`: contracted with the product above that is an fma's remainder, non-zero for a finite norm)
    stats[3] = __builtin_isfinite(norm) ? 0.f : 1.f;
  }
}

template <bool MAXN>
void gc_launch(const float* g, long total, long grid, float gscale, float max_norm, double* ws, float* stats,
               hipStream_t st) {
  if ((((uintptr_t)g) & 15) == 0)
    hipLaunchKernelGGL((grad_norm_partial_kernel<MAXN, true>), dim3((unsigned)grid), dim3(GC_THREADS), 0, st, g, total,
                       ws);
  else
    hipLaunchKernelGGL((grad_norm_partial_kernel<MAXN, false>), dim3((unsigned)grid), dim3(GC_THREADS), 0, st, g, total,
                       ws);
  hipLaunchKernelGGL((grad_norm_final_kernel<MAXN>), dim3(1), dim3(GC_FINAL_THREADS), 0, st, (const double*)ws,
                     (int)grid, gscale, max_norm, stats);
}

}  // namespace

extern "C" int64_t svl_grad_clip_ws_doubles(int64_t total) { return total > 0 ? gc_grid((long)total) : 0; }

extern "C" int svl_grad_clip_f32(const float* g, int64_t total, int norm_kind, float gscale, float max_norm, double* ws,
                                 float* stats, svl_stream_t stream) {
  SVL_CHECK_ARG(g && ws && stats && total > 0, "svl_grad_clip_f32: bad args (null pointer or total <= 0)");
  SVL_CHECK_ARG((((uintptr_t)g | (uintptr_t)stats) & 3) == 0 && (((uintptr_t)ws) & 7) == 0,
                "svl_grad_clip_f32: g and stats must be 4-byte aligned, ws 8-byte aligned");
  SVL_CHECK_ARG(norm_kind == 0 || norm_kind == 1, "svl_grad_clip_f32: norm_kind %d (0 = L2, 1 = max norm)", norm_kind);
  SVL_CHECK_ARG(gscale > 0.f && isfinite(gscale), "svl_grad_clip_f32: gscale %g must be positive and finite",
                (double)gscale);
  SVL_CHECK_ARG(max_norm > 0.f, "svl_grad_clip_f32: max_norm %g must be positive (+inf only reports the norm)",
                (double)max_norm);
  const long grid = gc_grid((long)total);
  if (norm_kind == 0) gc_launch<false>(g, (long)total, grid, gscale, max_norm, ws, stats, (hipStream_t)stream);
  else gc_launch<true>(g, (long)total, grid, gscale, max_norm, ws, stats, (hipStream_t)stream);
  SVL_LAUNCH_CHECK("svl_grad_clip_f32");
  return SVL_OK;
}
