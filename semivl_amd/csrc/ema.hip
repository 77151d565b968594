// The mean teacher's buffer pass (semivl_amd/ema.py): dst[s] = decay * dst[s] + (1 - decay) * src[s] over a table of
// independent segments -- the BatchNorm running statistics of the teacher against the student's.  The parameters' average
// is NOT formed here: it lives in the optimizer's EMA arena and is updated by the step kernels (optim.hip).  The workload
// is a few dozen to a few hundred segments of 48 - 2048 floats: ONE launch, latency-bound, one block per segment with a
// capped grid (a block takes segments blockIdx.x, blockIdx.x + gridDim.x, ...).  One owner per element, no atomics.
#include "svl_common.h"

namespace {

constexpr int EMA_THREADS = 256;
constexpr int EMA_GRID_CAP = 256;   // one block per CU; more segments take further trips

// decay * d + omd * s with the roundings pinned: the product omd * s is rounded, then ONE fused multiply-add.  Left to the
// compiler's contraction the 16-byte and the scalar path fused different products and differed in the last bit.
__device__ __forceinline__ float ema_elem(float d, float s, float decay, float omd) {
  return __fmaf_rn(decay, d, __fmul_rn(omd, s));
}

__global__ __launch_bounds__(EMA_THREADS) void ema_segments_kernel(float* const* __restrict__ dst,
                                                                   const float* const* __restrict__ src,
                                                                   const long long* __restrict__ seg_off, int nseg,
                                                                   float decay, float omd) {
  for (int s = blockIdx.x; s < nseg; s += gridDim.x) {
    const long n = (long)(seg_off[s + 1] - seg_off[s]);
    float* d = dst[s];
    const float* x = src[s];
    if (n <= 0 || d == nullptr || x == nullptr) continue;   // (block-uniform)
    long done = 0;
    if ((((uintptr_t)d | (uintptr_t)x) & 15) == 0) {
      const long n4 = n >> 2;
      for (long q = threadIdx.x; q < n4; q += EMA_THREADS) {
        float4 dv = reinterpret_cast<const float4*>(d)[q];
        const float4 sv = reinterpret_cast<const float4*>(x)[q];
        dv.x = ema_elem(dv.x, sv.x, decay, omd);
        dv.y = ema_elem(dv.y, sv.y, decay, omd);
        dv.z = ema_elem(dv.z, sv.z, decay, omd);
        dv.w = ema_elem(dv.w, sv.w, decay, omd);
        reinterpret_cast<float4*>(d)[q] = dv;
      }
      done = n4 << 2;   // the last n % 4 elements go the scalar way
    }
    for (long i = done + threadIdx.x; i < n; i += EMA_THREADS) d[i] = ema_elem(d[i], x[i], decay, omd);
  }
}

}  // namespace

extern "C" int svl_ema_segments_f32(float* const* dst, const float* const* src, const int64_t* seg_off, int nseg,
                                    float decay, svl_stream_t stream) {
  SVL_CHECK_ARG(nseg >= 0, "svl_ema_segments_f32: nseg %d is negative", nseg);
  if (nseg == 0) return SVL_OK;
  SVL_CHECK_ARG(dst && src && seg_off, "svl_ema_segments_f32: null table (dst, src or seg_off)");
  SVL_CHECK_ARG((const void*)dst != (const void*)src,
                "svl_ema_segments_f32: dst == src: a segment must not be averaged with itself");
  SVL_CHECK_ARG(decay >= 0.f && decay <= 1.f, "svl_ema_segments_f32: decay %g is outside [0, 1]", (double)decay);
  const float omd = (float)(1.0 - (double)decay);   // as svl_sgd_step forms ema_omd
  const int grid = nseg < EMA_GRID_CAP ? nseg : EMA_GRID_CAP;
  hipLaunchKernelGGL(ema_segments_kernel, dim3((unsigned)grid), dim3(EMA_THREADS), 0, (hipStream_t)stream, dst, src,
                     (const long long*)seg_off, nseg, decay, omd);
  SVL_LAUNCH_CHECK("svl_ema_segments_f32");
  return SVL_OK;
}
