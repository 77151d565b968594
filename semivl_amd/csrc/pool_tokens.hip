// Global average pooling and its broadcast on channels-last token slabs (gfx950): the image-pooling branch of the
// DeepLabV3+ ASPP (AdaptiveAvgPool2d(1) -> 1x1 conv -> BN -> ReLU -> resize of a 1 x 1 map = broadcast -> concat).
//   svl_gap_tokens_fwd   per-image column sum / mean, accumulated in double in a fixed order (no atomics)
//   svl_gap_tokens_bwd   dx (+)= dpool / HW
//   svl_bcast_rows_fwd   one row per image written into a channel slice of every pixel row of a wider slab
//   svl_bcast_rows_bwd   per-image column sum of that slice (the forward sum kernel without the division)
// Single passes over HBM; 16-byte accesses when C % 4 == 0 and strides / pointers allow it, scalar otherwise.
#include "svl_common.h"

namespace {

constexpr int POOL_GRID_CAP = 256 * 32;   // blocks of 256 threads per launch; the kernels loop beyond it
constexpr int GAP_CH = 64;                // channels one block of the column-sum kernel owns

inline int grid_for(long n) {
  long g = (n + 255) / 256;
  if (g < 1) g = 1;
  if (g > POOL_GRID_CAP) g = POOL_GRID_CAP;
  return (int)g;
}

// out[img * ldo + c] = (mean ? 1 / HW : 1) * sum_p x[(img * HW + p) * ldx + c].
// One work item = (image, 64-channel group), taken by one block: V channels per thread, 256 / (64 / V) row lanes that
// each sum rows lane, lane + LANES, ... in double, then one thread per channel adds the lanes' partial sums in lane order.
template <int V>
__global__ __launch_bounds__(256) void gap_sum_kernel(const float* __restrict__ x, long ldx, int imgs, long HW, int C,
                                                      float* __restrict__ out, long ldo, int mean) {
  constexpr int COLS = GAP_CH / V;        // threads across the channels of a group
  constexpr int LANES = 256 / COLS;       // row lanes
  __shared__ double red[LANES][GAP_CH];
  const int col = threadIdx.x % COLS, lane = threadIdx.x / COLS;
  const int groups = (C + GAP_CH - 1) / GAP_CH;
  const long items = (long)imgs * groups;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const long img = it / groups;
    const int c0 = (int)(it % groups) * GAP_CH + col * V;
    double acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.0;
    if (c0 < C) {                         // (V == 4: C % 4 == 0, so a quad is inside or outside as a whole)
      const float* p = x + img * HW * ldx + c0;
      for (long r = lane; r < HW; r += LANES) {
        if (V == 4) {
          const float4 v = *reinterpret_cast<const float4*>(p + r * ldx);
          acc[0] += (double)v.x; acc[1 % V] += (double)v.y; acc[2 % V] += (double)v.z; acc[3 % V] += (double)v.w;
        } else {
          acc[0] += (double)p[r * ldx];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) red[lane][col * V + k] = acc[k];
    __syncthreads();
    if (threadIdx.x < GAP_CH) {
      const int c = (int)(it % groups) * GAP_CH + threadIdx.x;
      if (c < C) {
        double s = 0.0;
        for (int l = 0; l < LANES; ++l) s += red[l][threadIdx.x];
        if (mean) s /= (double)HW;
        out[img * ldo + c] = (float)s;
      }
    }
    __syncthreads();
  }
}

// dst[(img * HW + p) * ldd + c] (=|+=) src[img * lds + c] [/ HW]
template <bool VEC, bool DIV>
__global__ __launch_bounds__(256) void bcast_kernel(const float* __restrict__ src, long lds, int imgs, long HW, int C,
                                                    float* __restrict__ dst, long ldd, int accumulate) {
  const int CQ = VEC ? (C >> 2) : C;
  const long total = (long)imgs * HW * CQ;
  const float hw = (float)HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % CQ) * (VEC ? 4 : 1);
    const long row = i / CQ;
    const long img = row / HW;
    if (VEC) {
      float4 v = *reinterpret_cast<const float4*>(src + img * lds + c);
      if (DIV) { v.x = __fdiv_rn(v.x, hw); v.y = __fdiv_rn(v.y, hw); v.z = __fdiv_rn(v.z, hw); v.w = __fdiv_rn(v.w, hw); }
      float4* d = reinterpret_cast<float4*>(dst + row * ldd + c);
      if (accumulate) {
        const float4 o = *d;
        v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
      }
      *d = v;
    } else {
      float v = src[img * lds + c];
      if (DIV) v = __fdiv_rn(v, hw);
      float* d = dst + row * ldd + c;
      *d = accumulate ? *d + v : v;
    }
  }
}

inline bool aligned16(const void* a, const void* b) { return ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0; }

int launch_gap_sum(const char* name, const float* x, int64_t ldx, int imgs, int64_t HW, int C, float* out, int64_t ldo,
                   int mean, svl_stream_t stream) {
  SVL_CHECK_ARG(x && out && imgs > 0 && HW > 0 && C > 0 && ldx >= C && ldo >= C, "%s: bad args", name);
  const long items = (long)imgs * ((C + GAP_CH - 1) / GAP_CH);
  const int grid = (int)(items < POOL_GRID_CAP ? items : POOL_GRID_CAP);
  if (C % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)x & 15) == 0)
    hipLaunchKernelGGL(gap_sum_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, imgs, (long)HW, C, out,
                       (long)ldo, mean);
  else
    hipLaunchKernelGGL(gap_sum_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, imgs, (long)HW, C, out,
                       (long)ldo, mean);
  SVL_LAUNCH_CHECK(name);
  return SVL_OK;
}

template <bool DIV>
int launch_bcast(const char* name, const float* src, int64_t lds, int imgs, int64_t HW, int C, float* dst, int64_t ldd,
                 int accumulate, svl_stream_t stream) {
  SVL_CHECK_ARG(src && dst && imgs > 0 && HW > 0 && C > 0 && lds >= C && ldd >= C, "%s: bad args", name);
  if (C % 4 == 0 && lds % 4 == 0 && ldd % 4 == 0 && aligned16(src, dst))
    hipLaunchKernelGGL((bcast_kernel<true, DIV>), dim3(grid_for((long)imgs * HW * (C / 4))), dim3(256), 0, (hipStream_t)stream,
                       src, (long)lds, imgs, (long)HW, C, dst, (long)ldd, accumulate);
  else
    hipLaunchKernelGGL((bcast_kernel<false, DIV>), dim3(grid_for((long)imgs * HW * C)), dim3(256), 0, (hipStream_t)stream, src,
                       (long)lds, imgs, (long)HW, C, dst, (long)ldd, accumulate);
  SVL_LAUNCH_CHECK(name);
  return SVL_OK;
}

}  // namespace

extern "C" int svl_gap_tokens_fwd(const float* x, int64_t ldx, int imgs, int64_t HW, int C, float* pool, int64_t ldp,
                                  svl_stream_t stream) {
  return launch_gap_sum("svl_gap_tokens_fwd", x, ldx, imgs, HW, C, pool, ldp, 1, stream);
}

extern "C" int svl_gap_tokens_bwd(const float* dpool, int64_t ldp, int imgs, int64_t HW, int C, float* dx, int64_t lddx,
                                  int accumulate, svl_stream_t stream) {
  SVL_CHECK_ARG(HW < (1L << 24), "svl_gap_tokens_bwd: HW must be exact in fp32");
  return launch_bcast<true>("svl_gap_tokens_bwd", dpool, ldp, imgs, HW, C, dx, lddx, accumulate, stream);
}

extern "C" int svl_bcast_rows_fwd(const float* v, int64_t ldv, int imgs, int64_t HW, int C, float* dst, int64_t ldd,
                                  int c_off, svl_stream_t stream) {
  SVL_CHECK_ARG(dst && c_off >= 0 && c_off + (int64_t)C <= ldd, "svl_bcast_rows_fwd: channel slice outside the row");
  return launch_bcast<false>("svl_bcast_rows_fwd", v, ldv, imgs, HW, C, dst + c_off, ldd, 0, stream);
}

extern "C" int svl_bcast_rows_bwd(const float* dy, int64_t lddy, int c_off, int imgs, int64_t HW, int C, float* dv,
                                  int64_t ldv, svl_stream_t stream) {
  SVL_CHECK_ARG(dy && c_off >= 0 && c_off + (int64_t)C <= lddy, "svl_bcast_rows_bwd: channel slice outside the row");
  return launch_gap_sum("svl_bcast_rows_bwd", dy + c_off, lddy, imgs, HW, C, dv, ldv, 0, stream);
}
