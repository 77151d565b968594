// Stochastic depth (drop-path) of the CLIP ViT's residual branches (maskclip_vit.py:120-144: x = identity + drop_path(branch)).
// One Bernoulli(keep) draw per sample scales the branch's T rows of that sample by s_b = mask[b] * scale (scale = 1 / keep).
//   droppath_fwd_kernel   out[b * T + t, e] = resid[...] + s_b * branch[...]   (out may be branch: every item reads its own
//                         elements before it writes them); rows of a dropped sample (mask[b] == 0) are copied from resid and
//                         branch is not read
//   droppath_bwd_kernel   dbranch[b * T + t, e] = s_b * dout[...]; rows of a dropped sample are written as zeros and dout is not
//                         read
// The sample of an item is (its row) / T, computed per item: a workgroup (or a wave) whose items span two samples uses both
// scales.  Memory-bound row passes: 16-byte accesses when E % 4 == 0 and every pointer is 16-byte aligned, scalar otherwise;
// 64-bit offsets; capped grids with grid-stride loops.  No atomics: two runs agree bit for bit.
#include "svl_common.h"

namespace {

constexpr int DROPPATH_GRID_CAP = 2048;   // blocks of 256 threads per launch (8 per CU); the kernels loop beyond it

inline int grid_for(long n) {
  long g = (n + 255) / 256;
  if (g < 1) g = 1;
  if (g > DROPPATH_GRID_CAP) g = DROPPATH_GRID_CAP;
  return (int)g;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int V> struct Vec;
template <> struct Vec<4> { typedef f32x4 type; };
template <> struct Vec<1> { typedef float type; };

// the product and the sum are rounded once each, whatever the contraction setting (the tests' bounds count roundings)
__device__ __forceinline__ float mul_rn(float s, float a) { return __fmul_rn(s, a); }
__device__ __forceinline__ f32x4 mul_rn(float s, f32x4 a) {
  f32x4 o = {__fmul_rn(s, a.x), __fmul_rn(s, a.y), __fmul_rn(s, a.z), __fmul_rn(s, a.w)};
  return o;
}
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ f32x4 add_rn(f32x4 a, f32x4 b) {
  f32x4 o = {__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w)};
  return o;
}
template <int V> __device__ __forceinline__ typename Vec<V>::type zero();
template <> __device__ __forceinline__ float zero<1>() { return 0.f; }
template <> __device__ __forceinline__ f32x4 zero<4>() {
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  return o;
}

// one item per V elements of the [B * T, E] matrix (V divides E: an item never crosses a row)
template <int V>
__global__ __launch_bounds__(256) void droppath_fwd_kernel(const float* branch, const float* __restrict__ resid,
                                                           const float* __restrict__ mask, float scale, float* out, long T,
                                                           long EQ, long total) {
  typedef typename Vec<V>::type VT;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = (i / EQ) / T;
    const float m = mask[b];
    VT v = *reinterpret_cast<const VT*>(resid + i * V);
    if (m != 0.f) v = add_rn(v, mul_rn(__fmul_rn(m, scale), *reinterpret_cast<const VT*>(branch + i * V)));
    *reinterpret_cast<VT*>(out + i * V) = v;
  }
}

template <int V>
__global__ __launch_bounds__(256) void droppath_bwd_kernel(const float* dout, const float* __restrict__ mask, float scale,
                                                           float* dbranch, long T, long EQ, long total) {
  typedef typename Vec<V>::type VT;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = (i / EQ) / T;
    const float m = mask[b];
    VT v = zero<V>();
    if (m != 0.f) v = mul_rn(__fmul_rn(m, scale), *reinterpret_cast<const VT*>(dout + i * V));
    *reinterpret_cast<VT*>(dbranch + i * V) = v;
  }
}

}  // namespace

extern "C" int svl_droppath_fwd_f32(const float* branch, const float* resid, const float* mask, float scale, float* out, int B,
                                    int T, int E, svl_stream_t stream) {
  SVL_CHECK_ARG(branch && resid && mask && out && B > 0 && T > 0 && E > 0, "svl_droppath_fwd_f32: bad args");
  SVL_CHECK_ARG(out != resid, "svl_droppath_fwd_f32: out may be branch, not resid");
  const long elems = (long)B * T * E;
  if (E % 4 == 0 && al16(branch) && al16(resid) && al16(out))
    hipLaunchKernelGGL(droppath_fwd_kernel<4>, dim3(grid_for(elems / 4)), dim3(256), 0, (hipStream_t)stream, branch, resid, mask,
                       scale, out, (long)T, (long)(E / 4), elems / 4);
  else
    hipLaunchKernelGGL(droppath_fwd_kernel<1>, dim3(grid_for(elems)), dim3(256), 0, (hipStream_t)stream, branch, resid, mask,
                       scale, out, (long)T, (long)E, elems);
  SVL_LAUNCH_CHECK("svl_droppath_fwd_f32");
  return SVL_OK;
}

extern "C" int svl_droppath_bwd_f32(const float* dout, const float* mask, float scale, float* dbranch, int B, int T, int E,
                                    svl_stream_t stream) {
  SVL_CHECK_ARG(dout && mask && dbranch && B > 0 && T > 0 && E > 0, "svl_droppath_bwd_f32: bad args");
  const long elems = (long)B * T * E;
  if (E % 4 == 0 && al16(dout) && al16(dbranch))
    hipLaunchKernelGGL(droppath_bwd_kernel<4>, dim3(grid_for(elems / 4)), dim3(256), 0, (hipStream_t)stream, dout, mask, scale,
                       dbranch, (long)T, (long)(E / 4), elems / 4);
  else
    hipLaunchKernelGGL(droppath_bwd_kernel<1>, dim3(grid_for(elems)), dim3(256), 0, (hipStream_t)stream, dout, mask, scale,
                       dbranch, (long)T, (long)E, elems);
  SVL_LAUNCH_CHECK("svl_droppath_bwd_f32");
  return SVL_OK;
}
