// Deep visual prompt tokens of the CLIP ViT (maskclip_vit.py:359-368,510-536): every block runs on
//   [class token | P prompt rows | patch tokens]   (T + P rows per image),
// the prompt rows are written before the block and dropped after it.  Two kernels:
//   prompt_rows_fwd_kernel   dst[b, 1 + j] = emb[j] * (mask[b, j] * scale), and in the expand form the other rows copied from a
//                            [B, T, E] matrix (one read, one write of the token matrix); the in-place form writes the B * P
//                            prompt rows only
//   prompt_rows_bwd_kernel   demb[j] (+)= sum_b dx[b, 1 + j] * (mask[b, j] * scale), one thread per output element, b ascending;
//                            the same thread then zeroes the rows it summed, or (compact form) the non-prompt rows are copied
//                            to a [B, T, E] matrix by the rest of the grid
// Memory-bound row passes: 16-byte accesses when E % 4 == 0 and every pointer is 16-byte aligned, scalar otherwise; 64-bit
// offsets; capped grids with grid-stride loops.  No atomics: two runs agree bit for bit.
#include "svl_common.h"

namespace {

constexpr int PROMPT_GRID_CAP = 256 * 32;   // blocks of 256 threads per launch; the kernels loop beyond it

inline int grid_for(long n) {
  long g = (n + 255) / 256;
  if (g < 1) g = 1;
  if (g > PROMPT_GRID_CAP) g = PROMPT_GRID_CAP;
  return (int)g;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }   // (a null pointer counts as aligned)

template <int V> struct Vec;
template <> struct Vec<4> { typedef f32x4 type; };
template <> struct Vec<1> { typedef float type; };

// every product and every sum below is rounded once, whatever the contraction setting (the tests' bounds count roundings)
__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ f32x4 mul_rn(f32x4 a, f32x4 b) {
  f32x4 o = {__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y), __fmul_rn(a.z, b.z), __fmul_rn(a.w, b.w)};
  return o;
}
__device__ __forceinline__ f32x4 add_rn(f32x4 a, f32x4 b) {
  f32x4 o = {__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w)};
  return o;
}
template <int V> __device__ __forceinline__ typename Vec<V>::type splat(float s);
template <> __device__ __forceinline__ float splat<1>(float s) { return s; }
template <> __device__ __forceinline__ f32x4 splat<4>(float s) {
  f32x4 o = {s, s, s, s};
  return o;
}

// emb * (mask * scale): two products
template <int V>
__device__ __forceinline__ typename Vec<V>::type prompt_value(const float* emb, const float* mask, float scale, long eo, long mo) {
  typedef typename Vec<V>::type VT;
  VT v = *reinterpret_cast<const VT*>(emb + eo);
  if (mask != nullptr) {
    const VT m = *reinterpret_cast<const VT*>(mask + mo);
    v = mul_rn(v, mul_rn(m, splat<V>(scale)));
  }
  return v;
}

// expand (src != null): one item per V elements of dst [B, T + P, E].  in place (src == null): one item per V elements of the
// B * P prompt rows.
template <int V>
__global__ __launch_bounds__(256) void prompt_rows_fwd_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                              const float* __restrict__ emb, const float* __restrict__ mask,
                                                              float scale, long B, long T, long P, int E) {
  typedef typename Vec<V>::type VT;
  const long EQ = E / V;
  const long rows = src != nullptr ? T + P : P;        // rows per image this launch writes
  const long total = B * rows * EQ;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long row = i / EQ;
    const long c = (i - row * EQ) * V;
    const long b = row / rows;
    long r = row - b * rows;                           // row of the image in dst (expand), prompt index (in place)
    if (src == nullptr) r += 1;
    VT v;
    if (r >= 1 && r <= P)
      v = prompt_value<V>(emb, mask, scale, (r - 1) * E + c, (b * P + (r - 1)) * E + c);
    else
      v = *reinterpret_cast<const VT*>(src + (b * T + (r == 0 ? 0 : r - P)) * E + c);
    *reinterpret_cast<VT*>(dst + (b * (T + P) + r) * E + c) = v;
  }
}

// items [0, P * EQ): element (j, c) of demb, summed over b in ascending order, every product and every sum rounded once
// (__fmul_rn / __fadd_rn: no contraction); without dx_out the summed elements of dx are then set to zero by the thread that
// read them.  items [P * EQ, P * EQ + B * T * EQ) exist with dx_out only: the non-prompt rows of dx copied to dx_out [B, T, E].
template <int V>
__global__ __launch_bounds__(256) void prompt_rows_bwd_kernel(float* dx, float* __restrict__ dx_out,
                                                              float* __restrict__ demb, const float* __restrict__ mask,
                                                              float scale, int accumulate, long B, long T, long P, int E) {
  typedef typename Vec<V>::type VT;
  const long EQ = E / V;
  const long nsum = P * EQ;
  const long total = nsum + (dx_out != nullptr ? B * T * EQ : 0);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    if (i < nsum) {
      const long j = i / EQ;
      const long c = (i - j * EQ) * V;
      VT acc = splat<V>(0.f);
      for (long b = 0; b < B; ++b) {
        float* p = dx + (b * (T + P) + 1 + j) * E + c;
        if (demb != nullptr) {
          VT g = *reinterpret_cast<const VT*>(p);
          if (mask != nullptr)
            g = mul_rn(g, mul_rn(*reinterpret_cast<const VT*>(mask + (b * P + j) * E + c), splat<V>(scale)));
          acc = add_rn(acc, g);
        }
        if (dx_out == nullptr) *reinterpret_cast<VT*>(p) = splat<V>(0.f);
      }
      if (demb != nullptr) {
        VT* d = reinterpret_cast<VT*>(demb + j * E + c);
        *d = accumulate ? add_rn(*d, acc) : acc;
      }
    } else {
      const long t = i - nsum;
      const long row = t / EQ;
      const long c = (t - row * EQ) * V;
      const long b = row / T;
      const long r = row - b * T;
      *reinterpret_cast<VT*>(dx_out + row * E + c) =
          *reinterpret_cast<const VT*>(dx + (b * (T + P) + (r == 0 ? 0 : r + P)) * E + c);
    }
  }
}

}  // namespace

extern "C" int svl_prompt_rows_fwd_f32(const float* src, float* dst, const float* emb, const float* mask, float scale, int B,
                                       int T, int P, int E, svl_stream_t stream) {
  SVL_CHECK_ARG(dst && emb && B > 0 && T > 0 && P > 0 && E > 0, "svl_prompt_rows_fwd_f32: bad args");
  SVL_CHECK_ARG(src != dst, "svl_prompt_rows_fwd_f32: the expand form does not run in place");
  const long elems = (long)B * (src ? T + P : P) * E;
  if (E % 4 == 0 && al16(src) && al16(dst) && al16(emb) && al16(mask))
    hipLaunchKernelGGL(prompt_rows_fwd_kernel<4>, dim3(grid_for(elems / 4)), dim3(256), 0, (hipStream_t)stream, src, dst, emb,
                       mask, scale, (long)B, (long)T, (long)P, E);
  else
    hipLaunchKernelGGL(prompt_rows_fwd_kernel<1>, dim3(grid_for(elems)), dim3(256), 0, (hipStream_t)stream, src, dst, emb,
                       mask, scale, (long)B, (long)T, (long)P, E);
  SVL_LAUNCH_CHECK("svl_prompt_rows_fwd_f32");
  return SVL_OK;
}

extern "C" int svl_prompt_rows_bwd_f32(float* dx, float* dx_out, float* demb, const float* mask, float scale, int accumulate,
                                       int B, int T, int P, int E, svl_stream_t stream) {
  SVL_CHECK_ARG(dx && B > 0 && T > 0 && P > 0 && E > 0, "svl_prompt_rows_bwd_f32: bad args");
  SVL_CHECK_ARG(dx_out != dx, "svl_prompt_rows_bwd_f32: the compact form does not run in place");
  const long elems = (long)P * E + (dx_out ? (long)B * T * E : 0);
  if (E % 4 == 0 && al16(dx) && al16(dx_out) && al16(demb) && al16(mask))
    hipLaunchKernelGGL(prompt_rows_bwd_kernel<4>, dim3(grid_for(elems / 4)), dim3(256), 0, (hipStream_t)stream, dx, dx_out, demb,
                       mask, scale, accumulate, (long)B, (long)T, (long)P, E);
  else
    hipLaunchKernelGGL(prompt_rows_bwd_kernel<1>, dim3(grid_for(elems)), dim3(256), 0, (hipStream_t)stream, dx, dx_out, demb,
                       mask, scale, accumulate, (long)B, (long)T, (long)P, E);
  SVL_LAUNCH_CHECK("svl_prompt_rows_bwd_f32");
  return SVL_OK;
}
