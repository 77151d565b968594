// The packed-planes operand format, in one place for every kernel that emits it (the pack passes of gemm_planes.hip and
// gemm_planes_h2.hip, the GEMM epilogues of gemm_planes_impl.h, the LayerNorm -> planes kernels of norm.hip): their outputs
// are compared bit for bit.
//   bf16 x 3 (NP = 3): x = h0 + h1 + h2.   fp16 x 2 (NP = 2): x = 2^e (h0 + h1) with one scale exponent e per row.
//   Chunk = the CH bytes of one (k-group, 32-row block, plane): 64 lanes x 16 B, lane = (lane half h, row % 32), holding
//   k = 16 kg + 4 h + {0..3, 8..11}; the NP planes of a (k-group, row block) are consecutive chunks.
#pragma once
#include "svl_common.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int CH = 1024;        // bytes of one (k-group, row block, plane) chunk

// x = x0 + x1 + x2: the three bf16 planes of 8 values
__device__ __forceinline__ void split3x8(const float (&x)[8], bf16x8& h0, bf16x8& h1, bf16x8& h2) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = x[j];
    h0[j] = (__bf16)v;
    v -= (float)h0[j];
    h1[j] = (__bf16)v;
    v -= (float)h1[j];
    h2[j] = (__bf16)v;
  }
}
// x 2^-e = h0 + h1: the two fp16 planes of 8 values (e = the row's scale exponent)
__device__ __forceinline__ void split2x8(const float (&x)[8], int e, f16x8& h0, f16x8& h1) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = __builtin_amdgcn_ldexpf(x[j], -e);
    h0[j] = (_Float16)v;
    h1[j] = (_Float16)(v - (float)h0[j]);
  }
}
// scale exponent of a row whose entries are bounded by `bound`: bound 2^-e < 2^15 (fp16 overflows at 65504)
__device__ __forceinline__ int scale_exp_of(float bound) {
  const int e = __builtin_amdgcn_frexp_expf(bound) - 15;      // bound = f 2^E, f in [0.5, 1)
  return e < -100 ? -100 : (e > 100 ? 100 : e);
}

// The convolutions' operands (conv_tiled.hip, conv_dil.hip) take their scale from a block MAXIMUM found while the block stages
// them: m 2^-e in [2^14, 2^15), clamped to +-100; an all-zero block takes `zero_e`.
__device__ __forceinline__ int max_exp_of(float m, int zero_e) {
  const int e = m > 0.f ? __builtin_amdgcn_frexp_expf(m) - 15 : zero_e;
  return e < -100 ? -100 : (e > 100 ? 100 : e);
}
// ... of an activation slab: all zeros take the floor, so that any later slab of the same accumulators raises the exponent
__device__ __forceinline__ int slab_exp_of(float m) { return max_exp_of(m, -100); }
// x 2^-e = h0 + h1 for a quad: two round-to-nearest fp16 terms (23 significand bits for every element within 2^-17 of the maximum)
__device__ __forceinline__ void split2x4(const float4 x, int e, f16x4& h0, f16x4& h1) {
  const float v[4] = {__builtin_amdgcn_ldexpf(x.x, -e), __builtin_amdgcn_ldexpf(x.y, -e), __builtin_amdgcn_ldexpf(x.z, -e),
                      __builtin_amdgcn_ldexpf(x.w, -e)};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    h0[j] = (_Float16)v[j];
    h1[j] = (_Float16)(v[j] - (float)h0[j]);
  }
}
__device__ __forceinline__ float absmax4(const float4 v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }
// The maximum's way through a four-wave block: every wave leaves its own in smax[wave]; after a barrier block_max4 reads all four
__device__ __forceinline__ float wave_max(float m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  return m;
}
__device__ __forceinline__ void wave_max_to(float m, float* smax, int lane, int wave) {
  m = wave_max(m);
  if (lane == 0) smax[wave] = m;
}
__device__ __forceinline__ float block_max4(const float* smax) { return fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3])); }

// The 16 bytes of (k-group kg, row rr of the plane buffer, lane half h) in plane 0; plane pl is CH * pl further on.
// p_ks = bytes between k-groups (rows_padded * 32 * NP).
template <int NP>
__device__ __forceinline__ char* plane_chunk(char* planes, long p_ks, long kg, long rr, int h) {
  return planes + kg * p_ks + (rr >> 5) * (NP * CH) + (h * 32 + (int)(rr & 31)) * 16;
}

// The 8 values of one such 16 bytes from a 16 B aligned row-major source: src = &x(r, 16 kg + 4 h)
__device__ __forceinline__ void load8(const float* src, float (&v)[8]) {
  const float4 f0 = *reinterpret_cast<const float4*>(src), f1 = *reinterpret_cast<const float4*>(src + 8);
  v[0] = f0.x; v[1] = f0.y; v[2] = f0.z; v[3] = f0.w; v[4] = f1.x; v[5] = f1.y; v[6] = f1.z; v[7] = f1.w;
}
// 8 values -> the NP planes at q = plane_chunk<NP>(...)   (e: NP = 2 only)
template <int NP>
__device__ __forceinline__ void split_store(const float (&v)[8], int e, char* q) {
  if constexpr (NP == 3) {
    bf16x8 h0, h1, h2;
    split3x8(v, h0, h1, h2);
    *reinterpret_cast<bf16x8*>(q) = h0;
    *reinterpret_cast<bf16x8*>(q + CH) = h1;
    *reinterpret_cast<bf16x8*>(q + 2 * CH) = h2;
  } else {
    f16x8 h0, h1;
    split2x8(v, e, h0, h1);
    *reinterpret_cast<f16x8*>(q) = h0;
    *reinterpret_cast<f16x8*>(q + CH) = h1;
  }
}
// The pack passes' step: load 8 values of a row (16 B loads when `fast`, else element stride ks; zeros when !valid:
// the padding rows of the last row block), split, store
template <int NP>
__device__ __forceinline__ void pack8(const float* src, long ks, bool fast, bool valid, int e, char* q) {
  float v[8];
  if (valid) {
    if (fast) {
      load8(src, v);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[j] = src[j * ks]; v[4 + j] = src[(8 + j) * ks]; }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
  }
  split_store<NP>(v, e, q);
}

// Phase 1 of the fp16 x 2 pack pass on a 16 B aligned row-major row: 8 threads per row (sub = 0..7, consecutive lanes),
// 16 B each -- a row's threads read 128 contiguous bytes per step.  Largest magnitude and squared norm (double: 1e25-sized
// rows must not overflow the sum); row_combine8 leaves both in all 8 threads.
__device__ __forceinline__ void row_scan16(const float* src, int K, int sub, float& amax, double& sq) {
  for (int k = sub * 4; k < K; k += 32) {
    const float4 f = *reinterpret_cast<const float4*>(src + k);
    amax = fmaxf(fmaxf(amax, fabsf(f.x)), fmaxf(fabsf(f.y), fmaxf(fabsf(f.z), fabsf(f.w))));
    sq += (double)f.x * f.x + (double)f.y * f.y + ((double)f.z * f.z + (double)f.w * f.w);
  }
}
__device__ __forceinline__ void row_combine8(float& amax, double& sq) {
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) {
    amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    sq += __shfl_xor(sq, o, 64);
  }
}
// The pack pass's row scale and norm bound (rounded up: it is used as a bound); padding rows get 0 / 0
__device__ __forceinline__ int pack_exp(bool valid, float amax) { return valid ? scale_exp_of(amax) : 0; }
__device__ __forceinline__ float pack_rnorm(bool valid, double sq) { return valid ? (float)(sqrt(sq) * (1.0 + 1e-6)) : 0.f; }

}  // namespace
