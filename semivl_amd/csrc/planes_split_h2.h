// The fp16 x 2 split of the packed-planes operand format: x = 2^e (h0 + h1) with one scale exponent e per row.  One
// definition for every kernel that emits such planes (the generic pack pass and the GEMM epilogues of gemm_planes_h2.hip,
// the LayerNorm -> planes kernels of norm.hip): their outputs are compared bit for bit.
#pragma once
#include "svl_common.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

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

}  // namespace
