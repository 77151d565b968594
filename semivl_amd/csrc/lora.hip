// LoRA adapters of the CLIP ViT as MERGED weights (model/backbone/lora.py, maskclip_vit.py:85-88,123-137): with
// lora_dropout == 0 the adapter b(a(x)) * s is linear in the projection's own input, so F.linear(x, W) + s * b(a(x)) ==
// F.linear(x, W + s * B @ A) and the block runs the existing GEMM / attention kernels on the effective weight.  Two kernels:
//   lora_merge_kernel   Weff = W + s * B @ A          one read of W, one write of Weff, A tile + B rows staged in LDS
//   lora_wgrad_kernel   dB (+)= s * dW @ A^T,  dA partials = s * B^T @ dW per 16-row tile      one read of dW for both
// and svl_reduce_slabs_f32 (gemm.hip) as the deterministic second stage of dA (partials added in tile order, in double).
// fp32 in / out / accumulate, 1 <= r <= 64, E % 4 == 0, 16-byte accesses on every E-wide matrix.  No atomics anywhere: two
// runs agree bit for bit.
#include "svl_common.h"

namespace {

constexpr int kMaxR = 64;
constexpr int kTE = 128;           // columns of E per tile (32 lanes x 16 B)
constexpr int kMergeRows = 32;     // rows of W per merge block (8 row lanes x 4)
constexpr int kWgradRows = 16;     // rows of dW per wgrad block == the fp32 chain length of a dA partial
constexpr int kLdA = kTE + 4;      // LDS row pitch of the A tile in the wgrad kernel (breaks the 128-float bank stride)

struct MergeBlocks {
  const float* A[3];
  const float* B[3];
};

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// acc + b * a with ONE rounding per component whatever the contraction setting (the tests' bounds count roundings)
__device__ __forceinline__ f32x4 fma4(float b, f32x4 a, f32x4 acc) {
  f32x4 o;
  o.x = fmaf(b, a.x, acc.x);
  o.y = fmaf(b, a.y, acc.y);
  o.z = fmaf(b, a.z, acc.z);
  o.w = fmaf(b, a.w, acc.w);
  return o;
}

// grid (cdiv(E, 128), nblk * cdiv(rows, 32)), 256 threads: thread = (row lane 0..7, column group 0..31); row block `blk` of
// W / Weff is rows [blk * rows, (blk + 1) * rows) and takes the adapter pair (A[blk], B[blk]) -- both null: a plain copy.
__global__ __launch_bounds__(256) void lora_merge_kernel(const float* W, long ldw, float* out, long ldo, MergeBlocks mb,
                                                         long ldb, int rows, int tiles, int E, int r, float s) {
  __shared__ __attribute__((aligned(16))) float As[kMaxR * kTE];
  __shared__ float Bs[kMergeRows * kMaxR];
  const int blk = blockIdx.y / tiles;
  const int r0 = (blockIdx.y - blk * tiles) * kMergeRows;
  const int e0 = blockIdx.x * kTE;
  const float* A = mb.A[blk];
  const float* B = mb.B[blk];
  const int tid = threadIdx.x, cg = tid & 31, rl = tid >> 5;
  if (A != nullptr) {      // (block-uniform)
    for (int i = tid; i < r * (kTE / 4); i += 256) {
      const int j = i >> 5, c = i & 31, cc = e0 + c * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (cc < E) v = *reinterpret_cast<const f32x4*>(A + (long)j * E + cc);
      *reinterpret_cast<f32x4*>(As + j * kTE + c * 4) = v;
    }
    for (int i = tid; i < kMergeRows * r; i += 256) {
      const int rr = i / r, j = i - rr * r;
      Bs[rr * kMaxR + j] = (r0 + rr < rows) ? B[(long)(r0 + rr) * ldb + j] : 0.f;
    }
    __syncthreads();
  }
  const int col = e0 + cg * 4;
  if (col >= E) return;
  const long base = (long)blk * rows;
#pragma unroll
  for (int k = 0; k < kMergeRows / 8; ++k) {
    const int rr = rl + 8 * k;
    if (r0 + rr >= rows) break;
    f32x4 w = *reinterpret_cast<const f32x4*>(W + (base + r0 + rr) * ldw + col);
    if (A != nullptr) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < r; ++j) {
        const float b = Bs[rr * kMaxR + j];                                   // one address per row lane: a broadcast
        const f32x4 a = *reinterpret_cast<const f32x4*>(As + j * kTE + cg * 4);
        acc = fma4(b, a, acc);
      }
      w = fma4(s, acc, w);
    }
    *reinterpret_cast<f32x4*>(out + (base + r0 + rr) * ldo + col) = w;
  }
}

// grid cdiv(rows, 16), 256 threads.  The block walks its 16 rows of dW across E in 128-column tiles (each element of dW is
// read from memory once, into LDS) and forms
//   dB[row, j] = s * sum_e dW[row, e] A[j, e]     complete inside the block: one fp32 chain over e in ascending order,
//   part[tile, j, e] = s * sum_{row in tile} B[row, j] dW[row, e]     one fp32 chain over the tile's rows in ascending order.
__global__ __launch_bounds__(256) void lora_wgrad_kernel(const float* dW, long lddw, const float* A, const float* B, long ldb,
                                                         int rows, int E, int r, float s, float* dB, int acc_b, float* part) {
  __shared__ __attribute__((aligned(16))) float As[kMaxR * kLdA];
  __shared__ __attribute__((aligned(16))) float Ds[kWgradRows * kTE];
  __shared__ float Bs[kWgradRows * kMaxR];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * kWgradRows;
  for (int i = tid; i < kWgradRows * r; i += 256) {
    const int rr = i / r, j = i - rr * r;
    Bs[rr * kMaxR + j] = (r0 + rr < rows) ? B[(long)(r0 + rr) * ldb + j] : 0.f;
  }
  const int brow = tid >> 4, jl = tid & 15;      // dB: thread = (row of the tile, j lane), j = jl + 16 k
  float accb[kMaxR / 16] = {0.f, 0.f, 0.f, 0.f};
  for (int e0 = 0; e0 < E; e0 += kTE) {
    __syncthreads();                             // the previous tile's readers are done (first pass: nothing to wait for)
    for (int i = tid; i < r * (kTE / 4); i += 256) {
      const int j = i >> 5, c = i & 31, cc = e0 + c * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (cc < E) v = *reinterpret_cast<const f32x4*>(A + (long)j * E + cc);
      *reinterpret_cast<f32x4*>(As + j * kLdA + c * 4) = v;
    }
    for (int i = tid; i < kWgradRows * (kTE / 4); i += 256) {
      const int rr = i >> 5, c = i & 31, cc = e0 + c * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (r0 + rr < rows && cc < E) v = *reinterpret_cast<const f32x4*>(dW + (long)(r0 + rr) * lddw + cc);
      *reinterpret_cast<f32x4*>(Ds + rr * kTE + c * 4) = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kMaxR / 16; ++k) {
      const int j = jl + 16 * k;
      if (j < r) {
        float a = accb[k];
        for (int e = 0; e < kTE; e += 4) {       // (columns past E are staged as zeros: exact no-ops of the chain)
          const f32x4 d = *reinterpret_cast<const f32x4*>(Ds + brow * kTE + e);
          const f32x4 av = *reinterpret_cast<const f32x4*>(As + j * kLdA + e);
          a = fmaf(d.x, av.x, a);
          a = fmaf(d.y, av.y, a);
          a = fmaf(d.z, av.z, a);
          a = fmaf(d.w, av.w, a);
        }
        accb[k] = a;
      }
    }
    for (int o = tid; o < r * (kTE / 4); o += 256) {
      const int j = o >> 5, c = o & 31, cc = e0 + c * 4;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int rr = 0; rr < kWgradRows; ++rr)    // (rows past `rows` are staged as zeros)
        acc = fma4(Bs[rr * kMaxR + j], *reinterpret_cast<const f32x4*>(Ds + rr * kTE + c * 4), acc);
      if (cc < E) *reinterpret_cast<f32x4*>(part + ((long)blockIdx.x * r + j) * E + cc) = s * acc;
    }
  }
  if (r0 + brow < rows) {
#pragma unroll
    for (int k = 0; k < kMaxR / 16; ++k) {
      const int j = jl + 16 * k;
      if (j < r) {
        float* p = dB + (long)(r0 + brow) * r + j;
        const float v = s * accb[k];
        *p = acc_b ? *p + v : v;
      }
    }
  }
}

bool shape_ok(int rows, int E, int r) { return rows > 0 && E > 0 && E % 4 == 0 && r >= 1 && r <= kMaxR; }

}  // namespace

extern "C" int svl_lora_merge_f32(const float* W, int64_t ldw, float* Weff, int64_t ldo, int nblk, int rows, int E, int r,
                                  float s, const float* const* A, const float* const* B, int64_t ldb, svl_stream_t stream) {
  SVL_CHECK_ARG(W && Weff && A && B, "svl_lora_merge_f32: null pointer");
  SVL_CHECK_ARG(shape_ok(rows, E, r), "svl_lora_merge_f32: rows=%d E=%d r=%d (need rows > 0, E %% 4 == 0, 1 <= r <= 64)",
                rows, E, r);
  SVL_CHECK_ARG(nblk >= 1 && nblk <= 3, "svl_lora_merge_f32: nblk=%d (1..3)", nblk);
  SVL_CHECK_ARG(ldw >= E && ldo >= E && ldw % 4 == 0 && ldo % 4 == 0 && ldb >= r && al16(W) && al16(Weff),
                "svl_lora_merge_f32: leading dimensions (%ld, %ld, %ld) / 16-byte alignment", (long)ldw, (long)ldo, (long)ldb);
  MergeBlocks mb = {};
  for (int i = 0; i < nblk; ++i) {
    SVL_CHECK_ARG(!A[i] == !B[i], "svl_lora_merge_f32: block %d has one of A / B only", i);
    SVL_CHECK_ARG(al16(A[i]), "svl_lora_merge_f32: A of block %d is not 16-byte aligned", i);
    mb.A[i] = A[i];
    mb.B[i] = B[i];
  }
  const int tiles = svl_cdiv(rows, kMergeRows);
  SVL_CHECK_ARG((long)tiles * nblk <= 65535, "svl_lora_merge_f32: %d rows x %d blocks exceed the grid", rows, nblk);
  hipLaunchKernelGGL(lora_merge_kernel, dim3(svl_cdiv(E, kTE), tiles * nblk), dim3(256), 0, (hipStream_t)stream, W, (long)ldw,
                     Weff, (long)ldo, mb, (long)ldb, rows, tiles, E, r, s);
  SVL_LAUNCH_CHECK("svl_lora_merge_f32");
  return SVL_OK;
}

extern "C" int64_t svl_lora_wgrad_ws_floats(int rows, int E, int r) {
  if (!shape_ok(rows, E, r)) return -1;
  return (int64_t)svl_cdiv(rows, kWgradRows) * r * E;
}

extern "C" int svl_lora_wgrad_f32(const float* dW, int64_t lddw, const float* A, const float* B, int64_t ldb, int rows, int E,
                                  int r, float s, float* dB, int accumulate_b, float* dA, int accumulate_a, float* ws,
                                  svl_stream_t stream) {
  SVL_CHECK_ARG(dW && A && B && dB && dA && ws, "svl_lora_wgrad_f32: null pointer");
  SVL_CHECK_ARG(shape_ok(rows, E, r), "svl_lora_wgrad_f32: rows=%d E=%d r=%d (need rows > 0, E %% 4 == 0, 1 <= r <= 64)",
                rows, E, r);
  SVL_CHECK_ARG(lddw >= E && lddw % 4 == 0 && ldb >= r && al16(dW) && al16(A) && al16(ws),
                "svl_lora_wgrad_f32: leading dimensions (%ld, %ld) / 16-byte alignment", (long)lddw, (long)ldb);
  const int tiles = svl_cdiv(rows, kWgradRows);
  hipLaunchKernelGGL(lora_wgrad_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, dW, (long)lddw, A, B, (long)ldb, rows,
                     E, r, s, dB, accumulate_b ? 1 : 0, ws);
  SVL_LAUNCH_CHECK("svl_lora_wgrad_f32");
  // second stage of dA: the per-tile partials added in tile order, in double, one rounding (onto dA when accumulating)
  return svl_reduce_slabs_f32(dA, ws, tiles, (int64_t)r * E, accumulate_a ? 1 : 0, stream);
}
