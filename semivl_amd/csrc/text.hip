// CLIP text tower (third_party/zegclip/models/backbones/text_encoder.py:79-87, utils.py:124-170): the pieces the library
// lacked.  Forward only; the tower is frozen and runs once per class list (tools/text_embeddings.py), so these kernels are
// written for exactness and bounded addressing first.  The GEMMs, LayerNorm and the L2 norm are the existing entry points.
//   text_embed_kernel    x[(i, t), :] = table[tok[i, t], :] + pos[t, :], one rounding per element; a token outside [0, V) is
//                        not dereferenced (its row is written as NaN)
//   text_eot_kernel      eot[i] = index of the first maximum of tok[i, :] (torch.argmax), a wave per sequence
//   causal_attn_kernel   a block per (sequence, head), K and V of that head in LDS (the layout of seqattn.hip: lane = key for
//                        the scores, lane = channel for the values); query t reads keys 0 .. t only: a 64-key tile that lies
//                        wholly above the row is skipped, the lanes above the row inside the diagonal tile are masked off, and
//                        the value loop ends at t.  Nothing of rows > t enters row t, so the mask is exact.
//   quickgelu_kernel     y = x * sigmoid(1.702 x); the sigmoid on exp(-|1.702 x|) so that it cannot overflow, the product
//                        1.702 x carried with its rounding error (and the constant's), so exp() sees the argument to ~2^-48
//   gather_rows_kernel   out[i, :] = x[i * L + idx[i], :]; an index outside [0, L) is not dereferenced (NaN row)
//   segment_mean_kernel  out[c, :] = (x[o_c] + x[o_c + 1] + ... in ascending order) / count, one thread per element
// 64-bit offsets, capped grids with grid-stride loops, no atomics: two runs agree bit for bit.
#include "svl_common.h"

namespace {

constexpr int D = 64;
constexpr int LDK = D + 1;   // padded LDS row, as seqattn.hip
constexpr int MAXT = 3;      // keys per lane -> L <= 192
constexpr int GRID_CAP = 2048;

inline int grid_for(long n) {
  long g = (n + 255) / 256;
  if (g < 1) g = 1;
  if (g > GRID_CAP) g = GRID_CAP;
  return (int)g;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ float qnan() { return __builtin_nanf(""); }

// ---- embedding ---------------------------------------------------------------------------------------------------------
// one item per V4 elements of x [n * L, W]
template <int V4>
__global__ __launch_bounds__(256) void text_embed_kernel(const int64_t* __restrict__ tok, const float* __restrict__ table,
                                                         const float* __restrict__ pos, long L, long V, long WQ, long total,
                                                         float* __restrict__ x) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long row = i / WQ, c = i - row * WQ;
    const long t = row % L;
    const int64_t id = tok[row];
    const bool ok = id >= 0 && id < V;
    if (V4 == 4) {
      f32x4 o = {qnan(), qnan(), qnan(), qnan()};
      if (ok) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(table + (id * WQ + c) * 4);
        const f32x4 b = *reinterpret_cast<const f32x4*>(pos + (t * WQ + c) * 4);
        o.x = __fadd_rn(a.x, b.x); o.y = __fadd_rn(a.y, b.y); o.z = __fadd_rn(a.z, b.z); o.w = __fadd_rn(a.w, b.w);
      }
      *reinterpret_cast<f32x4*>(x + i * 4) = o;
    } else {
      x[i] = ok ? __fadd_rn(table[id * WQ + c], pos[t * WQ + c]) : qnan();
    }
  }
}

// a wave per sequence: lane l scans t = l, l + 64, ... (ascending, strict >), then the wave keeps the larger value and, on a
// tie, the smaller index.  The 64-bit value travels as two 32-bit halves.
__global__ __launch_bounds__(256) void text_eot_kernel(const int64_t* __restrict__ tok, int n, int L, int* __restrict__ eot) {
  const int lane = threadIdx.x & 63;
  const int seq = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seq >= n) return;
  const int64_t* r = tok + (long)seq * L;
  int64_t bv = INT64_MIN;
  int bi = INT32_MAX;
  for (int t = lane; t < L; t += 64) {
    const int64_t v = r[t];
    if (bi == INT32_MAX || v > bv) { bv = v; bi = t; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int lo = __shfl_xor((int)(uint32_t)(uint64_t)bv, o, 64);
    const int hi = __shfl_xor((int)(uint32_t)((uint64_t)bv >> 32), o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    const int64_t ov = (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
    if (oi != INT32_MAX && (bi == INT32_MAX || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
  }
  if (lane == 0) eot[seq] = bi;
}

// ---- causal attention --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void causal_attn_kernel(const float* __restrict__ qkv, float* __restrict__ out, int L, int H) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int E = H * D;
  float* Ks = sm;                 // [L][LDK]
  float* Vs = Ks + L * LDK;       // [L][LDK]
  float* wbuf = Vs + L * LDK;     // per wave: q[64] + prow[L]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x / H, h = blockIdx.x % H;
  float* qrow = wbuf + wave * (D + L);
  float* prow = qrow + D;
  const long row0 = (long)s * L;

  for (int i = tid; i < L * D; i += 256) {
    const int j = i >> 6, d = i & 63;
    const float* r = qkv + (row0 + j) * (3L * E) + h * D + d;
    Ks[j * LDK + d] = r[E];
    Vs[j * LDK + d] = r[2 * E];
  }
  __syncthreads();

  // rows from the end first: the long rows are spread over the four waves before the short ones
  for (int t = L - 1 - wave; t >= 0; t -= 4) {
    const long row = row0 + t;
    qrow[lane] = qkv[row * (3L * E) + h * D + lane] * 0.125f;   // 64^-0.5, applied to q like nn.MultiheadAttention
    __builtin_amdgcn_wave_barrier();
    const int ntile = (t >> 6) + 1;   // wave-uniform: tiles whose first key is above the row are never entered
    float sc[MAXT];
    float m = -INFINITY;
#pragma unroll
    for (int tt = 0; tt < MAXT; ++tt) {
      sc[tt] = -INFINITY;
      if (tt < ntile) {
        const int j = lane + 64 * tt;
        if (j <= t) {
          float a = 0.f;
          for (int d = 0; d < D; ++d) a += qrow[d] * Ks[j * LDK + d];
          sc[tt] = a;
          m = fmaxf(m, a);
        }
      }
    }
    m = wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int tt = 0; tt < MAXT; ++tt) {
      const int j = lane + 64 * tt;
      sc[tt] = (tt < ntile && j <= t) ? expf(sc[tt] - m) : 0.f;
      sum += sc[tt];
    }
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
#pragma unroll
    for (int tt = 0; tt < MAXT; ++tt) {
      const int j = lane + 64 * tt;
      if (tt < ntile && j <= t) prow[j] = sc[tt] * inv;
    }
    __builtin_amdgcn_wave_barrier();
    float o = prow[0] * Vs[lane];     // the first term starts the chain: row 0 is v[0] itself, sign of zero included
    for (int j = 1; j <= t; ++j) o += prow[j] * Vs[j * LDK + lane];
    out[row * E + h * D + lane] = o;
    __builtin_amdgcn_wave_barrier();
  }
}

size_t causal_lds_bytes(int L) { return (size_t)(2 * L * LDK + 4 * (D + L)) * sizeof(float); }

// ---- QuickGELU ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float quickgelu(float x) {
  const float C = 1.702f;
  const float CLO = (float)(1.702 - (double)1.702f);   // what the fp32 constant leaves out
  const float t = C * x;
  float lo = 0.f;
  if (isfinite(t)) lo = fmaf(C, x, -t) + CLO * x;      // 1.702 x = t + lo
  const float la = x < 0.f ? lo : -lo;
  float e = expf(-fabsf(t));                           // in (0, 1]: no overflow for any x
  e = fmaf(e, la, e);                                  // exp(-|1.702 x|) with the argument's low part
  const float s = (x < 0.f ? e : 1.f) / (1.f + e);     // sigmoid(1.702 x)
  return x * s;
}

__global__ __launch_bounds__(256) void quickgelu_v4_kernel(const float* x, float* y, long nq) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (long)gridDim.x * blockDim.x) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + i * 4);
    f32x4 o = {quickgelu(a.x), quickgelu(a.y), quickgelu(a.z), quickgelu(a.w)};
    *reinterpret_cast<f32x4*>(y + i * 4) = o;
  }
}

__global__ __launch_bounds__(256) void quickgelu_s_kernel(const float* x, float* y, long first, long count) {
  for (long i = first + (long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long)gridDim.x * blockDim.x)
    y[i] = quickgelu(x[i]);
}

// ---- row gather / segment mean -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ x, const int* __restrict__ idx, long L,
                                                          long E, long total, float* __restrict__ out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / E, c = i - r * E;
    const int k = idx[r];
    out[i] = (k >= 0 && k < L) ? x[(r * L + k) * E + c] : qnan();
  }
}

__global__ __launch_bounds__(256) void segment_mean_kernel(const float* __restrict__ x, long m, long E,
                                                           const int* __restrict__ offs, long total, float* __restrict__ out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long c = i / E, e = i - c * E;
    long a = offs[c], b = offs[c + 1];
    a = a < 0 ? 0 : (a > m ? m : a);      // a row outside [0, m) is never read, whatever the table holds
    b = b < a ? a : (b > m ? m : b);
    float s = qnan();                     // an empty segment has no mean
    if (b > a) {
      s = x[a * E + e];
      for (long r = a + 1; r < b; ++r) s = __fadd_rn(s, x[r * E + e]);
      s = s / (float)(b - a);
    }
    out[i] = s;
  }
}

}  // namespace

extern "C" int svl_text_embed_f32(const int64_t* tokens, const float* table, const float* pos, int n, int L, int V, int W,
                                  float* x, int* eot, svl_stream_t stream) {
  SVL_CHECK_ARG(tokens, "svl_text_embed_f32: tokens is null");
  SVL_CHECK_ARG(table, "svl_text_embed_f32: table is null");
  SVL_CHECK_ARG(pos, "svl_text_embed_f32: pos is null");
  SVL_CHECK_ARG(x, "svl_text_embed_f32: x is null");
  SVL_CHECK_ARG(eot, "svl_text_embed_f32: eot is null");
  SVL_CHECK_ARG(n > 0, "svl_text_embed_f32: n %d < 1", n);
  SVL_CHECK_ARG(L > 0, "svl_text_embed_f32: L %d < 1", L);
  SVL_CHECK_ARG(V > 0, "svl_text_embed_f32: V %d < 1", V);
  SVL_CHECK_ARG(W > 0, "svl_text_embed_f32: W %d < 1", W);
  const long elems = (long)n * L * W;
  if (W % 4 == 0 && al16(table) && al16(pos) && al16(x))
    hipLaunchKernelGGL(text_embed_kernel<4>, dim3(grid_for(elems / 4)), dim3(256), 0, (hipStream_t)stream, tokens, table, pos,
                       (long)L, (long)V, (long)(W / 4), elems / 4, x);
  else
    hipLaunchKernelGGL(text_embed_kernel<1>, dim3(grid_for(elems)), dim3(256), 0, (hipStream_t)stream, tokens, table, pos,
                       (long)L, (long)V, (long)W, elems, x);
  SVL_LAUNCH_CHECK("svl_text_embed_f32");
  hipLaunchKernelGGL(text_eot_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, tokens, n, L, eot);
  SVL_LAUNCH_CHECK("svl_text_embed_f32");
  return SVL_OK;
}

extern "C" int svl_causal_attn_fwd_f32(const float* qkv, int n, int L, int H, float* out, svl_stream_t stream) {
  SVL_CHECK_ARG(qkv, "svl_causal_attn_fwd_f32: qkv is null");
  SVL_CHECK_ARG(out, "svl_causal_attn_fwd_f32: out is null");
  SVL_CHECK_ARG(n > 0, "svl_causal_attn_fwd_f32: n %d < 1", n);
  SVL_CHECK_ARG(L >= 1 && L <= 64 * MAXT, "svl_causal_attn_fwd_f32: L %d outside [1, %d]", L, 64 * MAXT);
  SVL_CHECK_ARG(H >= 1, "svl_causal_attn_fwd_f32: H %d < 1", H);
  SVL_CHECK_ARG((long)n * H <= INT32_MAX, "svl_causal_attn_fwd_f32: n %d x H %d blocks exceed the grid", n, H);
  const size_t lds = causal_lds_bytes(L);
  if (lds > 64 * 1024)   // idempotent per-device attribute, as svl_seqattn_fwd
    SVL_HIP_CHECK(hipFuncSetAttribute((const void*)causal_attn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(causal_attn_kernel, dim3(n * H), dim3(256), lds, (hipStream_t)stream, qkv, out, L, H);
  SVL_LAUNCH_CHECK("svl_causal_attn_fwd_f32");
  return SVL_OK;
}

extern "C" int svl_quickgelu_f32(const float* x, float* y, int64_t count, svl_stream_t stream) {
  SVL_CHECK_ARG(x, "svl_quickgelu_f32: x is null");
  SVL_CHECK_ARG(y, "svl_quickgelu_f32: y is null");
  SVL_CHECK_ARG(count > 0, "svl_quickgelu_f32: count %lld < 1", (long long)count);
  long done = 0;
  if (al16(x) && al16(y) && count >= 4) {
    const long nq = count / 4;
    hipLaunchKernelGGL(quickgelu_v4_kernel, dim3(grid_for(nq)), dim3(256), 0, (hipStream_t)stream, x, y, nq);
    SVL_LAUNCH_CHECK("svl_quickgelu_f32");
    done = nq * 4;
  }
  if (done < count) {   // the tail of an aligned pair, or everything when a pointer is off a 16-byte boundary
    hipLaunchKernelGGL(quickgelu_s_kernel, dim3(grid_for(count - done)), dim3(256), 0, (hipStream_t)stream, x, y, done,
                       (long)count);
    SVL_LAUNCH_CHECK("svl_quickgelu_f32");
  }
  return SVL_OK;
}

extern "C" int svl_gather_rows_f32(const float* x, const int* idx, int n, int L, int E, float* out, svl_stream_t stream) {
  SVL_CHECK_ARG(x, "svl_gather_rows_f32: x is null");
  SVL_CHECK_ARG(idx, "svl_gather_rows_f32: idx is null");
  SVL_CHECK_ARG(out, "svl_gather_rows_f32: out is null");
  SVL_CHECK_ARG(n > 0, "svl_gather_rows_f32: n %d < 1", n);
  SVL_CHECK_ARG(L > 0, "svl_gather_rows_f32: L %d < 1", L);
  SVL_CHECK_ARG(E > 0, "svl_gather_rows_f32: E %d < 1", E);
  const long total = (long)n * E;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, idx, (long)L, (long)E,
                     total, out);
  SVL_LAUNCH_CHECK("svl_gather_rows_f32");
  return SVL_OK;
}

extern "C" int svl_segment_mean_f32(const float* x, int64_t m, int E, const int* offsets, int N, float* out,
                                    svl_stream_t stream) {
  SVL_CHECK_ARG(x, "svl_segment_mean_f32: x is null");
  SVL_CHECK_ARG(offsets, "svl_segment_mean_f32: offsets is null");
  SVL_CHECK_ARG(out, "svl_segment_mean_f32: out is null");
  SVL_CHECK_ARG(m > 0, "svl_segment_mean_f32: m %lld < 1", (long long)m);
  SVL_CHECK_ARG(E > 0, "svl_segment_mean_f32: E %d < 1", E);
  SVL_CHECK_ARG(N > 0, "svl_segment_mean_f32: N %d < 1", N);
  SVL_CHECK_ARG(N <= m, "svl_segment_mean_f32: N %d segments over m %lld rows: one of them is empty", N, (long long)m);
  const long total = (long)N * E;
  hipLaunchKernelGGL(segment_mean_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, (long)m, (long)E,
                     offsets, total, out);
  SVL_LAUNCH_CHECK("svl_segment_mean_f32");
  return SVL_OK;
}
