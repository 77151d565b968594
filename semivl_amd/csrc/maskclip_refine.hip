// MaskCLIP's two training-free refinements of a dense zero-shot prediction (maskclip_head.py:129-155): prompt denoising and
// key smoothing, as the streaming passes around the two svl_gemm_f32 products of k^ (k^T P) (include/semivl_hip.h).
// Every pass moves a few MB once: HBM / Infinity-Cache bound, no matrix-core work, no atomics, plain vector stores.
#include "svl_common.h"

#define MC_COLS 32        // columns of a column-reduction tile: 128 bytes of every row
#define MC_MAX_GRID 4096  // blocks of a launch; the tiles beyond are walked grid-stride

static inline bool mc_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// max that keeps a NaN once it has seen one (torch.max): NaN > m is false, so the second test takes it; a NaN m stays.
__device__ __forceinline__ float nanmax(float m, float v) { return (v > m || v != v) ? v : m; }

// ---------------------------------------------------------------------------------------------
// Column reductions per image: a block owns (image, 32-column tile), its 256 threads are CW column lanes x 256 / CW row lanes
// (VEC = 4: 8 lanes of one float4, VEC = 1: 32 scalar lanes).  A row lane walks its rows in ascending order, the row lanes
// are folded in ascending order: one fixed order per (HW, C, VEC).
// ---------------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void mc_class_peak_kernel(const float* __restrict__ P, long ld, int B, int HW, int N,
                                                            float* __restrict__ peak) {
  constexpr int CW = MC_COLS / VEC, RL = 256 / CW;
  __shared__ float red[RL][MC_COLS + 1];
  const int cl = threadIdx.x % CW, rl = threadIdx.x / CW;
  const int ctiles = (N + MC_COLS - 1) / MC_COLS;
  for (long t = blockIdx.x; t < (long)B * ctiles; t += gridDim.x) {
    const int b = (int)(t / ctiles), c0 = (int)(t % ctiles) * MC_COLS + cl * VEC;
    float m[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) m[j] = -INFINITY;
    if (c0 < N) {   // VEC = 4 only runs with N % 4 == 0: a lane's four columns are inside together
      const float* src = P + (long)b * HW * ld + c0;
      for (int r = rl; r < HW; r += RL) {
        if constexpr (VEC == 4) {
          const float4 v = *reinterpret_cast<const float4*>(src + (long)r * ld);
          m[0] = nanmax(m[0], v.x); m[1] = nanmax(m[1], v.y); m[2] = nanmax(m[2], v.z); m[3] = nanmax(m[3], v.w);
        } else {
          m[0] = nanmax(m[0], src[(long)r * ld]);
        }
      }
    }
    __syncthreads();   // the tile before has been read out of red
#pragma unroll
    for (int j = 0; j < VEC; ++j) red[rl][cl * VEC + j] = m[j];
    __syncthreads();
    if (threadIdx.x < MC_COLS) {
      const int c = (int)(t % ctiles) * MC_COLS + threadIdx.x;
      if (c < N) {
        float a = red[0][threadIdx.x];
        for (int q = 1; q < RL; ++q) a = nanmax(a, red[q][threadIdx.x]);
        peak[(long)b * N + c] = a;
      }
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(256) void col_invsq_kernel(const float* __restrict__ k, long ld, int B, int HW, int E, double eps,
                                                        float* __restrict__ s) {
  constexpr int CW = MC_COLS / VEC, RL = 256 / CW;
  __shared__ double red[RL][MC_COLS + 1];
  const int cl = threadIdx.x % CW, rl = threadIdx.x / CW;
  const int ctiles = (E + MC_COLS - 1) / MC_COLS;
  for (long t = blockIdx.x; t < (long)B * ctiles; t += gridDim.x) {
    const int b = (int)(t / ctiles), c0 = (int)(t % ctiles) * MC_COLS + cl * VEC;
    double q[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) q[j] = 0.0;
    if (c0 < E) {
      const float* src = k + (long)b * HW * ld + c0;
      for (int r = rl; r < HW; r += RL) {
        if constexpr (VEC == 4) {
          const float4 v = *reinterpret_cast<const float4*>(src + (long)r * ld);
          q[0] += (double)v.x * v.x; q[1] += (double)v.y * v.y; q[2] += (double)v.z * v.z; q[3] += (double)v.w * v.w;
        } else {
          const float v = src[(long)r * ld];
          q[0] += (double)v * v;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < VEC; ++j) red[rl][cl * VEC + j] = q[j];
    __syncthreads();
    if (threadIdx.x < MC_COLS) {
      const int c = (int)(t % ctiles) * MC_COLS + threadIdx.x;
      if (c < E) {
        double a = red[0][threadIdx.x];
        for (int i = 1; i < RL; ++i) a += red[i][threadIdx.x];
        const double n = fmax(sqrt(a), eps);     // F.normalize: x / max(||x||, eps); the square of it divides k^ k^T
        s[(long)b * E + c] = (float)(1.0 / (n * n));
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Masked row softmax, one wave per token row (N is a class count: 21 .. 171 on the project's data; the two re-reads of a
// row hit L1).  z_c = 100 x_c, or -10000 where the class was dropped (peak < pd_thresh; a NaN peak keeps its class).
// fill_only: the filled logits themselves are written (x, or -100), no softmax.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mc_softmax_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ peak,
                                                         float pd, long rows, int HW, int N, int fill_only,
                                                         float* __restrict__ P, long ldp, float* __restrict__ rowmax) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long r = (long)blockIdx.x * 4 + wave; r < rows; r += (long)gridDim.x * 4) {
    const float* xr = x + r * ldx;
    const float* pk = peak ? peak + (r / HW) * N : nullptr;
    float* pr = P + r * ldp;
    if (fill_only) {
      for (int i = lane; i < N; i += 64) pr[i] = (pk && pk[i] < pd) ? -100.f : xr[i];
      continue;
    }
    float m = -INFINITY;
    for (int i = lane; i < N; i += 64) m = fmaxf(m, ((pk && pk[i] < pd) ? -100.f : xr[i]) * 100.f);
    m = wave_max(m);
    float sum = 0.f;
    for (int i = lane; i < N; i += 64) sum += expf(((pk && pk[i] < pd) ? -100.f : xr[i]) * 100.f - m);
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    float pm = -INFINITY;
    for (int i = lane; i < N; i += 64) {
      const float p = expf(((pk && pk[i] < pd) ? -100.f : xr[i]) * 100.f - m) * inv;
      pr[i] = p;
      pm = nanmax(pm, p);
    }
    if (rowmax) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) pm = nanmax(pm, __shfl_xor(pm, o, 64));
      if (lane == 0) rowmax[r] = pm;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Row select + transpose into class planes: out[b, c, i] = (rowmax[b HW + i] < ks) ? O[b HW + i, c] : P[b HW + i, c].
// A block moves tiles of 64 tokens x 32 classes through LDS: token rows are read along the classes, planes are written along
// the tokens (float4 when HW % 4 == 0 and out is 16-byte aligned).
// ---------------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void mc_select_kernel(const float* __restrict__ P, long ldp, const float* __restrict__ O,
                                                        long ldo, const float* __restrict__ rowmax, float ks, int B, int HW,
                                                        int N, float* __restrict__ out) {
  __shared__ float tile[64][32 + 1];     // [token][class], odd pitch: both the row-wise fill and the column-wise read spread over the banks
  const int rt = (HW + 63) / 64, ct = (N + 31) / 32;
  for (long t = blockIdx.x; t < (long)B * rt * ct; t += gridDim.x) {
    const int b = (int)(t / ((long)rt * ct));
    const int i0 = (int)((t / ct) % rt) * 64, c0 = (int)(t % ct) * 32;
    __syncthreads();   // the tile before has been written out
    {
      const int c = threadIdx.x & 31, c_g = c0 + c;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = (threadIdx.x >> 5) + 8 * j, i_g = i0 + i;
        if (i_g < HW && c_g < N) {
          const long row = (long)b * HW + i_g;
          const bool sel = O && rowmax && rowmax[row] < ks;      // a NaN maximum keeps P (NaN < ks is false)
          tile[i][c] = sel ? O[row * ldo + c_g] : P[row * ldp + c_g];
        }
      }
    }
    __syncthreads();
    if constexpr (VEC == 4) {
      const int i = (threadIdx.x & 15) * 4, i_g = i0 + i;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = (threadIdx.x >> 4) + 16 * j, c_g = c0 + c;
        if (i_g < HW && c_g < N)   // HW % 4 == 0: the four tokens are inside together
          *reinterpret_cast<float4*>(out + ((long)b * N + c_g) * HW + i_g) =
              make_float4(tile[i][c], tile[i + 1][c], tile[i + 2][c], tile[i + 3][c]);
      }
    } else {
      const int i = threadIdx.x & 63, i_g = i0 + i;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = (threadIdx.x >> 6) + 4 * j, c_g = c0 + c;
        if (i_g < HW && c_g < N) out[((long)b * N + c_g) * HW + i_g] = tile[i][c];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
static inline int mc_grid(long tiles) { return (int)(tiles < MC_MAX_GRID ? tiles : MC_MAX_GRID); }

extern "C" int svl_mc_class_peak_f32(const float* P, int64_t ld, int B, int HW, int N, float* peak, svl_stream_t stream) {
  SVL_CHECK_ARG(P && peak, "svl_mc_class_peak_f32: null pointer (P %p, peak %p)", (const void*)P, (void*)peak);
  SVL_CHECK_ARG(B >= 1 && HW >= 1 && N >= 1, "svl_mc_class_peak_f32: B %d, HW %d, N %d must be >= 1", B, HW, N);
  SVL_CHECK_ARG(ld >= N, "svl_mc_class_peak_f32: ld %lld below the width N %d", (long long)ld, N);
  const int grid = mc_grid((long)B * ((N + MC_COLS - 1) / MC_COLS));
  if (N % 4 == 0 && ld % 4 == 0 && mc_al16(P))
    hipLaunchKernelGGL(mc_class_peak_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, P, (long)ld, B, HW, N, peak);
  else
    hipLaunchKernelGGL(mc_class_peak_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, P, (long)ld, B, HW, N, peak);
  SVL_LAUNCH_CHECK("svl_mc_class_peak_f32");
  return SVL_OK;
}

extern "C" int svl_col_invsq_f32(const float* k, int64_t ld, int B, int HW, int E, float eps, float* s, svl_stream_t stream) {
  SVL_CHECK_ARG(k && s, "svl_col_invsq_f32: null pointer (k %p, s %p)", (const void*)k, (void*)s);
  SVL_CHECK_ARG(B >= 1 && HW >= 1 && E >= 1, "svl_col_invsq_f32: B %d, HW %d, E %d must be >= 1", B, HW, E);
  SVL_CHECK_ARG(ld >= E, "svl_col_invsq_f32: ld %lld below the width E %d", (long long)ld, E);
  SVL_CHECK_ARG(eps >= 0.f, "svl_col_invsq_f32: eps %g must be >= 0", (double)eps);
  const int grid = mc_grid((long)B * ((E + MC_COLS - 1) / MC_COLS));
  if (E % 4 == 0 && ld % 4 == 0 && mc_al16(k))
    hipLaunchKernelGGL(col_invsq_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, k, (long)ld, B, HW, E, (double)eps, s);
  else
    hipLaunchKernelGGL(col_invsq_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, k, (long)ld, B, HW, E, (double)eps, s);
  SVL_LAUNCH_CHECK("svl_col_invsq_f32");
  return SVL_OK;
}

extern "C" int svl_mc_softmax_f32(const float* x, int64_t ldx, const float* peak, float pd_thresh, int B, int HW, int N,
                                  int fill_only, float* P, int64_t ldp, float* rowmax, svl_stream_t stream) {
  SVL_CHECK_ARG(x && P, "svl_mc_softmax_f32: null pointer (x %p, P %p)", (const void*)x, (void*)P);
  SVL_CHECK_ARG(B >= 1 && HW >= 1 && N >= 1, "svl_mc_softmax_f32: B %d, HW %d, N %d must be >= 1", B, HW, N);
  SVL_CHECK_ARG(ldx >= N && ldp >= N, "svl_mc_softmax_f32: ldx %lld / ldp %lld below the width N %d", (long long)ldx,
                (long long)ldp, N);
  SVL_CHECK_ARG(pd_thresh >= 0.f, "svl_mc_softmax_f32: pd_thresh %g must be >= 0", (double)pd_thresh);
  SVL_CHECK_ARG(!(fill_only && rowmax), "svl_mc_softmax_f32: fill_only writes logits, they have no rowmax");
  const long rows = (long)B * HW;
  const int grid = mc_grid((rows + 3) / 4);
  hipLaunchKernelGGL(mc_softmax_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, peak, pd_thresh, rows, HW,
                     N, fill_only, P, (long)ldp, rowmax);
  SVL_LAUNCH_CHECK("svl_mc_softmax_f32");
  return SVL_OK;
}

extern "C" int svl_mc_select_f32(const float* P, int64_t ldp, const float* O, int64_t ldo, const float* rowmax, float ks_thresh,
                                 int B, int HW, int N, float* out, svl_stream_t stream) {
  SVL_CHECK_ARG(P && out, "svl_mc_select_f32: null pointer (P %p, out %p)", (const void*)P, (void*)out);
  SVL_CHECK_ARG((O == nullptr) == (rowmax == nullptr), "svl_mc_select_f32: O and rowmax come together or not at all");
  SVL_CHECK_ARG(B >= 1 && HW >= 1 && N >= 1, "svl_mc_select_f32: B %d, HW %d, N %d must be >= 1", B, HW, N);
  SVL_CHECK_ARG(ldp >= N && (!O || ldo >= N), "svl_mc_select_f32: ldp %lld / ldo %lld below the width N %d", (long long)ldp,
                (long long)ldo, N);
  SVL_CHECK_ARG(ks_thresh >= 0.f, "svl_mc_select_f32: ks_thresh %g must be >= 0", (double)ks_thresh);
  const int grid = mc_grid((long)B * ((HW + 63) / 64) * ((N + 31) / 32));
  if (HW % 4 == 0 && mc_al16(out))
    hipLaunchKernelGGL(mc_select_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, P, (long)ldp, O, (long)ldo, rowmax,
                       ks_thresh, B, HW, N, out);
  else
    hipLaunchKernelGGL(mc_select_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, P, (long)ldp, O, (long)ldo, rowmax,
                       ks_thresh, B, HW, N, out);
  SVL_LAUNCH_CHECK("svl_mc_select_f32");
  return SVL_OK;
}
