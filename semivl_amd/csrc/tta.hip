// Test-time augmentation of the evaluator (mmseg 0.x MultiScaleFlipAug + EncoderDecoder.aug_test): svl_tta_view_f32 builds a
// resized / mirrored view of the image planes, svl_tta_accum_f32 forms the class scores of one view at the target
// resolution (bilinear resize, softmax or normalised probability sums, horizontal un-flip) and adds them, scaled, to the
// running mean in ONE pass over the [B, N, H, W] destination.  Index math: bilinear_index.h.
#include "svl_common.h"
#include "bilinear_index.h"

namespace {

// 256 CUs x 2048 threads: every wave slot of the chip once, the rest by grid stride.
constexpr long TTA_GRID_THREADS = 2048 * 256;

inline int grid_for(long n, int threads = 256) {
  long g = (n + threads - 1) / threads;
  if (g < 1) g = 1;
  if (g > TTA_GRID_THREADS / threads) g = TTA_GRID_THREADS / threads;
  return (int)g;
}

// V = 4: four consecutive output columns per thread, one 16 B store.  `same` (h == H && w == W, wave-uniform): the resize
// is the identity, so the element is moved, not interpolated (1 * v + 0 * v' would lose the sign of -0 and turn an
// infinity into NaN): a bit-exact copy, or with flip a bit-exact mirror.
template <int V>
__global__ __launch_bounds__(256) void tta_view_kernel(const float* __restrict__ x, long planes, int h, int w, int flip,
                                                       int H, int W, float* __restrict__ y) {
  const bool same = h == H && w == W;
  const float sh = area_scale(h, H, false), sw = area_scale(w, W, false);
  const int WV = W / V;
  const long total = planes * H * WV;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int oxq = (int)(i % WV) * V;
    const long t = i / WV;
    const int oy = (int)(t % H);
    const long pl = t / H;
    const float* b = x + pl * h * w;
    float o[V];
    if (same) {
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = b[(long)oy * w + (flip ? W - 1 - (oxq + j) : oxq + j)];
    } else {
      int y0, y1;
      float ly0, ly1;
      src_index(oy, sh, h, false, y0, y1, ly0, ly1);
      const float* r0 = b + (long)y0 * w;
      const float* r1 = b + (long)y1 * w;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        int x0, x1;
        float lx0, lx1;
        src_index(flip ? W - 1 - (oxq + j) : oxq + j, sw, w, false, x0, x1, lx0, lx1);
        o[j] = ly0 * (lx0 * r0[x0] + lx1 * r0[x1]) + ly1 * (lx0 * r1[x0] + lx1 * r1[x1]);
      }
    }
    if constexpr (V == 4) *reinterpret_cast<float4*>(y + i * 4) = make_float4(o[0], o[1], o[2], o[3]);
    else y[i] = o[0];
  }
}

// One thread owns V consecutive columns of one destination row (b, y) for ALL N classes: it is the only reader and the only
// writer of those N x V destination elements (no atomics; two runs agree bit for bit), and a wave's stores of one class are
// 64 x V consecutive floats with or without flip (the mirror is applied to the SOURCE column, xs = W - 1 - x).  The tap
// indices and weights are per pixel, not per class, and stay in registers (4 + 4 V of them) across the passes over the classes
// (kind 0: maximum, sum of exponentials, write; kind 1: total, write).
//
// CACHE: the N x V interpolated values of a thread are formed ONCE, in the first pass, and kept in LDS for the later ones, in
// a column of its own (class c of thread t at [c][t][V]: consecutive lanes, consecutive 4 V bytes, no bank conflict, and no
// barrier, since nobody else touches the column).  Recomputing them instead costs 4 gathered loads per value and pass, and the
// gathers, not the 4 N H W bytes of stores, then set the pace.  Blocks are single waves so that the N x V x 256 bytes of a
// block stay small next to the 160 KB of a CU (21.5 KB at N = 21, V = 4: 7 waves per CU).  !CACHE: the values are recomputed
// in every pass (blocks of 256 threads, no LDS); N x V registers do not exist at N = 150, and the source is the small operand
// (read with a 2 x 2 footprint shared by neighbouring lanes), so the re-reads are served by L1 / L2.  The launcher chooses.
template <int V, int KIND, bool CACHE>
__global__ __launch_bounds__(256) void tta_accum_kernel(const float* __restrict__ src, int B, int N, int h, int w, int align,
                                                        int flip, int H, int W, float scale, int accumulate,
                                                        float* __restrict__ dst) {
  extern __shared__ float4 tta_lds[];
  float* mine = reinterpret_cast<float*>(tta_lds) + threadIdx.x * V;
  const int cstride = blockDim.x * V;
  const float sh = area_scale(h, H, align), sw = area_scale(w, W, align);
  const int WV = W / V;
  const long total = (long)B * H * WV;
  const long hw = (long)h * w, HW = (long)H * W;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % WV) * V;
    const long t = i / WV;
    const int oy = (int)(t % H);
    const long b = t / H;
    int y0, y1, xa[V], xb[V];
    float ly0, ly1, la[V], lb[V];
    src_index(oy, sh, h, align, y0, y1, ly0, ly1);
#pragma unroll
    for (int j = 0; j < V; ++j) src_index(flip ? W - 1 - (ox + j) : ox + j, sw, w, align, xa[j], xb[j], la[j], lb[j]);
    const float* r0 = src + b * N * hw + (long)y0 * w;
    const float* r1 = src + b * N * hw + (long)y1 * w;
    auto interp = [&](int c, int j) {
      const float* p0 = r0 + c * hw;
      const float* p1 = r1 + c * hw;
      return ly0 * (la[j] * p0[xa[j]] + lb[j] * p0[xb[j]]) + ly1 * (la[j] * p1[xa[j]] + lb[j] * p1[xb[j]]);
    };
    auto value = [&](int c, int j) { return CACHE ? mine[c * cstride + j] : interp(c, j); };
    float m[V], s[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { m[j] = -INFINITY; s[j] = 0.f; }
#pragma unroll 4
    for (int c = 0; c < N; ++c) {
      float u[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        u[j] = interp(c, j);
        if constexpr (KIND == 0) m[j] = fmaxf(m[j], u[j]);
        else s[j] += u[j];
      }
      if constexpr (CACHE) {
        if constexpr (V == 4) *reinterpret_cast<float4*>(mine + c * cstride) = make_float4(u[0], u[1], u[2], u[3]);
        else mine[c * cstride] = u[0];
      }
    }
    if constexpr (KIND == 0) {
      for (int c = 0; c < N; ++c)
#pragma unroll
        for (int j = 0; j < V; ++j) s[j] += expf(value(c, j) - m[j]);
#pragma unroll
      for (int j = 0; j < V; ++j) s[j] = 1.f / s[j];
    }
    float* d = dst + (b * N * H + oy) * W + ox;
    for (int c = 0; c < N; ++c, d += HW) {
      float o[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float u = value(c, j);
        if constexpr (KIND == 0) o[j] = expf(u - m[j]) * s[j];
        else o[j] = s[j] == 0.f ? 0.f : u / s[j];
      }
      if constexpr (V == 4) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (accumulate) a = *reinterpret_cast<const float4*>(d);
        *reinterpret_cast<float4*>(d) = make_float4(a.x + scale * o[0], a.y + scale * o[1], a.z + scale * o[2], a.w + scale * o[3]);
      } else {
        const float a = accumulate ? d[0] : 0.f;
        d[0] = a + scale * o[0];
      }
    }
  }
}

// Which form runs.  A single-wave block's cached columns take N x V x 256 bytes of LDS; up to 24 KB (six waves per CU or more)
// caching wins (measured at N = 21: 27 - 31 us per view against 42 - 66 us recomputed), at N = 150 (37.5 KB, four waves per CU)
// it loses (564 - 856 us against 311 - 612 us): too few waves to cover the latency of the gathers and the destination reads.
//   16-byte stores possible and N <= 24   V = 4, cached
//   otherwise N <= 96                     V = 1, cached
//   otherwise                             recomputed in every pass, V = 4 where the stores allow it
constexpr int TTA_CACHE_N_V4 = 24, TTA_CACHE_N_V1 = 96;

template <int V, bool CACHE>
void launch_accum(const float* src, int B, int N, int h, int w, float* dst, int H, int W, int kind, int align, int flip,
                  float scale, int accumulate, hipStream_t st) {
  const int threads = CACHE ? 64 : 256;
  const dim3 grid(grid_for((long)B * H * (W / V), threads));
  const size_t lds = CACHE ? (size_t)N * V * threads * sizeof(float) : 0;
  if (kind == 0)
    hipLaunchKernelGGL((tta_accum_kernel<V, 0, CACHE>), grid, dim3(threads), lds, st, src, B, N, h, w, align, flip, H, W, scale,
                       accumulate, dst);
  else
    hipLaunchKernelGGL((tta_accum_kernel<V, 1, CACHE>), grid, dim3(threads), lds, st, src, B, N, h, w, align, flip, H, W, scale,
                       accumulate, dst);
}

}  // namespace

extern "C" int svl_tta_view_f32(const float* src, int64_t planes, int h, int w, int oh, int ow, int flip, float* dst,
                                svl_stream_t stream) {
  SVL_CHECK_ARG(src && dst && planes > 0 && h > 0 && w > 0 && oh > 0 && ow > 0, "svl_tta_view_f32: bad args");
  if (ow % 4 == 0 && ((uintptr_t)dst & 15) == 0)
    hipLaunchKernelGGL(tta_view_kernel<4>, dim3(grid_for(planes * oh * (ow / 4))), dim3(256), 0, (hipStream_t)stream, src,
                       (long)planes, h, w, flip ? 1 : 0, oh, ow, dst);
  else
    hipLaunchKernelGGL(tta_view_kernel<1>, dim3(grid_for(planes * oh * ow)), dim3(256), 0, (hipStream_t)stream, src,
                       (long)planes, h, w, flip ? 1 : 0, oh, ow, dst);
  SVL_LAUNCH_CHECK("svl_tta_view_f32");
  return SVL_OK;
}

extern "C" int svl_tta_accum_f32(const float* src, int B, int N, int h, int w, float* dst, int H, int W, int kind,
                                 int align_corners, int flip, float scale, int accumulate, svl_stream_t stream) {
  SVL_CHECK_ARG(src && dst && B > 0 && N > 0 && h > 0 && w > 0 && H > 0 && W > 0, "svl_tta_accum_f32: bad args");
  SVL_CHECK_ARG(kind == 0 || kind == 1, "svl_tta_accum_f32: kind %d (0: logits, 1: summed window probabilities)", kind);
  const int align = align_corners ? 1 : 0, fl = flip ? 1 : 0, acc = accumulate ? 1 : 0;
  const bool vec = W % 4 == 0 && ((uintptr_t)dst & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  if (vec && N <= TTA_CACHE_N_V4) launch_accum<4, true>(src, B, N, h, w, dst, H, W, kind, align, fl, scale, acc, st);
  else if (N <= TTA_CACHE_N_V1) launch_accum<1, true>(src, B, N, h, w, dst, H, W, kind, align, fl, scale, acc, st);
  else if (vec) launch_accum<4, false>(src, B, N, h, w, dst, H, W, kind, align, fl, scale, acc, st);
  else launch_accum<1, false>(src, B, N, h, w, dst, H, W, kind, align, fl, scale, acc, st);
  SVL_LAUNCH_CHECK("svl_tta_accum_f32");
  return SVL_OK;
}
