// Debug panels of the training driver (panel.py): the per-epoch figure of semivl.py:371-406 / utils/plot_utils.py drawn on the
// device.  Two streaming kernels write RGB tiles into one u8 canvas [B][rows * S][4 * S][3]: a normalised fp32 NCHW image
// de-normalised to bytes, and an int64 label map looked up in a palette.  Both read their input once with 16-byte loads and
// write 12 bytes (4 pixels) per thread: three 4-byte stores where the destination address is 4-byte aligned, single bytes
// otherwise -- a tile may start at any byte of the canvas.  No atomics, nothing depends on the order: reruns agree bit for bit.
//
// A thread's 4 pixels are consecutive in the sample's flattened H x W index (they may run over a row's end when W % 4 != 0;
// such a group, and the last one of a sample when H W % 4 != 0, is written pixel by pixel).  The planes of a sample start at
// multiples of H W elements, so a group's loads are only element-aligned in general: the vector types below carry the
// element's alignment, which gfx950's global loads take at full width.
#include "svl_common.h"

namespace {

constexpr int PANEL_MAX_GRID = 256;   // one block per CU, the rest is grid-strided: 256 x 256 threads x 4 pixels per trip

typedef float f32x4_e __attribute__((ext_vector_type(4), aligned(4)));
typedef long long i64x2_e __attribute__((ext_vector_type(2), aligned(8)));

struct PanelNorm { float mean[3], std[3]; };

// The group's pixels px[e] = r | g << 8 | b << 16 (e < n) to the tile: sample b, flattened pixel p0 ..
__device__ __forceinline__ void store_group(const unsigned int (&px)[4], int n, int b, unsigned int p0, unsigned int W,
                                            uint8_t* __restrict__ dst, long bs, long rs) {
  const unsigned int y = p0 / W, x = p0 - y * W;
  uint8_t* o = dst + (long)b * bs + (long)y * rs + 3L * x;
  if (n == 4 && x + 3 < W && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
    unsigned int* o4 = reinterpret_cast<unsigned int*>(o);
    o4[0] = px[0] | (px[1] << 24);
    o4[1] = (px[1] >> 8) | (px[2] << 16);
    o4[2] = (px[2] >> 16) | (px[3] << 8);
    return;
  }
  unsigned int xe = x;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e < n) {
      o[0] = (uint8_t)px[e]; o[1] = (uint8_t)(px[e] >> 8); o[2] = (uint8_t)(px[e] >> 16);
      if (++xe == W) { xe = 0; o += rs - 3L * (W - 1); } else { o += 3; }
    }
  }
}

// v = x * std + mean, clamped to [0, 1] (NaN -> 0), then (uint8)(v * 255 + 0.5): every product and every sum rounded once --
// the bytes are compared exactly with a numpy restatement of torch's .mul(std).add(mean).  (The pragma, not __fmul_rn /
// __fadd_rn: under the default -ffp-contract=fast those two were fused into v_fma_f32 here, read in the assembly.)
__device__ __forceinline__ unsigned int to_byte(float x, float s, float m) {
#pragma clang fp contract(off)
  const float t = x * s;
  float v = t + m;
  v = v > 0.f ? v : 0.f;     // NaN compares false: 0
  v = v < 1.f ? v : 1.f;
  const float u = v * 255.0f;
  return (unsigned int)(u + 0.5f);
}

__global__ __launch_bounds__(256) void panel_image_kernel(const float* __restrict__ img, int B, unsigned int HW, unsigned int W,
                                                          PanelNorm nm, uint8_t* __restrict__ dst, long bs, long rs) {
  const unsigned int G = (HW + 3) / 4, total = (unsigned int)B * G;
  for (unsigned int i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned int b = i / G, p0 = (i - b * G) * 4;
    const int n = HW - p0 < 4u ? (int)(HW - p0) : 4;
    unsigned int px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* src = img + ((long)b * 3 + c) * HW + p0;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (n == 4) {
        const f32x4_e q = *reinterpret_cast<const f32x4_e*>(src);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
#pragma unroll
        for (int e = 0; e < 3; ++e)
          if (e < n) v[e] = src[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) px[e] |= to_byte(v[e], nm.std[c], nm.mean[c]) << (8 * c);
    }
    store_group(px, n, (int)b, p0, W, dst, bs, rs);
  }
}

__global__ __launch_bounds__(256) void panel_label_kernel(const int64_t* __restrict__ label, int B, unsigned int HW,
                                                          unsigned int W, const uint8_t* __restrict__ palette, int K,
                                                          uint8_t* __restrict__ dst, long bs, long rs) {
  __shared__ unsigned int pal[256];
  {
    const int k = threadIdx.x;
    pal[k] = k < K ? ((unsigned int)palette[3 * k] | ((unsigned int)palette[3 * k + 1] << 8) |
                      ((unsigned int)palette[3 * k + 2] << 16)) : 0xFFFFFFu;
  }
  __syncthreads();
  const unsigned int G = (HW + 3) / 4, total = (unsigned int)B * G;
  for (unsigned int i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned int b = i / G, p0 = (i - b * G) * 4;
    const int n = HW - p0 < 4u ? (int)(HW - p0) : 4;
    const int64_t* src = label + (long)b * HW + p0;
    long long l[4] = {-1, -1, -1, -1};
    if (n == 4) {
      const i64x2_e q0 = *reinterpret_cast<const i64x2_e*>(src);
      const i64x2_e q1 = *reinterpret_cast<const i64x2_e*>(src + 2);
      l[0] = q0.x; l[1] = q0.y; l[2] = q1.x; l[3] = q1.y;
    } else {
#pragma unroll
      for (int e = 0; e < 3; ++e)
        if (e < n) l[e] = src[e];
    }
    unsigned int px[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)   // the key is checked before anything is indexed with it: -1, K, 254, 255, 2^40 stay white
      px[e] = (unsigned long long)l[e] < (unsigned long long)K ? pal[(int)l[e]] : 0xFFFFFFu;
    store_group(px, n, (int)b, p0, W, dst, bs, rs);
  }
}

// What both entry points refuse about the tile; the caller (panel.py) checks that the tile lies inside its canvas.
int check_tile(const char* name, const void* src, int B, int H, int W, const void* dst, int64_t bs, int64_t rs) {
  SVL_CHECK_ARG(src && dst, "%s: null pointer", name);
  SVL_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "%s: B = %d, H = %d, W = %d: every one must be >= 1", name, B, H, W);
  SVL_CHECK_ARG((int64_t)B * H * W + 3 < (1LL << 31), "%s: B H W = %lld pixels do not fit the kernel's 32-bit index", name,
                (long long)B * H * W);
  SVL_CHECK_ARG(rs >= 3LL * W, "%s: row_stride = %lld bytes < 3 W = %lld: the tile's rows would overlap", name, (long long)rs,
                3LL * W);
  SVL_CHECK_ARG(B == 1 || bs >= (int64_t)(H - 1) * rs + 3LL * W,
                "%s: batch_stride = %lld bytes < (H - 1) row_stride + 3 W = %lld: the samples' tiles would overlap", name,
                (long long)bs, (long long)((int64_t)(H - 1) * rs + 3LL * W));
  return SVL_OK;
}

unsigned panel_grid(int B, int H, int W) {
  const long groups = (long)B * (((long)H * W + 3) / 4);
  const long grid = (groups + 255) / 256;
  return (unsigned)(grid > PANEL_MAX_GRID ? PANEL_MAX_GRID : grid);
}

}  // namespace

extern "C" int svl_panel_image_u8(const float* img, int B, int H, int W, const float* mean3, const float* std3, uint8_t* dst,
                                  int64_t batch_stride, int64_t row_stride, svl_stream_t stream) {
  if (int rc = check_tile("svl_panel_image_u8", img, B, H, W, dst, batch_stride, row_stride)) return rc;
  SVL_CHECK_ARG(mean3 && std3, "svl_panel_image_u8: null mean3 / std3 (host pointers to 3 floats each)");
  SVL_CHECK_ARG(reinterpret_cast<uintptr_t>(img) % 4 == 0, "svl_panel_image_u8: img is not 4-byte aligned");
  PanelNorm nm;
  for (int c = 0; c < 3; ++c) { nm.mean[c] = mean3[c]; nm.std[c] = std3[c]; }
  hipLaunchKernelGGL(panel_image_kernel, dim3(panel_grid(B, H, W)), dim3(256), 0, (hipStream_t)stream, img, B,
                     (unsigned int)(H * W), (unsigned int)W, nm, dst, (long)batch_stride, (long)row_stride);
  SVL_LAUNCH_CHECK("svl_panel_image_u8");
  return SVL_OK;
}

extern "C" int svl_panel_label_u8(const int64_t* label, int B, int H, int W, const uint8_t* palette, int K, uint8_t* dst,
                                  int64_t batch_stride, int64_t row_stride, svl_stream_t stream) {
  if (int rc = check_tile("svl_panel_label_u8", label, B, H, W, dst, batch_stride, row_stride)) return rc;
  SVL_CHECK_ARG(palette, "svl_panel_label_u8: null palette");
  SVL_CHECK_ARG(K >= 1 && K <= 256, "svl_panel_label_u8: K = %d outside [1, 256]", K);
  SVL_CHECK_ARG(reinterpret_cast<uintptr_t>(label) % 8 == 0, "svl_panel_label_u8: label is not 8-byte aligned");
  hipLaunchKernelGGL(panel_label_kernel, dim3(panel_grid(B, H, W)), dim3(256), 0, (hipStream_t)stream, label, B,
                     (unsigned int)(H * W), (unsigned int)W, palette, K, dst, (long)batch_stride, (long)row_stride);
  SVL_LAUNCH_CHECK("svl_panel_label_u8");
  return SVL_OK;
}
