// Fused multi-tensor AdamW over a flat parameter arena (semivl.py:123-125,328: torch.optim.AdamW with one param
// group per tensor as built by mmcv's DefaultOptimizerConstructor; poly LR is rewritten into seg_lr by the host,
// semivl.py:339-345).  One launch replaces ~120 tensors x ~6 ATen kernels.  HBM-bound: 28 B per parameter.
#include "svl_common.h"

namespace {

// The gradient scale of a step kernel: a host float passed by value (svl_adamw_step, svl_sgd_step), or ONE device float the
// kernel reads (the *_dscale entry points: stats[2] of svl_grad_clip_f32).  Same arithmetic after the read, so the same
// scale value gives the same bits.
__device__ __forceinline__ float scale_of(float s) { return s; }
__device__ __forceinline__ float scale_of(const float* s) { return *s; }

template <typename SCALE>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v,
                                                    const long long* __restrict__ seg_off,
                                                    const float* __restrict__ seg_lr, const float* __restrict__ seg_wd,
                                                    int nseg, long total, float beta1, float beta2, float eps,
                                                    float bc1, float bc2_sqrt, SCALE gscale_arg, float* __restrict__ ema,
                                                    float ema_decay) {
  const float gscale = scale_of(gscale_arg);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    // segment lookup: largest s with seg_off[s] <= i
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (seg_off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const float lr = seg_lr[lo], wd = seg_wd[lo];
    const float gr = g[i] * gscale;
    float pw = p[i];
    pw *= (1.f - lr * wd);
    float mm = m[i];
    mm = mm + (gr - mm) * (1.f - beta1);  // exp_avg.lerp_(grad, 1 - beta1)
    float vv = v[i] * beta2 + (1.f - beta2) * gr * gr;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    pw = pw - (lr / bc1) * (mm / denom);
    p[i] = pw;
    m[i] = mm;
    v[i] = vv;
    if (ema) ema[i] = ema_decay * ema[i] + (1.f - ema_decay) * pw;
  }
}

// torch.optim.SGD (maximize=False) over the same arena (semivl.py:118-121: the optimizer the reference builds when cfg has
// no 'optimizer' key; its two learning rates are rewritten into seg_lr by the host, semivl.py:330-337).  HBM-bound: 20 B
// per parameter (28 with EMA).  One 16-byte load / store per lane and array: segments start on 16-byte boundaries, so a
// float4 lies in one segment.  A block's trip covers SGD_TRIP consecutive floats; the segments of its first and last float
// are block-uniform (scalar binary searches), and a lane searches only between them -- not at all on the trips, nearly
// every one on a real model, that lie inside one tensor.
constexpr int SGD_THREADS = 256;
constexpr int SGD_TRIP = SGD_THREADS * 4;   // floats per block and trip
constexpr long SGD_GRID_CAP = 2048;         // 256 CUs x 8 blocks; longer arenas take further trips

__device__ __forceinline__ int seg_search(const long long* __restrict__ seg_off, int lo, int hi, long i) {
  while (lo < hi) {  // largest s in [lo, hi] with seg_off[s] <= i
    const int mid = (lo + hi + 1) >> 1;
    if (seg_off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <bool MOM, bool FIRST, bool NEST>
__device__ __forceinline__ void sgd_elem(float& pw, float gr, float& mm, float lr, float wd, float momentum, float omd,
                                         float gscale) {
  float d = gr * gscale + wd * pw;
  if (MOM) {
    mm = FIRST ? d : momentum * mm + omd * d;
    d = NEST ? d + momentum * mm : mm;
  }
  pw = pw - lr * d;
}

template <bool MOM, bool FIRST, bool NEST, bool EMA, typename SCALE>
__global__ __launch_bounds__(SGD_THREADS) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, const long long* __restrict__ seg_off,
                                                          const float* __restrict__ seg_lr,
                                                          const float* __restrict__ seg_wd, int nseg, long total,
                                                          float momentum, float omd, SCALE gscale_arg,
                                                          float* __restrict__ ema, float ema_decay, float ema_omd) {
  const float gscale = scale_of(gscale_arg);
  for (long base = (long)blockIdx.x * SGD_TRIP; base < total; base += (long)gridDim.x * SGD_TRIP) {
    const long last = (base + SGD_TRIP <= total ? base + SGD_TRIP : total) - 1;
    const int s_lo = seg_search(seg_off, 0, nseg - 1, base);
    const int s_hi = seg_search(seg_off, s_lo, nseg - 1, last);
    const long i = base + (long)threadIdx.x * 4;
    if (i >= total) continue;
    const int s = seg_search(seg_off, s_lo, s_hi, i);
    const float lr = seg_lr[s], wd = seg_wd[s];
    if (i + 4 <= total) {
      float4 pw = *reinterpret_cast<const float4*>(p + i);
      const float4 gr = *reinterpret_cast<const float4*>(g + i);
      float4 mm = make_float4(0.f, 0.f, 0.f, 0.f);
      if (MOM && !FIRST) mm = *reinterpret_cast<const float4*>(m + i);
      float4 ev;
      if (EMA) ev = *reinterpret_cast<const float4*>(ema + i);
      sgd_elem<MOM, FIRST, NEST>(pw.x, gr.x, mm.x, lr, wd, momentum, omd, gscale);
      sgd_elem<MOM, FIRST, NEST>(pw.y, gr.y, mm.y, lr, wd, momentum, omd, gscale);
      sgd_elem<MOM, FIRST, NEST>(pw.z, gr.z, mm.z, lr, wd, momentum, omd, gscale);
      sgd_elem<MOM, FIRST, NEST>(pw.w, gr.w, mm.w, lr, wd, momentum, omd, gscale);
      *reinterpret_cast<float4*>(p + i) = pw;
      if (MOM) *reinterpret_cast<float4*>(m + i) = mm;
      if (EMA) {
        ev.x = ema_decay * ev.x + ema_omd * pw.x;
        ev.y = ema_decay * ev.y + ema_omd * pw.y;
        ev.z = ema_decay * ev.z + ema_omd * pw.z;
        ev.w = ema_decay * ev.w + ema_omd * pw.w;
        *reinterpret_cast<float4*>(ema + i) = ev;
      }
    } else {  // total % 4 != 0: the last, partial float4 (it starts a 16-byte unit, so it too lies in segment s)
      for (long j = i; j < total; ++j) {
        float pw = p[j], mm = (MOM && !FIRST) ? m[j] : 0.f;
        sgd_elem<MOM, FIRST, NEST>(pw, g[j], mm, lr, wd, momentum, omd, gscale);
        p[j] = pw;
        if (MOM) m[j] = mm;
        if (EMA) ema[j] = ema_decay * ema[j] + ema_omd * pw;
      }
    }
  }
}

template <bool MOM, bool FIRST, bool NEST, typename SCALE>
void sgd_launch(bool with_ema, unsigned grid, hipStream_t st, float* p, const float* g, float* m, const long long* seg_off,
                const float* seg_lr, const float* seg_wd, int nseg, long total, float momentum, float omd, SCALE gscale,
                float* ema, float ema_decay, float ema_omd) {
  if (with_ema)
    hipLaunchKernelGGL((sgd_kernel<MOM, FIRST, NEST, true, SCALE>), dim3(grid), dim3(SGD_THREADS), 0, st, p, g, m, seg_off,
                       seg_lr, seg_wd, nseg, total, momentum, omd, gscale, ema, ema_decay, ema_omd);
  else
    hipLaunchKernelGGL((sgd_kernel<MOM, FIRST, NEST, false, SCALE>), dim3(grid), dim3(SGD_THREADS), 0, st, p, g, m, seg_off,
                       seg_lr, seg_wd, nseg, total, momentum, omd, gscale, ema, ema_decay, ema_omd);
}

template <typename SCALE>
int adamw_step(const char* name, float* p, const float* g, float* m, float* v, const int64_t* seg_off, const float* seg_lr,
               const float* seg_wd, int nseg, int64_t total, float beta1, float beta2, float eps, int step, SCALE gscale,
               float* ema, float ema_decay, svl_stream_t stream) {
  SVL_CHECK_ARG(p && g && m && v && seg_off && seg_lr && seg_wd && nseg > 0 && total > 0 && step >= 1, "%s: bad args",
                name);
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  long grid = (total + 1023) / 1024;
  if (grid > 4096) grid = 4096;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(adamw_kernel<SCALE>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                     (const long long*)seg_off, seg_lr, seg_wd, nseg, (long)total, beta1, beta2, eps, (float)bc1,
                     (float)sqrt(bc2), gscale, ema, ema_decay);
  SVL_LAUNCH_CHECK(name);
  return SVL_OK;
}

template <typename SCALE>
int sgd_step(const char* name, float* p, const float* g, float* m, const int64_t* seg_off, const float* seg_lr,
             const float* seg_wd, int nseg, int64_t total, float momentum, float dampening, int nesterov, int step,
             SCALE gscale, float* ema, float ema_decay, svl_stream_t stream) {
  SVL_CHECK_ARG(p && g && seg_off && seg_lr && seg_wd && nseg > 0 && total > 0 && step >= 1, "%s: bad args", name);
  SVL_CHECK_ARG(m || momentum == 0.f, "%s: momentum %g needs a momentum buffer (m is null)", name, (double)momentum);
  SVL_CHECK_ARG(!nesterov || (momentum > 0.f && dampening == 0.f),
                "%s: nesterov momentum requires a momentum and zero dampening (momentum %g, dampening %g)", name,
                (double)momentum, (double)dampening);
  SVL_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)ema) & 15) == 0,
                "%s: p, g, m and ema must be 16-byte aligned", name);
  const float omd = (float)(1.0 - (double)dampening), ema_omd = (float)(1.0 - (double)ema_decay);
  long grid = (total + SGD_TRIP - 1) / SGD_TRIP;
  if (grid > SGD_GRID_CAP) grid = SGD_GRID_CAP;
  const bool mom = momentum != 0.f, first = step == 1, with_ema = ema != nullptr;
  const hipStream_t st = (hipStream_t)stream;
  const long long* so = (const long long*)seg_off;
#define SVL_SGD_GO(MOM, FIRST, NEST)                                                                                     \
  sgd_launch<MOM, FIRST, NEST, SCALE>(with_ema, (unsigned)grid, st, p, g, m, so, seg_lr, seg_wd, nseg, (long)total, momentum, \
                                      omd, gscale, ema, ema_decay, ema_omd)
  if (!mom) SVL_SGD_GO(false, false, false);
  else if (first && nesterov) SVL_SGD_GO(true, true, true);
  else if (first) SVL_SGD_GO(true, true, false);
  else if (nesterov) SVL_SGD_GO(true, false, true);
  else SVL_SGD_GO(true, false, false);
#undef SVL_SGD_GO
  SVL_LAUNCH_CHECK(name);
  return SVL_OK;
}

}  // namespace

extern "C" int svl_adamw_step(float* p, const float* g, float* m, float* v, const int64_t* seg_off, const float* seg_lr,
                              const float* seg_wd, int nseg, int64_t total, float beta1, float beta2, float eps, int step,
                              float gscale, float* ema, float ema_decay, svl_stream_t stream) {
  return adamw_step<float>("svl_adamw_step", p, g, m, v, seg_off, seg_lr, seg_wd, nseg, total, beta1, beta2, eps, step,
                           gscale, ema, ema_decay, stream);
}

extern "C" int svl_adamw_step_dscale(float* p, const float* g, float* m, float* v, const int64_t* seg_off,
                                     const float* seg_lr, const float* seg_wd, int nseg, int64_t total, float beta1,
                                     float beta2, float eps, int step, const float* gscale_dev, float* ema,
                                     float ema_decay, svl_stream_t stream) {
  SVL_CHECK_ARG(gscale_dev, "svl_adamw_step_dscale: gscale_dev is null");
  return adamw_step<const float*>("svl_adamw_step_dscale", p, g, m, v, seg_off, seg_lr, seg_wd, nseg, total, beta1, beta2,
                                  eps, step, gscale_dev, ema, ema_decay, stream);
}

extern "C" int svl_sgd_step(float* p, const float* g, float* m, const int64_t* seg_off, const float* seg_lr,
                            const float* seg_wd, int nseg, int64_t total, float momentum, float dampening, int nesterov,
                            int step, float gscale, float* ema, float ema_decay, svl_stream_t stream) {
  return sgd_step<float>("svl_sgd_step", p, g, m, seg_off, seg_lr, seg_wd, nseg, total, momentum, dampening, nesterov, step,
                         gscale, ema, ema_decay, stream);
}

extern "C" int svl_sgd_step_dscale(float* p, const float* g, float* m, const int64_t* seg_off, const float* seg_lr,
                                   const float* seg_wd, int nseg, int64_t total, float momentum, float dampening,
                                   int nesterov, int step, const float* gscale_dev, float* ema, float ema_decay,
                                   svl_stream_t stream) {
  SVL_CHECK_ARG(gscale_dev, "svl_sgd_step_dscale: gscale_dev is null");
  return sgd_step<const float*>("svl_sgd_step_dscale", p, g, m, seg_off, seg_lr, seg_wd, nseg, total, momentum, dampening,
                                nesterov, step, gscale_dev, ema, ema_decay, stream);
}
