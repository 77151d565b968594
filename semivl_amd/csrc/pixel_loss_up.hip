// Pixel losses on logits that exist only at the head's resolution (round 5).
//
// The reference resizes the head's [B, N, h, w] map to the crop size (vlg_head.py:247 / builder.py:93-97, bilinear) and
// computes softmax-max (semivl.py:232,252) and the per-pixel cross entropies (semivl.py:267-323) on the [B, N, H, W]
// result; autograd then runs the resize backwards.  Here the resize is evaluated INSIDE the loss kernels: a block owns
// TC x TC low-resolution cells, stages them (plus one halo cell per side) in LDS, forms each full-resolution pixel's N
// interpolated logits from the staged cells (ATen's upsample_bilinear2d index math, the expression of
// bilinear_planes_fwd_kernel), and -- for the cross entropy -- gathers d(loss)/d(low-resolution logit) of its own cells
// from every pixel whose taps touch them.  Full-resolution logits and their gradient are never written:
// (N / 2 r^2 + 28) B per pixel instead of (8 N + 28) + the two resize passes (16 N + ...) at upsampling ratio r.
//
// Deterministic: a pixel's loss terms are counted by the block that owns its upper-left tap; every low-resolution cell's
// gradient is ONE thread's sum over the pixels of its footprint in fixed (row, column) order -- halo pixels are evaluated
// by each block that needs them instead of being exchanged through atomics.
#include "svl_common.h"
#include "bilinear_index.h"
#include <atomic>
#include <stdlib.h>

namespace {

constexpr int TC = 8;            // low-resolution cells per block edge
constexpr int LR = TC + 3;       // staged cells per edge: one halo cell on either side + the far cell once more (clamped),
                                 // so that a pixel's second column tap is ALWAYS the next staged cell (one ds_read2_b32 per row)
constexpr int CSTR = LR * LR;    // class stride of the staged tile
constexpr int RMAX = 40;         // full-resolution rows / columns a block evaluates (checked per tile on the host)
constexpr int CG = 8;            // classes per gradient round
constexpr int NT = 512;          // threads of the cross-entropy kernel (CG x TC x TC)
constexpr int MAXF = 10;         // full-resolution columns in one cell's footprint
constexpr float MIN_SCALE = 2.f / (MAXF - 1);   // a cell's footprint (at most 2 / scale + 1 destination columns with a tap of
                                                // non-zero weight on it) fits MAXF

struct UpP {
  const float* logits;   // [B, N, h, w]
  int B, N, h, w, H, W, align;
  const int64_t* target;
  int use_ignore_t;
  const float* conf;
  const int64_t* ign;
  float conf_thresh;
  int all_pixels;
  const int64_t* mc;
  float* partials;
  float* dlogits;        // [B, N, h, w] or null
  const float* gscale;
  const float* img_weight;
  float* conf_out;       // softmax-max mode
  int64_t* label_out;
  int ncy, ncx;
  int pstr;             // stride of the per-pixel LDS arrays: >= the largest region (rows x columns) of any block
};
// label_smoothing / class weights of the labelled criterion (pixel_loss.hip's CeLswP): ce_up_kernel<true> only
struct UpLswP : UpP {
  float eps;
  const float* cw;      // [N] or null (all ones)
};
template <bool LSW> struct up_param { using type = UpP; };
template <> struct up_param<true> { using type = UpLswP; };
constexpr int UP_MAX_N = 160;   // class counts the resize-fused kernels take (up_ok)

__device__ __host__ inline int imin_(int a, int b) { return a < b ? a : b; }
__device__ __host__ inline int imax_(int a, int b) { return a > b ? a : b; }
// One axis of a block: owned cells [c0, c1), staged cells [s0, s0 + ns), evaluated destination indices [r0, r0 + nr).
// HALO: every destination index one of whose taps is an owned cell (gradient gather); else: those whose FIRST tap is.
// (host + device: svl_ce_up_num_blocks runs the same function over all tiles to check nr <= RMAX)
template <bool HALO>
__device__ __host__ inline void up_axis(int tile, int in, int out, float scale, bool align, int& c0, int& c1, int& s0, int& ns,
                                        int& r0, int& nr) {
  c0 = tile * TC;
  c1 = imin_(in, c0 + TC);
  s0 = HALO ? imax_(c0 - 1, 0) : c0;
  ns = imin_(c1, in - 1) - s0 + 1;
  const float off = align ? 0.f : 0.5f;
  int lo = (int)floorf((float)(c0 - 2 + off) / scale - off) - 2;
  lo = imax_(lo, 0);
  for (; lo < out - 1; ++lo) {
    int i0, i1;
    float l0, l1;
    src_index(lo, scale, in, align, i0, i1, l0, l1);
    if ((HALO ? i1 : i0) >= c0) break;
  }
  int hi = (int)ceilf((float)(c1 + off) / scale - off) + 2;
  hi = imin_(hi, out - 1);
  for (; hi > lo; --hi) {
    int i0, i1;
    float l0, l1;
    src_index(hi, scale, in, align, i0, i1, l0, l1);
    if (i0 <= c1 - 1) break;
  }
  r0 = lo;
  nr = hi - lo + 1;      // (<= RMAX: checked on the host for every tile, up_ok)
}

struct Taps {
  int o00, o10;          // upper-left tap of each row; the right tap is the next staged cell
  float ly0, ly1, lx0, lx1;
};
__device__ __forceinline__ float up_interp(const float* __restrict__ t, const Taps& k) {
  return k.ly0 * (k.lx0 * t[k.o00] + k.lx1 * t[k.o00 + 1]) + k.ly1 * (k.lx0 * t[k.o10] + k.lx1 * t[k.o10 + 1]);
}
// The cross-entropy kernel works in BASE 2: the staged logits are multiplied by log2(e) once (the resize is linear), so every
// exponential of the two class loops is ONE v_exp_f32 instead of the ~12 instructions of expf (the compiler then unrolls the
// class loops by four on packed fp32 math); log-sum-exp and the loss terms are scaled back by ln 2 once per pixel.
constexpr float LOG2E = 1.44269504088896340736f, LN2 = 0.69314718055994530942f;
// one branch-free step of the online softmax (one exponential per class; m = -inf at the start gives s = 1)
__device__ __forceinline__ void up_online(float x, float& m, float& s) {
  const float d = x - m, e = __builtin_amdgcn_exp2f(-fabsf(d));
  s = d > 0.f ? fmaf(s, e, 1.f) : s + e;
  m = fmaxf(m, x);
}

// A block after up_prologue: its image b; per axis the owned cells [c0, c1), the first staged cell s0 and the evaluated
// destination indices [r0, r0 + nr); the tap tables (LDS) of evaluated row r / column q: both source taps and their weights.
struct UpBlock {
  int b, c0y, c1y, s0y, r0y, nry, c0x, c1x, s0x, r0x, nrx;
  const int *ry0, *ry1, *cx0, *cx1;
  const float *rl0, *rl1, *cl0, *cl1;
  // whether the pixel with upper-left tap (y0, x0) is counted by this block (else: by a neighbour)
  __device__ __forceinline__ bool owns(int y0, int x0) const { return y0 >= c0y && y0 < c1y && x0 >= c0x && x0 < c1x; }
  // index of evaluated pixel (r, q) in a [B, H, W] map
  __device__ __forceinline__ long pixel(const UpP& p, int r, int q) const {
    return (long)b * p.H * p.W + (long)(r0y + r) * p.W + (r0x + q);
  }
};
// What every kernel here starts with: block -> (image, tile), up_axis on both axes, the tap tables, and the block's cells of
// all N classes staged as tile[N][CSTR] (BASE2: multiplied by log2(e)).  THREADS = blockDim.x; the caller places the barrier.
template <bool HALO, int THREADS, bool BASE2>
__device__ __forceinline__ UpBlock up_prologue(const UpP& p, float* __restrict__ tile) {
  __shared__ int ry0[RMAX], ry1[RMAX], cx0[RMAX], cx1[RMAX];
  __shared__ float rl0[RMAX], rl1[RMAX], cl0[RMAX], cl1[RMAX];
  const int tid = threadIdx.x;
  const int per = p.ncy * p.ncx;
  const int b = blockIdx.x / per, rem = blockIdx.x - b * per;
  const int ty = rem / p.ncx, tx = rem - ty * p.ncx;
  const float sh = area_scale(p.h, p.H, p.align), sw = area_scale(p.w, p.W, p.align);
  int c0y, c1y, s0y, nsy, r0y, nry, c0x, c1x, s0x, nsx, r0x, nrx;
  up_axis<HALO>(ty, p.h, p.H, sh, p.align, c0y, c1y, s0y, nsy, r0y, nry);
  up_axis<HALO>(tx, p.w, p.W, sw, p.align, c0x, c1x, s0x, nsx, r0x, nrx);
  if (tid < nry) src_index(r0y + tid, sh, p.h, p.align, ry0[tid], ry1[tid], rl0[tid], rl1[tid]);
  else if (tid >= 64 && tid < 64 + nrx) src_index(r0x + tid - 64, sw, p.w, p.align, cx0[tid - 64], cx1[tid - 64], cl0[tid - 64], cl1[tid - 64]);
  {
    const int cell = tid & 127, cl = tid >> 7;
    if (cell < (nsy + 1) * (nsx + 1)) {
      const int cr = cell / (nsx + 1), cc = cell - cr * (nsx + 1);
      const float* g = p.logits + (long)b * p.N * p.h * p.w + (long)imin_(s0y + cr, p.h - 1) * p.w + imin_(s0x + cc, p.w - 1);
      float* d = tile + cr * LR + cc;
      const long hw = (long)p.h * p.w;
      for (int c = cl; c < p.N; c += THREADS / 128) d[c * CSTR] = BASE2 ? g[c * hw] * LOG2E : g[c * hw];
    }
  }
  return {b, c0y, c1y, s0y, r0y, nry, c0x, c1x, s0x, r0x, nrx, ry0, ry1, cx0, cx1, rl0, rl1, cl0, cl1};
}
__device__ __forceinline__ Taps up_taps(const UpBlock& g, int r, int q) {
  Taps k;
  k.o00 = (g.ry0[r] - g.s0y) * LR + (g.cx0[q] - g.s0x);
  k.o10 = (g.ry1[r] - g.s0y) * LR + (g.cx0[q] - g.s0x);
  k.ly0 = g.rl0[r]; k.ly1 = g.rl1[r]; k.lx0 = g.cl0[q]; k.lx1 = g.cl1[q];
  return k;
}

// ------------------------------------------------------------------------------------------------
// softmax-max of the resized logits: conf = 1 / sum_c exp(x_c - max), label = first argmax.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void softmax_max_up_kernel(const UpP p) {
  extern __shared__ __attribute__((aligned(16))) float tile[];   // [N][CSTR]
  const UpBlock g = up_prologue<false, 256, false>(p, tile);
  __syncthreads();
  const int npx = g.nry * g.nrx;
  for (int px = threadIdx.x; px < npx; px += 256) {
    const int r = px / g.nrx, q = px - r * g.nrx;
    if (!g.owns(g.ry0[r], g.cx0[q])) continue;   // (owned by a neighbour)
    const Taps k = up_taps(g, r, q);
    float m = -INFINITY, s = 0.f;
    int idx = 0;
    for (int c = 0; c < p.N; ++c) softmax_max_step(up_interp(tile + c * CSTR, k), c, m, s, idx);
    const long o = g.pixel(p, r, q);
    p.conf_out[o] = 1.f / s;
    p.label_out[o] = idx;
  }
}

// ------------------------------------------------------------------------------------------------
// OHEM's target-class probability of the resized logits (ohem.py:36-45): p = softmax(x)[target], 1.0 where target == 255.
// Staged in base 2 and reduced with up_online in class order exactly like ce_up_kernel: p = exp2(x_t - lse) is the number
// ce_up_kernel's gradient sees for the target class (the same interpolated value -- the same cell read through the same
// up_interp -- and the same lse).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void target_prob_up_kernel(const UpP p, float* __restrict__ prob) {
  extern __shared__ __attribute__((aligned(16))) float tile[];   // [N][CSTR]
  const UpBlock g = up_prologue<false, 256, true>(p, tile);
  __syncthreads();
  const int npx = g.nry * g.nrx;
  for (int px = threadIdx.x; px < npx; px += 256) {
    const int r = px / g.nrx, q = px - r * g.nrx;
    if (!g.owns(g.ry0[r], g.cx0[q])) continue;   // (owned by a neighbour)
    const long o = g.pixel(p, r, q);
    const long t = p.target[o];
    float pr = 1.f;
    if (t != 255) {
      const Taps k = up_taps(g, r, q);
      float m = -INFINITY, s = 0.f;
      for (int c = 0; c < p.N; ++c) up_online(up_interp(tile + c * CSTR, k), m, s);
      const float lse = m + log2f(s);
      // (a label outside [0, N) reads no logit and is never a hard pixel; the reference's indexing would fail there)
      pr = (t >= 0 && t < p.N) ? __builtin_amdgcn_exp2f(up_interp(tile + (int)t * CSTR, k) - lse) : 1.f;
    }
    prob[o] = pr;
  }
}

// ------------------------------------------------------------------------------------------------
// Cross entropy (+ confidence weighting + guidance term) forward and backward on the resized logits; the gradient
// arrives at the LOW resolution.  partials[block] = { sum w_t*ce_t, sum ce_m, sum conf*valid, #valid } like ce_fused_kernel.
//
// LSW (labelled branch only, a separate instantiation: the plain one keeps its code and its LDS): label_smoothing eps and
// class weights w (staged in LDS once per block; ones when absent), W = sum_c w_c, g = gscale[0], everything in the staged
// base 2 until the one LN2 per pixel:
//   numerator(pixel) = LN2 [ (1 - eps) w_t (lse - x_t) + (eps / N) (W lse - sum_c w_c x_c) ]   (sum_c w_c x_c: phase A's class loop)
//   d(loss)/d(resized logit c) = a p_c - b [c == t] - e w_c,  a = g ((1 - eps) w_t + (eps / N) W), b = g (1 - eps) w_t, e = g eps / N
// The pixel arrays hold a and b where the plain kernel holds g_t and g_m; e is one number per launch and applies exactly where
// the stored target index is >= 0, so no further per-pixel state is needed.  partials = { sum numerator, 0, 0, sum [t != 255] w_t }.
// ------------------------------------------------------------------------------------------------
// Phase A's pixel body, one per instantiation: px's log-sum-exp, its two gradient coefficients and its (target | guidance
// << 16) indices into the pixel arrays, and -- where the block owns the pixel -- its terms into the four block sums.
struct UpPix {
  float *lse, *gt, *gm;   // [pstr] each
  int* ix;
};
struct UpSums {
  float s_t = 0.f, s_m = 0.f, s_c = 0.f, n_v = 0.f;
};
// per launch: the two gradient scales (0 without dlogits); plain: the image's weight; LSW: 1 - eps, eps / N, W
struct UpConsts {
  float g0, g1, iw, om, en, wsum;
};
// the pixel's maps: target t; with p.conf its confidence cf and ignore label ig, with p.mc its guidance label mm
__device__ __forceinline__ void ce_up_pixel(const UpP& p, const float* tile, const Taps& k, bool owned, long t, long ig,
                                            float cf, long mm, int px, const UpConsts& u, const UpPix& st, UpSums& a) {
  float m = -INFINITY, s = 0.f;
  for (int c = 0; c < p.N; ++c) {
    up_online(up_interp(tile + c * CSTR, k), m, s);
  }
  const float lse = m + log2f(s);                 // (base 2, like the staged logits)
  const bool t_ok = !(p.use_ignore_t && t == 255);
  const int ti = t_ok ? (int)t : -1;
  const int mi = mm != 255 ? (int)mm : -1;        // (255 without a guidance map)
  float w = 1.f;
  bool valid = t_ok;
  float sc = 0.f;
  if (p.conf) {
    const bool v = ig != 255;
    w = p.all_pixels ? 1.f : ((cf >= p.conf_thresh && v) ? 1.f : 0.f);
    w *= u.iw;
    valid = v;
    sc = v ? cf : 0.f;
  }
  if (owned) {
    const float xt = (ti >= 0 && ti < p.N) ? up_interp(tile + ti * CSTR, k) : 0.f;
    const float xm = (mi >= 0 && mi < p.N) ? up_interp(tile + mi * CSTR, k) : 0.f;
    a.n_v += valid ? 1.f : 0.f;
    a.s_t += t_ok ? w * (LN2 * (lse - xt)) : 0.f;
    a.s_m += mi >= 0 ? LN2 * (lse - xm) : 0.f;
    a.s_c += sc;
  }
  st.lse[px] = lse;
  st.gt[px] = t_ok ? u.g0 * w : 0.f;
  st.gm[px] = mi >= 0 ? u.g1 : 0.f;
  st.ix[px] = (int)((unsigned)(ti & 0xffff) | ((unsigned)mi << 16));
}
// LSW: the pixel arrays hold a and b; wsh = the staged class weights
__device__ __forceinline__ void ce_up_pixel_lsw(const UpP& p, const float* tile, const float* wsh, const Taps& k, bool owned,
                                                long t, int px, const UpConsts& u, const UpPix& st, UpSums& a) {
  float m = -INFINITY, s = 0.f, swx = 0.f;
  for (int c = 0; c < p.N; ++c) {
    const float x = up_interp(tile + c * CSTR, k);
    up_online(x, m, s);
    swx = fmaf(wsh[c], x, swx);
  }
  const float lse = m + log2f(s);               // (base 2, like the staged logits and swx)
  const bool t_ok = t != 255, in = t_ok && t >= 0 && t < p.N;
  const float wt = in ? wsh[(int)t] : 0.f;      // (a label outside [0, N) reads no logit and no weight)
  if (t_ok && owned) {
    const float xt = in ? up_interp(tile + (int)t * CSTR, k) : 0.f;
    a.n_v += wt;
    a.s_t += LN2 * (u.om * wt * (lse - xt) + u.en * (u.wsum * lse - swx));
  }
  // (selected, not multiplied: with every target 255 the scale g0 is 1 / 0)
  st.lse[px] = lse;
  st.gt[px] = t_ok ? u.g0 * (u.om * wt + u.en * u.wsum) : 0.f;
  st.gm[px] = t_ok ? u.g0 * (u.om * wt) : 0.f;
  st.ix[px] = (int)((unsigned)((t_ok ? (int)t : -1) & 0xffff) | 0xffff0000u);
}

template <bool LSW>
__global__ __launch_bounds__(NT) void ce_up_kernel(const typename up_param<LSW>::type p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int cr_lo[TC], cr_hi[TC], cc_lo[TC], cc_hi[TC];
  __shared__ float red[NT / 64][4];
  float* wsh = nullptr;                     // LSW: the class weights
  if constexpr (LSW) {
    __shared__ float wsh_[UP_MAX_N];
    wsh = wsh_;
  }
  // (the pixel arrays are strided by the launch's largest region, not by RMAX^2: 72 KB in all at N = 21 and 128 -> 512, two
  //  blocks per CU -- the kernel waits on LDS round trips more than on anything else, profiles/r5_h_pmc_sq_ce_up.txt)
  const int PS = p.pstr;
  float* tile = smem;                       // [N][CSTR]
  float* st_lse = smem + p.N * CSTR;        // per evaluated pixel: log-sum-exp, g_t, g_m, (target | guidance << 16)
  float* st_gt = st_lse + PS;
  float* st_gm = st_gt + PS;
  const UpPix st = {st_lse, st_gt, st_gm, reinterpret_cast<int*>(st_gm + PS)};
  float* dbuf = st_gm + 2 * PS;             // [CG][PS]: d(loss)/d(resized logit) of one class round

  const int tid = threadIdx.x;
  const UpBlock g = up_prologue<true, NT, true>(p, tile);
  if constexpr (LSW) {
    if (tid < p.N) wsh[tid] = p.cw ? p.cw[tid] : 1.f;     // (N <= UP_MAX_N < NT)
  }
  __syncthreads();
  // footprint of each owned cell row / column inside the evaluated region (first and last index with a tap on it)
  if (tid < 2 * TC) {
    const bool rows = tid < TC;
    const int i = rows ? tid : tid - TC;
    const int cell = (rows ? g.c0y : g.c0x) + i, n = rows ? g.nry : g.nrx;
    const int* a0 = rows ? g.ry0 : g.cx0;
    const int* a1 = rows ? g.ry1 : g.cx1;
    const float* w0 = rows ? g.rl0 : g.cl0;
    const float* w1 = rows ? g.rl1 : g.cl1;
    int lo = 0, hi = -1;
    if (cell < (rows ? g.c1y : g.c1x)) {
      lo = n;
      // (taps of weight 0 do not count: the destination indices clamped at the low border all name cell 1 as their second
      //  tap with weight 0, and at ratios above 4 they stretched cell 1's columns past MAXF -- its last column was dropped)
      for (int r = 0; r < n; ++r)
        if ((a0[r] == cell && w0[r] != 0.f) || (a1[r] == cell && w1[r] != 0.f)) {
          lo = min(lo, r);
          hi = r;
        }
    }
    (rows ? cr_lo : cc_lo)[i] = lo;
    (rows ? cr_hi : cc_hi)[i] = hi;
  }

  // ---- phase A: per evaluated pixel log-sum-exp, loss terms (owned pixels), gradient coefficients ----------------
  const int npx = g.nry * g.nrx, nrx = g.nrx;
  UpConsts u = {p.dlogits ? p.gscale[0] : 0.f, p.dlogits ? p.gscale[1] : 0.f, p.img_weight ? p.img_weight[g.b] : 1.f,
                1.f, 0.f, 0.f};
  if constexpr (LSW) {
    u.om = 1.f - p.eps;
    u.en = p.eps / (float)p.N;
    for (int c = 0; c < p.N; ++c) u.wsum += wsh[c];   // (class order: the same in every thread)
  }
  UpSums a;
  for (int px = tid; px < npx; px += NT) {
    const int r = px / nrx, q = px - r * nrx;
    const Taps k = up_taps(g, r, q);
    const bool owned = g.owns(g.ry0[r], g.cx0[q]);
    const long o = g.pixel(p, r, q);
    const long t = p.target[o];
    long ig = 0, mm = 255;
    float cf = 0.f;
    if (p.conf) { ig = p.ign[o]; cf = p.conf[o]; }
    if (p.mc) mm = p.mc[o];
    if constexpr (LSW) ce_up_pixel_lsw(p, tile, wsh, k, owned, t, px, u, st, a);
    else ce_up_pixel(p, tile, k, owned, t, ig, cf, mm, px, u, st, a);
  }
  // block partial sums: fixed shuffle tree per wave, waves in order
  {
    float a0 = a.s_t, a1 = a.s_m, a2 = a.s_c, a3 = a.n_v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      a0 += __shfl_xor(a0, off, 64);
      a1 += __shfl_xor(a1, off, 64);
      a2 += __shfl_xor(a2, off, 64);
      a3 += __shfl_xor(a3, off, 64);
    }
    if ((tid & 63) == 0) {
      red[tid >> 6][0] = a0; red[tid >> 6][1] = a1; red[tid >> 6][2] = a2; red[tid >> 6][3] = a3;
    }
  }
  __syncthreads();
  if (tid < 4) {
    float a = 0.f;
#pragma unroll
    for (int wv = 0; wv < NT / 64; ++wv) a += red[wv][tid];
    p.partials[(long)blockIdx.x * 4 + tid] = a;
  }
  if (!p.dlogits) return;

  // ---- phase B: rounds of CG classes -- B1: d(loss)/d(resized logit) of every evaluated pixel into LDS; B2: thread
  //      (class of the round, owned cell) gathers its footprint with the resize's own weights --------------------------
  const int bj = tid >> 6, bcell = tid & 63, cyi = bcell >> 3, cxi = bcell & 7;
  const int yl = g.c0y + cyi, xl = g.c0x + cxi;
  const bool cell_ok = yl < g.c1y && xl < g.c1x;
  const int rlo = cr_lo[cyi], rhi = cr_hi[cyi], clo = cc_lo[cxi];
  float wx[MAXF];
  {
    const int chi = cc_hi[cxi];
#pragma unroll
    for (int f = 0; f < MAXF; ++f) {
      const int cc = min(clo + f, nrx - 1);
      wx[f] = (cell_ok && clo + f <= chi) ? ((g.cx0[cc] == xl ? g.cl0[cc] : 0.f) + (g.cx1[cc] == xl ? g.cl1[cc] : 0.f)) : 0.f;
    }
  }
  const float ge = u.en > 0.f ? u.g0 * u.en : 0.f;  // LSW: e = g eps / N (0 in the plain kernel)
  float* dl = p.dlogits + (long)g.b * p.N * p.h * p.w + (long)yl * p.w + xl;
  for (int cg0 = 0; cg0 < p.N; cg0 += CG) {
    for (int px = tid; px < npx; px += NT) {
      const int r = px / nrx, q = px - r * nrx;
      const Taps k = up_taps(g, r, q);
      const float lse = st.lse[px], gt = st.gt[px], gm = st.gm[px], gs = gt + gm;
      const int ix = st.ix[px];
      const int ti = (int)(short)(ix & 0xffff), mi = ix >> 16;
#pragma unroll
      for (int j = 0; j < CG; ++j) {
        const int c = cg0 + j;
        float d = 0.f;
        if constexpr (LSW) {
          if (c < p.N && ti >= 0) {                 // gt = a, gm = b of the pixel; e w_c on every labelled pixel
            d = gt * __builtin_amdgcn_exp2f(up_interp(tile + c * CSTR, k) - lse) - ge * wsh[c];
            if (c == ti) d -= gm;
          }
        } else if (c < p.N && gs != 0.f) {
          d = gs * __builtin_amdgcn_exp2f(up_interp(tile + c * CSTR, k) - lse);
          if (c == ti) d -= gt;
          if (c == mi) d -= gm;
        }
        dbuf[j * PS + px] = d;
      }
    }
    __syncthreads();
    if (cell_ok && cg0 + bj < p.N) {
      const float* dj = dbuf + bj * PS;
      float acc = 0.f;
      for (int r = rlo; r <= rhi; ++r) {
        const float wy = (g.ry0[r] == yl ? g.rl0[r] : 0.f) + (g.ry1[r] == yl ? g.rl1[r] : 0.f);
        const float* row = dj + r * nrx;
        float ra = 0.f;
#pragma unroll
        for (int f = 0; f < MAXF; ++f) ra += wx[f] * row[min(clo + f, nrx - 1)];
        acc += wy * ra;
      }
      dl[(long)(cg0 + bj) * p.h * p.w] = acc;
    }
    __syncthreads();
  }
}

inline bool up_axis_ok(int in, int out, bool align, int* max_region = nullptr) {
  if (in < 2 || out < in) return false;
  const float sc = area_scale(in, out, align);
  if (!(sc >= MIN_SCALE)) return false;
  int mx = 0;
  for (int t = 0; t * TC < in; ++t) {
    int c0, c1, s0, ns, r0, nr;
    up_axis<true>(t, in, out, sc, align, c0, c1, s0, ns, r0, nr);
    if (nr > RMAX || ns + 1 > LR) return false;
    mx = nr > mx ? nr : mx;
    up_axis<false>(t, in, out, sc, align, c0, c1, s0, ns, r0, nr);
    if (nr > RMAX || ns + 1 > LR) return false;
  }
  if (max_region) *max_region = mx;
  return true;
}
inline bool up_ok(int N, int h, int w, int H, int W, int align) {
  return N > 0 && N <= UP_MAX_N && up_axis_ok(h, H, align != 0) && up_axis_ok(w, W, align != 0);
}
inline size_t ce_up_lds(int N, int pstr) { return ((size_t)N * CSTR + (size_t)(4 + CG) * pstr) * sizeof(float); }

// "Allow this kernel `max_lds` bytes of dynamic LDS, once; then launch it": one block per (image, tile) of p's geometry.
// hipFuncSetAttribute is per device: one bit per device ordinal (the mask is the kernel's own), set only AFTER the call
// succeeded (a failed or still running first call must not let later launches skip the attribute; two threads racing here
// both set it: idempotent)
template <auto KERNEL, typename... Args>
int up_launch(const char* fn, int max_lds, const UpP& p, int threads, size_t lds, svl_stream_t stream, const Args&... args) {
  static std::atomic<uint64_t> mask{0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t bit = 1ull << (dev & 63);
  if (!(mask.load(std::memory_order_acquire) & bit)) {
    SVL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
    mask.fetch_or(bit, std::memory_order_acq_rel);
  }
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)((long)p.B * p.ncy * p.ncx)), dim3(threads), lds, (hipStream_t)stream, args...);
  SVL_LAUNCH_CHECK(fn);
  return SVL_OK;
}
// LDS a workgroup may allocate on the current device (gfx950: 160 KB); without a device (host-only geometry queries in the
// build container) the figure of the one target this library is compiled for
size_t device_lds_limit() {
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && v > 0)
    return (size_t)v;
  (void)hipGetLastError();
  return 160 * 1024;
}
// the largest dynamic allocation a launch of this geometry asks for (pixel arrays strided by the launch's largest region)
inline bool up_fits(int N, int h, int w, int H, int W, int align, size_t fixed = 1024) {
  int my = 0, mx = 0;
  if (!up_axis_ok(h, H, align != 0, &my) || !up_axis_ok(w, W, align != 0, &mx)) return false;
  static const size_t limit = device_lds_limit();
  return ce_up_lds(N, ((my * mx + 31) / 32) * 32) + fixed <= limit;     // (+ the kernels' static LDS)
}
// ce_up_kernel<true>: its static LDS is the index / footprint / reduction arrays (1536 B) and the staged class weights
// (640 B); 3 KB keeps the dynamic part within the 157 KB its launch asks the runtime for
constexpr size_t UP_LSW_FIXED = 3 * 1024;
static_assert(1536 + UP_MAX_N * sizeof(float) <= UP_LSW_FIXED, "static LDS of ce_up_kernel<true>");


int64_t up_num_blocks(int B, int N, int h, int w, int H, int W, int align, size_t fixed) {
  if (B <= 0 || !up_ok(N, h, w, H, W, align) || !up_fits(N, h, w, H, W, align, fixed)) return -1;
  return (int64_t)B * ((h + TC - 1) / TC) * ((w + TC - 1) / TC);
}
// kernel parameters of a launch on logits [B, N, h, w] -> [H, W]: everything else zero
UpP up_geom(const float* logits, int B, int N, int h, int w, int H, int W, int align) {
  UpP p = {};
  p.logits = logits; p.B = B; p.N = N; p.h = h; p.w = w; p.H = H; p.W = W; p.align = align != 0;
  p.ncy = (h + TC - 1) / TC; p.ncx = (w + TC - 1) / TC;
  return p;
}
// descriptor -> kernel parameters, with the stride of the pixel arrays (geometry checked before: up_ok)
void up_fill(UpP& p, const svl_ce_up_desc* d) {
  p = up_geom(d->logits, d->B, d->N, d->h, d->w, d->H, d->W, d->align_corners);
  p.target = d->target; p.use_ignore_t = d->use_ignore_t;
  p.conf = d->conf; p.ign = d->ign; p.conf_thresh = d->conf_thresh; p.all_pixels = d->all_pixels;
  p.mc = d->mc_target; p.partials = d->partials; p.dlogits = d->dlogits; p.gscale = d->gscale;
  p.img_weight = d->img_weight;
  int my = 0, mx = 0;
  (void)up_axis_ok(d->h, d->H, p.align != 0, &my);
  (void)up_axis_ok(d->w, d->W, p.align != 0, &mx);
  p.pstr = ((my * mx + 31) / 32) * 32;
}
// `query`: the function whose negative result announces the refusal
int up_geom_check(const char* fn, bool ok, const char* query, int N, int h, int w, int H, int W) {
  SVL_CHECK_ARG(ok, "%s: unsupported geometry N=%d %dx%d -> %dx%d (%s < 0)", fn, N, h, w, H, W, query);
  return SVL_OK;
}
// The argument checks of svl_ce_up_fused_f32 and, with `eps` (its label_smoothing), of svl_ce_up_fused_lsw_f32, in one order
// and under the entry point's name.
int up_check(const char* fn, const svl_ce_up_desc* d, const float* eps) {
  SVL_CHECK_ARG(d && d->logits && d->target && d->partials, "%s: null args", fn);
  if (eps) {
    const int rc = svl_ce_lsw_check(fn, d, *eps);
    if (rc) return rc;
  }
  const bool ok = d->B > 0 && up_ok(d->N, d->h, d->w, d->H, d->W, d->align_corners) &&
                  (!eps || up_fits(d->N, d->h, d->w, d->H, d->W, d->align_corners, UP_LSW_FIXED));
  const int rc = up_geom_check(fn, ok, eps ? "svl_ce_up_lsw_num_blocks" : "svl_ce_up_num_blocks", d->N, d->h, d->w, d->H, d->W);
  if (rc) return rc;
  if (!eps) {
    SVL_CHECK_ARG((d->conf == nullptr) == (d->ign == nullptr), "%s: conf and ign go together", fn);
    SVL_CHECK_ARG(d->img_weight == nullptr || d->conf != nullptr, "%s: img_weight must be NULL without conf", fn);
  }
  SVL_CHECK_ARG(d->dlogits == nullptr || d->gscale != nullptr, "%s: gscale required with dlogits", fn);
  return SVL_OK;
}

}  // namespace

extern "C" int64_t svl_ce_up_num_blocks(int B, int N, int h, int w, int H, int W, int align_corners) {
  return up_num_blocks(B, N, h, w, H, W, align_corners, 1024);
}

extern "C" int svl_softmax_max_up_f32(const float* logits, int B, int N, int h, int w, int H, int W, int align_corners,
                                      float* conf, int64_t* label, svl_stream_t stream) {
  SVL_CHECK_ARG(logits && conf && label && B > 0, "svl_softmax_max_up_f32: bad args");
  const int rc = up_geom_check("svl_softmax_max_up_f32", up_ok(N, h, w, H, W, align_corners), "svl_ce_up_num_blocks", N, h, w, H, W);
  if (rc) return rc;
  UpP p = up_geom(logits, B, N, h, w, H, W, align_corners);
  p.conf_out = conf; p.label_out = label;
  return up_launch<softmax_max_up_kernel>("svl_softmax_max_up_f32", 96 * 1024, p, 256, (size_t)N * CSTR * sizeof(float), stream, p);
}

extern "C" int svl_ce_up_fused_f32(const svl_ce_up_desc* d, svl_stream_t stream) {
  const int rc = up_check("svl_ce_up_fused_f32", d, nullptr);
  if (rc) return rc;
  UpP p;
  up_fill(p, d);
  return up_launch<ce_up_kernel<false>>("svl_ce_up_fused_f32", 158 * 1024, p, NT, ce_up_lds(p.N, p.pstr), stream, p);
}

extern "C" int64_t svl_ce_up_lsw_num_blocks(int B, int N, int h, int w, int H, int W, int align_corners) {
  return up_num_blocks(B, N, h, w, H, W, align_corners, UP_LSW_FIXED);
}

extern "C" int svl_ce_up_fused_lsw_f32(const svl_ce_up_desc* d, float label_smoothing, const float* class_weight,
                                       svl_stream_t stream) {
  const int rc = up_check("svl_ce_up_fused_lsw_f32", d, &label_smoothing);
  if (rc) return rc;
  UpLswP p;
  up_fill(p, d);
  p.eps = label_smoothing; p.cw = class_weight;
  return up_launch<ce_up_kernel<true>>("svl_ce_up_fused_lsw_f32", 157 * 1024, p, NT, ce_up_lds(p.N, p.pstr), stream, p);
}

extern "C" int svl_target_prob_up_f32(const float* logits, int B, int N, int h, int w, int H, int W, int align_corners,
                                      const int64_t* target, float* prob, svl_stream_t stream) {
  SVL_CHECK_ARG(logits && target && prob && B > 0, "svl_target_prob_up_f32: bad args");
  const int rc = up_geom_check("svl_target_prob_up_f32", up_ok(N, h, w, H, W, align_corners), "svl_ce_up_num_blocks", N, h, w, H, W);
  if (rc) return rc;
  UpP p = up_geom(logits, B, N, h, w, H, W, align_corners);
  p.target = target;
  return up_launch<target_prob_up_kernel>("svl_target_prob_up_f32", 96 * 1024, p, 256, (size_t)N * CSTR * sizeof(float), stream, p,
                                          prob);
}
