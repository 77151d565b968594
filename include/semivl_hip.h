/*
 * semivl_hip.h — C-ABI of libsemivl_hip.so: the MI355X (gfx950) kernels behind the SemiVL training hot path.
 *
 * The reference (google-research/semivl) has no FFI layer: its boundary is Python
 * (`model/builder.py:56-159`, `model/vlm.py:90-127`, `utils/train_utils.py:19-49`, `semivl.py:52-58,223-345`).
 * This header is the operator boundary a maintainer would bind from Python (ctypes stub in INTEGRATION.md);
 * `semivl_amd/` is the host-side mirror of the reference's Python surface built on top of it.
 *
 * Conventions (all entry points) -- what is TRUE of the library, checked by tests/test_abi.py and
 * tests/test_ops_gpu.py::test_two_streams_*:
 *   - plain pointers + sizes, no torch types; every pointer is DEVICE memory owned by the caller, including every
 *     scratch buffer (svl_*_ws_* size queries): the library never allocates or frees device memory;
 *   - it never synchronises the device or a stream.  Work is enqueued on `stream` of the caller's CURRENT device.
 *     Two entry-point families (svl_gemm_f32 on ragged token counts, svl_attention_{fwd,bwd}) additionally run a thin,
 *     disjoint-output launch on a HELPER stream that is event-forked from and event-joined back into `stream` inside
 *     the same call (capture-legal: events only), so from the caller's point of view everything is ordered on `stream`;
 *   - host-side state: one helper stream + two events per (device, caller stream) pair, created lazily under a mutex on
 *     first use and kept until svl_stream_release(stream) / svl_shutdown(); per-device kernel attributes set once per
 *     device; the process-wide arithmetic mode svl_set_gemm_emulation (a relaxed atomic seeded from the environment,
 *     read once per call) and the environment's A/B switches (svl_switches, read once per process), all selecting
 *     between kernels that compute the same function.  Nothing else is mutable: the library is re-entrant across host threads, devices and streams -- calls
 *     that use different streams never share a helper stream, an event or a buffer;
 *   - tensors are dense fp32 unless stated; token tensors are [rows, C] row-major ("NHWC"/[B,T,C]);
 *   - returns 0 (SVL_OK) or a negative svl_status; svl_last_error() gives the message (thread-local).
 */
#ifndef SEMIVL_HIP_H_
#define SEMIVL_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* svl_stream_t; /* hipStream_t */

typedef enum svl_status {
  SVL_OK = 0,
  SVL_ERR_INVALID_ARG = -1,
  SVL_ERR_LAUNCH = -2,
  SVL_ERR_UNSUPPORTED = -3
} svl_status;

int svl_version(void); /* 607: + svl_gemm_route (the routing of svl_gemm_f32 as a host-only query), svl_switches; - svl_set_conv_tiled; 606: + svl_grad_clip_f32, svl_grad_clip_ws_doubles, svl_adamw_step_dscale, svl_sgd_step_dscale (gradient-norm clipping on the arena, formed and applied on the device); 605: + svl_ce_fused_lsw_f32, svl_ce_up_fused_lsw_f32, svl_ce_up_lsw_num_blocks, svl_class_weight_sum_f64, svl_class_weight_sum_ws_doubles, svl_scale_from_sum_f32 (label_smoothing / class weights of the labelled cross entropy); 604: + svl_gap_tokens_{fwd,bwd}, svl_bcast_rows_{fwd,bwd} (the pooling branch of the DeepLabV3+ head); 603: + svl_layernorm_{fwd,bwd}_pack_f16x2, tensor_amax of svl_split_planes_f16x2, svl_gemm_desc::a_amax / b_amax, svl_absmax_launches (ViT glue passes read each matrix once); 602: + svl_target_prob_f32, svl_target_prob_up_f32, svl_ohem_ws_bytes, svl_ohem_threshold_f32, svl_ohem_relabel_i64 (the OHEM supervised criterion); 601: + SVL_B_NC_GELU / SVL_B_NC_LN / SVL_B_PATCHT producers, svl_gemm_desc::b_stats / b_gamma / b_beta (ViT fine-tuning weight gradients); 600: round-6 ABI (+ svl_permute4_f32, svl_bound2_f32, svl_attention tail kernels replace the row kernels); 502: + svl_ce_up_fused_f32, svl_softmax_max_up_f32, svl_ce_up_num_blocks (pixel losses on head-resolution logits); 501: + svl_attention_{fwd,bwd}_h2, svl_attention_h2_ws_bytes (fused attention on fp16 x 2 pre-packed operands); 500: round-5 ABI (fp16 x 2 planes: svl_split_planes_f16x2, svl_planes_bytes_fmt, fmt / scale fields of svl_pgemm_desc); 401: + svl_conv3x3_weight_planes, svl_gemm_desc::conv_w_planes, w_planes of svl_conv3x3_gn_f32; 400: round-4 ABI (gn_in / svl_conv3x3_gn_f32 / svl_groupnorm_apply / _scale_shift, svl_permute_rows_f32,
                           svl_stream_prepare, svl_last_gemm_path; gn_in arguments of the tiled weight gradient and the Conv2d(C -> 1)
                           entries, `accumulate` of svl_avgpool_cat_bwd); 300: round-3 ABI (packed-planes operands; planes outputs of LayerNorm / attention; loss-mode arguments of
                           the pixel-loss entries; 200 = round 2: helper-stream contexts, caller-owned scratch everywhere) */
/* Destroys the helper stream/events this library created for `stream` on the current device (no-op if none), or for
 * every stream.  Call after the stream has been synchronised; not required before process exit. */
int svl_stream_release(svl_stream_t stream);
/* Creates the helper stream/events of `stream` NOW instead of on first use (no-op if they exist).  The HIP runtime maps a
 * process's streams onto its hardware queues in creation order: a caller that wants a reproducible map (the data-parallel
 * reducer creates the step's streams before its communication stream) creates them up front.  No reference counterpart. */
int svl_stream_prepare(svl_stream_t stream);
/* The helper stream svl_stream_prepare(stream) created (a hipStream_t): for probing hardware-queue sharing only. */
int svl_stream_helper(svl_stream_t stream, void** helper);
int svl_shutdown(void);
int svl_num_stream_contexts(void); /* live (device, stream) helper contexts -- introspection for tests */
/* Copies the calling thread's last error message (NUL-terminated) into buf; returns its length. */
int svl_last_error(char* buf, size_t len);
/* Measurement aid (bench.py's `roofline.clock_mhz`; no counterpart in the reference): n_waves <= 1024 single-wave
 * workgroups compare the shader-clock counter with the constant 100 MHz counter for `ticks_100mhz` (<= 1e9 = 10 s) and
 * leave out[2 i] = shader-clock cycles, out[2 i + 1] = 100 MHz ticks (device memory, 16 n_waves bytes).  Launched on a
 * stream of its own next to a kernel under measurement: cycles / ticks x 100 = the MHz sustained under that kernel. */
int svl_clock_probe(unsigned long long* out, int n_waves, unsigned long long ticks_100mhz, svl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GEMM / implicit-GEMM core (fp32 in, fp32 accumulate on v_mfma_f32_32x32x2_f32: exact f32 fma chain).
 * C[z][m][n] = epilogue( alpha * sum_k A[z](m,k) * B[z](n,k) )
 * Replaces every dense contraction of the path: F.linear / nn.MultiheadAttention in_proj+out_proj
 * (maskclip_vit.py:110-118,141 via mmcv), FFN (maskclip_vit.py:94-100,142), PatchEmbed conv
 * (maskclip_vit.py:266-276,495), proj 1x1 (maskclip_vit.py:338,554), the cosine-sim einsum
 * (vlg_head.py:217), F.conv2d text classifier (vlm.py:99), all VLGHead convs (vlg_head.py:70-137,169-190),
 * q k^T / p v bmm inside attention, and all their dgrad / wgrad counterparts (autograd in the reference).
 * ---------------------------------------------------------------------------------------------- */
enum {
  SVL_A_KCONTIG = 0, /* A(m,k) = A[m*lda + k]                       (activations x, dY, Q)           */
  SVL_A_MCONTIG = 1, /* A(m,k) = A[k*lda + m]                       (dY^T for wgrad, P^T)            */
  SVL_A_CONV = 2,    /* A(m,k): m = NHWC pixel, k = (tap, ci): implicit im2col (see svl_conv_geom)   */
  SVL_A_PATCH = 3    /* A(m,k): m = (img, py, px), k = (c, i, j) of an NCHW image, patch P x P       */
};
enum {
  SVL_B_KCONTIG = 0, /* B(n,k) = B[n*ldb + k]   (torch Linear weight [out,in], K rows, packed conv w) */
  SVL_B_NCONTIG = 1, /* B(n,k) = B[k*ldb + n]   (dgrad: W as [K=out][N=in]; V in P·V; X in wgrad)     */
  SVL_B_CONVW = 2,   /* B(n,k): n = (tap, ci), k = NHWC pixel: im2col^T for conv wgrad                */
  /* B-operand producers of the weight gradients (A = SVL_A_MCONTIG only): the operand is computed while staging, never
   * materialised in fp32.  Every arithmetic of svl_set_gemm_emulation serves them; the operand-maximum pass of the fp16 x 2
   * form (emu_ws) sees the transformed values. */
  SVL_B_NC_GELU = 3, /* B(n,k) = gelu_erf(B[k*ldb + n]) (the SVL_ACT_GELU function of a saved pre-activation)       */
  SVL_B_NC_LN = 4,   /* B(n,k) = (B[k*ldb + n] - mean_k) * rstd_k * b_gamma[n] + b_beta[n], {mean, rstd} =
                      * b_stats[2k], b_stats[2k+1] (the statistics svl_layernorm_fwd wrote)                           */
  SVL_B_PATCHT = 5   /* B(n,k): n = (c, i, j), k = (img, py, px) of an NCHW image, patch P = conv.patch, grid
                      * ceil(H/P) x ceil(W/P) with bottom / right zero fill: the transposed twin of SVL_A_PATCH     */
};
enum {
  SVL_ACT_NONE = 0,
  SVL_ACT_GELU = 1,      /* erf GELU */
  SVL_ACT_RELU = 2,
  /* backward forms (SVL_OUT_STRIDED): `resid` is NOT added but read as the saved pre-activation z[m][n] */
  SVL_ACT_MUL_DGELU = 3, /* v *= GELU'(z)      -- dgrad of Linear -> GELU fused with the activation's derivative */
  SVL_ACT_MUL_DRELU = 4  /* v  = z > 0 ? v : 0 */
};
enum {
  SVL_OUT_STRIDED = 0, /* C + zo*bs_outer + zi*bs_inner + m*ld_m + n*ld_n                              */
  SVL_OUT_CONVT2X = 1, /* ConvTranspose2d k2 s2: m=(img,h,w), n=(a,b,co) -> pixel (img,2h+a,2w+b), co  */
  SVL_OUT_PATCH = 2    /* patch tokens: row m=(img,p) -> img*(P+1)+1+p ; resid row = 1+p (pos_embed)   */
  /* SVL_OUT_CONVT2X / SVL_OUT_PATCH: batch == 1 (SVL_ERR_INVALID_ARG otherwise: the batch strides address the strided
   * output only); `resid` with SVL_OUT_CONVT2X is refused (SVL_ERR_UNSUPPORTED: no residual addressing is defined for it).
   * K == 0 is valid for the dense modes: the result is the epilogue of a zero sum (so is an empty split-K range). */
};

typedef struct svl_operand {
  const float* ptr;
  int64_t ld;        /* leading dimension (elements)                                   */
  int64_t bs_outer;  /* batch stride for zo = z / batch_inner                          */
  int64_t bs_inner;  /* batch stride for zi = z % batch_inner                          */
} svl_operand;

/* Stride-1, same-size NHWC convolution geometry used by SVL_A_CONV / SVL_B_CONVW.
 * Logical input channel ci in [0, C1+C2): ci < C1 reads src1 (the operand ptr, pixel stride ld),
 * otherwise src2 (pixel stride ld2) of image (img / rep) — the `repeat`+`cat` of vlg_head.py:131-134
 * without materialising it. Tap (ti,tj) reads pixel (oh*stride + sign*(ti*dil - pad), ow*stride + sign*(tj*dil - pad));
 * sign=+1 for forward/wgrad, -1 for dgrad. Out-of-range pixels read 0. */
typedef struct svl_conv_geom {
  int H, W;          /* INPUT spatial size (bounds + addressing)                                  */
  int Ho, Wo;        /* OUTPUT spatial size used to decompose the pixel index (0 -> same as H, W) */
  int stride;        /* output -> input pixel stride (0/1 -> 1); >1 only with sign=+1 (ConvT k2s2 backward = conv k2 s2) */
  int C1, C2;
  int rep;
  int KH, KW, dil, pad, sign;
  const float* src2;
  int64_t ld2;
  int patch;  /* SVL_A_PATCH: patch size P; image is [img, C1, H, W] NCHW */
} svl_conv_geom;

typedef struct svl_gemm_desc {
  int a_mode, b_mode;
  int M, N, K;
  int batch;        /* number of z slices (>=1)                                              */
  int batch_inner;  /* z -> (zo, zi) = (z / batch_inner, z % batch_inner); >=1               */
  int ksplit;       /* >0: split-K — z indexes K ranges [z*ksplit, min(K,(z+1)*ksplit)), operand batch strides ignored */
  svl_operand A, B;
  svl_conv_geom conv;
  /* output */
  float* C;
  int out_mode;
  int64_t ldc_m, ldc_n, c_bs_outer, c_bs_inner;
  int ct_H, ct_W, ct_Cout; /* SVL_OUT_CONVT2X: input spatial size and Cout; SVL_OUT_PATCH: ct_H = patches per image */
  /* epilogue: v = alpha*acc; v += bias[n % bias_mod]; v = act(v); v += resid; if(accumulate) v += C */
  float alpha;
  const float* bias;
  int bias_mod;     /* 0: bias[n]; >0: bias[n % bias_mod] */
  int act;
  float* preact;    /* optional: value BEFORE act is also stored here (same addressing as C, SVL_OUT_STRIDED only) */
  const float* resid; /* addressed like C for SVL_OUT_STRIDED (own strides below); see SVL_OUT_PATCH */
  int64_t ldr_m, ldr_n, r_bs_outer, r_bs_inner;
  int accumulate;
  const void* conv_w_planes; /* optional, SVL_A_CONV with a 3x3 / stride 1 geometry: the weights B once more as
                              * svl_conv3x3_weight_planes(B, N, C1 + C2) wrote them (two fp16 planes + per-output-channel
                              * exponents).  Used in emulation mode 6 by (a) the spatially tiled kernel (pad 1, dilation 1,
                              * N = 32 / 64: three fp16 products per term instead of six bf16 ones) and (b) the whole-image
                              * kernel of the DILATED convolutions (pad = dilation > 1 on 32 x 32 maps, one source, N % 64 == 0,
                              * no bias / activation: the ASPP branches of vlg_head.py:38-50 and their input gradients);
                              * ignored otherwise. */
  void* emu_ws;              /* optional (round 5): 8 bytes of device scratch private to this call.  With it, emulation mode 6
                              * serves a large launch of the in-register split kernel (implicit-GEMM convolutions, their weight
                              * gradients, dense GEMMs outside the packed-planes path; >= 4 GFLOP) on fp16 x 2 terms -- three
                              * products instead of six -- with ONE power-of-two scale per operand tensor, found by a maximum
                              * pass over exactly the elements the launch reads (a per-row scale does not factor out of a
                              * convolution's taps).  Same error level vs fp64 (tests/test_ops_gpu.py); NULL: bf16 x 3 terms. */
  const float* b_stats;      /* SVL_B_NC_LN: [K][2] row statistics {mean, rstd} of the B source rows                     */
  const float* b_gamma;      /* SVL_B_NC_LN: [N] LayerNorm weight                                                         */
  const float* b_beta;       /* SVL_B_NC_LN: [N] LayerNorm bias                                                           */
  const unsigned* a_amax;    /* optional, with emu_ws: one device word each, the bit pattern of the largest |x| of the WHOLE A / B */
  const unsigned* b_amax;    /* operand this call reads (what svl_split_planes_f16x2's tensor_amax leaves for the same matrix,
                              * unwritten since).  The dense launches and the A side (SVL_B_PATCHT: both sides) of the
                              * producer launches then take the word instead of running their maximum pass over that operand;
                              * every other launch ignores them.  NULL: the pass runs. */
} svl_gemm_desc;

/* Validates the descriptor (SVL_ERR_INVALID_ARG / SVL_ERR_UNSUPPORTED before anything is launched), ROUTES it and runs the
 * route.  The route is host arithmetic on the descriptor, the arithmetic mode and svl_switches() alone -- svl_gemm_route
 * returns it without launching.  Families, in the order they are tried: the short-K row stream (fp32, or the split pipe in
 * mode 6), the elementwise Conv2d(1 -> N) kernel, the spatially tiled narrow 3x3 convolution, the whole-image dilated 3x3
 * convolution, then -- with a ragged row count (M >= 8192, M % 128 != 0) cut into a 128-aligned part and the leftover rows
 * on the helper stream, each routed on its own -- the in-register split kernel (modes 3 / 6: bf16 x 2, bf16 x 3 or, with
 * emu_ws, fp16 x 2 after the operand-maximum passes) or the exact fp32 kernel. */
int svl_gemm_f32(const svl_gemm_desc* d, svl_stream_t stream);

/* What svl_gemm_f32(d) would do, without doing it: same validation and status, same routing function, no launch and no device
 * call.  Pointers are read for their alignment (and for being null) only, so host addresses serve. */
typedef struct svl_gemm_route_info {
  int path;          /* the value svl_last_gemm_path() reports after the launch                                             */
  int h2;            /* 1: the in-register split kernel runs on fp16 x 2 terms (emu_ws given and worth its maximum passes)  */
  int tile_m, tile_n;/* block tile of the exact fp32 / in-register split kernel that serves the launch (the 128-aligned part  */
  int blocks_per_cu; /* of a ragged launch) and the blocks of it a CU holds; 0 for the families that do not tile this way    */
  int max_passes;    /* operand-maximum passes the launch makes (svl_absmax_launches() grows by this; both parts of a ragged
                      * launch together; the producers' transformed B operand has a pass of its own kind, not counted)      */
  int ragged_rows;   /* rows of the leftover part of a ragged launch (M % 128), else 0                                      */
} svl_gemm_route_info;
int svl_gemm_route(const svl_gemm_desc* d, svl_gemm_route_info* out);

/* Process-wide (relaxed-atomic, read once per call) arithmetic mode of the LARGE dense GEMMs (M >= 256, N >= 96, K >= 64, dense operand modes):
 *   0  v_mfma_f32_32x32x2_f32, exact fp32 fma chain (default);
 *   6  fp32-accurate emulation on the bf16 matrix pipe: every operand element is split into 3 bf16 terms and the 6
 *      leading cross products are accumulated in fp32 (error <= the fp32 path's, 2.7x the MFMA rate).  Mode 6 also
 *      covers svl_attention_{fwd,bwd} (all five products of the fused attention; S is recomputed bit-identically in
 *      the backward), the forward / input gradient of the spatially tiled 3x3 convolutions, and the K = 64 / 128 row
 *      streams with the ConvTranspose2d(k 2, s 2) pixel-shuffle store (SVL_OUT_CONVT2X; csrc/gemm_shortk.hip);
 *   3  2-term split, 3 products (~16 mantissa bits, 5.3x the MFMA rate); dense GEMMs only.
 * Initial value: environment variable SVL_GEMM_EMU (0 if unset).  Inputs, outputs and accumulation stay fp32. */
int svl_set_gemm_emulation(int mode);
int svl_get_gemm_emulation(void);
/* The environment's A/B switches of the GEMM / convolution dispatch as SVL_SW_* bits; every bit is set unless its variable
 * is.  The library reads the four variables here, once per process, and nowhere else. */
enum {
  SVL_SW_EMU_H2 = 1,         /* SVL_GEMM_EMU_NO_H2: mode 6 keeps the bf16 x 3 form where emu_ws would allow fp16 x 2         */
  SVL_SW_SHORTK = 2,         /* SVL_GEMM_NO_SHORTK: no short-K row stream, no elementwise Conv2d(1 -> N) kernel             */
  SVL_SW_CONV_TILED = 4,     /* SVL_CONV_NO_TILED: narrow / dilated 3x3 convolutions stay on the implicit GEMM              */
  SVL_SW_CONV_TILED_EMU = 8  /* SVL_CONV_TILED_NO_EMU: mode 6 keeps the tiled 3x3 kernels on the fp32 pipe                  */
};
int svl_switches(void);
/* Measurement aid (bench.py prices a launch against the pipe that served it; no reference counterpart): which kernel family
 * the calling thread's LAST svl_gemm_f32 (or svl_conv3x3_gn_f32 / svl_conv3x3_wgrad_tiled) call dispatched to -- 0 exact fp32 MFMA (v_mfma_f32_32x32x2_f32), 1 bf16 split
 * products (v_mfma_f32_32x32x16_bf16; emulation mode 3 / 6: dense, implicit-GEMM forward / input gradient / weight gradient,
 * tiled 3x3), 2 the short-K row stream (fp32 MFMA, HBM-bound), 3 an elementwise kernel (no MFMA), 4 the in-register split
 * kernel on fp16 x 2 terms (three products; svl_gemm_desc::emu_ws). */
int svl_last_gemm_path(void);
/* Introspection for tests: operand-maximum passes (the fp16 x 2 form's absmax kernels) this process has launched so far. */
int64_t svl_absmax_launches(void);

/* ------------------------------------------------------------------------------------------------
 * fp32-accurate GEMM with PRE-SPLIT, fragment-packed operands (the fast form of emulation mode 6; csrc/gemm_planes.hip).
 * An fp32 matrix X [rows, K] (K % 16 == 0) is held as three bf16 "planes" x = x0 + x1 + x2, packed in the register image
 * of the MFMA operand fragments: for k-group kg = k / 16, row block rb = row / 32 and plane pl one 1 KiB chunk
 *     planes[((kg * rows_padded / 32 + rb) * 3 + pl) * 1024 + (h * 32 + row % 32) * 16 .. + 16)
 * holds, for h = 0 / 1, the 8 bf16 values of row `row` at k = kg * 16 + 4 h + {0, 1, 2, 3, 8, 9, 10, 11}.  rows_padded =
 * svl_planes_rows(rows) (a multiple of 256: tiles read whole 256-row bands; the padding is never stored from);
 * svl_planes_bytes(rows, K) bytes, 1 KiB aligned.  Weights are packed once per parameter version, activations by their
 * producer (svl_layernorm_* planes outputs, the previous GEMM's epilogue, svl_split_planes_bf16x3 as the generic pass);
 * the GEMM then runs LDS-DMA + ds_read_b128 + v_mfma_f32_32x32x16_bf16 only (6 cross products, fp32 accumulate).
 * Replaces F.linear / its input gradient on the ViT linears (maskclip_vit.py:110-144 via mmcv MultiheadAttention / FFN)
 * when svl_set_gemm_emulation(6) is active.
 *   svl_split_planes_bf16x3   element (r, k) read at x[r * ld + k * k_stride] (k_stride 1: row-major; ld 1 + k_stride =
 *                             leading dim: the transpose of a row-major matrix), written to rows [row_off, row_off+rows)
 *                             of a plane buffer with planes_rows (% 256 == 0) rows; row_off % 32 == 0; the rest of the
 *                             last 32-row block is zero-filled
 *   svl_gemm_planes_f32       C[m, n] = epi(sum_k A[m, k] B[n, k]) for rows m in [m_off, m_off + M) (m_off % 32 == 0):
 *                             bias[n], act (svl_act: GELU / RELU; MUL_DGELU / MUL_DRELU multiply by the activation
 *                             derivative at resid = saved pre-activation), preact (pre-activation copy out), resid
 *                             (added), accumulate (into C); outputs: C fp32 row-major (ldc) and / or planes_out = the
 *                             result as packed planes [M, N] (p_rows % 256 == 0 rows, N % 16 == 0) for the next GEMM.
 *                             Either may be NULL, not both. */
typedef struct svl_pgemm_desc {
  const void* A;        /* packed planes of [a_rows, K], a_rows % 256 == 0 */
  const void* B;        /* packed planes of [b_rows, K], b_rows % 256 == 0, b_rows >= N */
  int64_t a_rows, b_rows;
  int m_off, M, N, K;
  float* C;
  int64_t ldc;
  void* planes_out;
  int64_t p_rows;
  const float* bias;
  int act;
  float* preact;
  const float* resid;
  int64_t ldr;
  int accumulate;
  /* round 5: the fp16 x 2 operand format (below).  All zero / NULL = the bf16 x 3 form above. */
  int fmt;                /* format of A and B: 0 = bf16 x 3 planes (six products), 1 = fp16 x 2 planes + row scales (three) */
  int p_fmt;              /* format of planes_out: 0 / 1; 1 needs fmt = 1, a_rnorm, b_bound, p_sexp and no residual add */
  const int32_t* a_sexp;  /* fmt 1: scale exponents of A's rows [a_rows] / of B's rows [b_rows]; NULL = all zero */
  const int32_t* b_sexp;
  const float* a_rnorm;   /* p_fmt 1: upper bounds of the L2 norms of A's rows [a_rows] ...                          */
  const float* b_bound;   /* ... and a device float[2] = {max row L2 norm of B, max |bias|}: row m of the result is   */
  int32_t* p_sexp;        /* bounded by a_rnorm[m] b_bound[0] + b_bound[1]; its scale exponent is written to p_sexp[m] */
} svl_pgemm_desc;
int64_t svl_planes_rows(int64_t rows);             /* rows rounded up to the 256-row band a tile reads */
int64_t svl_planes_bytes(int64_t rows, int K);
int svl_split_planes_bf16x3(const float* x, int64_t ld, int64_t k_stride, int64_t rows, int K, void* planes,
                            int64_t planes_rows, int64_t row_off, svl_stream_t stream);
/* The fp16 x 2 operand format (round 5; csrc/gemm_planes_h2.hip): x(r, k) = 2^e(r) (h0 + h1), h0 = fp16(x 2^-e(r)), h1 =
 * fp16(x 2^-e(r) - h0), one scale exponent e(r) per ROW placing the row's largest magnitude in [2^14, 2^15); chunk layout as
 * above with two planes per (k-group, row block): svl_planes_bytes_fmt(rows, K, 1) = 4 bytes per element.  Two
 * round-to-nearest fp16 terms carry 23 significand bits, the three leading cross products (v_mfma_f32_32x32x16_f16, fp32
 * accumulate) leave out a1 b1 <= 2^-22 |a b|: half the matrix work of the bf16 x 3 form at an error vs fp64 at or below the
 * plain fp32 MFMA chain's for K >= 48 (tests/test_ops_gpu.py::test_gemm_planes_path).  The GEMM multiplies its
 * accumulators by 2^(e_A(m) + e_B(n)) (exact).  svl_split_planes_f16x2 is the generic pack pass (arguments as
 * svl_split_planes_bf16x3); it also writes sexp[row_off + r] and, if rnorm != NULL, an upper bound of each row's L2 norm --
 * what a GEMM needs to scale a planes OUTPUT in this format (svl_pgemm_desc::a_rnorm / b_bound).  tensor_amax (optional,
 * one device word, zeroed by the call): receives the bit pattern of the matrix's largest |x| -- the pass holds every row's
 * maximum anyway -- in the convention of svl_gemm_desc::a_amax / b_amax (non-negative float bits, NaNs take no part). */
int64_t svl_planes_bytes_fmt(int64_t rows, int K, int fmt);
int svl_split_planes_f16x2(const float* x, int64_t ld, int64_t k_stride, int64_t rows, int K, void* planes,
                           int64_t planes_rows, int64_t row_off, int32_t* sexp, float* rnorm, unsigned* tensor_amax,
                           svl_stream_t stream);
int svl_gemm_planes_f32(const svl_pgemm_desc* d, svl_stream_t stream);
/* Weight gradient of a narrow (Co = 32 / 64) 3x3 / stride 1 / pad 1 convolution over NHWC activations with an optional
 * second concat source (read at image img / rep): slabs[g][co][tap * (C1 + C2) + ci] for g < groups (forward-pack
 * layout per slab); the caller sums the slabs (svl_reduce_slabs_f32).  Replaces the conv2d weight-gradient of
 * vlg_head.py:121-127 (Up.conv) for the layers whose implicit-GEMM form is im2col-address bound.  C1, C2 % 4 == 0, (C1 + C2) % 32 == 0.
 * Under svl_set_gemm_emulation(6) the split (fp16 x 2) kernel serves Co = 64, Co = 32 with (C1 + C2) % 64 == 0, and additionally
 * Co = 128 (an error in mode 0); svl_conv3x3_wgrad_tiled_groups sizes `groups` for the kernel the current mode selects
 * (any groups >= 1 is valid for either). */
int svl_conv3x3_wgrad_tiled_groups(int imgs, int H, int W, int Ct, int Co);
/* gn_in (may be NULL; both entry points that take it): a [imgs][2][C1] table of svl_groupnorm_scale_shift -- src1 then holds
 * the PRE-normalisation output of the previous convolution and the operand relu(fma(src1, scale, shift)) = GroupNorm + ReLU
 * (vlg_head.py:122-123) is formed while the tile is staged: the normalised tensor is never written (round 4). */
int svl_conv3x3_wgrad_tiled(const float* dy, int64_t lddy, int Co, const float* src1, int64_t ld1, int C1,
                            const float* src2, int64_t ld2, int C2, int rep, int imgs, int H, int W, float* slabs,
                            int groups, const float* gn_in, svl_stream_t stream);

/* out[i] = (accumulate ? out[i] : 0) + sum_s slabs[s*count + i]  — deterministic split-K combine. */
int svl_reduce_slabs_f32(float* out, const float* slabs, int nslab, int64_t count, int accumulate,
                         svl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Pixel-loss family (semivl.py:232,252,267-323; utils/train_utils.py:19-49; semivl.py:52-58).
 * logits are NCHW [B, N, H, W] fp32; label-like maps are int64 [B, H, W] (reference dtype).
 * ---------------------------------------------------------------------------------------------- */

/* conf[b,h,w] = max_c softmax(logits)[b,c,h,w]; label = argmax (ties -> lowest index). semivl.py:232,252 */
int svl_softmax_max_f32(const float* logits, int B, int N, int64_t HW, float* conf, int64_t* label,
                        svl_stream_t stream);

/* out = where(box == 1, b, a) elementwise over [B, HW] maps broadcast over C channels
 * (cutmix_img_: C=3 fp32 in place when out==a; cutmix_mask: C=1). utils/train_utils.py:19-27 */
int svl_cutmix_f32(float* out, const float* a, const float* b, const float* box, int B, int C, int64_t HW,
                   svl_stream_t stream);
int svl_cutmix_i64(int64_t* out, const int64_t* a, const int64_t* b, const float* box, int B, int64_t HW,
                   svl_stream_t stream);

/* Fused per-branch loss, forward + backward in one pass over the logits.
 *   ce_t(p)  = -log_softmax(logits)[target[p]]          (target == ignore_index -> 0, if use_ignore_t)
 *   ce_m(p)  = -log_softmax(logits)[mc_target[p]]       (mc_target == 255 -> 0)
 * Per block (deterministic, no atomics) partials[blk] = {
 *   sum_p w_t(p) * ce_t(p)      with w_t = 1 (supervised, conf==NULL) or
 *                                [conf >= conf_thresh && ign != 255] (pixelwise, train_utils.py:36-38),
 *   sum_p ce_m(p)               (mc term, semivl.py:52-58; 0 when mc_target == NULL),
 *   sum_p conf(p) * [ign != 255]   (pixelavg bookkeeping, train_utils.py:43-46),
 *   #(target != ignore) (supervised) or #(ign != 255) }
 * svl_ce_finalize() reduces the partials in double, in a fixed order, to sums[4].
 * If dlogits != NULL: dlogits = gscale_t * w_t * (softmax - onehot(target)) + gscale_m * [mc valid] * (softmax - onehot(mc))
 * where gscale_* are read from DEVICE memory (gscale[0], gscale[1]) so no host sync is needed.
 * A label (target or mc_target) that is not ignored and lies outside [0, N) -- 254, or 255 with use_ignore_t == 0 -- reads
 * no logit: the pixel's term is log-sum-exp - 0 and its gradient is the scale times softmax, without a one-hot term.
 * svl_ce_fused_f32 and svl_ce_up_fused_f32 agree on this, like their label-smoothing variants.
 * img_weight multiplies w_t of the confidence-weighted forms only: a descriptor with img_weight but without conf is
 * refused (status -1, the message names the field) by both entry points.
 *
 * svl_ce_fused_lsw_f32 / svl_ce_up_fused_lsw_f32 (the labelled criterion with label_smoothing eps and class weights w,
 * below) fill the same four slots with another meaning: partials[blk] = {
 *   sum_p [t != 255] ( (1 - eps) w_t ce_t(p) + (eps / N) sum_c w_c (-log_softmax(logits)[c]) ),
 *   0, 0,
 *   sum_p [t != 255] w_t }       (integer-valued without weights: the count of labelled pixels)
 * so that sums[0] / sums[3] is torch's weighted, smoothed mean and svl_semivl_loss reads it unchanged.
 */
typedef struct svl_ce_desc {
  const float* logits;   /* [B, N, HW] */
  int B, N;
  int64_t HW;
  const int64_t* target; /* [B, HW] */
  int use_ignore_t;      /* 1: target==255 ignored (criterion_l, ignore_index=255); 0: criterion_u */
  const float* conf;     /* [B, HW] or NULL */
  const int64_t* ign;    /* [B, HW] or NULL */
  float conf_thresh;
  int all_pixels;        /* 1: conf_mode 'pixelavg' — w_t = 1 on every pixel (train_utils.py:43-46 sums the whole CE map) */
  const int64_t* mc_target; /* [B, HW] or NULL */
  float* partials;       /* workspace [svl_ce_num_blocks(B,N,HW)][4]: per-block {sum w*ce_t, sum ce_m, sum conf*valid, #valid} */
  float* dlogits;        /* [B, N, HW] or NULL */
  const float* gscale;   /* [2] device scalars, required when dlogits != NULL */
  const float* img_weight; /* [B] device or NULL: per-image factor on w_t -- conf_mode 'pixelratio' (train_utils.py:39-42:
                              the whole CE map of image b times its share of confident valid pixels; with all_pixels = 1).
                              Needs conf: refused without it */
} svl_ce_desc;
int64_t svl_ce_num_blocks(int B, int N, int64_t HW); /* -1 if N is unsupported (N > 256) */
int svl_ce_fused_f32(const svl_ce_desc* d, svl_stream_t stream);
int svl_ce_finalize(const float* partials, int64_t nblocks, double* sums /* [4] device */, svl_stream_t stream);
/* The labelled criterion as nn.CrossEntropyLoss(ignore_index=255, label_smoothing=eps, weight=w) (semivl.py:142-143: the
 * reference passes cfg['criterion']['kwargs'] to torch).  With W = sum_c w_c, p = softmax(logits), lse = logsumexp(logits):
 *   numerator(pixel) = (1 - eps) w_t (lse - x_t) + (eps / N) sum_c w_c (lse - x_c)                  (t != 255, else 0)
 *   dlogits_c = g [t != 255] ( (1 - eps) w_t (p_c - [c == t]) + (eps / N) (W p_c - w_c) ),   g = gscale[0] (device)
 * and the loss is sum numerator / sum [t != 255] w_t: partials as described above, reduced by svl_ce_finalize.
 * label_smoothing in [0, 1]; class_weight: float[N] on the device, or NULL for all ones.  Labelled branch only: a
 * descriptor with conf, ign, mc_target, img_weight or all_pixels set, or with use_ignore_t == 0, is refused (status -1,
 * the message names the field).  Same workspace (svl_ce_num_blocks), tiling and determinism as svl_ce_fused_f32; an
 * ignored pixel's gradient is exactly 0 and is never multiplied by g (g is 1 / 0 when every target is 255). */
int svl_ce_fused_lsw_f32(const svl_ce_desc* d, float label_smoothing, const float* class_weight, svl_stream_t stream);

/* Round 5: the same two pixel-loss entry points on logits that exist ONLY at the head's resolution.  The reference
 * resizes the head's [B, N, h, w] map to the crop (vlg_head.py:247, builder.py:93-97: bilinear, align_corners as
 * configured) and runs semivl.py:232,252 / 267-323 on the [B, N, H, W] result; here the resize (ATen upsample_bilinear2d
 * index math) is evaluated inside the kernels and the gradient is returned at the LOW resolution -- what
 * F.interpolate's backward would hand to the head.  Full-resolution logits / dlogits are never written.
 * Geometry: upsampling only (H >= h, W >= w), ratio <= 4.5 with at most 40 resized rows / columns per 8 head-resolution cells, N <= 160; svl_ce_up_num_blocks < 0 when unsupported
 * (callers then resize with svl_bilinear_planes_fwd and use svl_ce_fused_f32).  Maps (target, conf, ign, mc_target) are
 * full resolution [B, H, W]; partials: [svl_ce_up_num_blocks][4], reduced by svl_ce_finalize.  Deterministic. */
typedef struct svl_ce_up_desc {
  const float* logits;   /* [B, N, h, w] */
  int B, N;
  int h, w, H, W;
  int align_corners;
  const int64_t* target; /* [B, H, W] */
  int use_ignore_t;
  const float* conf;     /* [B, H, W] or NULL */
  const int64_t* ign;    /* [B, H, W] or NULL */
  float conf_thresh;
  int all_pixels;
  const int64_t* mc_target; /* [B, H, W] or NULL */
  float* partials;
  float* dlogits;        /* [B, N, h, w] or NULL: d(loss)/d(logits) at the head's resolution */
  const float* gscale;   /* [2] device scalars, required when dlogits != NULL */
  const float* img_weight; /* [B] device or NULL; refused without conf, as in svl_ce_desc */
} svl_ce_up_desc;
int64_t svl_ce_up_num_blocks(int B, int N, int h, int w, int H, int W, int align_corners);
int svl_ce_up_fused_f32(const svl_ce_up_desc* d, svl_stream_t stream);
/* svl_ce_fused_lsw_f32 on the resized logits (same formulas, refusals and partials; the gradient arrives at the head's
 * resolution).  Its kernel stages the class weights in LDS beside the tile, so it has its own host-only geometry query:
 * svl_ce_up_lsw_num_blocks is the size of `partials` in blocks, or -1 when the geometry is unsupported or does not fit the
 * 160 KB of LDS (callers then resize with svl_bilinear_planes_fwd and use svl_ce_fused_lsw_f32). */
int64_t svl_ce_up_lsw_num_blocks(int B, int N, int h, int w, int H, int W, int align_corners);
int svl_ce_up_fused_lsw_f32(const svl_ce_up_desc* d, float label_smoothing, const float* class_weight, svl_stream_t stream);
/* conf / label [B, H, W] = softmax(dim 1).max(dim 1) of the resized logits (semivl.py:232,252); first maximum wins. */
int svl_softmax_max_up_f32(const float* logits, int B, int N, int h, int w, int H, int W, int align_corners, float* conf,
                           int64_t* label, svl_stream_t stream);

/* Loss assembly without host syncs (semivl.py:267-323).
 * counts: int64[4] device = #valid of {mask_x != 255, ignore_mask_mixed1, ignore_mask_mixed2, ignore_mask} != 255.
 * gscale out: float[4][2] device = {g_t, g_m} for the branches {x, s1, s2, fp}: the factor each per-pixel CE term
 * carries in d(loss)/d(logits).  numel_u = B*H*W of one unlabeled branch; lam = current mcc lambda.
 * mc_counts: int64[3] device or NULL -- the guidance loss's normalisers for the branches {s1, s2, fp} when
 * mcc_loss_reduce is not 'mean_all' (semivl.py:52-58,156-162): 'mean_valid' = #(ignore mask != 255) (= counts[1..3]),
 * 'mean' = #(guidance label != 255) (nn.CrossEntropyLoss(ignore_index=255) mean); NULL = numel_u ('mean_all'). */
int svl_semivl_gscale(const int64_t* counts, double numel_u, float lam, const double* factors, const int64_t* mc_counts,
                      float* gscale, svl_stream_t stream);
/* The supervised baseline's normaliser (third_party/unimatch/supervised.py:281-283: the loss is the plain mean of the
 * cross entropy over the kept pixels, weight 1).  out[0] (device float) = (float)(1.0 / (double)count[0]) for the device
 * int64 count[0] >= 0 read as unsigned: the g_t of svl_ce_fused_f32 / svl_ce_up_fused_f32, formed without a host
 * synchronisation.  Only out[0] is written: callers that pass it as `gscale` [2] zero g_m themselves.  count[0] == 0
 * gives +inf, which no pixel then multiplies (every target is 255). */
int svl_inv_count_f32(const int64_t* count, float* out, svl_stream_t stream);
/* The normaliser of a class-weighted mean (nn.CrossEntropyLoss(weight=w), reduction 'mean'), without a host
 * synchronisation: sum[0] (device double) = sum over the n pixels with target != 255 of class_weight[target], accumulated
 * in double in two stages with a fixed order (deterministic); a label outside [0, N) adds nothing.  class_weight: float[N]
 * on the device.  workspace: svl_class_weight_sum_ws_doubles(n) doubles of device memory, caller-owned, no initialisation. */
int64_t svl_class_weight_sum_ws_doubles(int64_t n);
int svl_class_weight_sum_f64(const int64_t* target, int64_t n, const float* class_weight, int N, double* sum,
                             double* workspace, svl_stream_t stream);
/* out[0] (device float) = (float)(factor / sum[0]) for the device double sum[0]: the weighted counterpart of
 * svl_inv_count_f32 (factor 1 for the supervised step, 0.5 for the labelled branch of the semi-supervised one, where it
 * overwrites gscale[0][0] after svl_semivl_gscale).  Only out[0] is written; sum[0] == 0 gives +inf, which no pixel
 * then multiplies. */
int svl_scale_from_sum_f32(const double* sum, double factor, float* out, svl_stream_t stream);
/* conf_mode 'pixelavg' (train_utils.py:43-46): factor[0] = sum over images b of mean_{valid pixels}(conf_b).  The
 * unsupervised branch loss is (sum over ALL pixels of CE) * factor / #valid.  `factors` above/below: double[3] device
 * for the branches {s1, s2, fp}, or NULL for 'pixelwise'. */
int64_t svl_conf_avg_ws_doubles(int B); /* size of `workspace` below, in doubles */
int svl_conf_avg_factor(const float* conf, const int64_t* ign, int B, int64_t HW, double* factor, double* workspace,
                        svl_stream_t stream);
/* conf_mode 'pixelratio' (train_utils.py:39-42): ratio[b] = #(conf_b >= thresh & valid) / #valid of image b, the fp32
 * quotient of the two counts (torch's int / int); fed to svl_ce_fused_f32 as img_weight with all_pixels = 1.
 * workspace: svl_conf_avg_ws_doubles(B) doubles. */
int svl_conf_ratio_f32(const float* conf, const int64_t* ign, int B, int64_t HW, float thresh, float* ratio,
                       double* workspace, svl_stream_t stream);
/* sums: double[4 branches][4] device (from svl_ce_finalize); out float[8] device =
 * {loss, loss_x, loss_s1, loss_s2, loss_fp, loss_mc_s1, loss_mc_s2, loss_mc_fp}. */
int svl_semivl_loss(const double* sums, double numel_u, float lam, const double* factors, const int64_t* mc_counts,
                    float* out, svl_stream_t stream);
/* out[b, c, p] = softmax over classes c of NCHW logits (probability accumulation of the sliding-window eval modes,
 * supervised.py:61,113). */
int svl_softmax_planes_f32(const float* logits, int B, int N, int64_t HW, float* out, svl_stream_t stream);

/* OHEM supervised criterion (third_party/unimatch/util/ohem.py: ProbOhemCrossEntropy2d, selected by cfg['criterion'] =
 * 'OHEM', semivl.py:142-149,267), one rank's batch, no host synchronisation.  The criterion relabels the target and then
 * runs the plain cross entropy (svl_ce_fused_f32 / svl_ce_up_fused_f32 on the relabelled map, its count as normaliser):
 *   svl_target_prob_f32     prob [B, HW] = softmax over classes of logits [B, N, HW] at the target class (svl_ce_fused_f32's
 *                           max-subtracted arithmetic); 1.0 where target == 255.  Targets are in [0, N) or 255;
 *   svl_target_prob_up_f32  the same on bilinear(logits [B, N, h, w] -> [H, W]) evaluated in the kernel (svl_ce_up_fused_f32's
 *                           index math, tiling and base-2 arithmetic; geometry: svl_ce_up_num_blocks > 0); prob [B, H, W];
 *   svl_ohem_threshold_f32  threshold[0] (device float) = the effective threshold of ohem.py:39-52 over prob [n]
 *                           (n <= 2^31 - 1, 16-byte aligned, values in [0, 1]): with v = the k-th smallest prob (exact radix
 *                           select over the fp32 bit patterns, bit-identical to torch.kthvalue; k = min(n, min_kept) from the
 *                           host) it is max(v, thresh) when num_valid > 0 and 0 < min_kept <= num_valid, else +inf (keep every
 *                           valid pixel: min_kept > num_valid, min_kept == 0, or nothing valid).  num_valid: device int64, the
 *                           count svl_count_valid_i64 produces for the target.  ws: svl_ohem_ws_bytes(n) bytes of device
 *                           memory (no initialisation needed); deterministic;
 *   svl_ohem_relabel_i64    out[i] = target[i] where target[i] != 255 and prob[i] <= threshold[0], else 255;
 *                           count (device int64, may be NULL) += the number of kept pixels. */
int svl_target_prob_f32(const float* logits, int B, int N, int64_t HW, const int64_t* target, float* prob,
                        svl_stream_t stream);
int svl_target_prob_up_f32(const float* logits, int B, int N, int h, int w, int H, int W, int align_corners,
                           const int64_t* target, float* prob, svl_stream_t stream);
int64_t svl_ohem_ws_bytes(int64_t n);
int svl_ohem_threshold_f32(const float* prob, int64_t n, int64_t k, const int64_t* num_valid, int64_t min_kept,
                           float thresh, void* ws, float* threshold, svl_stream_t stream);
int svl_ohem_relabel_i64(const int64_t* target, const float* prob, int64_t n, const float* threshold, int64_t* out,
                         int64_t* count, svl_stream_t stream);

/* counts-only pre-pass so the normalisers of semivl.py:38/57 exist before the fused pass:
 * counts[0] += #(map != 255) over [n] */
int svl_count_valid_i64(const int64_t* map, int64_t n, int64_t* count, svl_stream_t stream);

/* MaskCLIP guidance tail (vlm.py:100-109): dense [B, N, h, w] class scores ->
 * bilinear(align_corners=False) to [H, W] -> softmax(100 x) -> max/argmax -> (<thr -> 255); then
 * ign == 255 -> 255 (semivl.py:239-240). out int64 [B, H, W]. */
int svl_maskclip_labels(const float* dense, int B, int N, int h, int w, int H, int W, float scale,
                        float thresh, const int64_t* ign, int64_t* out, svl_stream_t stream);

/* per class max over its concept channels (text_embeddings.py:188-193).
 * concept_offsets [N+1] device int32, concepts of class c are channels [off[c], off[c+1]). */
int svl_concept_max_f32(const float* pred, int B, int NC, int64_t HW, const int* concept_offsets, int N,
                        float* out, svl_stream_t stream);

/* Evaluation: intersectionAndUnion of third_party/unimatch/util/utils.py:91-103 as integer histograms.
 * hist int64 [3K] (caller zeroes; accumulated): [0,K) intersection, [K,2K) prediction area, [2K,3K) target area;
 * pixels with target == ignore_index are dropped from all three. */
int svl_iou_hist_i64(const int64_t* pred, const int64_t* target, int64_t n, int K, int ignore_index, int64_t* hist,
                     svl_stream_t stream);

/* Pseudo-label / guidance quality counts of the semi-supervised step (monitor.py): one pass over the n = B H W pixels of
 *   mask_w int64 [n]  pseudo-label            conf float [n]  its confidence          ign int64 [n]  255 = padding
 *   mc     int64 [n] or NULL  MaskCLIP guidance, 255 = none
 *   gt     int64 [n] or NULL  held-back annotation; anything outside [0, N) = no annotation (255 void, 254 padding)
 * adds (+=, the caller zeroes and accumulates over steps) into stats int64 [13 N + 2 bins + 1].  With
 *   v = ign != 255;  k = v && conf >= thresh (fp32, as the cross-entropy kernels compare; NaN is not confident);
 *   m = v && 0 <= mc < N;  g = v && 0 <= gt < N;  p = mask_w (outside [0, N): counts nowhere as a prediction)
 * the rows, [N] each, count the pixels with
 *    0 pl_area      v, p==c              7 plc_gt_area  k, g, gt==c
 *    1 plc_area     k, p==c              8 plc_inter    k, g, gt==c, p==c
 *    2 mc_area      m, mc==c             9 plc_area_gt  k, g, p==c
 *    3 agree        m, mc==c, p==c      10 mc_gt_area   m, g, gt==c
 *    4 gt_area      g, gt==c            11 mc_inter     m, g, gt==c, mc==c
 *    5 pl_inter     g, gt==c, p==c      12 mc_area_gt   m, g, mc==c
 *    6 pl_area_gt   g, p==c
 * then conf_hist [bins] over v, conf_hist_correct [bins] over g && p==gt, and one slot that receives n.  The bin is
 * min((int)(conf * (float)bins), bins - 1) in fp32; a conf that is not >= 0 goes to bin 0.  Rows (5, 6, 4), (8, 9, 7) and
 * (11, 12, 10) are intersectionAndUnion(pred, target', N, 255)'s (intersection, prediction area, target area) with target' =
 * gt where the row's condition holds and 255 elsewhere.  Rows of a NULL mc / gt get nothing added.  Integer counts: two
 * runs agree bit for bit.  The int64 maps are read with 16-byte loads when all of them are 16-byte aligned and conf is
 * 8-byte aligned, with scalar loads otherwise.  Refused (SVL_ERR_INVALID_ARG): null mask_w / conf / ign / stats, n < 1,
 * N < 1, bins < 1, a table (13 N + 2 bins 32-bit counters) beyond 64 KB of LDS, n so large that one block of the capped
 * grid would see 2^32 pixels. */
int svl_pl_stats_i64(const int64_t* mask_w, const float* conf, const int64_t* ign, const int64_t* mc, const int64_t* gt,
                     int64_t n, int N, int bins, float thresh, int64_t* stats, svl_stream_t stream);
/* pixels one trip of svl_pl_stats_i64's capped grid covers on the 16-byte path (host only) */
int64_t svl_pl_stats_pass_pixels(void);
/* the meter's per-step bookkeeping: sum[i] += losses[i] for i < k (k <= 64), steps[0] += 1; one launch, stream-ordered */
int svl_pl_add_losses(const float* losses, int k, double* sum, int64_t* steps, svl_stream_t stream);

/* Confusion table of the evaluation report (report.py): one pass over the n pixels of pred / target (int64) adds (+=, the
 * caller zeroes and accumulates over batches) into table int64 [(K+1) x (K+1)], rows = annotation, columns = prediction.
 * A pixel with target == ignore_index is counted nowhere; any other pixel adds 1 at table[r][c] with
 *   r = target if 0 <= target < K else K        (254, -1: targets that are neither a class nor ignored)
 *   c = pred   if 0 <= pred   < K else K
 * -- both keys are formed before anything is indexed with them.  The table is a superset of svl_iou_hist_i64's rows:
 *   intersection[k] = table[k][k];  prediction area[k] = sum_{r=0..K} table[r][k];  target area[k] = sum_{c=0..K} table[k][c].
 * Integer counts: two runs agree bit for bit.  K <= svl_confusion_lds_max_classes(): block-private 32-bit counters in LDS
 * ((K+1)^2 x 4 bytes; above 64 KB one block per CU), flushed with 64-bit atomics before they could wrap; above it the waves'
 * aggregated counts go straight into 64-bit global atomics.  The maps are read with 16-byte loads when both are 16-byte
 * aligned, with scalar loads otherwise.  Refused (SVL_ERR_INVALID_ARG, table untouched): null pointers, n <= 0, K < 1,
 * K > 1024, 0 <= ignore_index < K (the reference's intersectionAndUnion counts an ignored class as a hit there; not
 * reproduced). */
int svl_confusion_i64(const int64_t* pred, const int64_t* target, int64_t n, int K, int ignore_index, int64_t* table,
                      svl_stream_t stream);
/* the largest K whose table svl_confusion_i64 keeps in LDS (host only) */
int svl_confusion_lds_max_classes(void);
/* measurement aid (tools/time_confusion.py): moves that boundary process-wide; K < 0 restores the built-in value, K above
 * 201 ((K+1)^2 x 4 bytes beyond the 160 KB of LDS) is refused.  Results do not depend on it. */
int svl_set_confusion_lds_max_classes(int K);
/* out[i] = (uint8_t)label[i] (numpy's astype(np.uint8): the low byte) for the palette PNG export: 16-byte loads and 8-byte
 * stores when label is 16-byte and out 8-byte aligned, one by one otherwise and on the n % 8 tail.  Refused: null, n <= 0. */
int svl_label_u8_i64(const int64_t* label, int64_t n, uint8_t* out, svl_stream_t stream);

/* Debug panels of the training driver (panel.py; the figure of semivl.py:371-406 / utils/plot_utils.py): RGB tiles written
 * into a u8 canvas.  `dst` points at the tile's first byte for sample 0; pixel (b, y, x), channel c lands at
 * dst[b * batch_stride + y * row_stride + 3 x + c] (strides in bytes; dst may have any byte alignment).  Nothing outside the
 * B tiles of H x W x 3 bytes is written.  Both read their input once, 4 consecutive pixels of a sample per thread with
 * 16-byte loads, and store the 12 bytes as three 4-byte words where the address is 4-byte aligned and the 4 pixels share a
 * row, byte by byte otherwise; capped grid, grid-strided, no atomics: reruns agree bit for bit.
 * Refused by both (SVL_ERR_INVALID_ARG, nothing written): null pointers, B / H / W < 1, B H W >= 2^31 - 3,
 * row_stride < 3 W, B > 1 and batch_stride < (H - 1) row_stride + 3 W (tiles would overlap).
 *
 * svl_panel_image_u8: img fp32 [B][3][H][W] (4-byte aligned), normalised with mean3 / std3 (HOST pointers, 3 floats each):
 *   v = img * std3[c] + mean3[c]   -- two separately rounded fp32 operations, torch's .mul(std).add(mean), no contraction
 *   v = clamp(v, 0, 1), NaN -> 0;   byte = (uint8_t)(v * 255.0f + 0.5f)   -- again separately rounded
 * svl_panel_label_u8: label int64 [B][H][W] (8-byte aligned); palette: DEVICE u8 [K][3], 1 <= K <= 256 (refused otherwise):
 *   pixel = palette[l] for 0 <= l < K, (255, 255, 255) otherwise (-1, K, 254, 255, 2^40: plot_utils.py's colorize_label);
 *   the key is checked before anything is indexed with it. */
int svl_panel_image_u8(const float* img, int B, int H, int W, const float* mean3, const float* std3, uint8_t* dst,
                       int64_t batch_stride, int64_t row_stride, svl_stream_t stream);
int svl_panel_label_u8(const int64_t* label, int B, int H, int W, const uint8_t* palette, int K, uint8_t* dst,
                       int64_t batch_stride, int64_t row_stride, svl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Normalisation / elementwise / attention helpers (maskclip_vit.py:120-144, vlg_head.py:39-137).
 * ---------------------------------------------------------------------------------------------- */

/* LayerNorm over the last dim C of x [rows, C] (C % 4 == 0); stats [rows, 2] = (mean, rstd):
 *   mean = sum(x) / C;  var = sum((x - mean)^2) / C (two passes, biased);  rstd = 1 / sqrt(var + eps);
 *   y = (x - mean) * rstd * gamma + beta   (left to right in fp32; a product and the sum behind it may be fused).
 * Every LayerNorm entry point below reads and writes x / y / gamma / beta / dy / dx / dx_add as 16-byte channel quads: a
 * pointer that is not 16-byte aligned is refused (SVL_ERR_INVALID_ARG) before anything is launched. */
int svl_layernorm_fwd(const float* x, const float* gamma, const float* beta, float eps, int64_t rows, int C,
                      float* y, float* stats, svl_stream_t stream);
/* The same with the result ALSO (y != NULL) or ONLY (y == NULL) emitted as packed bf16x3 planes, the A operand of the
 * following svl_gemm_planes_f32 (C % 16 == 0; planes_rows % 256 == 0 rows in the plane buffer, rows start at 0):
 * LN1 -> qkv and LN2 -> FFN-1 of every ViT block (maskclip_vit.py:120-144). */
int svl_layernorm_fwd_planes(const float* x, const float* gamma, const float* beta, float eps, int64_t rows, int C,
                             float* y, float* stats, void* planes, int64_t planes_rows, svl_stream_t stream);
/* The same with the result as fp16 x 2 planes (svl_pgemm_desc.fmt = 1): sexp [planes_rows] receives the rows' scale exponents,
 * rnorm [planes_rows] (optional) upper bounds of their L2 norms; the planes are bit-identical to svl_split_planes_f16x2 over
 * the fp32 result (which `y`, optional here, still receives). */
int svl_layernorm_fwd_planes_f16x2(const float* x, const float* gamma, const float* beta, float eps, int64_t rows, int C,
                                   float* y, float* stats, void* planes, int64_t planes_rows, int32_t* sexp, float* rnorm,
                                   svl_stream_t stream);
/* LayerNorm forward / backward (no weight-gradient partials) with the fp16 x 2 planes of the result as a by-product of ONE
 * pass, C = 768 (other widths: SVL_ERR_UNSUPPORTED; run the row kernel, then svl_split_planes_f16x2).  The finished rows are
 * packed from an LDS copy instead of a second read: y (optional) / dx / stats carry the bits of svl_layernorm_fwd / _bwd,
 * planes / sexp / rnorm / tensor_amax those of svl_split_planes_f16x2(result, rows, C, planes, planes_rows, row_off, ...),
 * padding rows of the last 32-row block included.  row_rnorm != 0 (forward): sexp / rnorm as svl_layernorm_fwd_planes_f16x2
 * leaves them instead (the norm bound from the row pass's fp32 sum of squares; padding rows untouched). */
int svl_layernorm_fwd_pack_f16x2(const float* x, const float* gamma, const float* beta, float eps, int64_t rows, int C,
                                 float* y, float* stats, void* planes, int64_t planes_rows, int64_t row_off, int32_t* sexp,
                                 float* rnorm, int row_rnorm, unsigned* tensor_amax, svl_stream_t stream);
int svl_layernorm_bwd_pack_f16x2(const float* dy, const float* x, const float* stats, const float* gamma, int64_t rows, int C,
                                 const float* dx_add, float* dx, void* planes, int64_t planes_rows, int64_t row_off,
                                 int32_t* sexp, float* rnorm, unsigned* tensor_amax, svl_stream_t stream);
/* dx = LN backward (+ dx_add if non-NULL, fused residual-grad add), C <= 1024, from the stats it is given:
 *   xhat = (x - mean) * rstd;  m1 = sum_c(dy gamma) / C;  m2 = sum_c(dy gamma xhat) / C;
 *   dx = rstd * (dy gamma - m1 - xhat m2) (+ dx_add).
 * If dgamma_part != NULL (dbeta_part then too) also writes per-block partial sums dgamma_part/dbeta_part [nparts, C]
 * (nparts = svl_layernorm_bwd_parts(rows)) of dy * xhat and of dy over the block's rows, in a fixed order:
 *   dgamma = sum_r dy xhat = column sum of dgamma_part,  dbeta = sum_r dy = column sum of dbeta_part. */
int svl_layernorm_bwd_parts(int64_t rows);
int svl_layernorm_bwd(const float* dy, const float* x, const float* stats, const float* gamma, int64_t rows,
                      int C, const float* dx_add, float* dx, float* dgamma_part, float* dbeta_part,
                      svl_stream_t stream);
/* Row softmax in place over the first `cols` entries of rows with stride ld: p = softmax(scale * s).
 * Entries [cols, ld) are zeroed. */
int svl_softmax_rows_fwd(float* s, int64_t rows, int cols, int64_t ld, float scale, svl_stream_t stream);
/* ds = scale * p * (dp - sum_j dp_j p_j), in place on dp. */
int svl_softmax_rows_bwd(float* dp, const float* p, int64_t rows, int cols, int64_t ld, float scale,
                         svl_stream_t stream);

/* y = x / max(||x||_2, eps) over rows of [rows, C]; inv_norm [rows] = 1 / max(||x||_2, eps) saved.
 * (maskclip_vit.py:555, vlg_head.py:215)   Backward: dx = inv_norm * (dy - y * <dy, y>).  This is the gradient of
 * x / max(||x||_2, eps) only while the clamp is inactive (||x||_2 >= eps); where it is active the gradient is dy / eps, from
 * which the formula differs by y <dy, y> / eps (nothing for a zero row, y = 0).  The project calls it with eps in
 * {0, 1e-12} on CLIP embeddings, whose norms are far above either. */
int svl_l2norm_fwd(const float* x, int64_t rows, int C, float eps, float* y, float* inv_norm, svl_stream_t stream);
int svl_l2norm_bwd(const float* dy, const float* y, const float* inv_norm, int64_t rows, int C, float* dx,
                   svl_stream_t stream);

/* out[c] (+)= sum_r x[r*ld + c]  (bias gradients). Two deterministic stages through ws
 * (svl_colsum_ws_floats(rows, C) floats): the order of the additions is fixed for a given (rows, C, ld, alignment), so two
 * calls give the same bits; which order it is is not part of the contract (no chain is longer than rows + 8 additions). */
int64_t svl_colsum_ws_floats(int64_t rows, int C);
int svl_colsum_f32(const float* x, int64_t rows, int C, int64_t ld, float* out, int accumulate, float* ws,
                   svl_stream_t stream);

/* Elementwise: mode 0: out = a + b; 1: out = a * gelu'(b) (a = dY, b = pre-activation); 2: out = a * (b > 0) (relu bwd,
 * b = post-activation); 3: out = a * b; 4: out = a (copy); 5: out = gelu(a); 6: out = relu(a); 7: out = a / b. n elements. */
int svl_eltwise_f32(int mode, const float* a, const float* b, float* out, int64_t n, svl_stream_t stream);
/* out[r, c] = x[r, c] * mask[(r / rows_per_img) * C + c] * scale  — F.dropout2d on token layout (builder.py:79-85). */
int svl_chanmask_f32(const float* x, const float* mask, float scale, int64_t rows, int rows_per_img, int C,
                     float* out, svl_stream_t stream);
int svl_fill_f32(float* p, float v, int64_t n, svl_stream_t stream);
/* p[i] = 1 with probability keep_prob else 0: the per-(sample, channel) draws of F.dropout2d (builder.py:79-85; torch's
 * own generator stream is not reproduced -- the reference's masks are random too).  Counter-based: element i is a hash of
 * (seed, offset + i); the caller advances `offset` by n between calls. */
int svl_bernoulli_f32(float* p, int64_t n, float keep_prob, uint64_t seed, uint64_t offset, svl_stream_t stream);
/* y = ((x * k[0][c] + k[1][c]) - k[2][c]) / k[3][c] on NCHW planes (planes = B * C, k4 = float[4][C] device): the loader
 * (ImageNet) -> CLIP statistics re-normalisation of VLM.renormalize_img_for_clip (model/vlm.py:69-78), same op order. */
int svl_affine_planes_f32(const float* x, int64_t planes, int C, int64_t HW, const float* k4, float* y, svl_stream_t stream);
/* Strided row copy / gather / scatter / broadcast of `rows` rows of C floats:
 *   dst[(i / dgrp)*dst_go + (i % dgrp)*dst_ld + c] (=|+=) src[(i / sgrp)*src_go + (i % sgrp)*src_ld + c]
 * (token slicing x[:, 1:], cls-row scatter, torch.cat into channel slices, batch broadcast, strided grad adds).
 * Destination rows of one call must be distinct: each element is one plain load / store (no atomics), so two rows that
 * land on the same destination leave one of them (plain copy) or lose addends (accumulate).  A sum over rows takes one
 * call per addend (the pos_embed gradient: one call per image). */
int svl_copy2d_f32(const float* src, int64_t sgrp, int64_t src_go, int64_t src_ld, float* dst, int64_t dgrp,
                   int64_t dst_go, int64_t dst_ld, int64_t rows, int C, int accumulate, svl_stream_t stream);
/* dst (contiguous [n0, n1, n2, n3]) = src read through the element strides (s0 .. s3): the weight-sized permutes between the
 * nn.Conv2d / nn.ConvTranspose2d parameter layouts ([Co, Ci, kh, kw], vlg_head.py:84-137) and the kernels' packs. */
int svl_permute4_f32(const float* src, float* dst, int64_t n0, int64_t n1, int64_t n2, int64_t n3, int64_t s0, int64_t s1,
                     int64_t s2, int64_t s3, svl_stream_t stream);
/* out2 = {max_r rnorm[r], max_i |bias[i]|} (bias may be null: 0): svl_pgemm_desc::b_bound of an fp16 x 2 planes output from
 * the row norms svl_split_planes_f16x2 leaves (F.linear's bias, maskclip_vit.py:110-144). */
int svl_bound2_f32(const float* rnorm, int64_t rows, const float* bias, int64_t nbias, float* out2, svl_stream_t stream);
/* Row permutation [outer, A, B, C] -> [outer, B, A, C] (C % 4 == 0): einops '(b n) (h w) c -> (b h w) n c' of the
 * SemanticTransformer (vlg_head.py:44-62) when its class sequences run on svl_attention_fwd / _bwd (N >= 64). */
int svl_permute_rows_f32(const float* src, int64_t outer, int A, int B, int C, float* dst, svl_stream_t stream);

/* GroupNorm (+ optional ReLU) on NHWC class-images: x [imgs, HW, C] (pixel stride ldx), groups of C/G channels,
 * stats [imgs, G, 2] = (mean, rstd); y pixel stride ldy (lets the result land in a concat slice). vlg_head.py:74-137
 * Every entry point of the family takes C % 4 == 0, C <= 1024 with 256 % (C / 4) == 0, G <= 64, (C / G) % 4 == 0, pixel
 * strides that are multiples of 4 and >= C, 16-byte aligned x / y / dy / dx / gamma / beta / scsh (all accesses are
 * channel quads) and imgs <= 65535 (the apply passes put the images on gridDim.y); anything else is
 * SVL_ERR_INVALID_ARG with nothing launched. */
int svl_groupnorm_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, int imgs,
                      int64_t HW, int C, int G, int relu, float* y, int64_t ldy, float* stats, svl_stream_t stream);
/* Conv2d(3x3, stride 1, pad 1, no bias; NHWC, optional second concat source read at image img / rep) of the Up blocks
 * FUSED with the statistics of the GroupNorm that follows it (vlg_head.py:120-127, groups of 16 channels): out [imgs H W, N]
 * (pixel stride ldo) and stats [imgs, N / 16, 2] = (mean, rstd), the latter from per-tile partial sums left by the
 * convolution's epilogue (ws: svl_conv3x3_gn_ws_doubles(...) doubles of device scratch) -- the separate statistics pass
 * over the result (4 B per element of HBM reads) disappears.  w = the forward pack [N, 9 (C1 + C2)].  Returns
 * SVL_ERR_UNSUPPORTED without launching anything when the spatially tiled kernel does not take the shape (N not 32 / 64,
 * channels not a multiple of 16, fewer than 16384 pixels): run svl_gemm_f32 + svl_groupnorm_fwd instead. */
int64_t svl_conv3x3_gn_ws_doubles(int imgs, int H, int W, int N);
int svl_conv3x3_gn_f32(const float* src1, int64_t ld1, int C1, const float* src2, int64_t ld2, int C2, int rep,
                       const float* w, int imgs, int H, int W, int N, float* out, int64_t ldo, float eps, double* ws,
                       float* stats, const float* gn_in, const void* w_planes, svl_stream_t stream);
/* The weights of a 3x3 convolution (forward pack [N, 9 Ct], or the input-gradient pack [Cin, 9 Cout]; N % 32 == 0,
 * Ct % 16 == 0) split ONCE into two fp16 planes scaled by a power of two per OUTPUT channel (w = 2^e[n] (h0 + h1), e[n] from
 * the channel's largest |w|), in the LDS image of the tiled kernel (per slab of 16 input channels: [plane][tap N + n][16]),
 * followed by the N int32 exponents -- svl_conv3x3_weight_planes_bytes(N, Ct) = 4 bytes per weight + 4 N.  Optional operand
 * `w_planes` of svl_conv3x3_gn_f32 / svl_conv3x3_dgrad_gnb_f32 and `conv_w_planes` of svl_gemm_desc (N a multiple of 32; the
 * dilated whole-image kernel takes N % 64 == 0): with it the tiled kernel
 * runs three fp16 MFMA products per term with a running per-tile exponent on the pixel operand (error below the exact fp32
 * kernel's on the step's shapes); null = the kernel splits the fp32 weights into three bf16 planes in every block (six
 * products, ~25 % slower).  Build it once per weight version (the reference has no counterpart: cuDNN re-lays its filters out
 * internally).  Replaces nothing of the reference by itself: vlg_head.py:120-127's Conv2d weights. */
int64_t svl_conv3x3_weight_planes_bytes(int N, int Ct);
int svl_conv3x3_weight_planes(const float* w, int N, int Ct, void* planes, svl_stream_t stream);
/* scsh [imgs][2][C]: the per-(image, channel) affine form of GroupNorm, y = fma(x, scsh[img][0][c], scsh[img][1][c]), from
 * statistics [imgs, G, 2] -- the table the tiled convolutions apply (+ ReLU) to a pre-normalisation operand (gn_in). */
int svl_groupnorm_scale_shift(const float* stats, const float* gamma, const float* beta, int imgs, int C, int G, float* scsh,
                              svl_stream_t stream);
/* The apply pass of svl_groupnorm_fwd alone, on given statistics: bit-identical y.  Backward uses it to re-materialise a
 * normalised activation from the kept pre-normalisation tensor instead of keeping both (no reference counterpart: autograd
 * keeps every intermediate, vlg_head.py:84-137). */
int svl_groupnorm_apply(const float* x, int64_t ldx, const float* gamma, const float* beta, int imgs, int64_t HW, int C, int G,
                        int relu, const float* stats, float* y, int64_t ldy, svl_stream_t stream);
/* dy has pixel stride lddy.  ReLU mask: from y (post-activation, stride ldy) when given; with y == NULL it is
 * re-derived from x, stats, gamma and beta with the forward's own fma (bit for bit the sign the forward saw) -- one tensor
 * pass less in each of the two kernels.  beta is only read in that case.
 * chan_sums [imgs, 2, C] out: per image (sum_p dy', sum_p dy' * xhat); dbeta / dgamma are their column sums
 * over images (svl_colsum_f32 with ld = 2C). */
int svl_groupnorm_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* y, int64_t ldy,
                      const float* stats, const float* gamma, const float* beta, int imgs, int64_t HW, int C, int G,
                      int relu, float* dx, int64_t lddx, float* chan_sums, svl_stream_t stream);
/* Round 6: the GroupNorm-backward statistics from the epilogue of the kernel that PRODUCES dy.  svl_conv3x3_dgrad_gnb_f32 = the
 * input gradient of a narrow 3x3 convolution (dgrad pack w [N, 9 C1], mirrored taps; N = 32 / 64) whose result out [pix, N] is
 * the dy of a GroupNorm + ReLU over gnb_x [pix, N] (same pixel stride ldo; vlg_head.py:120-127: conv -> GN -> ReLU -> conv):
 * besides out it leaves chan_sums [imgs][2][N] = (sum dy', sum dy' xhat) per (image, channel) -- what svl_groupnorm_bwd's first
 * pass computes from a read of dy and x.  gnb_table = that GroupNorm's [imgs][2][N] (scale, shift) (svl_groupnorm_scale_shift),
 * gnb_stats its [imgs][N / 16][2] (mean, rstd); ws = svl_conv3x3_gnb_ws_doubles(...) doubles of scratch.  Returns
 * SVL_ERR_UNSUPPORTED without launching when the split tiled kernel does not take the shape or the arithmetic mode is not 6
 * (callers then run svl_gemm_f32 + svl_groupnorm_bwd).  svl_groupnorm_bwd_apply = svl_groupnorm_bwd's second pass on given sums. */
int64_t svl_conv3x3_gnb_ws_doubles(int imgs, int H, int W, int N);
int svl_conv3x3_dgrad_gnb_f32(const float* dy, int64_t lddy, int C1, const float* w, int imgs, int H, int W, int N, float* out,
                              int64_t ldo, int accumulate, const float* gnb_x, const float* gnb_table, const float* gnb_stats,
                              double* ws, float* chan_sums, const void* w_planes, svl_stream_t stream);
int svl_groupnorm_bwd_apply(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* stats, const float* gamma,
                            const float* beta, int imgs, int64_t HW, int C, int G, int relu, const float* chan_sums, float* dx,
                            int64_t lddx, svl_stream_t stream);


/* Fused (flash-style) multi-head self-attention of the ViT blocks, head dim 64, softmax scale 64^-0.5, fp32 MFMA
 * (or the bf16 x 6 split emulation with fp32 accumulation under svl_set_gemm_emulation(6): same error level vs fp64)
 * (nn.MultiheadAttention inside mmcv's wrapper, maskclip_vit.py:77-84,141).  qkv [B*T, 3E] = in-proj output
 * (q | k | v, E = 64*H); out [B*T, E]; lse [B*H*T] (log-sum-exp per query, saved for backward; may be NULL).
 * Backward: dqkv [B*T, 3E] fully written; dsum_ws is a [B*H*T] float workspace.  Deterministic.
 * Optional packed bf16x3 planes of the results (the A-operand format of svl_gemm_planes_f32, emulation mode 6 only --
 * SVL_ERR_UNSUPPORTED otherwise): out_planes = the attention output [B*T, E] (then `out` may be NULL: gradient-free
 * passes only feed it to the out-projection GEMM); dq_planes = dqkv [B*T, 3E] (in_proj's input-gradient operand).
 * planes_rows = the buffers' padded row count (svl_planes_rows(B*T)).  NULL = not wanted. */
int svl_attention_fwd(const float* qkv, int B, int T, int H, float* out, float* lse, void* out_planes,
                      int64_t planes_rows, svl_stream_t stream);
int svl_attention_bwd(const float* qkv, const float* out, const float* dout, const float* lse, int B, int T, int H,
                      float* dsum_ws, float* dqkv, void* dqkv_planes, int64_t planes_rows, svl_stream_t stream);
/* The same two operations on fp16 x 2 PRE-PACKED operands (round 5; csrc/attn_h2.hip): a pack pass writes the (image, head)
 * slices of q / k / v / dout as two fp16 planes with one power-of-two scale per slice, in the fragment layouts the MFMA
 * kernels read (LDS-DMA, no operand split inside the loops); three products h1 b0 + a0 h1' + a0 b0 per term on
 * v_mfma_f32_32x32x16_f16 with fp32 accumulation replace the six of the bf16 x 3 form -- error vs fp64 at the level of the
 * fp32 kernels' (tests/test_ops_gpu.py).  `ws` = caller-provided scratch of svl_attention_h2_ws_bytes(B, T, H, backward)
 * bytes, 1 KiB aligned, private to the call's stream until the call's work has finished.  Results, argument meaning and the
 * optional bf16 x 3 planes outputs as above (the planes outputs need no emulation mode here).  Match
 * maskclip_vit.py:77-84,141 (q pre-scaled by 64^-0.5 -- exact --, fp32 softmax).
 * Operand sets are ROW-MAJOR only (the kernels form the transposed fragments while reading LDS): with S = B H roundup(T, 64)
 * 256 bytes per set the workspace holds 3 sets forward (backward = 0: Q | K | V), 4 backward (backward = 1: + dO) and 1
 * (backward = 2: dO alone) for svl_attention_bwd_h2_sets, each plus a few KiB of exponents, norms and per-query pairs.
 * KEPT SETS: svl_attention_fwd_h2 leaves its workspace valid -- Q | K | V sets, exponents, norms, a pure function of qkv --
 * and svl_attention_bwd_h2_sets takes it as `sets` (sets_bytes >= the backward = 0 size; read only, 1 KiB aligned) together
 * with a backward = 2 workspace: it packs dout alone and launches the same grids as svl_attention_bwd_h2, whose results it
 * reproduces bit for bit when `sets` came from the forward of the same qkv (qkv itself is then not read).
 * svl_attention_h2_tr_sets(on): the A/B switch (also SVL_ATTN_TR_SETS=1 in the environment at first use).  on = 1 restores
 * the previous sequence -- transposed sets packed and read, 7 sets backward, svl_attention_bwd_h2_sets refused --, on = 0 the
 * default, on < 0 only queries; returns the value that held before.  Same bits either way; the workspace sizes follow it. */
int64_t svl_attention_h2_ws_bytes(int B, int T, int H, int backward);
int svl_attention_h2_tr_sets(int on);
int svl_attention_bwd_h2_sets(const float* qkv, const float* out, const float* dout, const float* lse, int B, int T, int H,
                              float* dsum_ws, float* dqkv, const void* sets, int64_t sets_bytes, void* ws, int64_t ws_bytes,
                              svl_stream_t stream);
int svl_attention_fwd_h2(const float* qkv, int B, int T, int H, float* out, float* lse, void* out_planes,
                         int64_t planes_rows, void* ws, int64_t ws_bytes, svl_stream_t stream);
int svl_attention_bwd_h2(const float* qkv, const float* out, const float* dout, const float* lse, int B, int T, int H,
                         float* dsum_ws, float* dqkv, void* dqkv_planes, int64_t planes_rows, void* ws, int64_t ws_bytes,
                         svl_stream_t stream);

/* Small-sequence multi-head attention for the SemanticTransformer (vlg_head.py:39-67; seq = num classes).
 * qkv rows: token (g, s) at row  (g / inner) * outer_stride + (g % inner) * inner_stride + s * seq_stride,
 * each row = [q(E) | k(E) | v(E)], E = heads*D, D = 64. out has the same row mapping, width E. */
typedef struct svl_seqattn_desc {
  int groups, inner, seq, heads;
  int64_t outer_stride, inner_stride, seq_stride; /* in rows */
  const float* qkv;  /* [rows, 3E] */
  float* out;        /* [rows, E] */
  float* probs;      /* [groups, heads, seq, seq] saved for backward */
  /* backward */
  const float* dout; /* [rows, E] */
  float* dqkv;       /* [rows, 3E] */
  float* dscores;    /* workspace [groups, heads, seq, seq] */
} svl_seqattn_desc;
int svl_seqattn_fwd(const svl_seqattn_desc* d, svl_stream_t stream);
int svl_seqattn_bwd(const svl_seqattn_desc* d, svl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Thin (HBM-bound) convolutions of the VLG head, NHWC, stride 1, same size.
 * ---------------------------------------------------------------------------------------------- */
/* Conv2d(C -> 1): y[pix] = bias[0] + sum_{tap,ci} x[pix + off(tap)][ci] * w[tap*C + ci]  (vlg_head.py:190,239; w is the
 * forward pack [1, KH*KW*C]). */
/* gn_in (NULL or the [imgs][2][C] table of svl_groupnorm_scale_shift; both entry points): x is the PRE-normalisation output
 * of the last Up convolution and relu(fma(x, scale, shift)) = GroupNorm + ReLU (vlg_head.py:126-127) is formed on the way
 * in -- the forward through an LDS-tiled kernel (3x3, pad 1, C = 16 / 32 / 64: one HBM read per input element). */
int svl_conv_cout1_fwd(const float* x, int64_t ldx, int imgs, int H, int W, int C, int KH, int KW, int dil, int pad,
                       const float* w, const float* bias, const float* gn_in, float* y, svl_stream_t stream);
/* Weight gradient of Conv2d(C -> 1, 3x3): per-block partial sums slabs[nblocks][9*C] (nblocks =
 * svl_conv_cout1_wgrad_blocks); combine with svl_reduce_slabs_f32. */
int svl_conv_cout1_wgrad_blocks(int imgs, int H, int W);
int svl_conv_cout1_wgrad(const float* dy, const float* x, int64_t ldx, int imgs, int H, int W, int C, int dil, int pad,
                         const float* gn_in, float* slabs, svl_stream_t stream);
/* out[p] = sum_tap T[p - sign*off(tap)][tap] with T [pix, KH*KW]: the shifted-tap sum that completes a Cin=1 input
 * gradient (conv1 7x7, vlg_head.py:169,221) after the GEMM T = dY . W. */
int svl_tap_gather(const float* T, int imgs, int H, int W, int KH, int KW, int dil, int pad, int sign, float* out,
                   svl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Resampling on NHWC / NCHW maps.
 * ---------------------------------------------------------------------------------------------- */
/* Bilinear resize, channels-last: x [imgs, h, w, C] (pixel stride ldx) -> y [imgs*rep, H, W, :] written at channel
 * offset 0 with pixel stride ldy; output image i reads input image i / rep (`repeat`, vlg_head.py:133).
 * accumulate: y += . */
int svl_bilinear_nhwc_fwd(const float* x, int64_t ldx, int imgs, int h, int w, int C, int align_corners, int rep,
                          int H, int W, float* y, int64_t ldy, int accumulate, svl_stream_t stream);
/* dx[imgs,h,w,C] (=|+=) sum over rep and taps of dy. Deterministic gather form. */
/* out[g][row][c] = sum_{r < rep} src[g * rep + r][row][c]  (src rows `ld` apart, out packed [groups][rows][C]): the
 * class-repeated skip gradient of vlg_head.py:131-135 summed over its classes before the bilinear backward. */
int svl_sum_rep_f32(const float* src, int64_t ld, int64_t groups, int rep, int64_t rows, int C, float* out,
                    svl_stream_t stream);
int svl_bilinear_nhwc_bwd(const float* dy, int64_t lddy, int imgs, int h, int w, int C, int align_corners, int rep,
                          int H, int W, float* dx, int64_t lddx, int accumulate, svl_stream_t stream);
/* Bilinear resize of planes: x [planes, h, w] -> y [planes, H, W] (NCHW logits, vlg_head.py:247, builder.py:93-97). */
int svl_bilinear_planes_fwd(const float* x, int64_t planes, int h, int w, int align_corners, int H, int W, float* y,
                            svl_stream_t stream);
int svl_bilinear_planes_bwd(const float* dy, int64_t planes, int h, int w, int align_corners, int H, int W,
                            float* dx, svl_stream_t stream);
/* AvgPool PH x PW (floor) on NHWC + concat of a per-class text vector: x [imgs, H, W, C] ->
 * y [imgs, H/PH, W/PW, C + Ct], y[..., C:] = text[(img % nclass), :] (vlg_head.py:43-53; PH = H, PW = W is the global
 * average pool of ASPPPooling, vlg_head.py:70-81, on any map shape). text may be NULL (Ct=0). */
int svl_avgpool_cat_fwd(const float* x, int imgs, int H, int W, int C, int PH, int PW, const float* text, int Ct,
                        int nclass, float* y, svl_stream_t stream);
/* dx [imgs,H,W,C] (=|+=) avgpool backward of dy[..., :C] (ld = C+Ct); pixels outside the floor region get 0 (accumulate:
 * the pooled gradient is ADDED to dx -- the residual sum of SemanticTransformer / ASPP pooling without an extra pass). */
int svl_avgpool_cat_bwd(const float* dy, int imgs, int H, int W, int C, int PH, int PW, int Ct, float* dx,
                        int accumulate, svl_stream_t stream);
/* dtext [nclass, Ct] = sum over images of class n (img % nclass == n) and pooled pixels of dy[..., C + ct]; part: imgs * Ct
 * floats of scratch (per-image partial sums, added up per class in image order). */
int svl_avgpool_cat_bwd_text(const float* dy, int imgs, int64_t HWp, int C, int Ct, int nclass, float* part, float* dtext,
                             svl_stream_t stream);

/* Test-time augmentation of the evaluator (mmseg 0.x MultiScaleFlipAug + EncoderDecoder.aug_test; csrc/tta.hip).
 * A view of the image: src [planes, h, w] -> dst [planes, oh, ow], bilinear with ATen's upsample_bilinear2d arithmetic,
 * align_corners = False (one fp32 scale per axis, area_pixel_compute_source_index, guard_index_and_lambda, as
 * svl_bilinear_planes_fwd); flip != 0 mirrors the columns: dst[p, y, x] = resized[p, y, ow - 1 - x], the unflipped
 * formula evaluated at column ow - 1 - x.  oh == h && ow == w moves the elements: a bit-exact copy, with flip a bit-exact
 * mirror. */
int svl_tta_view_f32(const float* src, int64_t planes, int h, int w, int oh, int ow, int flip, float* dst,
                     svl_stream_t stream);
/* The class scores of one view, formed at the target resolution and added to the running mean in one pass:
 * src [B, N, h, w], dst [B, N, H, W].  For every destination pixel (b, y, x): xs = flip ? W - 1 - x : x, u_c = the bilinear
 * value (arithmetic as above, align_corners as given) of plane c of src at destination index (y, xs);
 *   kind 0 (logits):                       s_c = softmax_c(u)  (the maximum is subtracted first)
 *   kind 1 (summed window probabilities):  s_c = u_c / sum_k u_k, and s_c = 0 for every c where that total is 0
 *   dst[b, c, y, x] = (accumulate ? dst[b, c, y, x] : 0) + scale * s_c.
 * One owner per destination element, no atomics: two runs agree bit for bit.  dst is read at most once (not at all
 * with accumulate == 0) and written once per element; consecutive lanes own consecutive x (16-byte stores when W % 4 == 0
 * and dst is 16-byte aligned, scalar stores otherwise).  Any N >= 1.  kind outside {0, 1}: status -1. */
int svl_tta_accum_f32(const float* src, int B, int N, int h, int w, float* dst, int H, int W, int kind,
                      int align_corners, int flip, float scale, int accumulate, svl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Optimiser (semivl.py:123-125,328,339-345: torch AdamW, one param group per tensor, poly LR).
 * Flat arena of `nseg` segments; seg_* arrays are DEVICE arrays of length nseg.
 * p,g,m,v are flat fp32 arenas; segment s covers [seg_off[s], seg_off[s+1]).
 * Update (torch.optim.AdamW, amsgrad=False):  p *= 1 - lr*wd; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
 *   p -= lr / (1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps).  gscale multiplies g first (1/world_size).
 * If ema != NULL: ema = ema_decay*ema + (1-ema_decay)*p_new (extension).
 * ---------------------------------------------------------------------------------------------- */
int svl_adamw_step(float* p, const float* g, float* m, float* v, const int64_t* seg_off, const float* seg_lr,
                   const float* seg_wd, int nseg, int64_t total, float beta1, float beta2, float eps, int step,
                   float gscale, float* ema, float ema_decay, svl_stream_t stream);
/* torch.optim.SGD (maximize=False) on the same arena: the optimizer of semivl.py:118-121 (cfg without an 'optimizer' key:
 * SGD([backbone @ lr, every parameter whose name lacks 'backbone' @ lr * lr_multi], momentum=0.9, weight_decay=1e-4)), whose
 * two learning rates the host re-schedules into seg_lr after every step (semivl.py:330-337).  Per element, in this order:
 *   d = g * gscale + wd * p;
 *   if momentum != 0:  m = d when step == 1 (torch clones the gradient), else m = momentum * m + (1 - dampening) * d;
 *                      d = d + momentum * m if nesterov, else d = m;
 *   p -= lr * d;   if ema != NULL: ema = ema_decay * ema + (1 - ema_decay) * p.
 * m may be NULL only when momentum == 0; nesterov with momentum <= 0 or dampening != 0 is SVL_ERR_INVALID_ARG (torch raises).
 * p, g, m, ema 16-byte aligned and every seg_off[s] a multiple of 4 (FusedAdamW's / FusedSGD's arenas): the kernel moves
 * one float4 per lane and array, 20 B per parameter (28 with ema).  Padding between segments (p = g = m = 0) stays 0. */
int svl_sgd_step(float* p, const float* g, float* m, const int64_t* seg_off, const float* seg_lr, const float* seg_wd,
                 int nseg, int64_t total, float momentum, float dampening, int nesterov, int step, float gscale,
                 float* ema, float ema_decay, svl_stream_t stream);
/* The same two steps with the gradient scale read from the DEVICE: gscale_dev points to one fp32 value (stats + 2 of
 * svl_grad_clip_f32), read by the kernel when it runs -- nothing about it is known to the host.  Every other argument, check
 * and rule as above; the kernels are further instantiations of the same templates and do the same arithmetic after the read:
 * for the same scale value both forms produce the same bits in p, m, v and ema. */
int svl_adamw_step_dscale(float* p, const float* g, float* m, float* v, const int64_t* seg_off, const float* seg_lr,
                          const float* seg_wd, int nseg, int64_t total, float beta1, float beta2, float eps, int step,
                          const float* gscale_dev, float* ema, float ema_decay, svl_stream_t stream);
int svl_sgd_step_dscale(float* p, const float* g, float* m, const int64_t* seg_off, const float* seg_lr,
                        const float* seg_wd, int nseg, int64_t total, float momentum, float dampening, int nesterov,
                        int step, const float* gscale_dev, float* ema, float ema_decay, svl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Gradient-norm clipping over the gradient arena: torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type) over all
 * tensors of the arena at once (its padding is zero, so the arena's norm is the norm over the tensors).  Replaces NOTHING of
 * the reference: semivl.py does not clip; this is what mmcv's OptimizerHook(grad_clip=dict(max_norm, norm_type)) calls.
 *   norm_kind 0: L2, norm = gscale * sqrt(sum_i g_i^2);   norm_kind 1: max norm, norm = gscale * max_i |g_i|
 *   coef = min(max_norm / (norm + 1e-6), 1);   stats = {norm, coef, gscale * coef, 1.0 if norm is not finite else 0.0}
 * stats[2] is the scale a step applies to g (svl_adamw_step_dscale / svl_sgd_step_dscale): the clip never rewrites g.
 * Rounding and order: stage 1 is one launch that reads g once (16-byte loads when g is 16-byte aligned, 4-byte loads
 * otherwise and for the last total % 4 elements); a lane adds its g_i^2 in double (fma, one chain per position in its group
 * of four) or keeps its largest |g_i| and a NaN flag (fmax alone would lose a NaN); lanes fold by cross-lane shuffles, waves
 * through LDS, and every block writes ONE double into ws.  Which lane and block reads which element depends on `total` alone:
 * not on the alignment of g, not on its values.  Stage 2 is a second launch of one block that folds the partials in a fixed
 * order and forms norm, coef and gscale * coef in double, each rounded to fp32 ONCE.  No atomics and no combination across
 * workgroups inside a launch: two calls on the same g give the same bits.
 * Non-finite gradients as in torch (error_if_nonfinite=False): the norm is inf or NaN, coef = max_norm / inf = 0 or NaN,
 * stats[3] = 1 and nothing is skipped.  max_norm = +inf needs no special case: coef = 1, the call only reports the norm.
 * gscale (the 1 / world_size of the data-parallel mean, applied to the norm as it is to the step) must be positive and
 * finite, max_norm positive: anything else, a null pointer or total <= 0 is SVL_ERR_INVALID_ARG.
 * ws: svl_grad_clip_ws_doubles(total) doubles of device memory (host-only query; at most 1024), caller-owned, no
 * initialisation; exactly that many are written.  stats: 4 floats. */
int64_t svl_grad_clip_ws_doubles(int64_t total);
int svl_grad_clip_f32(const float* g, int64_t total, int norm_kind, float gscale, float max_norm, double* ws,
                      float* stats /* [4] */, svl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Moving average over a table of independent segments: the mean teacher's BatchNorm running statistics against the
 * student's (semivl_amd/ema.py; the parameters' average is the `ema` arena of the step entries above, not this).
 *   dst[s][i] = decay * dst[s][i] + (1 - decay) * src[s][i]     for i < seg_off[s + 1] - seg_off[s],  s < nseg
 * dst, src: DEVICE arrays of nseg pointers; seg_off: DEVICE array of nseg + 1 offsets (only the differences are used).
 * decay in [0, 1]; 1 - decay is formed on the host as (float)(1.0 - (double)decay), like the SGD step's ema factor, and
 * the expression is evaluated in fp32 as fma(decay, dst, fl((1 - decay) * src)): two roundings, the same on every path.
 * ONE launch: one block per segment, the grid capped at 256 blocks (further segments take further trips); one owner per
 * element, no atomics, no host sync: two calls on the same data give the same bits.  A segment whose two pointers are
 * 16-byte aligned moves 16 bytes per lane (its last length % 4 elements singly), any other segment 4 bytes per lane; the
 * arithmetic per element is the same, so both give the same bits.  decay == 0 copies src.
 * The tables live on the device, so the entry cannot compare the pointers they hold: segments must not overlap, and
 * dst[s] != src[s] for every s is the business of whoever builds the tables (ops.ema_segment_tables refuses it by this
 * entry's name); passing the SAME table as dst and src is refused here.  nseg == 0 returns SVL_OK without a launch; a
 * negative nseg, a null table or a decay outside [0, 1] is SVL_ERR_INVALID_ARG. */
int svl_ema_segments_f32(float* const* dst, const float* const* src, const int64_t* seg_off /* [nseg + 1] */, int nseg,
                         float decay, svl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * BatchNorm2d (batch statistics, SyncBN-ready) and MaxPool2d(3, 2, 1) on channels-last [rows, C] activations: the ops of
 * the Cityscapes recipe's convolutional side encoder (`conv_encoder` = mmseg ResNetV1c deep stem + layer1 with
 * norm_cfg SyncBN; reference model/vlm.py:50-53,120-121, configs/_base_/models/vlm-vlg-aspp-s2p4-skr04-ftap-mcvitb.py:50-60).
 * Replaces torch.nn.SyncBatchNorm forward/backward (sum / sum-of-squares and sum dy / sum dy*xhat are produced as ONE
 * [2][C] double vector each, which is what the data-parallel ranks all-reduce) and F.max_pool2d + its backward.
 * C % 4 == 0, 16-byte aligned rows. */
int64_t svl_bn_ws_doubles(int64_t rows, int C);
/* sums[0][c] = sum_r x, sums[1][c] = sum_r x^2 */
int svl_bn_stats(const float* x, int64_t ldx, int64_t rows, int C, double* sums, double* ws, svl_stream_t stream);
/* mean, invstd from (all-reduced) sums over `count` rows; running stats updated like torch (unbiased variance) if given */
int svl_bn_finalize(const double* sums, double count, float eps, float momentum, float* running_mean, float* running_var,
                    int C, float* mean, float* invstd, svl_stream_t stream);
int svl_bn_eval_invstd(const float* running_var, float eps, int C, float* invstd, svl_stream_t stream);
/* y = [relu]((x - mean) * invstd * gamma + beta [+ resid]) */
int svl_bn_apply(const float* x, int64_t ldx, int64_t rows, int C, const float* mean, const float* invstd,
                 const float* gamma, const float* beta, const float* resid, int64_t ldr, int relu, float* y, int64_t ldy,
                 svl_stream_t stream);
/* sums[0][c] = sum dy', sums[1][c] = sum dy' * xhat, dy' = dy masked by the fused ReLU: y > 0 when y is given; with
 * y == NULL and remask_gamma / remask_beta given, the forward's own output expression re-evaluated from x (bit-identical
 * sign; BatchNorm + ReLU WITHOUT a residual input only) -- one tensor pass less; all three NULL = no ReLU. */
int svl_bn_bwd_reduce(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* y, int64_t ldy,
                      const float* mean, const float* invstd, const float* remask_gamma, const float* remask_beta,
                      int64_t rows, int C, double* sums, double* ws, svl_stream_t stream);
/* dx = gamma * invstd * (dy' - sums0/count - xhat * sums1/count); dres (optional) = dy' for the residual branch;
 * dgamma = sums1, dbeta = sums0 (of this rank's rows, i.e. BEFORE the all-reduce) */
int svl_bn_bwd_apply(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* y, int64_t ldy,
                     const float* mean, const float* invstd, const float* gamma, const float* remask_beta,
                     const double* sums, double count, int64_t rows, int C, float* dx, int64_t lddx, float* dres,
                     int64_t lddr, svl_stream_t stream);
/* NHWC max pooling, kernel 3, stride 2, padding 1 (Ho = (H-1)/2+1); idx = winning tap 0..8 per output element */
int svl_maxpool3x3s2_fwd(const float* x, int imgs, int H, int W, int C, float* y, unsigned char* idx,
                         svl_stream_t stream);
int svl_maxpool3x3s2_bwd(const float* dy, const unsigned char* idx, int imgs, int H, int W, int C, float* dx,
                         svl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Global average pooling over the pixels of each image of a channels-last token slab, and the broadcast of one row per
 * image back over its pixels: the image-pooling branch of the DeepLabV3+ ASPP (reference
 * third_party/unimatch/model/semseg/deeplabv3plus.py:84-95 -- the bilinear resize of a 1 x 1 map is a broadcast -- and the
 * channel concat of :119-126 for that branch).  Rows are `ld*` floats apart; 16-byte accesses when C % 4 == 0, the strides
 * are multiples of 4 and the pointers are 16-byte aligned, scalar otherwise.  Sums run in double in a fixed order
 * (deterministic, no atomics) and are rounded once. */
/* pool[img * ldp + c] = (1 / HW) * sum_{p < HW} x[(img * HW + p) * ldx + c] */
int svl_gap_tokens_fwd(const float* x, int64_t ldx, int imgs, int64_t HW, int C, float* pool, int64_t ldp,
                       svl_stream_t stream);
/* dx[(img * HW + p) * lddx + c] (=|+=) dpool[img * ldp + c] / HW   (accumulate: +=) */
int svl_gap_tokens_bwd(const float* dpool, int64_t ldp, int imgs, int64_t HW, int C, float* dx, int64_t lddx,
                       int accumulate, svl_stream_t stream);
/* dst[(img * HW + p) * ldd + c_off + c] = v[img * ldv + c]: the concat of a per-image row into a channel slice of a wider slab */
int svl_bcast_rows_fwd(const float* v, int64_t ldv, int imgs, int64_t HW, int C, float* dst, int64_t ldd, int c_off,
                       svl_stream_t stream);
/* dv[img * ldv + c] = sum_{p < HW} dy[(img * HW + p) * lddy + c_off + c] */
int svl_bcast_rows_bwd(const float* dy, int64_t lddy, int c_off, int imgs, int64_t HW, int C, float* dv, int64_t ldv,
                       svl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * GPU-side input pipeline: the reference loader's per-sample PIL chain
 * (third_party/unimatch/dataset/semi.py:61-127, transform.py:9-84) on uint8 HWC device images.  Statistical parity
 * (the random streams differ); the deterministic arithmetic follows Pillow.
 *   svl_aug_resample_u8   resize to rh x rw -- mode 0 / 1: Pillow BILINEAR (antialiased) / NEAREST (transform.py:43-57, the
 *                         img_scale=None branch); mode 2 / 3: OpenCV INTER_LINEAR / INTER_NEAREST semantics (mmseg `Resize`
 *                         = mmcv.imrescale, semi.py:53-71: the img_scale branch and the val transform; mmcv/cv2 are
 *                         un-vendored -> parity unpinned, +-1 level vs cv2's fixed-point arithmetic) -- then pad
 *                         right/bottom with `fill` (transform.py:9-14), crop OH x OW at (x0, y0) (:16-20), hflip (:25-29)
 *   svl_aug_to_float      ToTensor + Normalize (transform.py:32-40) -> float CHW; mean3/std3 are HOST pointers
 *   svl_aug_mask_i64      uint8 mask -> int64 with one value remapped (semi.py:122-123: 254 -> 255 / ignore_mask)
 *   svl_aug_photometric_u8  in place: 0 brightness, 1 contrast, 2 saturation (ImageEnhance blends, semi.py:99-100 via
 *                         torchvision ColorJitter), 3 hue shift, 4 grayscale (semi.py:101); scratch = 1 device uint64
 *   svl_aug_gaussian_blur_u8  transform.py:60-64 (true separable Gaussian; Pillow approximates it with box filters) */
int svl_aug_resample_u8(const unsigned char* src, int H, int W, int C, int rh, int rw, int x0, int y0, int OH, int OW,
                        int flip, int mode, int fill, unsigned char* dst, svl_stream_t stream);
int svl_aug_to_float(const unsigned char* src, int npix, const float* mean3, const float* std3, float* dst,
                     svl_stream_t stream);
int svl_aug_mask_i64(const unsigned char* src, int npix, int from, int to, int64_t* dst, svl_stream_t stream);
int svl_aug_photometric_u8(unsigned char* img, int npix, int op, float factor, unsigned long long* scratch,
                           svl_stream_t stream);
int svl_aug_gaussian_blur_u8(const unsigned char* src, int H, int W, float sigma, unsigned char* tmp, unsigned char* dst,
                             svl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * LoRA adapters of the CLIP ViT as merged weights (model/backbone/lora.py; maskclip_vit.py:85-88,123-137).  With
 * lora_dropout == 0, F.linear(x, W) + s * b(a(x)) == F.linear(x, W + s * B @ A) for A = a.weight [r, E], B = b.weight
 * [rows, r]: a LoRA block runs the ordinary kernels on the effective weight.  fp32 throughout; 1 <= r <= 64, E % 4 == 0,
 * every E-wide matrix 16-byte aligned with a leading dimension % 4 == 0; anything else (or a null pointer) is
 * SVL_ERR_INVALID_ARG and nothing is written.  No atomics: results are bitwise reproducible.
 *   svl_lora_merge_f32   row block i < nblk (<= 3) of W / Weff is rows [i * rows, (i + 1) * rows):
 *                        Weff[i] = W[i] + s * B[i] @ A[i].  A, B: HOST arrays of nblk device pointers; a block with
 *                        A[i] == B[i] == NULL is a plain copy (the k rows of in_proj under lora_targets='qv').
 *                        One read of W, one write of Weff.
 *   svl_lora_wgrad_f32   from one dW [rows, E] block: dB [rows, r] (+)= s * dW @ A^T and dA [r, E] (+)= s * B^T @ dW, one
 *                        read of dW for both.  dB: one fp32 chain over E per element.  dA: a 16-row fp32 chain per row tile
 *                        into ws (svl_lora_wgrad_ws_floats(rows, E, r) floats), then the tiles in order in double
 *                        (svl_reduce_slabs_f32, launched here).  Each result has its own accumulate flag. */
int svl_lora_merge_f32(const float* W, int64_t ldw, float* Weff, int64_t ldo, int nblk, int rows, int E, int r, float s,
                       const float* const* A, const float* const* B, int64_t ldb, svl_stream_t stream);
int64_t svl_lora_wgrad_ws_floats(int rows, int E, int r);
int svl_lora_wgrad_f32(const float* dW, int64_t lddw, const float* A, const float* B, int64_t ldb, int rows, int E, int r,
                       float s, float* dB, int accumulate_b, float* dA, int accumulate_a, float* ws, svl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Deep visual prompt tokens of the CLIP ViT (maskclip_vit.py:359-368,510-536).  With num_prompt_tokens = P every block
 * runs on [class token | P prompt rows | patch tokens] = T + P rows per image; the prompt rows are written before the block
 * and dropped after it.  fp32, row-major [B, rows, E] matrices without padding.  mask [B, P, E] of 0 / 1 floats, or NULL (no
 * dropout: scale is ignored).  16-byte accesses when E % 4 == 0 and every pointer is 16-byte aligned, scalar otherwise.  A
 * null required pointer or a non-positive size is SVL_ERR_INVALID_ARG and nothing is written.  No atomics: results are
 * bitwise reproducible.
 *   svl_prompt_rows_fwd_f32  expand (src [B, T, E] != NULL): dst [B, T + P, E] with dst[b, 0] = src[b, 0],
 *                            dst[b, 1 + j] = emb[j] * (mask[b, j] * scale), dst[b, 1 + P + t] = src[b, 1 + t]; one read of
 *                            src, one write of dst.  in place (src == NULL): only the B * P prompt rows of dst are written;
 *                            the other rows are neither read nor written.  emb [P, E].
 *   svl_prompt_rows_bwd_f32  dx [B, T + P, E].  demb [P, E] (may be NULL: no sum): demb[j, e] (+)= sum_b dx[b, 1 + j, e] *
 *                            (mask[b, j, e] * scale), one thread per element, b ascending, every product and sum rounded
 *                            once.  zero (dx_out == NULL): rows 1 .. P of dx are then set to zero in place.  compact
 *                            (dx_out [B, T, E] != NULL): dx without its prompt rows is written to dx_out; dx is only read. */
int svl_prompt_rows_fwd_f32(const float* src, float* dst, const float* emb, const float* mask, float scale, int B, int T,
                            int P, int E, svl_stream_t stream);
int svl_prompt_rows_bwd_f32(float* dx, float* dx_out, float* demb, const float* mask, float scale, int accumulate, int B,
                            int T, int P, int E, svl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Stochastic depth (drop-path) of the CLIP ViT's residual branches (maskclip_vit.py:120-144).  One draw per sample scales
 * the T rows of that sample: s_b = mask[b] * scale (mask [B] floats, scale = 1 / keep).  fp32, row-major [B * T, E] matrices
 * without padding; the sample of a row is row / T.  16-byte accesses when E % 4 == 0 and the matrix pointers are 16-byte
 * aligned, scalar otherwise.  A null pointer or a non-positive size is SVL_ERR_INVALID_ARG and nothing is written.  No
 * atomics: results are bitwise reproducible.
 *   svl_droppath_fwd_f32  out = resid + s_b * branch (the product and the sum rounded once each).  out may be branch (not
 *                         resid).  Rows of a dropped sample (mask[b] == 0) are copied from resid; branch is not read there.
 *   svl_droppath_bwd_f32  dbranch = s_b * dout (dbranch may be dout).  Rows of a dropped sample are written as zeros; dout
 *                         is not read there. */
int svl_droppath_fwd_f32(const float* branch, const float* resid, const float* mask, float scale, float* out, int B, int T,
                         int E, svl_stream_t stream);
int svl_droppath_bwd_f32(const float* dout, const float* mask, float scale, float* dbranch, int B, int T, int E,
                         svl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * CLIP text tower (third_party/zegclip/models/backbones/text_encoder.py:79-87): the forward-only pieces beside the GEMMs,
 * svl_layernorm_fwd and svl_l2norm_fwd.  fp32, row-major matrices without padding.  A null pointer or a size outside its
 * range is SVL_ERR_INVALID_ARG, named in svl_last_error(), and nothing is written.  No atomics: results are bitwise
 * reproducible.
 *   svl_text_embed_f32       tokens int64 [n, L], table [V, W], pos [L, W] -> x [n * L, W] with x[(i, t)] = table[tok[i, t]] +
 *                            pos[t] (one fp32 addition) and eot int32 [n] = index of the first maximum of tok[i, :]
 *                            (torch.argmax).  A token outside [0, V) is never dereferenced: its row of x is NaN.  16-byte
 *                            accesses when W % 4 == 0 and table, pos and x are 16-byte aligned.
 *   svl_causal_attn_fwd_f32  qkv [n * L, 3 W] laid out q | k | v with W = 64 H (head dim 64, scale 64^-0.5), 1 <= L <= 192
 *                            -> out [n * L, W].  Query t attends keys 0 .. t of its own sequence: the -inf upper triangle
 *                            of CLIPTextEncoder.build_attention_mask.  Keys above t are not read for row t (no score, no
 *                            exponential, no value term), so row t does not depend on them in any bit.  No probabilities are
 *                            written.
 *   svl_quickgelu_f32        y = x * sigmoid(1.702 x) on `count` elements; y may be x.  16-byte accesses when both pointers
 *                            are 16-byte aligned (scalar for the last count % 4 elements), scalar otherwise.
 *   svl_gather_rows_f32      out[i, :] = x[i * L + idx[i], :] for x [n * L, E], idx int32 [n].  An index outside [0, L) is
 *                            never dereferenced: its row of out is NaN.
 *   svl_segment_mean_f32     x [m, E], offsets int32 [N + 1] on the device (prefix offsets, offsets[0] = 0, offsets[N] = m)
 *                            -> out [N, E]: the rows offsets[c] .. offsets[c + 1] - 1 added in ascending order, then divided
 *                            by their count; a segment of one row is a copy.  N > m (some segment must be empty) is refused;
 *                            rows outside [0, m) are never read and an empty segment yields NaN (callers check the table on
 *                            the host). */
int svl_text_embed_f32(const int64_t* tokens, const float* table, const float* pos, int n, int L, int V, int W, float* x,
                       int* eot, svl_stream_t stream);
int svl_causal_attn_fwd_f32(const float* qkv, int n, int L, int H, float* out, svl_stream_t stream);
int svl_quickgelu_f32(const float* x, float* y, int64_t count, svl_stream_t stream);
int svl_gather_rows_f32(const float* x, const int* idx, int n, int L, int E, float* out, svl_stream_t stream);
int svl_segment_mean_f32(const float* x, int64_t m, int E, const int* offsets, int N, float* out, svl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * MaskCLIP's training-free refinements of a dense zero-shot prediction (maskclip_head.py:129-155), the passes around the two
 * svl_gemm_f32 products of key smoothing.  x [B * HW, N] are cosine logits (token rows, leading dimension ldx), k [B * HW, E]
 * the last block's keys.  With P = softmax(100 x') over the classes, x' = x with every class c of image b whose peak
 * max_i softmax(100 x)[b, i, c] is < pd_thresh set to -100, the smoothed rows are O = k^ (k^^T P) per image, k^ = k scaled per
 * CHANNEL over the HW tokens of its image (F.normalize's default dim = 1 on [B, HW, E]); W = k^ k^^T is never formed.
 * fp32; 16-byte accesses where the pointers and strides allow them, scalar otherwise; grids are capped and walked
 * grid-stride.  A null pointer, B, HW, N or E < 1, a leading dimension below the width or a negative threshold is
 * SVL_ERR_INVALID_ARG, named in svl_last_error(), and nothing is written.  No atomics: two runs agree bit for bit.
 *   svl_mc_class_peak_f32  peak[b, c] = max_i P[b * HW + i, c] for P [B * HW, N] with leading dimension ld.  A NaN in a
 *                          column gives NaN (torch.max): NaN < pd_thresh is false, so such a class is kept.  The rows of a
 *                          column are folded in one fixed order.
 *   svl_col_invsq_f32      s[b, c] = 1 / max(sqrt(sum_i k[b * HW + i, c]^2), eps)^2: the squares are accumulated in double, in
 *                          one fixed order per column, and the quotient is rounded to fp32 once.
 *   svl_mc_softmax_f32     P[r, :] = softmax(100 x'[r, :]) as exp(z - max z) / sum exp(z - max z), z = 100 x', and
 *                          rowmax[r] = max_c P[r, c] (NaN if the row holds one; rowmax may be null).  peak null: nothing is
 *                          dropped (x' = x).  fill_only != 0: P receives x' itself (x, or exactly -100.0), rowmax must be null.
 *   svl_mc_select_f32      out[b, c, i] = rowmax[b * HW + i] < ks_thresh ? O[b * HW + i, c] : P[b * HW + i, c], written straight
 *                          into the class-planes layout [B, N, HW] (svl_bilinear_planes_fwd, svl_maskclip_labels).  A NaN
 *                          rowmax keeps P.  O and rowmax both null: the transpose of P alone, bit for bit. */
int svl_mc_class_peak_f32(const float* P, int64_t ld, int B, int HW, int N, float* peak, svl_stream_t stream);
int svl_col_invsq_f32(const float* k, int64_t ld, int B, int HW, int E, float eps, float* s, svl_stream_t stream);
int svl_mc_softmax_f32(const float* x, int64_t ldx, const float* peak, float pd_thresh, int B, int HW, int N, int fill_only,
                       float* P, int64_t ldp, float* rowmax, svl_stream_t stream);
int svl_mc_select_f32(const float* P, int64_t ldp, const float* O, int64_t ldo, const float* rowmax, float ks_thresh, int B,
                      int HW, int N, float* out, svl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SEMIVL_HIP_H_ */
