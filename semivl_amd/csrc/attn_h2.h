// Launchers of the fp16 x 2 fused attention (attn_h2.hip), called by the C-ABI entry points in attention.hip.
#pragma once
#include "attn_shared.h"

namespace svl_attn_h2 {

// The tr switch (SVL_ATTN_TR_SETS in the environment, or set here): 1 = the operand sets of rounds 5-7 (transposed sets packed
// and read, no kept sets).  on >= 0 sets it; returns the value that held before.  An entry point takes it ONCE and hands it to
// every launcher below as `tr`.
int tr_sets(int on);
// bytes of the operand workspace: the packed (z = image x head)-major fp16 x 2 operand sets + scale exponents
// (+ the per-query (14 - LSE log2 e, D 2^-g) pairs of the backward).  mode 0 = forward, 1 = backward, 2 = backward on kept sets.
long ws_bytes(int B, int T, int H, int mode, int tr);
// fwd_pack: the pack pass (Q, K, V row-major; tr: V transposed); fwd: the MFMA grid over `nb` blocks of 256 queries per (image,
// head).  The workspace stays valid after the call: with tr = 0 it is what bwd_prepare takes as `sets`.
int fwd(const AttnP& p, int nb, void* ws, long wsb, int tr, hipStream_t st);
// pack pass (Q, K, V, dO row-major -- `sets` given: dO alone, Q / K / V read from the forward's workspace; tr: also Q, K, dO
// transposed) + D = rowsum(dO * O) (also written to dsum_ws for the leftover-row kernels); then the two MFMA grids
int bwd_prepare(const AttnP& p, const float* out, float* dsum_ws, void* ws, long wsb, const void* sets, long setsb, int tr,
                hipStream_t st);
int bwd_main(const AttnP& p, int nb, void* ws, const void* sets, int tr, hipStream_t st);
// the rows past the last full 256-row block (at most 4, from row0) as four-wave MFMA workgroups on the packed operands; they
// read what the pack pass / bwd_prepare wrote: launch them on a stream ordered AFTER those (the helper stream forked behind)
int fwd_pack(const AttnP& p, void* ws, long wsb, int tr, hipStream_t st);
int fwd_tail(const AttnP& p, int row0, void* ws, int tr, hipStream_t aux);
int bwd_tail(const AttnP& p, int row0, void* ws, const void* sets, int tr, hipStream_t aux);

}  // namespace svl_attn_h2
