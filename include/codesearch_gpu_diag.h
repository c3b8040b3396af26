/*
 * codesearch_gpu_diag.h — operator-level diagnostics of libcsgpu, exported ONLY by codesearch_amd/libcsgpu_diag.so (the
 * product library built once more with -DCS_DIAGNOSTICS: it additionally holds csrc/diagnostics.hip, the ablation
 * instantiations of the wide GEMM kernel and its in-kernel clock stamps).  Used by tests/test_gpu_gemm_split.py, tests/test_gpu_gemm_wide.py,
 * tests/test_gpu_quantized.py, tests/test_gpu_q8_ln.py, tests/test_gpu_attention.py, tests/test_gpu_rows.py, tests/test_gpu_attention_cls.py, tests/test_gpu_small_path.py, tests/test_gpu_filter_kernels.py (operator parity) and benchmarks/ (A/B timing); nothing in INTEGRATION.md binds it and a
 * deployment does not ship it.  The diagnostic library exports every symbol of include/codesearch_gpu.h as well, so a
 * process may use it in place of libcsgpu.so.
 */
#ifndef CODESEARCH_GPU_DIAG_H
#define CODESEARCH_GPU_DIAG_H

#include "codesearch_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostics: one dense layer of the encoder on host buffers, for unit parity tests of the
 * GEMM kernels (E2/E4/E5/E6).  C[M,N] = A[M,K] W[N,K]^T + bias, epilogue 0 = none,
 * 1 = erf-GELU, 2 = + resid[M,N]; mode = cs_gemm_mode (| 2: the persistent wide kernel).  N % 128 == 0, K % 32 == 0.
 * Wide kernel, N = 384 only: 3 = + resid, then LayerNorm (gamma = bias + 1, beta = -bias) in the same kernel, f32 and
 * split outputs; 4 = the same with the residual handed over in split form in the output buffer and no f32 output (how
 * the encoder runs it).  *range_flag (optional) is set when a split-f16 operand left the f16 range. */
CS_API int32_t cs_debug_gemm(int32_t device, int32_t mode, int32_t epilogue, const float* A,
                      const float* W, const float* bias, const float* resid, float* C,
                      uint32_t M, uint32_t N, uint32_t K, uint32_t* range_flag);

/* Diagnostics: the persistent wide kernel (csrc/gemm_wide.hip, csrc/gemm_wide32.hip) alone on host buffers, every block shape,
 * MFMA form and epilogue, for unit parity against float64 (tests/test_gpu_gemm_wide.py; bounds: tests/gemm_wide_ref.py).
 * A [M, K], W [N, K], bias [N] f32 (A and W are staged into split form by launch_split_rows), N % 192 == 0, K % 32 == 0,
 * |w| <= 31.98.
 *   epi 0  C [M, N] = A W^T + bias, f32 store
 *       1  erf-GELU, split store            2  + resid [M, N], f32 store            3  split store (SH_OUT_SPLIT)
 *       4  GW_OUT_SWIGLU, 5 GW_OUT_GEGLU: W's rows and the bias hold value and gate rows interleaved in groups of 16 (16
 *          value rows, then their 16 gate rows); C [M, N / 2] = value * silu(gate) | value * gelu_erf(gate); N % 64 == 0
 *       6 / 7  N = 384: + resid, LayerNorm (gamma = bias + 1, beta = -bias, eps 1e-12), exactly as cs_debug_gemm's epilogues
 *          3 / 4 run it (6: f32 residual, in place, f32 and split outputs, which must agree; 7: the residual in split form
 *          in the output buffer, no f32 output)
 *   shape  0 = the launcher's own rule, 192 | 384 | 256 = that block asked for (128 x 192, 128 x 384, 256 x 192)
 *   mfma   0 = the launcher's own rule, 16 | 32 = the main loop's MFMA form (32: epilogues 0 - 3, 6, 7, not on the 256-row block)
 * *block_out receives the block the launch ran on (384, 192 or 256: gemm_wide_route, the rule the launcher itself follows;
 * a request the rule does not grant — 384 at an N it cannot take — shows here).  Split stores are read back as hi + lo / 2048.
 * Every output buffer is pre-filled with NaN bits (an element the launch does not write comes back as NaN) and followed by
 * 16 guard rows of a bit pattern: *guard_changed receives how many guard words came back changed.  *range_flag (optional):
 * the kernel's flag, set when a split-stored value left the f16 range. */
CS_API int32_t cs_debug_gemm_wide(int32_t device, int32_t epi, int32_t shape, int32_t mfma, const float* A, const float* W,
                           const float* bias, const float* resid, float* C, uint32_t M, uint32_t N, uint32_t K,
                           int32_t* block_out, uint32_t* guard_changed, uint32_t* range_flag);

/* Diagnostics: one dynamically quantised dense layer on host buffers (unit parity of csrc/gemm_q8.hip against the ONNX
 * definitions of DynamicQuantizeLinear / MatMulInteger).  A [M,K] f32 activations (a_split & 1: staged through the
 * split-f16 form first, as attention and GELU hand them over; a_split & 4: the few-rows kernel (one launch: range from
 * pairs, quantisation and product; epilogues 0 / 1 / 2 / 4 as built for the encoder's chain, acc not reported); a_split & 8: the row-block products that quantise their own
 * rows on the way in — K = 384, M >= 4,096, epilogues 4 (f32 source), 2 (split source) and 5; acc then not reported; a_split & 16:
 * the slab kernel (csrc/gemm_q8_slab.hip: f32 rows, K = 384, epilogues 4 and 5, any M; | 32: its FFN-up store pass takes the s8
 * rows its range pass left instead of quantising again)); W [N,K] f32 = integer multiples of wscale[n]; epilogue as
 * cs_debug_gemm 0 / 1 / 2, 4 = bias -> split store.  Optional outputs: xq [M,K] the uint8 activations, xparams[2] =
 * (x_scale, x_zero_point), acc [M,N] the int32 MatMulInteger result.  N % 128 == 0, K % 128 == 0.
 * epilogue 5 = the FFN-up form (GELU, then quantised again for the next Linear, two passes over the product): C receives
 * the uint8 output as floats, xparams (then FOUR floats) also its (scale, zero_point), the first M entries of acc each
 * output row's sum of uint8 values. */
CS_API int32_t cs_debug_gemm_q8(int32_t device, int32_t epilogue, int32_t a_split, const float* A, const float* W,
                         const float* wscale, const float* bias, const float* resid, float* C, uint32_t M, uint32_t N,
                         uint32_t K, uint8_t* xq, float* xparams, int32_t* acc);

/* Diagnostics: the same products over a tensor that holds SEVERAL quantisation units (queued calls sharing a device
 * batch, cs_embedder_submit_*): row_slot [M] = each row's unit (consecutive runs of rows, in order), bit 31 set where the
 * row lies beyond its call's own padded length (quantised with the unit's parameters, never part of a range).  Row-block
 * products only (K = 384, M >= 4,096); epilogue 4 (f32 source -> split store), 2 (split source, + residual), 5 (FFN-up:
 * GELU, quantised again per unit; C = the uint8 output as floats).  row_params [M][4] = per row (x_scale, x_zero_point,
 * out_scale, out_zero_point) (the last two: epilogue 5), rowsums [M] (epilogue 5) each output row's sum of uint8 values. */
CS_API int32_t cs_debug_gemm_q8_units(int32_t device, int32_t epilogue, const float* A, const float* W, const float* wscale,
                               const float* bias, const float* resid, float* C, uint32_t M, uint32_t N, uint32_t K,
                               const uint32_t* row_slot, uint32_t units, float* row_params, int32_t* rowsums);

/* Diagnostics: the LayerNorm-fused quantised product (gemm_q8_ln_kernel, csrc/gemm_q8.hip: out-proj and FFN-down of the
 * 384-wide quantised models from 4,096 token rows) alone on host buffers, at ANY M, for unit parity against float64
 * (tests/test_gpu_q8_ln.py; reference and bound: tests/q8_ln_ref.py).  A [M, K] f32 activations, W [384, K] f32 = integer
 * multiples of wscale[n] (packed by launch_q8_pack_weight; anything else: CS_ERR_BAD_ARG, "not a quantised matrix"), bias,
 * gamma, beta [384], resid [M, 384] the residual.
 *   source 0  "split" (out-proj, K = 384): launch_split_rows, launch_q8_range(Q8_SRC_SPLIT) by a pass over the tensor,
 *             launch_gemm_q8_ln(Q8_SRC_SPLIT): the kernel quantises its rows on the way in
 *          1  "prequant" (FFN-down, K = 384 | 1536): launch_q8_quantize(Q8_SRC_F32), launch_gemm_q8_ln(Q8_SRC_PREQUANT)
 *   flags & 1 the weight goes through launch_q8_stage_major (w_stage_major = true), else row-major
 *         & 2 the output range is widened into a zeroed slot by the kernel itself (d_out_slot), else left as pairs
 * out [M + CS_DEBUG_Q8_LN_GUARD_ROWS, 384]: the M normalised rows, then the guard rows behind them as they came back — the
 * device tensor holds the residual in its first M rows and CS_DEBUG_Q8_LN_GUARD_WORD in every word of the guard rows.
 * Pairs mode: pairs [ceil(M / 128) * 8][2] (pairs_cap >= that many) receives the pair buffer, pre-filled with NaN bits,
 * *out_pairs what the launcher reported; slot [2] the words 0, 1 of a zeroed slot after
 * launch_q8_range(Q8_SRC_F32, X, ..., pairs, *out_pairs), the reduction the forward runs next.  Slot mode: slot [2] the two
 * words the kernel widened, *out_pairs the launcher's count (0).
 * xq [M, K] (optional) and xparams [2] (optional): the uint8 activations and (x_scale, x_zero_point) of the SEPARATE
 * quantising pass over the same source (source 0: launch_q8_quantize(Q8_SRC_SPLIT) on the split tensor, run for this only). */
#define CS_DEBUG_Q8_LN_GUARD_ROWS 128u
#define CS_DEBUG_Q8_LN_GUARD_WORD 0xA5A5A5A5u
CS_API int32_t cs_debug_gemm_q8_ln(int32_t device, int32_t source, int32_t flags, const float* A, const float* W, const float* wscale,
                            const float* bias, const float* gamma, const float* beta, float eps, const float* resid, uint32_t M,
                            uint32_t K, float* out, float* pairs, uint32_t pairs_cap, uint32_t* out_pairs, uint32_t* slot,
                            uint8_t* xq, float* xparams);

/* Diagnostics: the unit bookkeeping of queued quantised batches (csrc/gemm_q8.hip) alone: seq_unit [B] the unit of each
 * sequence (a unit's sequences consecutive), unit_len [units] each unit's own padded length, L the batch's padded length.
 * row_slot [B * L] (optional) receives launch_q8_row_slots' output.  pairs [B * pairs_per_seq][2] (optional, with slots)
 * go through launch_q8_range_units (pairs_are_rows != 0: a pair per token row, pairs_per_seq == L) into slots
 * pre-filled with a non-zero pattern — the kernel writes words 0, 1 rather than widening them; slots [units][2] receives them. */
CS_API int32_t cs_debug_q8_unit_ranges(int32_t device, const uint32_t* seq_unit, const uint32_t* unit_len, uint32_t B, uint32_t units,
                                uint32_t L, const float* pairs, uint32_t pairs_per_seq, int32_t pairs_are_rows, uint32_t* row_slot,
                                uint32_t* slots);

/* Diagnostics: the one-launch forward of short queries (csrc/small_forward.hip; embed_one / embed_queries_batch,
 * src/embed/mod.rs:164-226) — mini-batches of a 384-d BERT model with at most 192 token rows in split-f16 mode as ONE kernel,
 * bit-identical to the kernel-by-kernel path and measured slower than it (profiles/r05_small_forward_ab.log), so it is built
 * into this library only and taken with CS_SMALL_FORWARD=1: how many mini-batches took it, and how many of those gave up at
 * a grid barrier and were re-run kernel by kernel. */
CS_API int32_t cs_debug_small_forward_counters(cs_embedder* h, uint64_t* forwards, uint64_t* fallbacks);

/* Diagnostics: the attention kernels (E3, csrc/attention_split.hip) alone on host buffers, for unit parity against a float64
 * softmax (tests/test_gpu_attention.py).  qkv [B*L, 3H] f32, a row = Q heads | K heads | V heads, head h at columns h * dh
 * (dh = H / heads = 32 or 64); mask [B, L], non-zero = a token.  The rows are split (launch_split_rows) and handed to
 * launch_attention_sh2 exactly as the encoder hands them; out [B*L, H] receives the split context read back as
 * hi + lo / 2048, padded query rows included.  Buffers hold exactly B * L rows.
 * alibi_slopes [heads] (optional): JinaBert's ALiBi, -slope_h |i - j| on every score; the kernel receives the slopes and the
 * slopes times log2 e in f32, as cs_embedder_create builds the table.  window (0: none): ModernBERT's local layers, keys with
 * |i - j| > window are masked.  Both together: the launcher's CS_ERR_BAD_ARG.
 * seq_unit [B], unit_len [units], units (all null / 0: one unit): the quantisation units of a queued device batch — query
 * rows at or beyond unit_len[seq_unit[b]] stay out of the range pairs.
 * range_pairs_out (optional, with range_pairs): the raw (lo, hi) float pairs every wave reports of what it stored, as the
 * quantised path reads them; *range_pairs = how many the launcher reported, CS_ERR_BAD_ARG when that exceeds
 * range_pairs_cap (heads * B * ceil(L / 128) * 4 always suffices).
 * proj_w [H, H], proj_bias [H], proj_resid [B*L, H] (all or none): attention INSIDE the out-projection instead
 * (launch_sp_attn_proj: H = 384, 12 heads, L <= 32, B * L <= 256; no ALiBi, window, units or pairs) — out [B*L, H] is then
 * attention(qkv) proj_w^T + proj_bias + proj_resid in f32.
 * *range_flag (optional) is set when a split-f16 value (an input or a stored context value) left the f16 range or was NaN. */
CS_API int32_t cs_debug_attention(int32_t device, const float* qkv, const int32_t* mask, uint32_t B, uint32_t L, uint32_t H,
                           uint32_t heads, const float* alibi_slopes, uint32_t window, const uint32_t* seq_unit,
                           const uint32_t* unit_len, uint32_t units, const float* proj_w, const float* proj_bias,
                           const float* proj_resid, float* out, float* range_pairs_out, uint32_t range_pairs_cap,
                           uint32_t* range_pairs, uint32_t* range_flag);

/* Diagnostics: the row kernels of csrc/encoder.hip alone on host buffers, for unit parity against float64
 * (tests/test_gpu_rows.py): launch_row_kernel(which, ...) exactly as the embedder calls it.  H = 384 | 768 | 1024.
 *   which 0  embed_ln_kernel: ids [T], word [vocab, H], pos [L, H] (optional: no position table), type_table [ntypes, H], types
 *            [T] (optional: every token has type 0); row t = LayerNorm((word[id] + type) + pos[t % L])
 *   which 1  layernorm_kernel: x [T, H], in place
 *   which 2  pool_normalize_kernel / mean_pool_normalize_kernel (the launcher chooses): x [B * L, H], mask [B, L], pooling =
 *            CS_POOL_CLS | CS_POOL_MEAN -> out [B, H]; T is not read
 *   which 3  layernorm_sum_kernel: x [T, H] the residual, parts [nparts, T, H] the slabs of a split-K product, bias [H]
 *   which 4  layernorm_to_kernel: x [T, H] the source, left as it is (src_after, optional, receives it back)
 * gamma / beta [H] and eps for which != 2.  out [T, H] receives the f32 rows; out_split (optional, which != 2) makes the
 * launch write the split form too and receives it read back as hi + lo / 2048.  range_mode 1 (which 0 | 1): range_out
 * [ceil(T / 4)][2] receives each block's (lo, hi); 2: [T][2], one pair per row; pairs the kernel does not write come back
 * as NaN.  *range_flag (optional): set when a split-form value left the f16 range. */
CS_API int32_t cs_debug_rows(int32_t device, int32_t which, uint32_t H, uint32_t T, uint32_t L, uint32_t B, float eps, int32_t pooling,
                      const int32_t* ids, const float* word, const float* pos, const float* type_table, const int32_t* types,
                      uint32_t ntypes, uint32_t vocab, const float* x, const int32_t* mask, const float* parts, uint32_t nparts,
                      const float* bias, const float* gamma, const float* beta, int32_t range_mode, float* out, float* out_split,
                      float* src_after, float* range_out, uint32_t* range_flag);

/* Diagnostics: the element-wise kernels of csrc/nomic.hip alone on host buffers (tests/test_gpu_rows.py), split != 0: the
 * split-f16 form (the f32 input goes through launch_split_rows first, the result is read back as hi + lo / 2048), else f32.
 *   op 0  launch_rope_split / launch_rope_f32: a = qkv [T, 3H], table = [L][dh / 2] (cos, sin) pairs, dh = H / heads; token
 *         t takes table row t % L.  out [T, 3H]: the whole tensor, V columns included.
 *   op 1  launch_swiglu_split: a = [T, 2I], every 32 columns = 16 values | their 16 gates (the interleaved order of the up
 *         projection's weight rows); launch_swiglu_f32: a = value [T, I], b = gate [T, I].  out [T, I] = value * act(gate),
 *         act = silu, or the erf-GELU with gelu_gate != 0.
 *   op 2  launch_qk_layernorm_split / _f32: a = qkv [T, 3H], table = gamma_q | beta_q | gamma_k | beta_k [4][H], eps.
 *         out [T, 3H]: the whole tensor.
 * flags [2] (optional): [0] the kernel's range flag, [1] that of the input's split. */
CS_API int32_t cs_debug_elementwise(int32_t device, int32_t op, int32_t split, uint32_t T, uint32_t L, uint32_t H, uint32_t heads,
                             uint32_t I, int32_t gelu_gate, float eps, const float* a, const float* b, const float* table,
                             float* out, uint32_t* flags);

/* Diagnostics: the kernels of the CLS tail (csrc/cls_tail.hip) alone on host buffers (tests/test_gpu_attention_cls.py).
 * qkv [B*L, 3H] f32 as cs_debug_attention takes it, mask [B, L] -> out [B, H]: the rows are split, the K and V lines of every
 * token become kvs [T][2H/32][64], the Q lines of the rows b * L become q_cls, and launch_attention_cls runs as the
 * embedder's last layer calls it; out receives the split context read back as hi + lo / 2048.
 * gather_src [B*L, H] f32 (optional, with x_cls [B, H] and xs_cls [B][H/32][64] f16 words): launch_gather_cls on its split
 * form.  Either part may be left out (all its pointers null).  flags [2] (optional): [0] the attention kernel's range flag,
 * [1] that of the inputs' split. */
CS_API int32_t cs_debug_attention_cls(int32_t device, const float* qkv, const int32_t* mask, uint32_t B, uint32_t L, uint32_t H,
                               uint32_t heads, float* out, uint32_t* flags, const float* gather_src, float* x_cls,
                               uint16_t* xs_cls);

/* Diagnostics: the exact-f32 attention kernels of csrc/encoder.hip alone on host buffers: launch_attention, as the f32
 * forward and every mini-batch that raised the range flag run it.  Arguments as cs_debug_attention's of the same names
 * (alibi_slopes [heads], optional); out [B*L, H] f32, padded query rows included.  L <= 512. */
CS_API int32_t cs_debug_attention_f32(int32_t device, const float* qkv, const int32_t* mask, uint32_t B, uint32_t L, uint32_t H,
                               uint32_t heads, const float* alibi_slopes, uint32_t window, float* out);

/* Diagnostics: the dense kernels of the small path (csrc/small_path.hip: forwards of under 200 token rows) alone on host
 * buffers, for unit parity against float64 (tests/test_gpu_small_path.py): the launchers exactly as Slice::run_small calls
 * them, the narrow or the wide form chosen by the launcher.  H = 384 | 768 | 1024, 1 <= T <= 256, N % 32 == 0.
 *   op 0  launch_sp_ln_gemm: a LayerNorm prologue, then Cs = LN rows x W^T + bias.  epi 0: split store, 1: erf-GELU, then
 *         split store.  gamma / beta [H], eps, W [N, H] and bias [N] f32 (W is staged into split form by launch_split_rows).
 *           pro 0  rows [T, H]: the rows to normalise
 *           pro 1  parts [4][T][H] (slab stride T, as the kernel indexes it), parts_bias [H], x [T, H] the residual: the
 *                  rows are ((p0 + p1 + p2 + p3) + bias) + x; x_after (optional) receives x back after the launch
 *           pro 2  ids [T], word [vocab, H], pos [L, H], type_table [ntypes, H], types [T] (optional: row 0 of the table):
 *                  row t = (word[id] + type) + pos[t % L], an id outside the table reads row 0, a type beyond it the last row
 *         xout [T, H] receives the normalised f32 rows (a buffer of its own, as in the embedder), cs_out [T, N] the split
 *         output read back as hi + lo / 2048.
 *   op 1  launch_sp_partial: rows = A [T, 4H], W [N, 4H] f32, both staged into split form; parts_out [4][T][N] f32 receives
 *         the four K-slice slabs, slab ks = A[:, ks H .. (ks + 1) H) W[:, the same]^T.
 * Every input holds exactly T rows (the kernels clamp their reads to row T - 1).  Every output is allocated with 16 guard
 * rows behind row T - 1 (parts_out: behind slab 3's; a store past row T - 1 of an earlier slab lands in the next slab's
 * first rows), filled with a bit pattern: *guard_changed receives how many guard words came back changed.  An output element
 * the launch does not write comes back as NaN.  flags [2] (optional): [0] the kernel's range flag, [1] that of the operands'
 * split. */
CS_API int32_t cs_debug_small_path(int32_t device, int32_t op, int32_t epi, int32_t pro, uint32_t H, uint32_t T, uint32_t N, uint32_t L,
                            float eps, const float* gamma, const float* beta, const float* rows, const float* parts,
                            const float* parts_bias, const float* x, const int32_t* ids, const float* word, const float* pos,
                            const float* type_table, const int32_t* types, uint32_t ntypes, uint32_t vocab, const float* W,
                            const float* bias, float* xout, float* cs_out, float* x_after, float* parts_out, uint32_t* flags,
                            uint32_t* guard_changed);

/* Diagnostics: ONE phase of the batched filter search (csrc/scan_filter.hip) alone on host buffers, for parity of the candidate
 * set with float64 cosines (tests/test_gpu_filter_kernels.py; references and decision rules: tests/filter_ref.py).  dim = 384 |
 * 768 | 1024; corpus [n_rows, dim], queries [nq, dim], tau [nq] f32; dead (optional) the tombstone bitmap, one bit per stored
 * row; mu_in [dim] (optional) the vector the int8 copy is centred on, else launch_unit_mean over the n_rows rows.
 * Runs launch_row_norms, launch_corpus_split (the f16 copy), launch_unit_mean and launch_corpus_q8 (the int8 copy: the
 * n_rows / 128 complete tiles), launch_prep_queries with the int8 plane and the hi / lo planes, then — tau overwritten with the
 * caller's, the counters zeroed — one launch_filter_phase filled by hand:
 *   kernel    a cs::FilterKernel value (filter_plan.hpp: 0 None, 1 Q8Tile256, 2 Q8Rq, 3 Q8Rq1, 4 Q8Rw, 5 Q8Rw2, 6 F16Rw,
 *             7 F16Tile256, 8 F16Tile128), nqt its 32-query groups per query tile (0 for the tile kernels)
 *   rows      [row_lo, row_hi), row_lo % 128 == 0; int8 kernels: whole complete tiles; f16: row_hi <= n_rows
 *   cap       candidate slots per query
 *   grid      0 = plan_filter's rule for that kernel, else the blocks to launch
 *   tail      [tail_lo, tail_hi), fewer than 128 rows: tail_candidates_kernel (equal: none)
 * A combination the launcher refuses is its CS_ERR_BAD_ARG: a (kernel, nqt) filter_insts<dim / 128>() does not hold, row_lo
 * off a tile, an int8 row_hi off a tile, a resident-query grid that is no multiple of 8 or below 8 per query tile.
 * Outputs (each optional but cnt_out, cand_out, guard_changed): norms_out [n_rows], mu_out [dim]; f16_out [n_rows, dim] the
 * f16 copy's bit patterns un-tiled; q8_out [n_rows / 128 * 128, dim] the int8 copy un-tiled, tmeta_out [n_rows / 128][4];
 * qunit_out [nq, dim] the f16 unit queries' bit patterns; q8q_out, q8q_hi_out, q8q_lo_out [nq, dim] the query planes;
 * qmeta_out [4 nq][4] (SplitQueryWs::d_qmeta), qmag_out [nq]; cnt_out [nq + CS_DEBUG_FILTER_CNT_PAD] the candidate counters
 * of the queries and of the padded queries behind them; cand_out [nq, cap] the low word of every candidate slot: query q's
 * candidates are its first min(cnt, cap) entries, the rest CS_DEBUG_FILTER_GUARD_WORD.
 * Guards: every candidate slot (both words) and every unused word of a counter line is pre-filled with
 * CS_DEBUG_FILTER_GUARD_WORD, and one spare query's slots lie behind the last query's; *guard_changed = the words that came
 * back changed among: the spare slots, a query's slots at or past min(cnt, cap), the high word of any slot, the unused
 * counter words. */
#define CS_DEBUG_FILTER_CNT_PAD 256u
#define CS_DEBUG_FILTER_GUARD_WORD 0xA5A5A5A5u
CS_API int32_t cs_debug_filter(int32_t device, uint32_t dim, const float* corpus, uint64_t n_rows, const float* queries, uint32_t nq,
                        const float* tau, const uint32_t* dead, const float* mu_in, int32_t kernel, uint32_t nqt, uint64_t row_lo,
                        uint64_t row_hi, uint32_t cap, uint32_t grid, uint64_t tail_lo, uint64_t tail_hi, float* norms_out,
                        float* mu_out, uint16_t* f16_out, int8_t* q8_out, float* tmeta_out, uint16_t* qunit_out, int8_t* q8q_out,
                        int8_t* q8q_hi_out, int8_t* q8q_lo_out, float* qmeta_out, float* qmag_out, uint32_t* cnt_out,
                        uint32_t* cand_out, uint32_t* guard_changed);

/* Diagnostics: device milliseconds per launch of one dense layer on synthetic operands resident in HBM.
 * mode 0 exact-f32 MFMA, 1 split-f16 (128 x 128 / skinny kernels), 2 split-f16 wide kernel (N % 384 == 0);
 * epilogue 0 f32, 1 GELU -> split, 2 + residual, 3 LayerNorm-fused (mode 2, N = 384), 4 bias -> split (QKV);
 * ablation (mode 2): 0 none; epilogue 4 only: 1 no LDS-DMA, 2 no MFMA, 3 DMAs issued at the start of a k-step, 4-10 see
 * gemm_wide.hip; any epilogue: 192 / 384 = that block shape of the product kernel.  CS_DEBUG_GEMM_ZERO=1: all-zero operands
 * (the same instruction stream at the clock the chip holds on trivial data). */
CS_API int32_t cs_debug_gemm_time(int32_t device, int32_t mode, int32_t epilogue, uint32_t M, uint32_t N, uint32_t K,
                           uint32_t iters, int32_t ablation, double* ms_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* CODESEARCH_GPU_DIAG_H */
