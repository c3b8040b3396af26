// forward_plan.hpp — the route of an encoder forward (embedder_forward.hip): into how many slices a mini-batch is cut, which
// launch sequence a slice takes and, inside it, which kernel runs each dense layer and what is fused.  Plain C++17, no HIP:
// tests/cpp/forward_plan_test.cpp pins the plans on the CPU, and forward / forward_range only launch what plan_streams /
// plan_forward return.  What a launcher chooses by itself (gemm_split's skinny kernel up to 1,100 rows, q8_slab_takes, the
// 16 x 64 forms of the few-rows products, sp_attn_proj's span) is not part of the plan.
#pragma once

#include <cstdint>

#include "../../include/cs_bert_params.h"  // CS_ARCH_*, CS_POOL_*, CS_GEMM_*, cs_arch_gated

namespace cs {

constexpr uint32_t SP_MAX_ROWS = 256;  // token rows the small path takes (small_path.hip; workspace: 5 x SP_MAX_ROWS x H floats)
constexpr int QR_KC = 3;               // K = 128 * QR_KC: the depth gemm_q8_rows_kernel is built for (gemm_q8.hip)
constexpr int QN_N = 384;              // the width gemm_q8_ln_kernel is built for (gemm_q8.hip)

// The thresholds of the route, read once per process (embedder_forward.hip forward_knobs_from_env; the name of each knob
// beside it: laboratory knobs unless it says deployment).
struct ForwardKnobs {
    uint32_t split_k_min = 1100;  // CS_GEMM_SPLITK_MIN_M
    uint32_t split_k_max = 6144;  // CS_GEMM_SPLITK_MAX_M
    // device us per forward, fused / FFN-down in 3 K slices / out-proj too: 1,280 rows 1320 / 1020 / 971, 2,048
    // 1331 / 1052 / 1021, 4,096 1538 / 1311 / 1328, 6,144 1841 / 1619 / 1654, 8,192 2210 / 2264 / -
    // two slices up to 10,240 rows: 7,168 rows 2048 -> 1891 us, 8,192 2203 -> 2060, 10,240 2443 -> 2369, 12,288 3034 -> 3167
    uint32_t split_k_max2 = 10240;   // CS_GEMM_SPLITK_MAX2_M
    uint32_t split_k_ao_max = 2560;  // CS_GEMM_SPLITK_AO_MAX_M
    // dense layer: the persistent 128 x 384 one-accumulator kernel from wide_min_m token rows on (gemm_wide.hip),
    // else the 128 x 128 / skinny kernels of gemm_split.hip
    // A persistent block owns whole 128 x 384 tiles, so a launch needs about one tile per CU to fill the chip: the wide
    // kernel takes a layer when its tiles cover >= 85 % of the CUs, or from wide_min_m rows when the other half-batch
    // runs beside it on the second stream (measured, device ms per forward, wide / 128 x 128: 32 x 256 tokens 2.67 /
    // 2.08, 64 x 256 4.01 / 3.57 — one stream, N = 384 layers leave half the chip idle — 128 x 256 5.95 / 6.40,
    // 256 x 256 11.4 / 12.5).
    uint32_t wide_min_m = 12288;  // CS_GEMM_WIDE_MIN_M (0 = never)
    // Mid-size launches (the reference's 32-chunk calls: 8,192 token rows): the 128 x 128 grid is 1.1 rounds of
    // blocks for QKV (576 tiles on 512 slots); 128 x 192 tiles at two blocks per CU make it ONE round (384 tiles for
    // QKV, 512 for FFN-up).  Taken when that single round is at least 70 % full.
    bool mid192 = true;  // CS_GEMM_WIDE_MID
    // N = 384 at indexing batch sizes: dense layer + residual + LayerNorm in one kernel (gemm_wide.hip)
    bool ln_fuse = true;  // CS_GEMM_WIDE_LN
    // the residual stream is carried in split form alone between the fused layers (read from xs, no f32
    // copy written: 100 MB less per layer and 65,536 rows); the last layer writes x for the pooling
    bool split_resid = true;  // CS_GEMM_WIDE_LN_SPLIT_RESID
    bool gate_fused = true;   // CS_NOMIC_GATE_FUSED: the gate as the product's epilogue: the raw [T, 2I] tensor never exists
    // several quantisation units in a batch the row-block kernels take: every product quantises its own rows with their
    // unit's parameters, the producers' pairs are reduced per unit (LayerNorm: a pair per row)
    bool q8_rows_units = true;  // CS_Q8_ROWS_UNITS
    // (q8_x_pairs == 0: the LayerNorm-fused product that wrote x widened this tensor's slot itself — CS_Q8_LN_SLOT=1; measured:
    // what the consumers save on the reduction launch, 4 us each, the producers pay for the block's meeting and its
    // agent-scope update, profiles/r05_q8_ln_epilogue_ab.log: opt-in.  Default: pairs + a reduction launch)
    bool q8_ln_slot = false;  // CS_Q8_LN_SLOT
    // The row-block kernel (gemm_q8_rows_kernel) takes K = 384 layers from rows_min_m rows on: below that a row block per CU
    // leaves most of the chip idle and the tile-per-block kernel spreads the same work over more CUs.  CS_Q8_ROWS=0: never.
    int q8_rows_min_m = 4096;         // CS_Q8_ROWS
    bool q8_rows_src = true;          // CS_Q8_ROWS_SRC (0 = the row-block products never quantise on load)
    uint32_t q8_skinny_max_m = 512;   // CS_Q8_SKINNY_MAX_M: rows up to which the few-rows products run (0 = never)
    // CLS pooling reads ONE row per sequence of the last layer: its attention needs every key and value but
    // only the CLS query, and everything behind it runs on nb rows instead of nb * L (cls_tail.hip).  Same
    // embedding, 1/12 less work at 12 layers.  Compact rows live in the (idle) intermediate buffer of the slice.
    bool cls_tail = true;                 // CS_ENCODER_CLS_TAIL (deployment)
    uint32_t cls_tail_min_tokens = 4096;  // CS_ENCODER_CLS_TAIL_MIN_TOKENS (deployment)
    // Slicing pays from ~20,000 tokens (device us per forward, one stream / two: 16,384 tokens 3505 / 3542,
    // 24,576 5267 / 4916, 32,768 6517 / 6275, 49,152 9568 / 9437); below that it only multiplies launches
    // of kernels that already leave the chip part-empty.
    uint64_t stream_min_tokens = 20000;  // CS_ENCODER_STREAM_MIN_TOKENS
};

// The switches read at the top of every forward: tests and A/B runs flip them mid-process.
struct ForwardToggles {
    bool small_path = true;      // CS_SMALL_PATH=0: the general small-batch kernels instead of small_path.hip
    bool small_fuse = true;      // CS_SMALL_FUSE=0: attention and out-projection of the small path as two launches
    bool q8_skinny_ln = true;    // CS_Q8_SKINNY_LN=0: the LayerNorm launches of the few-rows quantised path
    bool q8_ln_fused = true;     // CS_Q8_LN_FUSED=0 (laboratory): out-proj and FFN-down without gemm_q8_ln_kernel
    bool small_forward = false;  // CS_SMALL_FORWARD=1 (diagnostic library): the small path as ONE launch
};

// One slice of a mini-batch as the plan sees it (plan_streams: the whole mini-batch, nb = its sequences, b0 = 0).
struct ForwardShape {
    uint32_t arch = CS_ARCH_BERT, hidden = 0, intermediate = 0, heads = 0, layers = 0;
    int pooling = CS_POOL_CLS;
    int mode = CS_GEMM_SPLIT_F16;
    uint32_t nb = 0, L = 0, b0 = 0;  // sequences [b0, b0 + nb) of L positions each
    uint32_t units = 1;              // quantisation units of the mini-batch (q8)
    int streams_in_flight = 1;       // slices of the mini-batch running side by side
    int n_streams = 2;               // plan_streams: streams the embedder holds, and whether CS_ENCODER_STREAMS fixed them
    bool streams_forced = false;
    bool wide_ok = false;            // the one-accumulator kernels may run (every |w| < 31.98, CS_GEMM_WIDE)
    uint64_t cap_range_pairs = 0, cap_range_pairs2 = 0;  // (lo, hi) pairs the two range-pair buffers hold (q8)
    bool stage_profile = false;      // an event after every kernel (one stream)
    bool small_forward_ok = false;   // the one-launch forward is built, set up, not switched off and takes this shape
    int cus = 256;                   // the device's compute units
};

// One value per launch sequence of forward_range.  Refused: ModernBERT in the dynamic-quantisation mode (an error, nothing
// is launched).
enum class ForwardPath : uint8_t {
    Modern,          // ModernBERT's pre-norm layers (split-f16 or exact f32 by the mode)
    Small,           // under 200 token rows: small_path.hip
    SmallOneLaunch,  // ... as one launch (small_forward.hip, diagnostic library)
    Q8FewRows,       // q8, a few token rows: one launch per Linear
    Q8RowsSource,    // q8, one unit, a row block per CU: the products quantise their own rows on the way in
    Q8MultiUnit,     // q8, the same with every range kept per unit
    Q8Quantise,      // q8, quantising passes in front of the tile-per-block products
    Split,           // split-f16
    F32,             // exact f32
    Refused,
};

// Which kernel runs a dense layer of the split-f16 sequences: the persistent 128 x 384 kernel, its 128 x 192 form
// (gemm_wide.hip), or the 128 x 128 / skinny kernels of gemm_split.hip.
enum class DenseKernel : uint8_t { Split, Wide192, Wide384 };

struct ForwardPlan {
    ForwardPath path = ForwardPath::F32;
    // Split and Modern in split-f16 mode.  A field is set where the sequence reads it: `ao` / `down` only when that layer is
    // neither LayerNorm-fused nor cut into K slices, kv_tail only with cls_tail.
    DenseKernel qkv = DenseKernel::Split, kv_tail = DenseKernel::Split, ao = DenseKernel::Split, up = DenseKernel::Split,
                down = DenseKernel::Split;
    bool fuse_ln = false;      // the N = 384 layers (out-proj, FFN-down) with residual + LayerNorm as their epilogue
    bool split_resid = false;  // ... and the residual stream in split form only between them
    uint8_t ao_slices = 0;     // 0 | 3: out-proj as K slices summed by the LayerNorm that follows
    uint8_t down_slices = 0;   // 0 | 2 | 3: FFN-down likewise
    bool gate_epilogue = false;  // gated feed-forward: the gate as FFN-up's epilogue (on `up`'s tile: 384 | 192)
    bool cls_tail = false;       // the last layer on the CLS rows only
    bool attn_proj_fused = false;  // Small: attention inside the out-projection's blocks
    // q8
    bool fold_ln = false;        // Q8FewRows: the two LayerNorms as prologues of the products that read them
    bool ln_fused_ao = false;    // Q8RowsSource: out-proj with residual + LayerNorm in one kernel (gemm_q8_ln_kernel)
    bool ln_fused_down = false;  // ... and FFN-down
    bool ln_slot = false;        // ... which widen the next tensor's range slot themselves
    bool multi_unit = false;     // LayerNorm leaves a pair per row, reduced per unit (Q8MultiUnit)
};

// ---- what the kernels are built for (their launchers check their arguments with the same functions) -----------------------

inline bool gemm_wide_supported(uint32_t N, uint32_t K) { return N % 192 == 0 && K % 32 == 0 && N > 0 && K > 0; }

inline bool small_path_supported(uint32_t H, uint32_t I, uint32_t T) {
    return (H == 384 || H == 768 || H == 1024) && I == 4 * H && T >= 1 && T <= SP_MAX_ROWS;
}
// attention + out-projection in one launch: sequences of up to 32 tokens of a 384-wide, 12-head model
inline bool sp_attn_proj_supported(uint32_t H, uint32_t heads, uint32_t T, uint32_t L) {
    return H == 384 && heads == 12 && T >= 1 && T <= SP_MAX_ROWS && L >= 1 && L <= 32 && T % L == 0;
}

inline bool q8_rows_takes(const ForwardKnobs& kn, uint32_t M, uint32_t K) {
    return K == 128 * QR_KC && kn.q8_rows_min_m > 0 && M >= (uint32_t)kn.q8_rows_min_m;
}
// From 4,096 rows a K = 384 layer can take the f32-class tensor itself: the product kernel's blocks quantise their own rows
// on the way in, only the tensor's range is needed first.  One quantisation unit only.
inline bool q8_rows_from_source(const ForwardKnobs& kn, uint32_t M, uint32_t K) { return kn.q8_rows_src && q8_rows_takes(kn, M, K); }
// N = 384 layers of a one-unit batch from 4,096 rows: product + bias + residual + LayerNorm in ONE kernel
inline bool q8_ln_fused_takes(const ForwardKnobs& kn, const ForwardToggles& tg, uint32_t M, uint32_t N, uint32_t K) {
    return tg.q8_ln_fused && N == (uint32_t)QN_N && (K == 384 || K == 1536) && q8_rows_takes(kn, M, 384);
}

// ---- the plan --------------------------------------------------------------------------------------------------------------

constexpr uint32_t kSmallPathRows = 200;   // the small path takes fewer token rows than this
constexpr uint32_t kWideMinTiles = 218;    // 128 x 384 tiles from which one stream fills the chip (85 % of 256 CUs)
constexpr uint32_t kMid192MinTiles = 358;  // 128 x 192 tiles of ONE round of blocks that is at least 70 % full ...
constexpr uint32_t kMid192MaxTiles = 512;  // ... two blocks per CU

inline DenseKernel dense_kernel(const ForwardKnobs& kn, const ForwardShape& s, uint32_t M, uint32_t N, uint32_t K) {
    if (!s.wide_ok || !gemm_wide_supported(N, K)) return DenseKernel::Split;
    if (kn.wide_min_m && N % 384 == 0) {
        const uint32_t tiles = ((M + 127) / 128) * (N / 384);
        if (tiles >= kWideMinTiles || (s.streams_in_flight >= 2 && M >= kn.wide_min_m)) return DenseKernel::Wide384;
    }
    if (kn.mid192 && s.streams_in_flight < 2) {
        const uint32_t tiles = ((M + 127) / 128) * (N / 192);
        if (tiles >= kMid192MinTiles && tiles <= kMid192MaxTiles) return DenseKernel::Wide192;
    }
    return DenseKernel::Split;
}

// Into how many slices, each on a stream of its own, forward cuts the mini-batch (1 = none).
inline uint32_t plan_streams(const ForwardKnobs& kn, const ForwardShape& s) {
    // The persistent wide kernels give every CU a whole number of tiles when the tile counts of the three layer shapes
    // (T/128 x {1, 3, 4}) are multiples of the CU count; then one stream is as good or better (256 x 256 tokens: 11.05
    // vs 11.20 ms) and the second stream only helps where a last round of tiles would leave CUs idle (160 x 256: 8.08
    // one stream, 7.07 two).  CS_ENCODER_STREAMS forces the count either way.
    bool whole_rounds = false;
    if (s.mode == CS_GEMM_SPLIT_F16 && s.wide_ok && !s.streams_forced) {
        const uint64_t cus = s.cus > 0 ? (uint64_t)s.cus : 0, mt = ((uint64_t)s.nb * s.L + 127) / 128;
        auto eff = [&](uint64_t tiles) { return cus > 0 ? (double)tiles / (double)(((tiles + cus - 1) / cus) * cus) : 0.0; };
        whole_rounds = s.hidden == 384 && mt >= kWideMinTiles && eff(mt) >= 0.96 && eff(3 * mt) >= 0.96 && eff(4 * mt) >= 0.96;
    }
    // (a quantised tensor is the WHOLE mini-batch: slices on several streams would each see their own range)
    if (!s.stage_profile && !whole_rounds && s.mode != CS_GEMM_Q8_DYNAMIC && s.n_streams >= 2 && s.nb >= (uint32_t)s.n_streams &&
        (uint64_t)s.nb * s.L >= kn.stream_min_tokens)
        return (uint32_t)s.n_streams;
    return 1;
}

inline ForwardPlan plan_forward(const ForwardKnobs& kn, const ForwardToggles& tg, const ForwardShape& s) {
    ForwardPlan p;
    const uint32_t H = s.hidden, I = s.intermediate, T = s.nb * s.L;
    const bool q8 = s.mode == CS_GEMM_Q8_DYNAMIC, split = s.mode == CS_GEMM_SPLIT_F16;
    const bool gated = cs_arch_gated(s.arch);
    auto dense = [&](uint32_t N, uint32_t K) { return dense_kernel(kn, s, T, N, K); };
    if (s.arch == CS_ARCH_MODERN) {
        p.path = q8 ? ForwardPath::Refused : ForwardPath::Modern;
        if (split) {
            p.qkv = dense(3 * H, H);
            p.ao = dense(H, H);
            p.up = dense(2 * I, H);
            p.gate_epilogue = p.up != DenseKernel::Split;  // (this family's gate follows the kernel alone)
            p.down = dense(H, I);
        }
        return p;
    }
    // ---- a few short sequences (under 200 token rows: the query side) ----
    // small_path.hip: LayerNorm as the prologue of the dense layer that reads it, FFN-down as four K slices summed by the
    // LayerNorm that follows: 62 launches per 12-layer forward instead of 86, none of them pulling 196 KB through one CU
    // (CS_SMALL_PATH=0: the general small-batch kernels).  Diagnostic library, CS_SMALL_FORWARD=1: the same arithmetic as ONE
    // launch (small_forward.hip) — bit-identical, measured slower than the launches.
    if (split && tg.small_path && !gated && s.b0 == 0 && T < kSmallPathRows && small_path_supported(H, I, T)) {
        if (tg.small_forward && s.small_forward_ok && !s.stage_profile) {
            p.path = ForwardPath::SmallOneLaunch;
            return p;
        }
        p.path = ForwardPath::Small;
        // sequences of up to 32 tokens (a query and its variants) of a 384-wide model: attention inside the out-projection's
        // blocks, 50 instead of 62 launches per 12-layer forward
        p.attn_proj_fused = tg.small_fuse && sp_attn_proj_supported(H, s.heads, T, s.L);
        return p;
    }
    if (q8) {
        const bool one_unit = s.units <= 1;
        p.multi_unit = kn.q8_rows_units && !one_unit && q8_rows_from_source(kn, T, H) && T <= s.cap_range_pairs;
        if (one_unit && T <= kn.q8_skinny_max_m && I <= 3072 && (uint64_t)(I / 16) * ((T + 15) / 16) <= s.cap_range_pairs2) {
            // a few token rows (queries): one launch per Linear — range reduction and quantisation inside the product
            p.path = ForwardPath::Q8FewRows;
            // Up to 16 rows of a 384-wide model (one short query): the two LayerNorms of a layer are the prologues of the
            // products that read them — five launches per layer instead of seven
            p.fold_ln = tg.q8_skinny_ln && T <= 16 && H == 384;
        } else if (one_unit && q8_rows_from_source(kn, T, H)) {
            p.path = ForwardPath::Q8RowsSource;
            p.ln_fused_ao = q8_ln_fused_takes(kn, tg, T, H, H);
            p.ln_fused_down = q8_ln_fused_takes(kn, tg, T, H, I);
            p.ln_slot = kn.q8_ln_slot;
        } else {
            p.path = p.multi_unit ? ForwardPath::Q8MultiUnit : ForwardPath::Q8Quantise;
        }
        return p;
    }
    if (!split) return p;  // exact f32
    p.path = ForwardPath::Split;
    // ... the CLS tail where its kernels and scratch fit (else the full layer, never an error): attention_cls_kernel
    // takes <= 512 keys and head_dim 32 | 64; the compact rows (4 nb H + nb I floats) live in the slice's
    // [T, I] intermediate buffer
    const uint32_t dh = s.heads ? H / s.heads : 0;
    const bool tail_fits = s.L <= 512 && (dh == 32 || dh == 64) && H % s.heads == 0 && (uint64_t)(s.L - 1) * I >= (uint64_t)4 * H;
    p.cls_tail = kn.cls_tail && tail_fits && !gated && s.pooling == CS_POOL_CLS && T >= kn.cls_tail_min_tokens && s.L >= 16;
    if (p.cls_tail) p.kv_tail = dense(2 * H, H);
    p.qkv = dense(3 * H, H);
    p.fuse_ln = kn.ln_fuse && H == 384 && dense(H, H) == DenseKernel::Wide384;
    p.split_resid = p.fuse_ln && kn.split_resid;  // every N = 384 layer of this forward is fused or none is
    const bool slices = !p.fuse_ln && T > kn.split_k_min;
    // a few thousand token rows: FFN-down is 3 x T / 128 blocks walking 48 K stages one exposed latency each; three K slices
    // per tile (two from 6,144 rows: still one round of blocks), summed with bias and residual by the LayerNorm that follows
    if (slices && T <= kn.split_k_max && T <= kn.split_k_ao_max) p.ao_slices = 3;
    else if (!p.fuse_ln) p.ao = dense(H, H);
    p.up = dense(gated ? 2 * I : I, H);
    p.gate_epilogue = gated && kn.gate_fused && p.up != DenseKernel::Split;
    if (slices && T <= kn.split_k_max2) p.down_slices = T <= kn.split_k_max ? 3 : 2;
    else if (!p.fuse_ln) p.down = dense(H, I);
    return p;
}

}  // namespace cs
