// The route of an encoder forward (codesearch_amd/csrc/forward_plan.hpp) on the CPU: the launch sequence a slice of a
// mini-batch takes, the kernel of each dense layer and what is fused (plan_forward), and into how many slices the mini-batch
// is cut (plan_streams).  Every expected plan below was recorded from the decision expressions of emb::forward_range and
// emb::forward (embedder_forward.hip) and of the predicates they called in gemm_q8.hip, small_path.hip and gemm_wide.hip as
// they stood before the plan was split out of them; 12 layers, 256 compute units unless the case says otherwise, the range
// pair buffers as reserve() sizes them.  Form of a plan: the path, then every field of ForwardPlan that is not at its default
// (a dense kernel left out is gemm_split's; w192 / w384: the 128 x 192 / 128 x 384 persistent kernel).
#include <cstdio>
#include <string>

#include "../../codesearch_amd/csrc/forward_plan.hpp"

using namespace cs;

enum Knobs {
    kDefault, kSplitKMin3000, kSplitKMax4096, kSplitKMax2_8192, kSplitKAoMax5000, kWideMinM0, kWideMinM4096, kWideMid0, kWideLn0,
    kWideLnSplitResid0, kNomicGateFused0, kQ8RowsUnits0, kQ8LnSlot1, kQ8Rows0, kQ8Rows1024, kQ8RowsSrc0, kQ8SkinnyMaxM0, kClsTail0,
    kClsTailMin1000, kStreamMinTokens5000,
    // the per-forward toggles
    kSmallPath0, kSmallFuse0, kQ8SkinnyLn0, kQ8LnFused0, kSmallForward1
};

static void set_knobs(Knobs k, ForwardKnobs& kn, ForwardToggles& tg) {
    switch (k) {
        case kDefault: break;
        case kSplitKMin3000: kn.split_k_min = 3000; break;
        case kSplitKMax4096: kn.split_k_max = 4096; break;
        case kSplitKMax2_8192: kn.split_k_max2 = 8192; break;
        case kSplitKAoMax5000: kn.split_k_ao_max = 5000; break;
        case kWideMinM0: kn.wide_min_m = 0; break;
        case kWideMinM4096: kn.wide_min_m = 4096; break;
        case kWideMid0: kn.mid192 = false; break;
        case kWideLn0: kn.ln_fuse = false; break;
        case kWideLnSplitResid0: kn.split_resid = false; break;
        case kNomicGateFused0: kn.gate_fused = false; break;
        case kQ8RowsUnits0: kn.q8_rows_units = false; break;
        case kQ8LnSlot1: kn.q8_ln_slot = true; break;
        case kQ8Rows0: kn.q8_rows_min_m = 0; break;
        case kQ8Rows1024: kn.q8_rows_min_m = 1024; break;
        case kQ8RowsSrc0: kn.q8_rows_src = false; break;
        case kQ8SkinnyMaxM0: kn.q8_skinny_max_m = 0; break;
        case kClsTail0: kn.cls_tail = false; break;
        case kClsTailMin1000: kn.cls_tail_min_tokens = 1000; break;
        case kStreamMinTokens5000: kn.stream_min_tokens = 5000; break;
        case kSmallPath0: tg.small_path = false; break;
        case kSmallFuse0: tg.small_fuse = false; break;
        case kQ8SkinnyLn0: tg.q8_skinny_ln = false; break;
        case kQ8LnFused0: tg.q8_ln_fused = false; break;
        case kSmallForward1: tg.small_forward = true; break;
    }
}

// arch, hidden, intermediate, heads
struct Model { uint32_t arch, hidden, intermediate, heads; };
enum Models { kBge, kBgeHeads6, kBgeOddI, kBgeTinyI, kBgeBase, kBgeBaseHeads8, kBgeLarge, kNomic, kJina, kJinaQk, kModern };
static const Model kModels[] = {
    {CS_ARCH_BERT, 384, 1536, 12},   // BGE-small, all-MiniLM-L6 (the quantised default model)
    {CS_ARCH_BERT, 384, 1536, 6},    // head_dim 64
    {CS_ARCH_BERT, 384, 1024, 12},   // I != 4 H
    {CS_ARCH_BERT, 384, 96, 12},     // an intermediate buffer too small for the CLS tail's compact rows at 16 tokens
    {CS_ARCH_BERT, 768, 3072, 12},   // BGE-base
    {CS_ARCH_BERT, 768, 3072, 8},    // head_dim 96
    {CS_ARCH_BERT, 1024, 4096, 16},  // BGE-large
    {CS_ARCH_NOMIC, 768, 3072, 12},
    {CS_ARCH_JINA, 768, 3072, 12},
    {CS_ARCH_JINA_QKNORM, 768, 3072, 12},
    {CS_ARCH_MODERN, 1024, 2688, 16},
};

constexpr int kSplit = CS_GEMM_SPLIT_F16, kF32 = CS_GEMM_F32, kQ8 = CS_GEMM_Q8_DYNAMIC;
constexpr int kCls = CS_POOL_CLS, kMean = CS_POOL_MEAN;
enum Flags { kNoWide = 1, kStageProfile = 2, kOneLaunch = 4, kSmallPairBuffers = 8 };

struct PlanCase {
    Knobs knobs;
    Models model;
    int mode, pooling;
    uint32_t nb, L;   // the slice: nb sequences of L positions
    uint32_t units;   // quantisation units of the mini-batch
    int streams;      // slices in flight
    uint32_t b0;      // the slice's first sequence
    int flags;
    const char* plan;
};

static const PlanCase kCases[] = {
    // the query side: under 200 token rows take the small path (b0 = 0, split-f16, a BERT family with I = 4 H) ...
    {kDefault, kBge, kSplit, kCls, 1, 16, 1, 1, 0, 0, "small attn_proj_fused"},
    {kDefault, kBge, kSplit, kCls, 9, 16, 1, 1, 0, 0, "small attn_proj_fused"},
    {kDefault, kBge, kSplit, kCls, 1, 199, 1, 1, 0, 0, "small"},
    {kDefault, kBge, kSplit, kCls, 1, 200, 1, 1, 0, 0, "split"},
    {kDefault, kBge, kSplit, kCls, 1, 16, 1, 1, 7, 0, "split"},
    {kDefault, kBge, kF32, kCls, 1, 16, 1, 1, 0, 0, "f32"},
    {kDefault, kNomic, kSplit, kMean, 1, 16, 1, 1, 0, 0, "split"},
    {kDefault, kBgeOddI, kSplit, kCls, 1, 16, 1, 1, 0, 0, "split"},
    {kSmallPath0, kBge, kSplit, kCls, 1, 16, 1, 1, 0, 0, "split"},
    // ... with attention inside the out-projection for sequences of up to 32 tokens of a 384-wide, 12-head model
    {kDefault, kBge, kSplit, kCls, 6, 32, 1, 1, 0, 0, "small attn_proj_fused"},
    {kDefault, kBge, kSplit, kCls, 6, 33, 1, 1, 0, 0, "small"},
    {kDefault, kBge, kSplit, kCls, 2, 64, 1, 1, 0, 0, "small"},
    {kDefault, kBgeBase, kSplit, kCls, 1, 16, 1, 1, 0, 0, "small"},
    {kDefault, kBgeHeads6, kSplit, kCls, 1, 16, 1, 1, 0, 0, "small"},
    {kSmallFuse0, kBge, kSplit, kCls, 1, 16, 1, 1, 0, 0, "small"},
    // ... and as ONE launch where the diagnostic build has it set up, it is asked for and no stage profile runs
    {kSmallForward1, kBge, kSplit, kCls, 1, 16, 1, 1, 0, kOneLaunch, "small-one-launch"},
    {kSmallForward1, kBge, kSplit, kCls, 1, 16, 1, 1, 0, 0, "small attn_proj_fused"},
    {kSmallForward1, kBge, kSplit, kCls, 1, 16, 1, 1, 0, kOneLaunch | kStageProfile, "small attn_proj_fused"},
    {kDefault, kBge, kSplit, kCls, 1, 16, 1, 1, 0, kOneLaunch, "small attn_proj_fused"},
    // N = 384 layers in K slices: out-proj in 3 from 1,101 to 2,560 rows, FFN-down in 3 up to 6,144 and in 2 up to 10,240
    {kDefault, kBge, kSplit, kCls, 1100, 1, 1, 1, 0, 0, "split"},
    {kDefault, kBge, kSplit, kCls, 1101, 1, 1, 1, 0, 0, "split ao_slices=3 down_slices=3"},
    {kDefault, kBge, kSplit, kCls, 2560, 1, 1, 1, 0, 0, "split ao_slices=3 down_slices=3"},
    {kDefault, kBge, kSplit, kCls, 2561, 1, 1, 1, 0, 0, "split down_slices=3"},
    {kDefault, kBge, kSplit, kCls, 6144, 1, 1, 1, 0, 0, "split up=w192 down_slices=3"},
    {kDefault, kBge, kSplit, kCls, 6145, 1, 1, 1, 0, 0, "split up=w192 down_slices=2"},
    {kDefault, kBge, kSplit, kCls, 10240, 1, 1, 1, 0, 0, "split qkv=w384 up=w384 down_slices=2"},
    {kDefault, kBge, kSplit, kCls, 10241, 1, 1, 1, 0, 0, "split qkv=w384 up=w384"},
    {kSplitKMin3000, kBge, kSplit, kCls, 2048, 1, 1, 1, 0, 0, "split"},
    {kSplitKMax4096, kBge, kSplit, kCls, 5000, 1, 1, 1, 0, 0, "split down_slices=2"},
    {kSplitKMax2_8192, kBge, kSplit, kCls, 10240, 1, 1, 1, 0, 0, "split qkv=w384 up=w384"},
    {kSplitKAoMax5000, kBge, kSplit, kCls, 4096, 1, 1, 1, 0, 0, "split ao_slices=3 down_slices=3"},
    // the reference's 32-chunk calls (8,192 rows): 128 x 192 tiles make QKV one round of blocks (384 tiles); FFN-up's 256 tiles of 128 x 384 pass the
    // 218-tile bar first; the N = 384 layers take neither (128 tiles of 128 x 192)
    {kDefault, kBge, kSplit, kMean, 32, 256, 1, 1, 0, 0, "split qkv=w192 up=w384 down_slices=2"},
    {kDefault, kBge, kSplit, kCls, 32, 256, 1, 1, 0, 0, "split qkv=w192 up=w384 down_slices=2 cls_tail"},
    {kWideMid0, kBge, kSplit, kMean, 32, 256, 1, 1, 0, 0, "split up=w384 down_slices=2"},
    {kDefault, kBge, kSplit, kMean, 32, 256, 1, 1, 0, kNoWide, "split down_slices=2"},
    // the 128 x 192 form takes 358 ... 512 tiles: N = 384 at 178 / 179 row tiles (22,784 / 22,785 rows) and, with the 128 x 384 kernel off,
    // at 256 / 257 row tiles (32,768 / 32,769 rows); never on two streams (32 x 256 as one slice of two: QKV's 384 tiles stay on gemm_split)
    {kDefault, kBge, kSplit, kMean, 22784, 1, 1, 1, 0, 0, "split qkv=w384 up=w384"},
    {kDefault, kBge, kSplit, kMean, 22785, 1, 1, 1, 0, 0, "split qkv=w384 ao=w192 up=w384 down=w192"},
    {kWideMinM0, kBge, kSplit, kMean, 32768, 1, 1, 1, 0, 0, "split ao=w192 down=w192"},
    {kWideMinM0, kBge, kSplit, kMean, 32769, 1, 1, 1, 0, 0, "split"},
    {kDefault, kBge, kSplit, kMean, 32, 256, 1, 2, 0, 0, "split up=w384 down_slices=2"},
    {kDefault, kBge, kSplit, kMean, 32, 256, 1, 2, 32, 0, "split up=w384 down_slices=2"},
    // one stream: the 128 x 384 kernel from 218 tiles on (N = 384: 217 tiles are 27,776 rows - and one round of 128 x 192 tiles)
    {kDefault, kBge, kSplit, kMean, 27776, 1, 1, 1, 0, 0, "split qkv=w384 ao=w192 up=w384 down=w192"},
    {kDefault, kBge, kSplit, kMean, 27777, 1, 1, 1, 0, 0, "split qkv=w384 up=w384 fuse_ln split_resid"},
    {kDefault, kBge, kSplit, kMean, 9216, 1, 1, 1, 0, 0, "split qkv=w192 up=w384 down_slices=2"},
    {kDefault, kBge, kSplit, kMean, 9344, 1, 1, 1, 0, 0, "split qkv=w384 up=w384 down_slices=2"},
    // two streams: from 12,288 rows of the slice on, and never the 128 x 192 form
    {kDefault, kBge, kSplit, kMean, 12287, 1, 1, 2, 0, 0, "split qkv=w384 up=w384"},
    {kDefault, kBge, kSplit, kMean, 12288, 1, 1, 2, 0, 0, "split qkv=w384 up=w384 fuse_ln split_resid"},
    {kDefault, kBge, kSplit, kMean, 48, 256, 1, 2, 48, 0, "split qkv=w384 up=w384 fuse_ln split_resid"},
    {kDefault, kBge, kSplit, kMean, 48, 256, 1, 1, 0, 0, "split qkv=w384 up=w384"},
    {kWideMinM4096, kBge, kSplit, kMean, 4096, 1, 1, 2, 0, 0, "split qkv=w384 up=w384 fuse_ln split_resid"},
    {kWideMinM0, kBge, kSplit, kMean, 256, 256, 1, 1, 0, 0, "split"},
    // indexing batches: 256 x 256 tokens on one stream, 160 x 256 as two slices of 80; the LayerNorm fusion and the split-only residual stream
    {kDefault, kBge, kSplit, kMean, 256, 256, 1, 1, 0, 0, "split qkv=w384 up=w384 fuse_ln split_resid"},
    {kDefault, kBge, kSplit, kMean, 80, 256, 1, 2, 80, 0, "split qkv=w384 up=w384 fuse_ln split_resid"},
    {kWideLn0, kBge, kSplit, kMean, 256, 256, 1, 1, 0, 0, "split qkv=w384 ao=w384 up=w384 down=w384"},
    {kWideLnSplitResid0, kBge, kSplit, kMean, 256, 256, 1, 1, 0, 0, "split qkv=w384 up=w384 fuse_ln"},
    {kDefault, kBge, kSplit, kMean, 256, 256, 1, 1, 0, kNoWide, "split"},
    {kDefault, kBge, kF32, kMean, 256, 256, 1, 1, 0, 0, "f32"},
    {kDefault, kBgeBase, kSplit, kMean, 128, 256, 1, 1, 0, 0, "split qkv=w384 ao=w384 up=w384 down=w384"},
    {kDefault, kBgeLarge, kSplit, kMean, 128, 256, 1, 1, 0, 0, "split qkv=w384"},
    // the CLS tail: CLS pooling, >= 4,096 tokens, sequences of 16 ... 512 tokens, head_dim 32 | 64, compact rows that fit the slice's intermediate
    // buffer ((L - 1) I >= 4 H: I = 96 at 16 / 17 tokens); its K|V product picks its own kernel
    {kDefault, kBge, kSplit, kCls, 195, 21, 1, 1, 0, 0, "split down_slices=3"},
    {kDefault, kBge, kSplit, kCls, 256, 16, 1, 1, 0, 0, "split down_slices=3 cls_tail"},
    {kDefault, kBge, kSplit, kCls, 274, 15, 1, 1, 0, 0, "split down_slices=3"},
    {kDefault, kBge, kSplit, kMean, 256, 16, 1, 1, 0, 0, "split down_slices=3"},
    {kDefault, kBge, kSplit, kCls, 256, 256, 1, 1, 0, 0, "split qkv=w384 kv_tail=w384 up=w384 fuse_ln split_resid cls_tail"},
    {kDefault, kBge, kSplit, kCls, 48, 256, 1, 1, 0, 0, "split qkv=w384 kv_tail=w192 up=w384 cls_tail"},
    {kDefault, kBgeHeads6, kSplit, kCls, 256, 16, 1, 1, 0, 0, "split down_slices=3 cls_tail"},
    {kDefault, kBgeBaseHeads8, kSplit, kCls, 256, 16, 1, 1, 0, 0, "split qkv=w192 up=w384 down_slices=3"},
    {kDefault, kBge, kSplit, kCls, 128, 512, 1, 1, 0, 0, "split qkv=w384 kv_tail=w384 up=w384 fuse_ln split_resid cls_tail"},
    {kDefault, kBge, kSplit, kCls, 8, 512, 1, 1, 0, 0, "split down_slices=3 cls_tail"},
    {kDefault, kBge, kSplit, kCls, 8, 513, 1, 1, 0, 0, "split down_slices=3"},
    {kDefault, kBgeTinyI, kSplit, kCls, 256, 16, 1, 1, 0, 0, "split down_slices=3"},
    {kDefault, kBgeTinyI, kSplit, kCls, 256, 17, 1, 1, 0, 0, "split down_slices=3 cls_tail"},
    {kClsTail0, kBge, kSplit, kCls, 256, 256, 1, 1, 0, 0, "split qkv=w384 up=w384 fuse_ln split_resid"},
    {kClsTailMin1000, kBge, kSplit, kCls, 64, 16, 1, 1, 0, 0, "split cls_tail"},
    // gated feed-forwards: the gate as FFN-up's epilogue wherever a wide kernel takes the [T, 2I] product
    {kDefault, kNomic, kSplit, kMean, 128, 256, 1, 1, 0, 0, "split qkv=w384 ao=w384 up=w384 down=w384 gate_epilogue"},
    {kDefault, kNomic, kSplit, kMean, 1536, 1, 1, 1, 0, 0, "split up=w192 ao_slices=3 down_slices=3 gate_epilogue"},
    {kDefault, kNomic, kSplit, kMean, 1024, 1, 1, 1, 0, 0, "split"},
    {kNomicGateFused0, kNomic, kSplit, kMean, 128, 256, 1, 1, 0, 0, "split qkv=w384 ao=w384 up=w384 down=w384"},
    {kDefault, kJina, kSplit, kMean, 64, 256, 1, 2, 0, 0, "split qkv=w384 ao=w384 up=w384 down=w384 gate_epilogue"},
    {kDefault, kJinaQk, kSplit, kCls, 128, 256, 1, 1, 0, 0, "split qkv=w384 ao=w384 up=w384 down=w384 gate_epilogue"},
    {kDefault, kNomic, kF32, kMean, 128, 256, 1, 1, 0, 0, "f32"},
    // ModernBERT: its own sequence in both modes (N = 1024 is no wide shape; the gate follows the kernel alone), the quantised mode refused
    {kDefault, kModern, kSplit, kMean, 64, 256, 1, 1, 0, 0, "modern qkv=w384 up=w384 gate_epilogue"},
    {kDefault, kModern, kSplit, kMean, 3, 40, 1, 1, 0, 0, "modern"},
    {kNomicGateFused0, kModern, kSplit, kMean, 64, 256, 1, 1, 0, 0, "modern qkv=w384 up=w384 gate_epilogue"},
    {kDefault, kModern, kSplit, kMean, 13, 128, 1, 1, 0, 0, "modern up=w192 gate_epilogue"},
    {kDefault, kModern, kF32, kMean, 64, 256, 1, 1, 0, 0, "modern"},
    {kDefault, kModern, kQ8, kMean, 64, 256, 1, 1, 0, 0, "refused"},
    {kDefault, kModern, kQ8, kMean, 1, 16, 1, 1, 0, 0, "refused"},
    // q8, a few rows: one launch per Linear up to 512 rows, both LayerNorms folded in up to 16 rows of a 384-wide model
    {kDefault, kBge, kQ8, kMean, 1, 16, 1, 1, 0, 0, "q8-few-rows fold_ln"},
    {kDefault, kBge, kQ8, kMean, 1, 17, 1, 1, 0, 0, "q8-few-rows"},
    {kQ8SkinnyLn0, kBge, kQ8, kMean, 1, 16, 1, 1, 0, 0, "q8-few-rows"},
    {kDefault, kBgeBase, kQ8, kMean, 1, 16, 1, 1, 0, 0, "q8-few-rows"},
    {kDefault, kBge, kQ8, kMean, 32, 16, 1, 1, 0, 0, "q8-few-rows"},
    {kDefault, kBge, kQ8, kMean, 513, 1, 1, 1, 0, 0, "q8-quantise"},
    {kDefault, kBge, kQ8, kMean, 32, 16, 3, 1, 0, 0, "q8-quantise"},
    {kDefault, kBge, kQ8, kMean, 32, 16, 1, 1, 0, kSmallPairBuffers, "q8-quantise"},
    {kQ8SkinnyMaxM0, kBge, kQ8, kMean, 1, 16, 1, 1, 0, 0, "q8-quantise"},
    {kDefault, kBgeLarge, kQ8, kMean, 1, 16, 1, 1, 0, 0, "q8-quantise"},
    // q8 from 4,096 rows of a 384-wide model: the row-block products quantise on load, out-proj and FFN-down carry their LayerNorm
    {kDefault, kBge, kQ8, kMean, 4095, 1, 1, 1, 0, 0, "q8-quantise"},
    {kDefault, kBge, kQ8, kMean, 256, 16, 1, 1, 0, 0, "q8-rows-source ln_fused_ao ln_fused_down"},
    {kDefault, kBge, kQ8, kMean, 256, 256, 1, 1, 0, 0, "q8-rows-source ln_fused_ao ln_fused_down"},
    {kQ8LnFused0, kBge, kQ8, kMean, 256, 16, 1, 1, 0, 0, "q8-rows-source"},
    {kQ8LnSlot1, kBge, kQ8, kMean, 256, 16, 1, 1, 0, 0, "q8-rows-source ln_fused_ao ln_fused_down ln_slot"},
    {kQ8RowsSrc0, kBge, kQ8, kMean, 256, 16, 1, 1, 0, 0, "q8-quantise"},
    {kQ8Rows0, kBge, kQ8, kMean, 256, 16, 1, 1, 0, 0, "q8-quantise"},
    {kQ8Rows1024, kBge, kQ8, kMean, 64, 16, 1, 1, 0, 0, "q8-rows-source ln_fused_ao ln_fused_down"},
    {kDefault, kBgeOddI, kQ8, kMean, 256, 16, 1, 1, 0, 0, "q8-rows-source ln_fused_ao"},
    {kDefault, kBgeBase, kQ8, kMean, 256, 16, 1, 1, 0, 0, "q8-quantise"},
    // q8, several units in the batch: ranges per unit on the row-block kernels from 4,096 rows, quantising passes below
    {kDefault, kBge, kQ8, kMean, 256, 16, 3, 1, 0, 0, "q8-multi-unit multi_unit"},
    {kDefault, kBge, kQ8, kMean, 255, 16, 3, 1, 0, 0, "q8-quantise"},
    {kQ8RowsUnits0, kBge, kQ8, kMean, 256, 16, 3, 1, 0, 0, "q8-quantise"},
    {kDefault, kBge, kQ8, kMean, 256, 16, 3, 1, 0, kSmallPairBuffers, "q8-quantise"},
    {kDefault, kBgeBase, kQ8, kMean, 256, 16, 3, 1, 0, 0, "q8-quantise"},
};

struct StreamCase {
    Knobs knobs;
    Models model;
    int mode;
    uint32_t B, L;    // the mini-batch
    int n_streams, forced;
    int flags, cus;
    uint32_t slices;
};

static const StreamCase kStreamCases[] = {
    // slices from 20,000 tokens on
    {kDefault, kBge, kSplit, 1249, 16, 2, 0, 0, 256, 1},
    {kDefault, kBge, kSplit, 1250, 16, 2, 0, 0, 256, 2},
    {kDefault, kBge, kSplit, 78, 256, 2, 0, 0, 256, 1},
    {kDefault, kBge, kSplit, 79, 256, 2, 0, 0, 256, 2},
    {kStreamMinTokens5000, kBge, kSplit, 32, 256, 2, 0, 0, 256, 2},
    {kDefault, kBge, kSplit, 1, 512, 2, 0, 0, 256, 1},
    // ... but one stream where every CU gets whole rounds of tiles (384-wide, wide kernels, >= 218 row tiles, >= 96 % full rounds at 1, 3 and 4 tiles per row tile: 266 CUs 0.962, 270 CUs 0.948)
    {kDefault, kBge, kSplit, 256, 256, 2, 0, 0, 256, 1},
    {kDefault, kBge, kSplit, 160, 256, 2, 0, 0, 256, 2},
    {kDefault, kBge, kSplit, 128, 512, 2, 0, 0, 256, 1},
    {kDefault, kBge, kSplit, 256, 256, 2, 0, 0, 266, 1},
    {kDefault, kBge, kSplit, 256, 256, 2, 0, 0, 270, 2},
    {kDefault, kBge, kSplit, 256, 256, 2, 0, 0, 304, 2},
    {kDefault, kBge, kSplit, 256, 256, 2, 0, 0, 0, 2},
    {kDefault, kBge, kSplit, 256, 256, 2, 0, kNoWide, 256, 2},
    {kDefault, kBge, kF32, 256, 256, 2, 0, 0, 256, 2},
    {kDefault, kBgeBase, kSplit, 256, 256, 2, 0, 0, 256, 2},
    // CS_ENCODER_STREAMS decides by itself; a quantised tensor is the whole mini-batch; the stage profile runs on one stream
    {kDefault, kBge, kSplit, 256, 256, 4, 1, 0, 256, 4},
    {kDefault, kBge, kSplit, 256, 256, 3, 1, 0, 256, 3},
    {kDefault, kBge, kSplit, 256, 256, 1, 1, 0, 256, 1},
    {kDefault, kBge, kSplit, 3, 512, 4, 1, 0, 256, 1},
    {kStreamMinTokens5000, kBge, kSplit, 3, 2048, 4, 1, 0, 256, 1},
    {kDefault, kBge, kQ8, 160, 256, 2, 0, 0, 256, 1},
    {kDefault, kBge, kSplit, 160, 256, 2, 0, kStageProfile, 256, 1},
};

static ForwardShape shape_of(Models model, int mode, int pooling, uint32_t nb, uint32_t L, uint32_t units, int streams, uint32_t b0, int flags) {
    const Model& m = kModels[model];
    ForwardShape s;
    s.arch = m.arch; s.hidden = m.hidden; s.intermediate = m.intermediate; s.heads = m.heads; s.layers = 12;
    s.pooling = pooling; s.mode = mode; s.nb = nb; s.L = L; s.b0 = b0; s.units = units; s.streams_in_flight = streams;
    s.wide_ok = !(flags & kNoWide);
    s.stage_profile = (flags & kStageProfile) != 0;
    s.small_forward_ok = (flags & kOneLaunch) != 0;
    const uint64_t tokens = (uint64_t)nb * L, att = (uint64_t)m.heads * 4 * (tokens / 128 + nb);  // (embedder_forward.hip reserve)
    s.cap_range_pairs = (flags & kSmallPairBuffers) ? 64 : (tokens + 1 > att ? tokens + 1 : att);
    s.cap_range_pairs2 = (flags & kSmallPairBuffers) ? 64 : (uint64_t)(m.intermediate / 16) * (tokens / 16 + 1);
    return s;
}

static const char* const kPathNames[] = {"modern", "small", "small-one-launch", "q8-few-rows", "q8-rows-source", "q8-multi-unit",
                                         "q8-quantise", "split", "f32", "refused"};
static const char* const kKernelNames[] = {"split", "w192", "w384"};

static std::string describe(const ForwardPlan& p) {
    std::string s = kPathNames[(int)p.path];
    auto kernel = [&](const char* name, DenseKernel k) { if (k != DenseKernel::Split) s += std::string(" ") + name + "=" + kKernelNames[(int)k]; };
    auto flag = [&](const char* name, bool v) { if (v) s += std::string(" ") + name; };
    auto count = [&](const char* name, unsigned v) { if (v) s += std::string(" ") + name + "=" + std::to_string(v); };
    kernel("qkv", p.qkv); kernel("kv_tail", p.kv_tail); kernel("ao", p.ao); kernel("up", p.up); kernel("down", p.down);
    flag("fuse_ln", p.fuse_ln); flag("split_resid", p.split_resid); count("ao_slices", p.ao_slices); count("down_slices", p.down_slices);
    flag("gate_epilogue", p.gate_epilogue); flag("cls_tail", p.cls_tail); flag("attn_proj_fused", p.attn_proj_fused);
    flag("fold_ln", p.fold_ln); flag("ln_fused_ao", p.ln_fused_ao); flag("ln_fused_down", p.ln_fused_down); flag("ln_slot", p.ln_slot);
    flag("multi_unit", p.multi_unit);
    return s;
}

int main() {
    int bad = 0;
    // what the cases reach: every path, both values of every boolean, every slice count, every dense kernel of every product
    unsigned paths = 0, bools[2] = {0, 0}, ao_slices = 0, down_slices = 0, kernels[5] = {0, 0, 0, 0, 0};
    for (const PlanCase& c : kCases) {
        ForwardKnobs kn;
        ForwardToggles tg;
        set_knobs(c.knobs, kn, tg);
        const ForwardPlan p = plan_forward(kn, tg, shape_of(c.model, c.mode, c.pooling, c.nb, c.L, c.units, c.streams, c.b0, c.flags));
        const std::string got = describe(p);
        if (got != c.plan) {
            std::printf("FAIL knobs %d model %d mode %d pooling %d, %u x %u tokens, %u units, %d streams, b0 %u, flags %d: got \"%s\", recorded \"%s\"\n",
                        (int)c.knobs, (int)c.model, c.mode, c.pooling, c.nb, c.L, c.units, c.streams, c.b0, c.flags, got.c_str(), c.plan);
            ++bad;
        }
        paths |= 1u << (int)p.path;
        const bool b[] = {p.fuse_ln, p.split_resid, p.gate_epilogue, p.cls_tail, p.attn_proj_fused, p.fold_ln, p.ln_fused_ao, p.ln_fused_down,
                          p.ln_slot, p.multi_unit};
        for (unsigned i = 0; i < sizeof b / sizeof b[0]; ++i) bools[b[i]] |= 1u << i;
        ao_slices |= 1u << p.ao_slices;
        down_slices |= 1u << p.down_slices;
        const DenseKernel k[] = {p.qkv, p.kv_tail, p.ao, p.up, p.down};
        for (int i = 0; i < 5; ++i) kernels[i] |= 1u << (int)k[i];
    }
    if (paths != (1u << 10) - 1) { std::printf("FAIL the cases do not reach every path (%#x)\n", paths); ++bad; }
    if (bools[0] != (1u << 10) - 1 || bools[1] != (1u << 10) - 1) { std::printf("FAIL a boolean of the plan keeps one value (%#x, %#x)\n", bools[0], bools[1]); ++bad; }
    if (ao_slices != (1u << 0 | 1u << 3) || down_slices != (1u << 0 | 1u << 2 | 1u << 3)) { std::printf("FAIL slice counts %#x, %#x\n", ao_slices, down_slices); ++bad; }
    for (int i = 0; i < 5; ++i)
        if (kernels[i] != 7) { std::printf("FAIL dense layer %d does not reach every kernel (%#x)\n", i, kernels[i]); ++bad; }
    for (const StreamCase& c : kStreamCases) {
        ForwardKnobs kn;
        ForwardToggles tg;
        set_knobs(c.knobs, kn, tg);
        ForwardShape s = shape_of(c.model, c.mode, kMean, c.B, c.L, 1, 1, 0, c.flags);
        s.n_streams = c.n_streams; s.streams_forced = c.forced != 0; s.cus = c.cus;
        const uint32_t got = plan_streams(kn, s);
        if (got != c.slices) {
            std::printf("FAIL knobs %d model %d mode %d, %u x %u tokens, %d streams (forced %d), flags %d, %d CUs: %u slices, recorded %u\n", (int)c.knobs,
                        (int)c.model, c.mode, c.B, c.L, c.n_streams, c.forced, c.flags, c.cus, got, c.slices);
            ++bad;
        }
    }
    if (bad) return 1;
    std::printf("forward plan ok: %zu plans, %zu slicings\n", sizeof kCases / sizeof kCases[0], sizeof kStreamCases / sizeof kStreamCases[0]);
    return 0;
}
