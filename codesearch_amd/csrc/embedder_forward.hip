// embedder_forward.hip — one mini-batch through the encoder kernels: workspace, the launch sequence of every path the plan
// names (forward_plan.hpp: forward_range plans a slice, then runs that path's function), stream slicing (forward).
// (one of the translation units behind cs_embedder_*: see embedder_state.hpp)
#include "embedder_state.hpp"

using namespace cs;

namespace cs {
namespace emb {

size_t mid_width(const cs_bert_config& c) { return (size_t)c.intermediate * (cs_arch_gated(c.arch) ? 3 : 1); }

void free_workspace(cs_embedder* h) {
    if (h->d_ids) (void)hipFree(h->d_ids);
    if (h->d_mask) (void)hipFree(h->d_mask);
    if (h->d_types) (void)hipFree(h->d_types);
    if (h->d_x) (void)hipFree(h->d_x);
    if (h->d_xs) (void)hipFree(h->d_xs);
    if (h->d_qkv) (void)hipFree(h->d_qkv);
    if (h->d_ctx) (void)hipFree(h->d_ctx);
    if (h->d_mid) (void)hipFree(h->d_mid);
    if (h->d_pooled) (void)hipFree(h->d_pooled);
    if (h->d_perm) (void)hipFree(h->d_perm);
    if (h->d_rmeta) (void)hipFree(h->d_rmeta);
    if (h->d_rmeta2) (void)hipFree(h->d_rmeta2);
    if (h->d_range_pairs) (void)hipFree(h->d_range_pairs);
    if (h->d_seq_unit) (void)hipFree(h->d_seq_unit);
    if (h->d_unit_len) (void)hipFree(h->d_unit_len);
    if (h->d_row_slot) (void)hipFree(h->d_row_slot);
    if (h->d_range) (void)hipFree(h->d_range);
    h->d_rmeta = h->d_rmeta2 = nullptr;
    h->d_range_pairs = nullptr;
    h->d_seq_unit = h->d_unit_len = h->d_row_slot = h->d_range = nullptr;
    h->d_perm = nullptr;
    h->d_ids = h->d_mask = h->d_types = nullptr;
    h->cap_types = 0;
    h->d_x = h->d_xs = h->d_qkv = h->d_ctx = h->d_mid = h->d_pooled = nullptr;
    h->cap_tokens = h->cap_seqs = 0;
}

int32_t reserve(cs_embedder* h, size_t seqs, size_t tokens) {
    if (tokens <= h->cap_tokens && seqs <= h->cap_seqs) return CS_OK;
    free_workspace(h);
    const size_t H = h->cfg.hidden, I = h->cfg.intermediate;
    CS_HIP(hipMalloc(&h->d_ids, tokens * sizeof(int32_t)));
    CS_HIP(hipMalloc(&h->d_mask, tokens * sizeof(int32_t)));
    CS_HIP(hipMalloc(&h->d_x, tokens * H * sizeof(float)));
    CS_HIP(hipMalloc(&h->d_xs, tokens * H * sizeof(float)));
    CS_HIP(hipMalloc(&h->d_qkv, tokens * 3 * H * sizeof(float)));
    CS_HIP(hipMalloc(&h->d_ctx, tokens * H * sizeof(float)));
    CS_HIP(hipMalloc(&h->d_mid, tokens * mid_width(h->cfg) * sizeof(float)));
    CS_HIP(hipMalloc(&h->d_pooled, seqs * H * sizeof(float)));
    CS_HIP(hipMalloc(&h->d_perm, seqs * sizeof(uint32_t)));
    if (h->quantized) {
        CS_HIP(hipMalloc(&h->d_rmeta, tokens * sizeof(Q8RowMeta)));
        CS_HIP(hipMalloc(&h->d_rmeta2, tokens * sizeof(Q8RowMeta)));
        // LayerNorm: a pair per four rows (per row with several units in the batch); attention: four per (head group,
        // sequence, 128 queries)
        h->cap_range_pairs = std::max<size_t>(tokens + 1, (size_t)h->cfg.heads * 4 * (tokens / 128 + seqs));
        // (+ a second set for the few-rows path: FFN-up leaves a pair per 16 x 16 output tile while it reads the first set)
        h->cap_range_pairs2 = (size_t)(I / 16) * (tokens / 16 + 1);
        CS_HIP(hipMalloc(&h->d_range_pairs, (h->cap_range_pairs + h->cap_range_pairs2) * 2 * sizeof(float)));
        CS_HIP(hipMalloc(&h->d_seq_unit, seqs * sizeof(uint32_t)));
        CS_HIP(hipMalloc(&h->d_unit_len, seqs * sizeof(uint32_t)));
        CS_HIP(hipMalloc(&h->d_row_slot, tokens * sizeof(uint32_t)));
        // a range slot per (layer, quantised tensor, unit): at most one unit per sequence
        h->q8_units = (uint32_t)seqs;
        CS_HIP(hipMalloc(&h->d_range, (size_t)h->cfg.layers * 4 * Q8_RANGE_WORDS * h->q8_units * sizeof(uint32_t)));
    }
    h->cap_tokens = tokens;
    h->cap_seqs = seqs;
    return CS_OK;
}

SplitLayer split_layer(const cs_bert_config& c) {
    const size_t H = c.hidden, I = c.intermediate;
    SplitLayer o;
    o.qkv = 0;
    o.ao = o.qkv + 3 * H * H * 2;
    o.up = o.ao + H * H * 2;
    o.down = o.up + (cs_arch_gated(c.arch) ? 2 : 1) * I * H * 2;
    o.total = o.down + H * I * 2;
    return o;
}

}  // namespace emb

// Every threshold of the route, each name read the way it always was: laboratory knobs through cs_lab_env (the diagnostic
// library only), a deployment's through std::getenv.  The defaults are ForwardKnobs' own.
static ForwardKnobs forward_knobs_from_env() {
    ForwardKnobs kn;
    auto on = [](const char* e) { return !(e && e[0] == '0'); };
    if (const char* e = cs_lab_env("CS_GEMM_SPLITK_MIN_M")) kn.split_k_min = (uint32_t)std::atoi(e);
    if (const char* e = cs_lab_env("CS_GEMM_SPLITK_MAX_M")) kn.split_k_max = (uint32_t)std::atoi(e);
    if (const char* e = cs_lab_env("CS_GEMM_SPLITK_MAX2_M")) kn.split_k_max2 = (uint32_t)std::atoi(e);
    if (const char* e = cs_lab_env("CS_GEMM_SPLITK_AO_MAX_M")) kn.split_k_ao_max = (uint32_t)std::atoi(e);
    if (const char* e = cs_lab_env("CS_GEMM_WIDE_MIN_M")) kn.wide_min_m = (uint32_t)std::atoll(e);
    kn.mid192 = on(cs_lab_env("CS_GEMM_WIDE_MID"));
    kn.ln_fuse = on(cs_lab_env("CS_GEMM_WIDE_LN"));
    kn.split_resid = on(cs_lab_env("CS_GEMM_WIDE_LN_SPLIT_RESID"));
    kn.gate_fused = on(cs_lab_env("CS_NOMIC_GATE_FUSED"));
    kn.q8_rows_units = on(cs_lab_env("CS_Q8_ROWS_UNITS"));
    if (const char* e = cs_lab_env("CS_Q8_LN_SLOT")) kn.q8_ln_slot = e[0] == '1';
    if (const char* e = cs_lab_env("CS_Q8_ROWS")) kn.q8_rows_min_m = std::atoi(e);
    kn.q8_rows_src = on(cs_lab_env("CS_Q8_ROWS_SRC"));
    if (const char* e = cs_lab_env("CS_Q8_SKINNY_MAX_M")) kn.q8_skinny_max_m = (uint32_t)std::atoll(e);
    kn.cls_tail = on(std::getenv("CS_ENCODER_CLS_TAIL"));
    if (const char* e = std::getenv("CS_ENCODER_CLS_TAIL_MIN_TOKENS")) kn.cls_tail_min_tokens = (uint32_t)std::atoll(e);
    if (const char* e = cs_lab_env("CS_ENCODER_STREAM_MIN_TOKENS")) kn.stream_min_tokens = (uint64_t)std::atoll(e);
    return kn;
}
const ForwardKnobs& forward_knobs() {
    static const ForwardKnobs kn = forward_knobs_from_env();
    return kn;
}

namespace emb {
namespace {

// (read per forward: tests and A/B runs flip them mid-process)
ForwardToggles forward_toggles_from_env() {
    ForwardToggles tg;
    auto on = [](const char* e) { return !(e && e[0] == '0'); };
    tg.small_path = on(std::getenv("CS_SMALL_PATH"));
    tg.small_fuse = on(std::getenv("CS_SMALL_FUSE"));
    tg.q8_skinny_ln = on(std::getenv("CS_Q8_SKINNY_LN"));
    tg.q8_ln_fused = on(cs_lab_env("CS_Q8_LN_FUSED"));
    if (const char* e = cs_lab_env("CS_SMALL_FORWARD")) tg.small_forward = e[0] == '1';
    return tg;
}

ForwardShape shape_of(const cs_embedder* h, uint32_t b0, uint32_t nb, uint32_t L, int mode) {
    const cs_bert_config& c = h->cfg;
    ForwardShape s;
    s.arch = c.arch; s.hidden = c.hidden; s.intermediate = c.intermediate; s.heads = c.heads; s.layers = c.layers;
    s.pooling = c.pooling; s.mode = mode;
    s.nb = nb; s.L = L; s.b0 = b0; s.units = h->cur_units;
    s.streams_in_flight = h->streams_in_flight; s.n_streams = h->n_streams; s.streams_forced = h->streams_forced;
    s.wide_ok = h->wide_ok;
    s.cap_range_pairs = h->cap_range_pairs; s.cap_range_pairs2 = h->cap_range_pairs2;
    s.stage_profile = h->stage_profile;
    s.cus = h->cus;
    return s;
}

// What a layer of a quantised model launches with: its weights, column metadata and range slots (Slice::q8_layer_begin)
struct Q8LayerArgs {
    Q8Layer ql;
    const int8_t *wq, *wst;  // wst: (out-proj | FFN-down, stage-major)
    const Q8ColMeta* cm;
    const uint32_t* cmt;     // (slab kernel)
    uint32_t U, ln_pairs;
    uint32_t* rg;
    size_t rstep;
    // several units in the batch: every row carries its unit's slot, ranges come from passes over the tensors
    // (the producers' per-block ranges and the two-pass FFN-up assume one unit)
    const uint32_t* rs;
    int8_t* xq;              // [T][<= 4H] bytes
    Q8RowMeta* rm;
    float* rp;
};

// Sequences [b0, b0 + nb) of the mini-batch on stream s: the buffers at the slice's token offset, the row kernels' arguments
// and the stage profile's marks.  One run_* function per ForwardPath: each reads the plan and decides nothing.
struct Slice {
    cs_embedder* h;
    const cs_bert_config& cfg;
    hipStream_t s;
    uint32_t b0, nb, L, T, H, I;
    int mode;
    size_t t0;
    const float* P;
    float *x, *qkv, *ctx, *mid;
    const int32_t* mask;
    _Float16 *xs, *qkvs, *ctxs, *mids;  // the same buffers in split form ([T][3H/32][64] f16: same bytes as the f32 qkv)
    SplitLayer sl;
    EncoderLaunch a;
    // the layer being launched (layer_begin): its parameter offsets and its packed QKV bias
    cs_bert_layer_offsets lo;
    const float* bqkv;

    Slice(cs_embedder* h_, hipStream_t s_, uint32_t b0_, uint32_t nb_, uint32_t L_, int mode_, const ForwardPlan& p)
        : h(h_), cfg(h_->cfg), s(s_), b0(b0_), nb(nb_), L(L_), T(nb_ * L_), H(cfg.hidden), I(cfg.intermediate), mode(mode_),
          t0((size_t)b0_ * L_), P(h_->d_params), sl(split_layer(cfg)) {
        x = h->d_x + t0 * H;
        qkv = h->d_qkv + t0 * 3 * H;
        ctx = h->d_ctx + t0 * H;
        mid = h->d_mid + t0 * mid_width(cfg);
        mask = h->d_mask + t0;
        xs = reinterpret_cast<_Float16*>(h->d_xs + t0 * H);
        qkvs = reinterpret_cast<_Float16*>(qkv);
        ctxs = reinterpret_cast<_Float16*>(ctx);
        mids = reinterpret_cast<_Float16*>(mid);
        a.ids = h->d_ids + t0; a.mask = mask;
        a.word = P + h->off.word; a.pos = cs_arch_gated(cfg.arch) ? nullptr : P + h->off.pos; a.type0 = P + h->off.type;
        a.types = h->types_on ? h->d_types + t0 : nullptr; a.ntypes = cfg.type_vocab_size;
        a.g = P + h->off.emb_ln_g; a.b = P + h->off.emb_ln_b;
        a.eps = cfg.layer_norm_eps; a.T = T; a.L = L; a.B = nb; a.vocab = cfg.vocab_size;
        a.pooling = cfg.pooling; a.x = x; a.out = (h->pooled_dst ? h->pooled_dst : h->d_pooled) + (size_t)b0 * out_width(h);
        a.xs = mode == CS_GEMM_SPLIT_F16 ? (void*)(h->d_xs + t0 * H) : nullptr;  // q8: the xs buffer holds the quantised rows instead
        a.flag = h->d_flag;
        if (mode == CS_GEMM_Q8_DYNAMIC) a.range_out = h->d_range_pairs;  // LayerNorm leaves its blocks' ranges for the quantising pass that follows
        a.range_rows = p.multi_unit;
    }

    // stage profile: an event after each kernel (only on the one-stream path, see forward())
    int32_t mark(int tag) const {
        if (!h->stage_profile) return CS_OK;
        const size_t i = h->stage_tag.size() + 1;
        while (h->stage_ev.size() <= i) {
            hipEvent_t e;
            CS_HIP(hipEventCreate(&e));
            h->stage_ev.push_back(e);
        }
        if (tag < 0) { CS_HIP(hipEventRecord(h->stage_ev[0], s)); return CS_OK; }
        CS_HIP(hipEventRecord(h->stage_ev[i], s));
        h->stage_tag.push_back(tag);
        return CS_OK;
    }
    // a dense layer on the kernel the plan names
    int32_t dense(DenseKernel k, int epi, const _Float16* Ain, const _Float16* Wt, const float* bias, const float* resid, float* Cf,
                  _Float16* Csp, uint32_t Mr, uint32_t Nn, uint32_t Kk) const {
        if (k == DenseKernel::Wide384) return launch_gemm_wide(epi, Ain, Wt, bias, resid, Cf, Csp, Mr, Nn, Kk, h->d_flag, s);
        if (k == DenseKernel::Wide192) return launch_gemm_wide(epi, Ain, Wt, bias, resid, Cf, Csp, Mr, Nn, Kk, h->d_flag, s, 192);
        return launch_gemm_split(epi, Ain, Wt, bias, resid, Cf, Csp, Mr, Nn, Kk, h->d_flag, s);
    }
    int32_t embed() const {  // E1
        CS_TRY(mark(-1));
        CS_TRY(launch_row_kernel(0, a, H, s));
        return mark(CS_STAGE_EMBED_LN);
    }
    int32_t layer_norm(uint64_t g, uint64_t b) {  // of x, in place, with the parameters at these offsets
        a.g = P + g; a.b = P + b;
        return launch_row_kernel(1, a, H, s);
    }
    // the forward's last launch over the rows `e` describes: E7 + E8, or the score head on the CLS rows (rerank_head.hip)
    int32_t out_stage(const EncoderLaunch& e) const {
        if (h->head_on) return launch_rerank_head(e.x, (size_t)e.L * H, h->d_head, e.B, H, e.out, s);
        return launch_row_kernel(2, e, H, s);
    }
    int32_t pool() const {
        CS_TRY(out_stage(a));
        return mark(CS_STAGE_POOL);
    }
    void layer_begin(uint32_t l) {
        cs_bert_layer_layout(&cfg, &h->off, l, &lo);
        bqkv = h->d_bqkv + (size_t)l * 3 * H;
    }
    Q8LayerArgs q8_layer_begin(uint32_t l);
    int32_t run_modern(const ForwardPlan& p);
    int32_t run_small(const ForwardPlan& p);
    int32_t run_q8_few_rows(const ForwardPlan& p);
    int32_t run_q8_rows_source(const ForwardPlan& p);
    int32_t run_q8_multi_unit();
    int32_t run_q8_quantise();
    int32_t run_cls_tail(const ForwardPlan& p, const _Float16* ws);
    int32_t run_split(const ForwardPlan& p);
    int32_t run_f32();
};

// ---- ModernBERT (CS_ARCH_MODERN): pre-norm layers -----------------------------------------------------------------------------
// x is the residual stream and is only ever added to: x += Wo attention(rope(Wqkv LN_attn(x))) (layer 0 takes the embedding
// LayerNorm's output as it is); x += Wo_mlp(gelu(Wi_a LN_mlp(x)) * Wi_b LN_mlp(x)); a final LayerNorm in front of the
// pooling.  The LayerNorm outputs go to the context buffer (f32, free at both points) and to xs in split form; the rotary
// table and the attention window follow the layer's type (global every `global_every`-th layer, local otherwise); the
// gate is the up projection's epilogue at indexing sizes (GW_OUT_GEGLU, as for JinaBert: value = the half of Wi that is
// not activated).  The same kernels as every other family; exact-f32 mode included.
int32_t Slice::run_modern(const ForwardPlan& p) {
    const bool split = mode == CS_GEMM_SPLIT_F16;
    if (a.types) return fail(CS_ERR_UNSUPPORTED, "the ModernBERT encoder has no token-type table: token-type ids cannot be given");
    a.pos = nullptr; a.type0 = h->d_zero_row;
    CS_TRY(embed());  // E1 (its split copy is layer 0's operand: attn_norm is the identity there)
    EncoderLaunch n = a;   // LayerNorm of the residual stream into the context buffer (+ xs)
    n.src = x; n.x = ctx;
    for (uint32_t l = 0; l < cfg.layers; ++l) {
        layer_begin(l);
        const bool global = cfg.global_every == 0 || l % cfg.global_every == 0;
        const float2* rope = global ? h->d_rope : h->d_rope_local;
        const uint32_t window = global ? 0u : cfg.local_window;
        if (l) {
            n.g = P + lo.ao_ln_g; n.b = P + lo.ao_ln_b;
            CS_TRY(launch_row_kernel(4, n, H, s));  // attn_norm
        }
        if (split) {
            const _Float16* ws = h->d_wsplit + (size_t)l * sl.total;
            CS_TRY(dense(p.qkv, SH_OUT_SPLIT, xs, ws + sl.qkv, bqkv, nullptr, nullptr, qkvs, T, 3 * H, H));  // E2
            CS_TRY(launch_rope_split(qkvs, rope, T, L, H, cfg.heads, h->d_flag, s));
            CS_TRY(mark(CS_STAGE_QKV));
            CS_TRY(launch_attention_sh2(qkvs, mask, ctxs, h->d_flag, nb, L, H, cfg.heads, s, nullptr, nullptr, nullptr, nullptr, nullptr, window));  // E3
            CS_TRY(mark(CS_STAGE_ATTENTION));
            CS_TRY(dense(p.ao, SH_OUT_F32_RESID, ctxs, ws + sl.ao, P + lo.ao_b, x, x, nullptr, T, H, H));  // E4: x += Wo ctx
            CS_TRY(mark(CS_STAGE_OUT_PROJ));
            n.g = P + lo.out_ln_g; n.b = P + lo.out_ln_b;
            CS_TRY(launch_row_kernel(4, n, H, s));  // mlp_norm
            CS_TRY(mark(CS_STAGE_LN_ATTN));
            _Float16* gated = reinterpret_cast<_Float16*>(mid + (size_t)T * 2 * I);
            const float* bup = h->d_bup + (size_t)l * 2 * I;
            if (p.gate_epilogue) {
                CS_TRY(launch_gemm_wide(GW_OUT_GEGLU, xs, ws + sl.up, bup, nullptr, nullptr, gated, T, 2 * I, H, h->d_flag, s, p.up == DenseKernel::Wide192 ? 192 : 0));
            } else {
                CS_TRY(dense(p.up, SH_OUT_SPLIT, xs, ws + sl.up, bup, nullptr, nullptr, mids, T, 2 * I, H));
                CS_TRY(launch_swiglu_split(mids, gated, T, I, h->d_flag, s, true));
            }
            CS_TRY(mark(CS_STAGE_FFN_UP));
            CS_TRY(dense(p.down, SH_OUT_F32_RESID, gated, ws + sl.down, P + lo.down_b, x, x, nullptr, T, H, I));  // E6: x += Wo_mlp(...)
            CS_TRY(mark(CS_STAGE_FFN_DOWN));
        } else {
            const float* nin = l ? ctx : x;  // layer 0: the embedding LayerNorm's output itself
            const float* wqkv = h->d_wqkv + (size_t)l * 3 * H * H;
            CS_TRY(launch_gemm(GEMM_BIAS, nin, wqkv, bqkv, nullptr, qkv, T, 3 * H, H, s));
            CS_TRY(launch_rope_f32(qkv, rope, T, L, H, cfg.heads, s));
            CS_TRY(mark(CS_STAGE_QKV));
            CS_TRY(launch_attention(qkv, mask, ctx, nb, L, H, cfg.heads, s, nullptr, window));
            CS_TRY(mark(CS_STAGE_ATTENTION));
            CS_TRY(launch_gemm(GEMM_RESID, ctx, P + lo.ao_w, P + lo.ao_b, x, x, T, H, H, s));
            CS_TRY(mark(CS_STAGE_OUT_PROJ));
            n.g = P + lo.out_ln_g; n.b = P + lo.out_ln_b;
            CS_TRY(launch_row_kernel(4, n, H, s));
            CS_TRY(mark(CS_STAGE_LN_ATTN));
            float* gate = mid + (size_t)T * I;
            CS_TRY(launch_gemm(GEMM_BIAS, ctx, P + lo.up_w, P + lo.up_b, nullptr, mid, T, I, H, s));
            CS_TRY(launch_gemm(GEMM_BIAS, ctx, P + lo.gate_w, P + lo.gate_b, nullptr, gate, T, I, H, s));
            CS_TRY(launch_swiglu_f32(mid, gate, T, I, s, true));
            CS_TRY(mark(CS_STAGE_FFN_UP));
            CS_TRY(launch_gemm(GEMM_RESID, mid, P + lo.down_w, P + lo.down_b, x, x, T, H, I, s));
            CS_TRY(mark(CS_STAGE_FFN_DOWN));
        }
    }
    a.g = P + h->off.final_ln_g; a.b = P + h->off.final_ln_b; a.xs = nullptr;
    CS_TRY(launch_row_kernel(1, a, H, s));  // final_norm, in place
    CS_TRY(mark(CS_STAGE_LN_FFN));
    h->last_hidden_partial = false;
    return pool();
}

// ---- a few short sequences (under 200 token rows: the query side; small_path.hip) ----
// LayerNorm as the prologue of the dense layer that reads it, FFN-down as four K slices summed by the LayerNorm that
// follows; ForwardPath::SmallOneLaunch: the same arithmetic as ONE launch (small_forward.hip, diagnostic library).
int32_t Slice::run_small(const ForwardPlan& p) {
    if (!h->d_sp_ws) CS_HIP(hipMalloc(&h->d_sp_ws, (size_t)5 * SP_MAX_ROWS * H * sizeof(float)));
    float* parts = h->d_sp_ws;                                   // [4][T][H]
    float* xa = h->d_sp_ws + (size_t)4 * SP_MAX_ROWS * H;        // [T][H]
    float* y = h->d_xs + t0 * H;                                 // [T][H] (the split copy of x is not used on this path)
#ifdef CS_DIAGNOSTICS
    if (p.path == ForwardPath::SmallOneLaunch) {
        uint32_t hb = L <= 32 ? 4u : (L <= 64 ? 2u : 1u);  // heads per attention block, as launch_attention_sh2 packs them
        if (const char* ph = cs_lab_env("CS_ATTN_PACK_HEADS")) if (ph[0] == '0') hb = 1;
        while (cfg.heads % hb) hb >>= 1;
        SfArgs sa{};
        sa.ids = a.ids; sa.mask = mask; sa.word = a.word; sa.pos = a.pos; sa.type0 = a.type0; sa.types = a.types; sa.ntypes = a.ntypes; sa.emb_g = a.g; sa.emb_b = a.b;
        sa.layers = h->d_sf_layers; sa.n_layers = cfg.layers; sa.eps = cfg.layer_norm_eps;
        sa.T = T; sa.L = L; sa.B = nb; sa.vocab = cfg.vocab_size; sa.heads = cfg.heads; sa.hb = hb;
        sa.X = x; sa.XA = xa; sa.Y = y; sa.PARTS = parts; sa.QKVS = qkvs; sa.CTXS = ctxs;
        sa.MIDS = mids; sa.flag = h->d_flag; sa.sync = h->d_sf_sync;
        sa.dbg = h->d_sf_dbg;
        CS_HIP(hipMemsetAsync(h->d_sf_sync, 0, 16, s));
        CS_TRY(launch_small_forward(sa, s));
        h->sf_ran = true;
        h->last_hidden_partial = false;
        CS_TRY(out_stage(a));  // E7 + E8
        return CS_OK;
    }
#endif
    CS_TRY(mark(-1));
    for (uint32_t l = 0; l < cfg.layers; ++l) {
        cs_bert_layer_offsets lp;
        layer_begin(l);
        if (l) cs_bert_layer_layout(&cfg, &h->off, l - 1, &lp);
        const _Float16* ws = h->d_wsplit + (size_t)l * sl.total;
        SpLnGemmArgs g1{};
        g1.Y = y; g1.parts = parts; g1.parts_bias = l ? P + lp.down_b : nullptr; g1.X = x;
        g1.ids = a.ids; g1.word = a.word; g1.pos = a.pos; g1.type0 = a.type0; g1.types = a.types; g1.ntypes = a.ntypes; g1.L = L; g1.vocab = cfg.vocab_size;
        g1.ln_g = l ? P + lp.out_ln_g : a.g; g1.ln_b = l ? P + lp.out_ln_b : a.b; g1.eps = cfg.layer_norm_eps;
        g1.Xout = xa; g1.W = ws + sl.qkv; g1.bias = bqkv; g1.Cs = qkvs; g1.T = T; g1.N = 3 * H; g1.flag = h->d_flag;
        CS_TRY(launch_sp_ln_gemm(SH_OUT_SPLIT, l ? 1 : 2, g1, H, s));                                        // (E1 | LN) + E2
        CS_TRY(mark(CS_STAGE_QKV));
        if (p.attn_proj_fused) {  // E3 + E4 -> y in one launch: every out-projection block computes its rows' attention itself (small_path.hip)
            CS_TRY(mark(CS_STAGE_ATTENTION));
            CS_TRY(launch_sp_attn_proj(qkvs, mask, ws + sl.ao, P + lo.ao_b, xa, y, T, L, H, cfg.heads, h->d_flag, s));
        } else {
            CS_TRY(launch_attention_sh2(qkvs, mask, ctxs, h->d_flag, nb, L, H, cfg.heads, s));                      // E3
            CS_TRY(mark(CS_STAGE_ATTENTION));
            CS_TRY(launch_gemm_split(SH_OUT_F32_RESID, ctxs, ws + sl.ao, P + lo.ao_b, xa, y, nullptr, T, H, H, h->d_flag, s));  // E4 -> y
        }
        CS_TRY(mark(CS_STAGE_OUT_PROJ));
        SpLnGemmArgs g4 = g1;
        g4.ln_g = P + lo.ao_ln_g; g4.ln_b = P + lo.ao_ln_b; g4.Xout = x; g4.W = ws + sl.up; g4.bias = P + lo.up_b; g4.Cs = mids; g4.N = I;
        CS_TRY(launch_sp_ln_gemm(SH_OUT_SPLIT_GELU, 0, g4, H, s));                                           // LN + E5
        CS_TRY(mark(CS_STAGE_FFN_UP));
        CS_TRY(launch_sp_partial(mids, ws + sl.down, parts, T, H, H, s));                                  // E6, four K slices
        CS_TRY(mark(CS_STAGE_FFN_DOWN));
    }
    cs_bert_layer_offsets ll;
    cs_bert_layer_layout(&cfg, &h->off, cfg.layers - 1, &ll);
    a.parts = parts; a.nparts = 4; a.bias = P + ll.down_b; a.g = P + ll.out_ln_g; a.b = P + ll.out_ln_b;
    a.xs = nullptr;
    CS_TRY(launch_row_kernel(3, a, H, s));  // the last LayerNorm: (slabs + bias) + x -> x
    CS_TRY(mark(CS_STAGE_LN_FFN));
    h->last_hidden_partial = false;
    return pool();
}

// ---- dynamically quantised models ----
// Every Linear as the quantised file's graph runs it: DynamicQuantizeLinear of its input (one range per
// call tensor), MatMulInteger on the int8 MFMA, * (x_scale * W_scale), + bias (gemm_q8.hip)
Q8LayerArgs Slice::q8_layer_begin(uint32_t l) {
    layer_begin(l);
    Q8LayerArgs q;
    q.ql = q8_layer(H, I);
    q.wq = h->d_wq8 + (size_t)l * q.ql.total;
    q.cm = h->d_cmeta + (size_t)l * (5 * (size_t)H + I);
    q.wst = h->d_wq8_stages ? h->d_wq8_stages + (size_t)l * ((size_t)H * H + (size_t)H * I) : nullptr;
    q.cmt = (H % 128 == 0 && I % 128 == 0) ? h->d_cmeta_tiles + (size_t)l * (5 * (size_t)H + I) * 4 : nullptr;
    q.U = h->cur_units;
    q.rg = h->d_range + (size_t)l * 4 * Q8_RANGE_WORDS * q.U;
    q.rstep = (size_t)Q8_RANGE_WORDS * q.U;
    q.rs = q.U > 1 ? h->d_row_slot : nullptr;
    q.xq = reinterpret_cast<int8_t*>(h->d_xs + t0 * H);
    q.rm = h->d_rmeta + t0;
    q.rp = h->d_range_pairs;
    q.ln_pairs = (T + 3) / 4;
    return q;
}

// a few token rows (queries): one launch per Linear — range reduction and quantisation inside the product
int32_t Slice::run_q8_few_rows(const ForwardPlan& p) {
    CS_TRY(embed());
    for (uint32_t l = 0; l < cfg.layers; ++l) {
        const Q8LayerArgs q = q8_layer_begin(l);
        float* rp2 = q.rp + 2 * h->cap_range_pairs;
        // p.fold_ln (up to 16 rows of a 384-wide model: one short query): the two LayerNorms of a layer are the prologues of the products
        // that read them (Q8_SRC_LN: the block's 16 rows are the whole tensor, so it knows the range) — five launches per layer
        // instead of seven.  The products behind attention and GELU then write the PRE-norm rows to ybuf and add the
        // normalised ones (x, written by the prologue's column-tile-0 blocks) as their residual.  Same arithmetic, same bits.
        const bool fold = p.fold_ln;
        float* ybuf = h->d_xs + t0 * H;              // [T][H] f32 (the split copy of x is not used on this path)
        const bool last = l + 1 == cfg.layers;
        if (fold && l) {
            cs_bert_layer_offsets lp;
            cs_bert_layer_layout(&cfg, &h->off, l - 1, &lp);
            CS_TRY(launch_gemm_q8_skinny_ln(SH_OUT_SPLIT, ybuf, P + lp.out_ln_g, P + lp.out_ln_b, cfg.layer_norm_eps, x, q.wq + q.ql.qkv, q.cm, qkvs, T, 3 * H,
                                            h->d_flag, nullptr, nullptr, s));  // LN (layer l - 1's second) + E2
        } else {
            CS_TRY(launch_gemm_q8_skinny(SH_OUT_SPLIT, Q8_SRC_F32, x, q.rp, q.ln_pairs, q.wq + q.ql.qkv, q.cm, nullptr, nullptr, qkvs, T, 3 * H, H, h->d_flag,
                                         nullptr, nullptr, s));  // E2
        }
        CS_TRY(mark(CS_STAGE_QKV));
        uint32_t att_pairs = 0, up_pairs = 0;
        CS_TRY(launch_attention_sh2(qkvs, mask, ctxs, h->d_flag, nb, L, H, cfg.heads, s, q.rp, &att_pairs));  // E3
        CS_TRY(mark(CS_STAGE_ATTENTION));
        if (!att_pairs) return fail(CS_ERR_UNSUPPORTED, "attention kernel without range pairs in the few-rows quantised path");
        CS_TRY(launch_gemm_q8_skinny(SH_OUT_F32_RESID, Q8_SRC_SPLIT, ctxs, q.rp, att_pairs, q.wq + q.ql.ao, q.cm + 3 * H, x, fold ? ybuf : x, nullptr, T, H, H,
                                     h->d_flag, nullptr, nullptr, s));  // E4
        CS_TRY(mark(CS_STAGE_OUT_PROJ));
        if (fold) {
            CS_TRY(mark(CS_STAGE_LN_ATTN));
            CS_TRY(launch_gemm_q8_skinny_ln(SH_OUT_SPLIT_GELU, ybuf, P + lo.ao_ln_g, P + lo.ao_ln_b, cfg.layer_norm_eps, x, q.wq + q.ql.up, q.cm + 4 * H, mids, T, I,
                                            h->d_flag, rp2, &up_pairs, s));  // LN + E5
        } else {
            CS_TRY(layer_norm(lo.ao_ln_g, lo.ao_ln_b));
            CS_TRY(mark(CS_STAGE_LN_ATTN));
            CS_TRY(launch_gemm_q8_skinny(SH_OUT_SPLIT_GELU, Q8_SRC_F32, x, q.rp, q.ln_pairs, q.wq + q.ql.up, q.cm + 4 * H, nullptr, nullptr, mids, T, I, H,
                                         h->d_flag, rp2, &up_pairs, s));  // E5
        }
        CS_TRY(mark(CS_STAGE_FFN_UP));
        CS_TRY(launch_gemm_q8_skinny(SH_OUT_F32_RESID, Q8_SRC_SPLIT, mids, rp2, up_pairs, q.wq + q.ql.down, q.cm + 4 * H + I, x, fold && !last ? ybuf : x, nullptr,
                                     T, H, I, h->d_flag, nullptr, nullptr, s));  // E6
        CS_TRY(mark(CS_STAGE_FFN_DOWN));
        if (!fold || last) {  // (folded: the next layer's first product normalises ybuf)
            CS_TRY(layer_norm(lo.out_ln_g, lo.out_ln_b));
        }
        CS_TRY(mark(CS_STAGE_LN_FFN));
        if (last) h->last_hidden_partial = false;
    }
    return pool();
}

// one unit, K = 384, a row block per CU: the products quantise their own rows on the way in — per tensor only
// its range is needed first (a reduction of the pairs its producer left).  q8_x_pairs: how many pairs the
// kernel that wrote x left (LayerNorm: one per four rows; the LayerNorm-fused products: one per sixteen; 0: the
// LayerNorm-fused product that wrote x widened this tensor's slot itself, p.ln_slot)
int32_t Slice::run_q8_rows_source(const ForwardPlan& p) {
    CS_TRY(embed());
    for (uint32_t l = 0; l < cfg.layers; ++l) {
        const Q8LayerArgs q = q8_layer_begin(l);
        if (l == 0) h->q8_x_pairs = q.ln_pairs;
        if (h->q8_x_pairs) CS_TRY(launch_q8_range(Q8_SRC_F32, x, T, H, q.rg, s, q.rp, h->q8_x_pairs));
        CS_TRY(launch_gemm_q8_from_source(SH_OUT_SPLIT, Q8_SRC_F32, x, q.rg, q.wq + q.ql.qkv, q.cm, bqkv, nullptr, nullptr, qkvs, T, 3 * H, H, h->d_flag, s, nullptr, q.cmt,
                                          q.xq));  // E2 (xq: scratch for the quantised rows of a call of few slabs)
        CS_TRY(mark(CS_STAGE_QKV));
        uint32_t att_pairs = 0;
        CS_TRY(launch_attention_sh2(qkvs, mask, ctxs, h->d_flag, nb, L, H, cfg.heads, s, q.rp, &att_pairs));  // E3
        CS_TRY(mark(CS_STAGE_ATTENTION));
        CS_TRY(launch_q8_range(Q8_SRC_SPLIT, ctxs, T, H, q.rg + q.rstep, s, q.rp, att_pairs));
        if (p.ln_fused_ao) {  // E4 with its residual add and LayerNorm in one kernel (gemm_q8_ln_kernel)
            CS_TRY(launch_gemm_q8_ln(Q8_SRC_SPLIT, ctxs, nullptr, q.rg + q.rstep, q.wst ? q.wst : q.wq + q.ql.ao, q.cm + 3 * H, x, P + lo.ao_ln_g, P + lo.ao_ln_b,
                                     cfg.layer_norm_eps, T, H, q.rp, &h->q8_x_pairs, s, p.ln_slot ? q.rg + 2 * q.rstep : nullptr, q.wst != nullptr));
            CS_TRY(mark(CS_STAGE_OUT_PROJ));
        } else {
            CS_TRY(launch_gemm_q8_from_source(SH_OUT_F32_RESID, Q8_SRC_SPLIT, ctxs, q.rg + q.rstep, q.wq + q.ql.ao, q.cm + 3 * H, P + lo.ao_b, x, x, nullptr, T, H, H,
                                              h->d_flag, s));  // E4
            CS_TRY(mark(CS_STAGE_OUT_PROJ));
            CS_TRY(layer_norm(lo.ao_ln_g, lo.ao_ln_b));
            h->q8_x_pairs = q.ln_pairs;
        }
        CS_TRY(mark(CS_STAGE_LN_ATTN));
        if (h->q8_x_pairs) CS_TRY(launch_q8_range(Q8_SRC_F32, x, T, H, q.rg + 2 * q.rstep, s, q.rp, h->q8_x_pairs));
        int8_t* midq = reinterpret_cast<int8_t*>(mid);
        Q8RowMeta* rm2 = h->d_rmeta2 + t0;
        CS_TRY(launch_gemm_q8_gelu_requant_from_source(x, q.rg + 2 * q.rstep, q.wq + q.ql.up, q.cm + 4 * H, P + lo.up_b, T, I, H, q.rg + 3 * q.rstep, midq, rm2, s, nullptr,
                                                       q.cmt ? q.cmt + 4 * 4 * H : nullptr, q.xq));  // E5 (xq: the range pass's quantised rows for the store pass)
        CS_TRY(mark(CS_STAGE_FFN_UP));
        if (p.ln_fused_down) {  // E6 likewise
            // (the next layer's first slot; the last layer's output is not quantised again: pairs nobody reads)
            CS_TRY(launch_gemm_q8_ln(Q8_SRC_PREQUANT, midq, rm2, nullptr, q.wst ? q.wst + (size_t)H * H : q.wq + q.ql.down, q.cm + 4 * H + I, x, P + lo.out_ln_g, P + lo.out_ln_b,
                                     cfg.layer_norm_eps, T, I, q.rp, &h->q8_x_pairs, s, p.ln_slot && l + 1 < cfg.layers ? q.rg + 4 * q.rstep : nullptr, q.wst != nullptr));
            CS_TRY(mark(CS_STAGE_FFN_DOWN));
        } else {
            CS_TRY(launch_gemm_q8(SH_OUT_F32_RESID, midq, rm2, q.wq + q.ql.down, q.cm + 4 * H + I, P + lo.down_b, x, x, nullptr, T, H, I, h->d_flag, s));  // E6
            CS_TRY(mark(CS_STAGE_FFN_DOWN));
            CS_TRY(layer_norm(lo.out_ln_g, lo.out_ln_b));
            h->q8_x_pairs = q.ln_pairs;
        }
        CS_TRY(mark(CS_STAGE_LN_FFN));
        if (l + 1 == cfg.layers) h->last_hidden_partial = false;
    }
    return pool();
}

// several units in a batch the row-block kernels take: the one-unit path above with every range kept per unit
int32_t Slice::run_q8_multi_unit() {
    CS_TRY(embed());
    for (uint32_t l = 0; l < cfg.layers; ++l) {
        const Q8LayerArgs q = q8_layer_begin(l);
        if (q.rs && l == 0) CS_TRY(launch_q8_row_slots(h->d_seq_unit, h->d_unit_len, T, L, h->d_row_slot, s));
        const uint32_t* su = h->d_seq_unit + b0;
        CS_TRY(launch_q8_range_units(q.rp, L, true, su, h->d_unit_len, nb, q.U, q.rg, s));
        CS_TRY(launch_gemm_q8_from_source(SH_OUT_SPLIT, Q8_SRC_F32, x, q.rg, q.wq + q.ql.qkv, q.cm, bqkv, nullptr, nullptr, qkvs, T, 3 * H, H, h->d_flag, s, q.rs));  // E2
        CS_TRY(mark(CS_STAGE_QKV));
        uint32_t att_pairs = 0;
        CS_TRY(launch_attention_sh2(qkvs, mask, ctxs, h->d_flag, nb, L, H, cfg.heads, s, q.rp, &att_pairs, su, h->d_unit_len));  // E3
        CS_TRY(mark(CS_STAGE_ATTENTION));
        if (!att_pairs || att_pairs > h->cap_range_pairs)
            return fail(CS_ERR_HIP, "attention range pairs (%u) do not fit the pair buffer (%zu)", att_pairs, h->cap_range_pairs);
        CS_TRY(launch_q8_range_units(q.rp, att_pairs / nb, false, su, h->d_unit_len, nb, q.U, q.rg + q.rstep, s));
        CS_TRY(launch_gemm_q8_from_source(SH_OUT_F32_RESID, Q8_SRC_SPLIT, ctxs, q.rg + q.rstep, q.wq + q.ql.ao, q.cm + 3 * H, P + lo.ao_b, x, x, nullptr, T, H, H,
                                          h->d_flag, s, q.rs));  // E4
        CS_TRY(mark(CS_STAGE_OUT_PROJ));
        CS_TRY(layer_norm(lo.ao_ln_g, lo.ao_ln_b));
        CS_TRY(mark(CS_STAGE_LN_ATTN));
        CS_TRY(launch_q8_range_units(q.rp, L, true, su, h->d_unit_len, nb, q.U, q.rg + 2 * q.rstep, s));
        int8_t* midq = reinterpret_cast<int8_t*>(mid);
        Q8RowMeta* rm2 = h->d_rmeta2 + t0;
        CS_TRY(launch_gemm_q8_gelu_requant_from_source(x, q.rg + 2 * q.rstep, q.wq + q.ql.up, q.cm + 4 * H, P + lo.up_b, T, I, H, q.rg + 3 * q.rstep, midq, rm2, s, q.rs));  // E5
        CS_TRY(mark(CS_STAGE_FFN_UP));
        CS_TRY(launch_gemm_q8(SH_OUT_F32_RESID, midq, rm2, q.wq + q.ql.down, q.cm + 4 * H + I, P + lo.down_b, x, x, nullptr, T, H, I, h->d_flag, s));  // E6
        CS_TRY(mark(CS_STAGE_FFN_DOWN));
        CS_TRY(layer_norm(lo.out_ln_g, lo.out_ln_b));
        CS_TRY(mark(CS_STAGE_LN_FFN));
        if (l + 1 == cfg.layers) h->last_hidden_partial = false;
    }
    return pool();
}

// quantising passes in front of the tile-per-block products (any shape, any number of units)
int32_t Slice::run_q8_quantise() {
    CS_TRY(embed());
    for (uint32_t l = 0; l < cfg.layers; ++l) {
        const Q8LayerArgs q = q8_layer_begin(l);
        if (q.rs && l == 0) CS_TRY(launch_q8_row_slots(h->d_seq_unit, h->d_unit_len, T, L, h->d_row_slot, s));
        CS_TRY(launch_q8_quantize(Q8_SRC_F32, x, T, H, q.rg, q.rs, q.xq, q.rm, s, q.rp, q.ln_pairs));
        CS_TRY(launch_gemm_q8(SH_OUT_SPLIT, q.xq, q.rm, q.wq + q.ql.qkv, q.cm, bqkv, nullptr, nullptr, qkvs, T, 3 * H, H, h->d_flag, s));  // E2
        CS_TRY(mark(CS_STAGE_QKV));
        uint32_t att_pairs = 0;
        CS_TRY(launch_attention_sh2(qkvs, mask, ctxs, h->d_flag, nb, L, H, cfg.heads, s, q.rp, &att_pairs));  // E3
        if (att_pairs > h->cap_range_pairs) return fail(CS_ERR_HIP, "range pair buffer too small (%u > %zu)", att_pairs, h->cap_range_pairs);
        CS_TRY(mark(CS_STAGE_ATTENTION));
        CS_TRY(launch_q8_quantize(Q8_SRC_SPLIT, ctxs, T, H, q.rg + q.rstep, q.rs, q.xq, q.rm, s, q.rp, att_pairs));
        CS_TRY(launch_gemm_q8(SH_OUT_F32_RESID, q.xq, q.rm, q.wq + q.ql.ao, q.cm + 3 * H, P + lo.ao_b, x, x, nullptr, T, H, H, h->d_flag, s));  // E4
        CS_TRY(mark(CS_STAGE_OUT_PROJ));
        CS_TRY(layer_norm(lo.ao_ln_g, lo.ao_ln_b));
        CS_TRY(mark(CS_STAGE_LN_ATTN));
        CS_TRY(launch_q8_quantize(Q8_SRC_F32, x, T, H, q.rg + 2 * q.rstep, q.rs, q.xq, q.rm, s, q.rp, q.ln_pairs));
        // E5: GELU(x W1^T + b1) leaves already re-quantised for E6 (two passes over the int8 product instead of 1.2 GB of
        // f32-class hand-over at 65,536 rows: launch_gemm_q8_gelu_requant)
        int8_t* midq = reinterpret_cast<int8_t*>(mid);
        Q8RowMeta* rm2 = h->d_rmeta2 + t0;
        if (q.rs) {  // several units: GELU output in split form, then its own range + quantising passes (into the x_q buffer)
            CS_TRY(launch_gemm_q8(SH_OUT_SPLIT_GELU, q.xq, q.rm, q.wq + q.ql.up, q.cm + 4 * H, P + lo.up_b, nullptr, nullptr, mids, T, I, H, h->d_flag, s));
            CS_TRY(mark(CS_STAGE_FFN_UP));
            CS_TRY(launch_q8_quantize(Q8_SRC_SPLIT, mids, T, I, q.rg + 3 * q.rstep, q.rs, q.xq, q.rm, s));
            midq = q.xq;
            rm2 = q.rm;
        } else {
            CS_TRY(launch_gemm_q8_gelu_requant(q.xq, q.rm, q.wq + q.ql.up, q.cm + 4 * H, P + lo.up_b, T, I, H, q.rg + 3 * q.rstep, midq, rm2, s));
            CS_TRY(mark(CS_STAGE_FFN_UP));
        }
        CS_TRY(launch_gemm_q8(SH_OUT_F32_RESID, midq, rm2, q.wq + q.ql.down, q.cm + 4 * H + I, P + lo.down_b, x, x, nullptr, T, H, I, h->d_flag, s));  // E6
        CS_TRY(mark(CS_STAGE_FFN_DOWN));
        CS_TRY(layer_norm(lo.out_ln_g, lo.out_ln_b));
        CS_TRY(mark(CS_STAGE_LN_FFN));
        if (l + 1 == cfg.layers) h->last_hidden_partial = false;
    }
    return pool();
}

// ---- split-f16 ----
// The last layer of a CLS-pooled model on the rows the embedding reads (cls_tail.hip): its attention needs every key and
// value but only the CLS query, and everything behind it runs on nb rows instead of nb * L.  Compact rows live in the (idle)
// intermediate buffer of the slice.
int32_t Slice::run_cls_tail(const ForwardPlan& p, const _Float16* ws) {
    h->last_hidden_partial = true;
    float* x_cls = mid;                                            // [nb, H] f32
    _Float16* xs_cls = reinterpret_cast<_Float16*>(mid + (size_t)nb * H);       // [nb][H/32][64]
    _Float16* ctxs_cls = reinterpret_cast<_Float16*>(mid + (size_t)2 * nb * H);
    _Float16* q_cls = reinterpret_cast<_Float16*>(mid + (size_t)3 * nb * H);
    _Float16* mids_cls = reinterpret_cast<_Float16*>(mid + (size_t)4 * nb * H);  // [nb][I/32][64]
    // E2: K and V for every token (the packed weight's rows H .. 3H: [T][2H/32][64]), Q for the CLS rows only
    CS_TRY(dense(p.kv_tail, SH_OUT_SPLIT, xs, ws + sl.qkv + (size_t)H * H * 2, bqkv + H, nullptr, nullptr, qkvs, T, 2 * H, H));
    CS_TRY(launch_gather_cls(xs, x_cls, xs_cls, nb, L, H, s));
    CS_TRY(launch_gemm_split(SH_OUT_SPLIT, xs_cls, ws + sl.qkv, bqkv, nullptr, nullptr, q_cls, nb, H, H, h->d_flag, s));
    CS_TRY(mark(CS_STAGE_QKV));
    CS_TRY(launch_attention_cls(q_cls, qkvs, mask, ctxs_cls, h->d_flag, nb, L, H, cfg.heads, s));   // E3, one query per sequence
    CS_TRY(mark(CS_STAGE_ATTENTION));
    EncoderLaunch t = a;
    t.x = x_cls; t.xs = xs_cls; t.T = nb; t.L = 1; t.B = nb;
    CS_TRY(launch_gemm_split(SH_OUT_F32_RESID, ctxs_cls, ws + sl.ao, P + lo.ao_b, x_cls, x_cls, nullptr, nb, H, H, h->d_flag, s));  // E4
    CS_TRY(mark(CS_STAGE_OUT_PROJ));
    t.g = P + lo.ao_ln_g; t.b = P + lo.ao_ln_b;
    CS_TRY(launch_row_kernel(1, t, H, s));
    CS_TRY(mark(CS_STAGE_LN_ATTN));
    CS_TRY(launch_gemm_split(SH_OUT_SPLIT_GELU, xs_cls, ws + sl.up, P + lo.up_b, nullptr, nullptr, mids_cls, nb, I, H, h->d_flag, s));  // E5
    CS_TRY(mark(CS_STAGE_FFN_UP));
    CS_TRY(launch_gemm_split(SH_OUT_F32_RESID, mids_cls, ws + sl.down, P + lo.down_b, x_cls, x_cls, nullptr, nb, H, I, h->d_flag, s));  // E6
    CS_TRY(mark(CS_STAGE_FFN_DOWN));
    t.g = P + lo.out_ln_g; t.b = P + lo.out_ln_b;
    CS_TRY(launch_row_kernel(1, t, H, s));
    CS_TRY(mark(CS_STAGE_LN_FFN));
    CS_TRY(out_stage(t));  // E7 + E8 on the compact rows (L = 1: row b IS the CLS row)
    return mark(CS_STAGE_POOL);
}

int32_t Slice::run_split(const ForwardPlan& p) {
    // `nomic`: every family with a gated feed-forward and no position table (NomicBert, JinaBert); `rotary` / `jina` what
    // only one of them does (rotary map on Q / K | ALiBi on the scores, GELU gate, optional LayerNorm on Q / K rows)
    const bool nomic = cs_arch_gated(cfg.arch), rotary = cfg.arch == CS_ARCH_NOMIC, jina = cs_arch_alibi(cfg.arch);
    const bool qknorm = cfg.arch == CS_ARCH_JINA_QKNORM;
    const float* alibi = jina ? h->d_alibi : nullptr;
    CS_TRY(embed());
    for (uint32_t l = 0; l < cfg.layers; ++l) {
        layer_begin(l);
        const _Float16* ws = h->d_wsplit + (size_t)l * sl.total;
        if (l + 1 == cfg.layers) h->last_hidden_partial = false;
        if (p.cls_tail && l + 1 == cfg.layers) return run_cls_tail(p, ws);
        CS_TRY(dense(p.qkv, SH_OUT_SPLIT, xs, ws + sl.qkv, bqkv, nullptr, nullptr, qkvs, T, 3 * H, H));  // E2
        if (rotary) CS_TRY(launch_rope_split(qkvs, h->d_rope, T, L, H, cfg.heads, h->d_flag, s));  // rotary map on Q and K (nomic.hip)
        if (qknorm) CS_TRY(launch_qk_layernorm_split(qkvs, P + lo.qln_g, cfg.layer_norm_eps, T, H, h->d_flag, s));  // JinaBert qk-post-norm
        CS_TRY(mark(CS_STAGE_QKV));
        CS_TRY(launch_attention_sh2(qkvs, mask, ctxs, h->d_flag, nb, L, H, cfg.heads, s, nullptr, nullptr, nullptr, nullptr, alibi));  // E3
        CS_TRY(mark(CS_STAGE_ATTENTION));
        a.g = P + lo.ao_ln_g; a.b = P + lo.ao_ln_b;
        if (p.fuse_ln) {  // dense layer + residual + LayerNorm in one kernel (gemm_wide.hip); p.split_resid: no f32 copy of x between them
            CS_TRY(launch_gemm_wide_ln(ctxs, ws + sl.ao, P + lo.ao_b, x, a.g, a.b, cfg.layer_norm_eps,
                                       p.split_resid ? nullptr : x, xs, T, H, h->d_flag, s, p.split_resid ? xs : nullptr));  // E4
            CS_TRY(mark(CS_STAGE_OUT_PROJ));
        } else if (p.ao_slices) {
            CS_TRY(launch_gemm_split_partial(ctxs, ws + sl.ao, qkv, T, H, H, p.ao_slices, s));  // E4, K slices as for E6 below
            CS_TRY(mark(CS_STAGE_OUT_PROJ));
            a.parts = qkv; a.nparts = p.ao_slices; a.bias = P + lo.ao_b;
            CS_TRY(launch_row_kernel(3, a, H, s));
        } else {
            CS_TRY(dense(p.ao, SH_OUT_F32_RESID, ctxs, ws + sl.ao, P + lo.ao_b, x, x, nullptr, T, H, H));  // E4
            CS_TRY(mark(CS_STAGE_OUT_PROJ));
            CS_TRY(launch_row_kernel(1, a, H, s));
        }
        CS_TRY(mark(CS_STAGE_LN_ATTN));
        a.g = P + lo.out_ln_g; a.b = P + lo.out_ln_b;
        const _Float16* ffn_in = mids;  // E6's operand
        if (nomic) {
            // E5 of the gated feed-forward: ONE product over fc11's and fc12's rows ([2I, H], interleaved in groups of 16)
            // into the first 2I columns of the workspace, then value * silu(gate) into its last I columns — E6's operand
            _Float16* gated = reinterpret_cast<_Float16*>(mid + (size_t)T * 2 * I);
            const float* bup = h->d_bup + (size_t)l * 2 * I;
            if (p.gate_epilogue) {  // the gate as the product's epilogue: the raw [T, 2I] tensor never exists
                CS_TRY(launch_gemm_wide(jina ? GW_OUT_GEGLU : GW_OUT_SWIGLU, xs, ws + sl.up, bup, nullptr, nullptr, gated, T, 2 * I, H, h->d_flag, s, p.up == DenseKernel::Wide192 ? 192 : 0));
            } else {
                CS_TRY(dense(p.up, SH_OUT_SPLIT, xs, ws + sl.up, bup, nullptr, nullptr, mids, T, 2 * I, H));
                CS_TRY(launch_swiglu_split(mids, gated, T, I, h->d_flag, s, jina));
            }
            ffn_in = gated;
        } else {
            CS_TRY(dense(p.up, SH_OUT_SPLIT_GELU, xs, ws + sl.up, P + lo.up_b, nullptr, nullptr, mids, T, I, H));    // E5
        }
        CS_TRY(mark(CS_STAGE_FFN_UP));
        if (p.fuse_ln) {  // (the last layer writes x for the pooling)
            CS_TRY(launch_gemm_wide_ln(ffn_in, ws + sl.down, P + lo.down_b, x, a.g, a.b, cfg.layer_norm_eps,
                                       (p.split_resid && l + 1 < cfg.layers) ? nullptr : x, xs, T, I, h->d_flag, s,
                                       p.split_resid ? xs : nullptr));  // E6
            CS_TRY(mark(CS_STAGE_FFN_DOWN));
        } else if (p.down_slices) {
            // partial slabs in the qkv buffer (free by now), summed with bias and residual by the LayerNorm that follows
            CS_TRY(launch_gemm_split_partial(ffn_in, ws + sl.down, qkv, T, H, I, p.down_slices, s));  // E6
            CS_TRY(mark(CS_STAGE_FFN_DOWN));
            a.parts = qkv; a.nparts = p.down_slices; a.bias = P + lo.down_b;
            CS_TRY(launch_row_kernel(3, a, H, s));
        } else {
            CS_TRY(dense(p.down, SH_OUT_F32_RESID, ffn_in, ws + sl.down, P + lo.down_b, x, x, nullptr, T, H, I)); // E6
            CS_TRY(mark(CS_STAGE_FFN_DOWN));
            CS_TRY(launch_row_kernel(1, a, H, s));
        }
        CS_TRY(mark(CS_STAGE_LN_FFN));
    }
    return pool();
}

// ---- exact f32 ----
int32_t Slice::run_f32() {
    const bool nomic = cs_arch_gated(cfg.arch), rotary = cfg.arch == CS_ARCH_NOMIC, jina = cs_arch_alibi(cfg.arch);
    const bool qknorm = cfg.arch == CS_ARCH_JINA_QKNORM;
    const float* alibi = jina ? h->d_alibi : nullptr;
    CS_TRY(embed());
    for (uint32_t l = 0; l < cfg.layers; ++l) {
        layer_begin(l);
        const float* wqkv = h->d_wqkv + (size_t)l * 3 * H * H;
        CS_TRY(launch_gemm(GEMM_BIAS, x, wqkv, bqkv, nullptr, qkv, T, 3 * H, H, s));        // E2
        if (rotary) CS_TRY(launch_rope_f32(qkv, h->d_rope, T, L, H, cfg.heads, s));
        if (qknorm) CS_TRY(launch_qk_layernorm_f32(qkv, P + lo.qln_g, cfg.layer_norm_eps, T, H, s));
        CS_TRY(mark(CS_STAGE_QKV));
        CS_TRY(launch_attention(qkv, mask, ctx, nb, L, H, cfg.heads, s, alibi));              // E3
        CS_TRY(mark(CS_STAGE_ATTENTION));
        CS_TRY(launch_gemm(GEMM_RESID, ctx, P + lo.ao_w, P + lo.ao_b, x, x, T, H, H, s));   // E4
        CS_TRY(mark(CS_STAGE_OUT_PROJ));
        CS_TRY(layer_norm(lo.ao_ln_g, lo.ao_ln_b));
        CS_TRY(mark(CS_STAGE_LN_ATTN));
        if (nomic) {  // value and gate as two products, value *= silu(gate)
            float* gate = mid + (size_t)T * I;
            CS_TRY(launch_gemm(GEMM_BIAS, x, P + lo.up_w, P + lo.up_b, nullptr, mid, T, I, H, s));
            CS_TRY(launch_gemm(GEMM_BIAS, x, P + lo.gate_w, P + lo.gate_b, nullptr, gate, T, I, H, s));
            CS_TRY(launch_swiglu_f32(mid, gate, T, I, s, jina));
        } else {
            CS_TRY(launch_gemm(GEMM_GELU, x, P + lo.up_w, P + lo.up_b, nullptr, mid, T, I, H, s)); // E5
        }
        CS_TRY(mark(CS_STAGE_FFN_UP));
        CS_TRY(launch_gemm(GEMM_RESID, mid, P + lo.down_w, P + lo.down_b, x, x, T, H, I, s));  // E6
        CS_TRY(mark(CS_STAGE_FFN_DOWN));
        CS_TRY(layer_norm(lo.out_ln_g, lo.out_ln_b));
        CS_TRY(mark(CS_STAGE_LN_FFN));
    }
    return pool();
}

// Sequences [b0, b0 + nb) of the mini-batch on stream s.  Every kernel but attention is local to
// a token row and attention is local to a sequence, so a range of sequences is an independent job
// on the same buffers at a token offset.  The plan (forward_plan.hpp) names the launch sequence and everything it fuses.
int32_t forward_range(cs_embedder* h, hipStream_t s, const ForwardToggles& tg, uint32_t b0, uint32_t nb, uint32_t L, int mode) {
    ForwardShape shape = shape_of(h, b0, nb, L, mode);
#ifdef CS_DIAGNOSTICS
    if (tg.small_forward)
        shape.small_forward_ok = h->d_sf_layers && !h->sf_off && small_forward_supported(h->cfg.hidden, h->cfg.intermediate, h->cfg.heads, nb * L, L);
#endif
    const ForwardPlan p = plan_forward(forward_knobs(), tg, shape);
    if (p.path == ForwardPath::Refused) return fail(CS_ERR_UNSUPPORTED, "the dynamic-quantisation mode is not built for the ModernBERT encoder");
    Slice c(h, s, b0, nb, L, mode, p);
    if (p.path == ForwardPath::Modern) return c.run_modern(p);
    h->sf_ran = false;
    switch (p.path) {
        case ForwardPath::Small:
        case ForwardPath::SmallOneLaunch: return c.run_small(p);
        case ForwardPath::Q8FewRows: return c.run_q8_few_rows(p);
        case ForwardPath::Q8RowsSource: return c.run_q8_rows_source(p);
        case ForwardPath::Q8MultiUnit: return c.run_q8_multi_unit();
        case ForwardPath::Q8Quantise: return c.run_q8_quantise();
        case ForwardPath::Split: return c.run_split(p);
        default: return c.run_f32();
    }
}

}  // namespace

// One mini-batch already on the device (d_ids/d_mask) -> d_pooled [B, H].  Where plan_streams says so the batch is cut into
// slices on as many streams: each kernel alternates an MFMA-bound main loop with an HBM-bound
// epilogue (and attention / LayerNorm are memory-heavy throughout), so blocks of two different
// kernels sharing a CU keep both the matrix pipe and the memory system busy.
int32_t forward(cs_embedder* h, uint32_t B, uint32_t L, int mode) {
    hipStream_t s = h->stream;
    CS_HIP(hipEventRecord(h->ev0, s));
    if (mode != CS_GEMM_F32) CS_HIP(hipMemsetAsync(h->d_flag, 0, sizeof(uint32_t), s));
    if (mode == CS_GEMM_Q8_DYNAMIC)  // every range starts from (+0, +0)
        CS_HIP(hipMemsetAsync(h->d_range, 0, (size_t)h->cfg.layers * 4 * Q8_RANGE_WORDS * h->cur_units * sizeof(uint32_t), s));
    h->stage_tag.clear();
    const ForwardToggles tg = forward_toggles_from_env();
    const uint32_t ns = plan_streams(forward_knobs(), shape_of(h, 0, B, L, mode));
    h->streams_in_flight = (int)ns;
    if (ns >= 2) {
        hipStream_t st[4] = {s, h->stream2, h->xstreams[0], h->xstreams[1]};
        hipEvent_t jn[4] = {nullptr, h->ev_join, h->xjoin[0], h->xjoin[1]};
        CS_HIP(hipEventRecord(h->ev_fork, s));
        for (uint32_t i = ns; i-- > 0;) {  // slice 0 last, on the caller-visible stream
            const uint32_t lo = (uint32_t)((uint64_t)B * i / ns), hi = (uint32_t)((uint64_t)B * (i + 1) / ns);
            if (i) CS_HIP(hipStreamWaitEvent(st[i], h->ev_fork, 0));
            CS_TRY(forward_range(h, st[i], tg, lo, hi - lo, L, mode));
            if (i) CS_HIP(hipEventRecord(jn[i], st[i]));
        }
        for (uint32_t i = 1; i < ns; ++i) CS_HIP(hipStreamWaitEvent(s, jn[i], 0));
    } else {
        CS_TRY(forward_range(h, s, tg, 0, B, L, mode));
    }
    CS_HIP(hipEventRecord(h->ev1, s));
    h->last_B = B;
    h->last_L = L;
    return CS_OK;
}
}  // namespace emb
}  // namespace cs
