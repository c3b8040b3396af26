// reranker.hip — cs_reranker_*: the device half of the reference's NeuralReranker (src/rerank/neural.rs): a
// cross-encoder scores every (query, document) pair with one logit.  The handle owns an ordinary CLS-pooled cs_embedder and
// the score head's weights; a scoring call runs the embedder's forward with the head (rerank_head.hip) in place of the
// pooling, so every route of the forward (small path, skinny / mid / wide kernels, the CLS tail) serves it unchanged.
#include "embedder_state.hpp"

using namespace cs;
using namespace cs::emb;

struct cs_reranker {
    cs_embedder* emb = nullptr;
    float* d_head = nullptr;  // W_p [H, H] | b_p | w_c | b_c
};

extern "C" {

uint64_t cs_rerank_head_count(const cs_bert_config* cfg) {
    return cfg ? (uint64_t)cfg->hidden * cfg->hidden + 2ull * cfg->hidden + 1 : 0;
}

void cs_reranker_destroy(cs_reranker* h) {
    if (!h) return;
    if (h->emb) {
        DeviceGuard g(h->emb->device);
        if (h->emb->stream) (void)hipStreamSynchronize(h->emb->stream);
        h->emb->d_head = nullptr;
        if (h->d_head) (void)hipFree(h->d_head);
        cs_embedder_destroy(h->emb);
    }
    delete h;
}

int32_t cs_reranker_create(const cs_bert_config* cfg, const float* params, const float* head, uint64_t seed, int32_t device,
                           cs_reranker** out) {
    if (!out) return fail(CS_ERR_BAD_ARG, "out is null");
    *out = nullptr;
    if (!cfg || !head) return fail(CS_ERR_BAD_ARG, "cs_reranker_create: null argument");
    if (cfg->arch == CS_ARCH_MODERN)
        return fail(CS_ERR_UNSUPPORTED, "Failed to initialize reranker model: the ModernBERT encoder is not built as a cross-encoder");
    cs_bert_config c = *cfg;
    c.pooling = CS_POOL_CLS;  // the head reads the CLS row
    cs_reranker* h = new cs_reranker();
    // (never a quantised embedder: cs_embedder_set_gemm_mode then refuses CS_GEMM_Q8_DYNAMIC on the borrowed handle, so
    // neither scoring entry point can meet that mode)
    int32_t s = cs_embedder_create(&c, params, seed, device, &h->emb);
    if (s != CS_OK) { delete h; return s; }
    DeviceGuard g(device);
    const size_t bytes = cs_rerank_head_count(&c) * sizeof(float);
    if (hipMalloc(&h->d_head, bytes) != hipSuccess) s = fail(CS_ERR_OOM, "hipMalloc(score head) failed");
    else if (hipMemcpy(h->d_head, head, bytes, hipMemcpyHostToDevice) != hipSuccess) s = fail(CS_ERR_HIP, "score head upload failed");
    if (s != CS_OK) { cs_reranker_destroy(h); return s; }
    h->emb->d_head = h->d_head;
    *out = h;
    return CS_OK;
}

int32_t cs_reranker_create_from_dir(const char* model_dir, int32_t device, cs_reranker** out) {
    if (!out) return fail(CS_ERR_BAD_ARG, "null out pointer");
    *out = nullptr;
    cs_bert_config cfg;
    std::vector<float> params, head;
    CS_TRY(reranker_files_from_dir(model_dir, &cfg, params, head));
    return cs_reranker_create(&cfg, params.data(), head.data(), 0, device, out);
}

cs_embedder* cs_reranker_embedder(cs_reranker* h) { return h ? h->emb : nullptr; }

int32_t cs_reranker_score_ids(cs_reranker* h, const int32_t* ids, const int32_t* mask, const int32_t* types, uint64_t n,
                              uint32_t seq_len, uint32_t batch, float* out_logits, const volatile int32_t* cancel) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null reranker handle");
    struct HeadGuard { cs_embedder* e; ~HeadGuard() { e->head_on = false; } } guard{h->emb};
    h->emb->head_on = true;
    return embed_ids_entry(h->emb, ids, mask, n, seq_len, batch, out_logits, false, cancel, types);
}

int32_t cs_reranker_rerank_texts(cs_reranker* h, const cs_tokenizer* tok, const char* query, const char* docs_utf8,
                                 const uint64_t* doc_offsets, uint64_t n, uint32_t max_length, const float* rrf_scores,
                                 uint32_t* out_index, float* out_score) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null reranker handle");
    if (!tok) return fail(CS_ERR_BAD_ARG, "Failed to rerank: no tokenizer attached");
    if (n == 0) return CS_OK;  // neural.rs:57-59
    if (!query || !docs_utf8 || !doc_offsets || !out_index || !out_score) return fail(CS_ERR_BAD_ARG, "null buffer");
    if (n > 0xFFFFFFFFull) return fail(CS_ERR_BAD_ARG, "%llu documents (indices are 32-bit)", (unsigned long long)n);
    for (uint64_t i = 0; i < n; ++i)
        if (doc_offsets[i + 1] < doc_offsets[i]) return fail(CS_ERR_BAD_ARG, "text offsets must be non-decreasing");
    if (max_length == 0) max_length = 512;
    max_length = std::min(max_length, h->emb->cfg.max_position);
    const uint64_t q_off[2] = {0, std::strlen(query)};
    std::vector<std::vector<int32_t>> enc, ty;
    CS_TRY(tokenize_pairs(tok, query, q_off, 1, docs_utf8, doc_offsets, (uint32_t)n, max_length, enc, ty));
    // the pairs as one window of ragged rows: length-grouped mini-batches, each padded to its own longest pair (run_window)
    std::vector<SeqView> seqs;
    seqs.reserve(n);
    for (uint64_t i = 0; i < n; ++i) seqs.push_back(SeqView{enc[i].data(), nullptr, (uint32_t)enc[i].size(), ty[i].data()});
    const int32_t pad = cs_tokenizer_pad_id(tok);
    const uint32_t batch = default_batch(h->emb);
    std::vector<float> logits(n);
    std::vector<uint32_t> order;
    std::vector<int32_t> ids, mask;
    {
        struct HeadGuard { cs_embedder* e; ~HeadGuard() { e->head_on = false; } } guard{h->emb};
        h->emb->head_on = true;
        const uint64_t window = (uint64_t)batch * 16;
        for (uint64_t lo = 0; lo < n; lo += window) {
            const std::vector<SeqView> win(seqs.begin() + lo, seqs.begin() + std::min<uint64_t>(n, lo + window));
            CS_TRY(run_window(h->emb, win, batch, pad, logits.data() + lo, false, nullptr, order, ids, mask));
        }
    }
    if (rrf_scores) return cs_rerank_blend(logits.data(), rrf_scores, n, out_index, out_score);
    return cs_rerank_order(logits.data(), n, out_index, out_score);
}

}  // extern "C"
