// rerank_host.cpp — the host half of the reference's NeuralReranker (src/rerank/neural.rs): the ordering of `rerank` and the
// score blend of `rerank_and_blend` (neural.rs:77-121), in f32 as the reference computes them.  Pure host code: usable
// without a device.
#include <algorithm>
#include <cmath>
#include <limits>
#include <numeric>

#include "common.hpp"

// the blend is the reference's f32 expression: a rounding per product and one for the sum, never contracted into an FMA
#pragma clang fp contract(off)

namespace {

// neural.rs:125-127
inline float sigmoid(float x) { return 1.0f / (1.0f + std::exp(-x)); }

// (score desc, original index asc), NaN last: what a stable descending sort of the scores in index order leaves
void order_desc(const float* scores, uint64_t n, uint32_t* out_index, float* out_score) {
    std::vector<uint32_t> idx(n);
    std::iota(idx.begin(), idx.end(), 0u);
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
        const float x = scores[a], y = scores[b];
        if (std::isnan(x) || std::isnan(y)) return !std::isnan(x) && std::isnan(y);
        return x > y;
    });
    for (uint64_t i = 0; i < n; ++i) {
        out_index[i] = idx[i];
        out_score[i] = scores[idx[i]];
    }
}

}  // namespace

extern "C" {

int32_t cs_rerank_order(const float* scores, uint64_t n, uint32_t* out_index, float* out_score) {
    if (n == 0) return CS_OK;  // neural.rs:57-59
    if (!scores || !out_index || !out_score) return cs::fail(CS_ERR_BAD_ARG, "cs_rerank_order: null argument");
    if (n > 0xFFFFFFFFull) return cs::fail(CS_ERR_BAD_ARG, "cs_rerank_order: %llu scores (indices are 32-bit)", (unsigned long long)n);
    order_desc(scores, n, out_index, out_score);
    return CS_OK;
}

int32_t cs_rerank_blend(const float* logits, const float* rrf_scores, uint64_t n, uint32_t* out_index, float* out_score) {
    if (n == 0) return CS_OK;  // neural.rs:83-85
    if (!logits || !rrf_scores || !out_index || !out_score) return cs::fail(CS_ERR_BAD_ARG, "cs_rerank_blend: null argument");
    if (n > 0xFFFFFFFFull) return cs::fail(CS_ERR_BAD_ARG, "cs_rerank_blend: %llu scores (indices are 32-bit)", (unsigned long long)n);
    // neural.rs:103-105: f32::min / f32::max folds (a NaN operand is skipped, as fminf / fmaxf skip it)
    float lo = std::numeric_limits<float>::infinity(), hi = -std::numeric_limits<float>::infinity();
    for (uint64_t i = 0; i < n; ++i) {
        lo = std::fmin(lo, rrf_scores[i]);
        hi = std::fmax(hi, rrf_scores[i]);
    }
    const float range = std::fmax(hi - lo, 0.0001f);
    std::vector<float> blended(n);
    for (uint64_t i = 0; i < n; ++i) {
        const float rerank_norm = sigmoid(logits[i]);
        const float rrf_norm = (rrf_scores[i] - lo) / range;
        blended[i] = 0.575f * rerank_norm + 0.425f * rrf_norm;
    }
    order_desc(blended.data(), n, out_index, out_score);
    return CS_OK;
}

}  // extern "C"
