// rerank_head.hip — the score head of a cross-encoder (BertForSequenceClassification's pooler + classifier, which is
// RobertaClassificationHead's dense -> tanh -> out_proj under other names): for sequence b, with x its CLS row of the last layer,
//     logit_b = w_c . tanh(W_p x + b_p) + b_c
// in place of the pooling launch of an embedder that carries a head (embedder_forward.hip Slice::out_stage).
//
// One block serves RH_SEQS sequences, so W_p (590 KB at H = 384, 4 MB at 1024) is fetched once per RH_SEQS sequences and not
// once per sequence; the blocks' re-reads come out of L2.  The sequences' CLS rows sit in LDS.  Wave w takes the rows
// j = w, w + 4, ... of W_p: a lane holds W_p[j][lane + 64 i] (whole 256-byte lines per load), forms its part of every
// sequence's dot product with FMAs in i order, the wave adds the 64 parts by the xor butterfly (wave_sum: the same tree on
// every run), and every lane then carries z_j.  tanhf is the library's (-fno-fast-math).  The classifier's dot is one FMA
// per j in the wave's j order, and the four waves' parts are added in wave order: a fixed order throughout, so the same
// input gives the same bits whatever it is batched with.
// Measured (profiles/rerank_latency.jsonl, the turbo reranker's shape): 132 - 147 us whatever the number of pairs — the
// stage is latency-bound, a wave walks its 96 rows one L2 round trip after the other.
#include "encoder.hpp"
#include "encoder_rows.hpp"

namespace cs {

constexpr int RH_SEQS = 8;

template <int NPL>
__global__ void __launch_bounds__(256)
rerank_head_kernel(const float* __restrict__ x, size_t row_stride, const float* __restrict__ head, uint32_t B,
                   float* __restrict__ out) {
    constexpr int H = 64 * NPL;
    __shared__ float xs[RH_SEQS][H];
    __shared__ float part[4][RH_SEQS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t b0 = blockIdx.x * RH_SEQS;
    const float* Wp = head;
    const float* bp = head + (size_t)H * H;
    const float* wc = bp + H;
    const float* bc = wc + H;
    // the tile's CLS rows (a sequence past the batch's end reads the last one: its result is not stored)
    for (int i = threadIdx.x; i < RH_SEQS * H; i += 256) {
        const uint32_t s = i / H, b = b0 + s < B ? b0 + s : B - 1;
        xs[s][i % H] = x[(size_t)b * row_stride + (i % H)];
    }
    __syncthreads();
    float acc[RH_SEQS];
#pragma unroll
    for (int s = 0; s < RH_SEQS; ++s) acc[s] = 0.0f;
    for (int j = wave; j < H; j += 4) {
        float w[NPL];
#pragma unroll
        for (int i = 0; i < NPL; ++i) w[i] = Wp[(size_t)j * H + lane + 64 * i];
        const float bj = bp[j], cj = wc[j];
        float z[RH_SEQS];
#pragma unroll
        for (int s = 0; s < RH_SEQS; ++s) {
            z[s] = 0.0f;
#pragma unroll
            for (int i = 0; i < NPL; ++i) z[s] = fmaf(w[i], xs[s][lane + 64 * i], z[s]);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
            for (int s = 0; s < RH_SEQS; ++s) z[s] += __shfl_xor(z[s], m, 64);
#pragma unroll
        for (int s = 0; s < RH_SEQS; ++s) acc[s] = fmaf(cj, tanhf(z[s] + bj), acc[s]);
    }
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < RH_SEQS; ++s) part[wave][s] = acc[s];
    }
    __syncthreads();
    if (threadIdx.x < RH_SEQS && b0 + threadIdx.x < B) {
        const int s = threadIdx.x;
        out[b0 + s] = (((part[0][s] + part[1][s]) + part[2][s]) + part[3][s]) + bc[0];
    }
}

// x: the CLS row of sequence b at x + b * row_stride (L * H in the residual stream, H in the CLS tail's compact rows);
// head: W_p [H, H] | b_p | w_c | b_c on the device; out [B]
int32_t launch_rerank_head(const float* x, size_t row_stride, const float* head, uint32_t B, uint32_t H, float* out,
                           hipStream_t s) {
    if (B == 0) return CS_OK;
    const dim3 grid((B + RH_SEQS - 1) / RH_SEQS), block(256);
    switch (H) {
        case 384: hipLaunchKernelGGL(rerank_head_kernel<6>, grid, block, 0, s, x, row_stride, head, B, out); break;
        case 768: hipLaunchKernelGGL(rerank_head_kernel<12>, grid, block, 0, s, x, row_stride, head, B, out); break;
        case 1024: hipLaunchKernelGGL(rerank_head_kernel<16>, grid, block, 0, s, x, row_stride, head, B, out); break;
        default: return fail(CS_ERR_UNSUPPORTED, "hidden size %u not supported (384/768/1024)", H);
    }
    CS_HIP(hipGetLastError());
    return CS_OK;
}

}  // namespace cs
