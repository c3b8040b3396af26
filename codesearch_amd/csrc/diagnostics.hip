// diagnostics.hip — cs_debug_*: operator-level entry points for the parity tests of single kernels and for the A/B scripts
// under benchmarks/.  NOT part of libcsgpu.so: built into libcsgpu_diag.so only (-DCS_DIAGNOSTICS, include/codesearch_gpu_diag.h).
#include "embedder_state.hpp"
#include "gemm_wide.hpp"  // gemm_wide_route (cs_debug_gemm_wide)
#include "scan.hpp"  // launch_synth_fill (cs_debug_gemm_time)
#include "../../include/codesearch_gpu_diag.h"

using namespace cs;
using namespace cs::emb;

namespace {

// The LayerNorm epilogue of the wide kernel as the diagnostics run it (cs_debug_gemm epilogues 3 / 4, cs_debug_gemm_wide
// 6 / 7; N = 384): gamma = bias + 1, beta = -bias, eps 1e-12; sC [M][N/32][64] receives the split output.
//   split_resid = false: in place over the f32 residual dR, f32 and split outputs, which must describe the same values
//   split_resid = true:  the encoder's form: the residual handed over in split form in sC and overwritten, no f32 output
int32_t diag_wide_ln(bool split_resid, const _Float16* sA, const _Float16* sW, const float* dB, float* dR, _Float16* sC,
                     const float* bias, uint32_t M, uint32_t N, uint32_t K, uint32_t* dF) {
    const size_t c_n = (size_t)M * N;
    std::vector<float> gam(N), bet(N);
    for (uint32_t n = 0; n < N; ++n) { gam[n] = bias[n] + 1.0f; bet[n] = -bias[n]; }
    float *dG = nullptr, *dBe = nullptr;
    auto run = [&]() -> int32_t {
        CS_HIP(hipMalloc(&dG, (size_t)N * 4)); CS_HIP(hipMalloc(&dBe, (size_t)N * 4));
        CS_HIP(hipMemcpy(dG, gam.data(), (size_t)N * 4, hipMemcpyHostToDevice));
        CS_HIP(hipMemcpy(dBe, bet.data(), (size_t)N * 4, hipMemcpyHostToDevice));
        if (split_resid) {
            CS_TRY(launch_split_rows(dR, sC, M, N, dF, nullptr));
            return launch_gemm_wide_ln(sA, sW, dB, nullptr, dG, dBe, 1e-12f, nullptr, sC, M, K, dF, nullptr, sC);
        }
        return launch_gemm_wide_ln(sA, sW, dB, dR, dG, dBe, 1e-12f, dR, sC, M, K, dF, nullptr);  // in place over resid
    };
    const int32_t st = run();
    const hipError_t sync = hipDeviceSynchronize();
    (void)hipFree(dG); (void)hipFree(dBe);
    CS_TRY(st);
    CS_HIP(sync);
    if (split_resid) return CS_OK;
    // the two outputs must describe the same values
    std::vector<float> f32out(c_n);
    CS_HIP(hipMemcpy(f32out.data(), dR, c_n * 4, hipMemcpyDeviceToHost));
    std::vector<_Float16> hs(c_n * 2);
    CS_HIP(hipMemcpy(hs.data(), sC, c_n * 4, hipMemcpyDeviceToHost));
    for (size_t m = 0; m < M; ++m)
        for (size_t n = 0; n < N; ++n) {
            const _Float16* line = hs.data() + (m * (N / 32) + n / 32) * 64;
            const float v = (float)line[n % 32] + (float)line[32 + n % 32] * (1.0f / 2048.0f);
            if (!(fabsf(v - f32out[m * N + n]) <= 1e-6f * fmaxf(1.0f, fabsf(v))))
                return fail(CS_ERR_HIP, "LayerNorm epilogue: f32 and split outputs disagree at (%zu, %zu): %g vs %g", m, n,
                            (double)f32out[m * N + n], (double)v);
        }
    return CS_OK;
}

}  // namespace

extern "C" {

int32_t cs_debug_gemm(int32_t device, int32_t mode, int32_t epilogue, const float* A, const float* W,
                      const float* bias, const float* resid, float* C, uint32_t M, uint32_t N, uint32_t K,
                      uint32_t* range_flag) {
    if (!A || !W || !bias || !C || ((epilogue == 2 || epilogue == 3) && !resid)) return fail(CS_ERR_BAD_ARG, "null buffer");
    const bool wide = mode == 2;  // diagnostics only: the 128 x 384 one-accumulator kernel whatever M is
    if (wide) mode = CS_GEMM_SPLIT_F16;
    // epilogue 3 (wide only, N = 384): + resid, LayerNorm with gamma = bias + 1, beta = -bias, eps 1e-12; C receives
    // the f32 output re-assembled from the SPLIT output (hi + lo / 2048), so both stores are exercised
    if (epilogue == 3 && !(wide && N == 384)) return fail(CS_ERR_UNSUPPORTED, "epilogue 3 needs mode 2 and N = 384");
    if (epilogue < 0 || epilogue > 4 || (mode != CS_GEMM_F32 && mode != CS_GEMM_SPLIT_F16))
        return fail(CS_ERR_BAD_ARG, "unknown epilogue/mode");
    if (wide && !gemm_wide_supported(N, K)) return fail(CS_ERR_UNSUPPORTED, "wide kernel needs N %% 384 == 0");
    if (M == 0 || N % 128 || K % 32 || K == 0) return fail(CS_ERR_UNSUPPORTED, "cs_debug_gemm needs M > 0, N %% 128 == 0, K %% 32 == 0");
    int ndev = 0;
    CS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(CS_ERR_HIP, "HIP device %d not available (%d visible)", device, ndev);
    DeviceGuard g(device);
    const size_t a_n = (size_t)M * K, w_n = (size_t)N * K, c_n = (size_t)M * N;
    float *dA = nullptr, *dW = nullptr, *dB = nullptr, *dR = nullptr, *dC = nullptr;
    _Float16 *sA = nullptr, *sW = nullptr, *sC = nullptr;
    uint32_t* dF = nullptr;
    int32_t st = CS_OK;
    auto run = [&]() -> int32_t {
        CS_HIP(hipMalloc(&dA, a_n * 4)); CS_HIP(hipMalloc(&dW, w_n * 4)); CS_HIP(hipMalloc(&dB, (size_t)N * 4));
        CS_HIP(hipMalloc(&dC, c_n * 4)); CS_HIP(hipMalloc(&dF, 4));
        CS_HIP(hipMemcpy(dA, A, a_n * 4, hipMemcpyHostToDevice));
        CS_HIP(hipMemcpy(dW, W, w_n * 4, hipMemcpyHostToDevice));
        CS_HIP(hipMemcpy(dB, bias, (size_t)N * 4, hipMemcpyHostToDevice));
        CS_HIP(hipMemset(dF, 0, 4));
        if (epilogue >= 2) {
            CS_HIP(hipMalloc(&dR, c_n * 4));
            CS_HIP(hipMemcpy(dR, resid, c_n * 4, hipMemcpyHostToDevice));
        }
        if (mode == CS_GEMM_F32) {
            CS_TRY(launch_gemm(epilogue, dA, dW, dB, dR, dC, M, N, K, nullptr));
        } else {
            CS_HIP(hipMalloc(&sA, a_n * 4)); CS_HIP(hipMalloc(&sW, w_n * 4));
            CS_TRY(launch_split_rows(dA, sA, M, K, dF, nullptr));
            CS_TRY(launch_split_rows(dW, sW, N, K, dF, nullptr));
            auto run_gemm = [&](int e, const _Float16* a_, const _Float16* w_, const float* b_, const float* r_, float* c_, _Float16* cs_,
                                uint32_t m_, uint32_t n_, uint32_t k_, uint32_t* f_, hipStream_t st_) {
                return wide ? launch_gemm_wide(e, a_, w_, b_, r_, c_, cs_, m_, n_, k_, f_, st_, 0) : launch_gemm_split(e, a_, w_, b_, r_, c_, cs_, m_, n_, k_, f_, st_);
            };
            if (epilogue == 3 || epilogue == 4) {
                CS_HIP(hipMalloc(&sC, c_n * 4));
                CS_TRY(diag_wide_ln(epilogue == 4, sA, sW, dB, dR, sC, bias, M, N, K, dF));
            } else if (epilogue == 1) {  // the GELU epilogue writes split form: read it back through hi + lo / 2048
                CS_HIP(hipMalloc(&sC, c_n * 4));
                CS_TRY(run_gemm(SH_OUT_SPLIT_GELU, sA, sW, dB, nullptr, nullptr, sC, M, N, K, dF, nullptr));
            } else {
                CS_TRY(run_gemm(epilogue == 2 ? SH_OUT_F32_RESID : SH_OUT_F32, sA, sW, dB, dR, dC, nullptr, M, N, K, dF, nullptr));
            }
        }
        CS_HIP(hipDeviceSynchronize());
        if (sC) {
            std::vector<_Float16> hs(c_n * 2);
            CS_HIP(hipMemcpy(hs.data(), sC, c_n * 4, hipMemcpyDeviceToHost));
            const size_t nch = N / 32;
            for (size_t m = 0; m < M; ++m)
                for (size_t n = 0; n < N; ++n) {
                    const _Float16* line = hs.data() + (m * nch + n / 32) * 64;
                    C[m * N + n] = (float)line[n % 32] + (float)line[32 + n % 32] * (1.0f / 2048.0f);
                }
        } else {
            CS_HIP(hipMemcpy(C, dC, c_n * 4, hipMemcpyDeviceToHost));
        }
        if (range_flag) CS_HIP(hipMemcpy(range_flag, dF, 4, hipMemcpyDeviceToHost));
        return CS_OK;
    };
    st = run();
    for (void* p : {(void*)dA, (void*)dW, (void*)dB, (void*)dR, (void*)dC, (void*)sA, (void*)sW, (void*)sC, (void*)dF})
        if (p) (void)hipFree(p);
    return st;
}

int32_t cs_debug_gemm_q8(int32_t device, int32_t epilogue, int32_t a_split, const float* A, const float* W,
                         const float* wscale, const float* bias, const float* resid, float* C, uint32_t M, uint32_t N,
                         uint32_t K, uint8_t* xq_out, float* xparams, int32_t* acc_out) {
    if (!A || !W || !wscale || !bias || !C || (epilogue == 2 && !resid)) return fail(CS_ERR_BAD_ARG, "null buffer");
    if (epilogue != 0 && epilogue != 1 && epilogue != 2 && epilogue != 4 && epilogue != 5) return fail(CS_ERR_BAD_ARG, "unknown epilogue %d", epilogue);
    if (M == 0 || N % 128 || K % 128 || K == 0) return fail(CS_ERR_UNSUPPORTED, "cs_debug_gemm_q8 needs M > 0, N %% 128 == 0, K %% 128 == 0");
    int ndev = 0;
    CS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(CS_ERR_HIP, "HIP device %d not available (%d visible)", device, ndev);
    DeviceGuard g(device);
    const size_t a_n = (size_t)M * K, w_n = (size_t)N * K, c_n = (size_t)M * N;
    float *dA = nullptr, *dW = nullptr, *dS = nullptr, *dB = nullptr, *dR = nullptr, *dC = nullptr;
    _Float16 *sA = nullptr, *sC = nullptr;
    int8_t *dXq = nullptr, *dWq = nullptr;
    Q8RowMeta* dRm = nullptr;
    Q8ColMeta* dCm = nullptr;
    uint32_t *dF = nullptr, *dRange = nullptr, *dCmT = nullptr;
    int32_t* dAcc = nullptr;
    auto run = [&]() -> int32_t {
        CS_HIP(hipMalloc(&dA, a_n * 4)); CS_HIP(hipMalloc(&dW, w_n * 4)); CS_HIP(hipMalloc(&dS, (size_t)N * 4));
        CS_HIP(hipMalloc(&dB, (size_t)N * 4)); CS_HIP(hipMalloc(&dC, c_n * 4)); CS_HIP(hipMalloc(&dF, 16));
        CS_HIP(hipMalloc(&dXq, a_n)); CS_HIP(hipMalloc(&dWq, w_n)); CS_HIP(hipMalloc(&dRm, (size_t)M * sizeof(Q8RowMeta)));
        CS_HIP(hipMalloc(&dCm, (size_t)N * sizeof(Q8ColMeta))); CS_HIP(hipMalloc(&dRange, Q8_RANGE_WORDS * 4));
        CS_HIP(hipMemcpy(dA, A, a_n * 4, hipMemcpyHostToDevice));
        CS_HIP(hipMemcpy(dW, W, w_n * 4, hipMemcpyHostToDevice));
        CS_HIP(hipMemcpy(dS, wscale, (size_t)N * 4, hipMemcpyHostToDevice));
        CS_HIP(hipMemcpy(dB, bias, (size_t)N * 4, hipMemcpyHostToDevice));
        CS_HIP(hipMemset(dF, 0, 16));
        CS_HIP(hipMemset(dRange, 0, Q8_RANGE_WORDS * 4));
        if (epilogue == 2) {
            CS_HIP(hipMalloc(&dR, c_n * 4));
            CS_HIP(hipMemcpy(dR, resid, c_n * 4, hipMemcpyHostToDevice));
        }
        if (acc_out && epilogue != 5) CS_HIP(hipMalloc(&dAcc, c_n * 4));
        CS_TRY(launch_q8_pack_weight(dW, dS, dB, N, K, dWq, dCm, dF + 1, nullptr));
        if (a_split & 16) {
            if ((a_split & 1) || K != 384 || (epilogue != 4 && epilogue != 5)) return fail(CS_ERR_UNSUPPORTED, "cs_debug_gemm_q8: the slab kernel takes f32 rows, K = 384, epilogue 4 | 5");
            CS_HIP(hipMalloc(&dCmT, (size_t)N * sizeof(Q8ColMeta)));
            CS_TRY(launch_q8_cmeta_tiles(dCm, N, dCmT, nullptr));
        }
        if (a_split & 1) {
            CS_HIP(hipMalloc(&sA, a_n * 4));
            CS_TRY(launch_split_rows(dA, sA, M, K, dF, nullptr));
            CS_TRY(launch_q8_quantize(Q8_SRC_SPLIT, sA, M, K, dRange, nullptr, dXq, dRm, nullptr));
        } else {
            CS_TRY(launch_q8_quantize(Q8_SRC_F32, dA, M, K, dRange, nullptr, dXq, dRm, nullptr));
        }
        if (epilogue == 5) {  // GELU -> re-quantised (the two-pass FFN-up): C = the uint8 output, xparams[2..3] = its scale / zero point
            int8_t* dOut = nullptr;
            Q8RowMeta* dRm2 = nullptr;
            uint32_t* dRange2 = nullptr;
            CS_HIP(hipMalloc(&dOut, c_n)); CS_HIP(hipMalloc(&dRm2, (size_t)M * sizeof(Q8RowMeta))); CS_HIP(hipMalloc(&dRange2, Q8_RANGE_WORDS * 4));
            CS_HIP(hipMemset(dRange2, 0, Q8_RANGE_WORDS * 4));
            // (a_split & 16: the slab kernel, whatever M — gemm_q8_slab.hip)
            int32_t st5 = (a_split & 16) ? launch_gemm_q8_slab_gelu_requant(dA, dRange, dWq, dCmT, M, N, K, dRange2, dOut, dRm2, q8_gelu_table_on(), nullptr, (a_split & 32) ? dXq : nullptr)
                        : (a_split & 8) ? launch_gemm_q8_gelu_requant_from_source(dA, dRange, dWq, dCm, dB, M, N, K, dRange2, dOut, dRm2, nullptr)
                                        : launch_gemm_q8_gelu_requant(dXq, dRm, dWq, dCm, dB, M, N, K, dRange2, dOut, dRm2, nullptr);
            if (st5 == CS_OK && hipDeviceSynchronize() != hipSuccess) st5 = fail(CS_ERR_HIP, "requant GEMM failed");
            std::vector<int8_t> ho(c_n);
            std::vector<Q8RowMeta> hr(M);
            if (st5 == CS_OK && (hipMemcpy(ho.data(), dOut, c_n, hipMemcpyDeviceToHost) != hipSuccess ||
                                 hipMemcpy(hr.data(), dRm2, (size_t)M * sizeof(Q8RowMeta), hipMemcpyDeviceToHost) != hipSuccess))
                st5 = fail(CS_ERR_HIP, "requant GEMM read-back failed");
            (void)hipFree(dOut); (void)hipFree(dRm2); (void)hipFree(dRange2);
            CS_TRY(st5);
            for (size_t i = 0; i < c_n; ++i) C[i] = (float)((int)ho[i] + 128);
            if (acc_out) for (size_t m = 0; m < M; ++m) acc_out[m] = hr[m].rowsum + 128 * (int32_t)N;  // row sums of the uint8 output
            if (xparams) { xparams[2] = hr[0].xs; xparams[3] = (float)(hr[0].za + 128); }
            uint32_t flags5[2] = {0, 0};
            CS_HIP(hipMemcpy(flags5, dF, 8, hipMemcpyDeviceToHost));
            if (flags5[1]) return fail(CS_ERR_BAD_ARG, "cs_debug_gemm_q8: W is not a quantised matrix for these column scales (flag %u)", flags5[1]);
            if (xq_out || xparams) {
                std::vector<int8_t> hq(a_n);
                Q8RowMeta rm0;
                CS_HIP(hipMemcpy(hq.data(), dXq, a_n, hipMemcpyDeviceToHost));
                CS_HIP(hipMemcpy(&rm0, dRm, sizeof(rm0), hipMemcpyDeviceToHost));
                if (xq_out) for (size_t i = 0; i < a_n; ++i) xq_out[i] = (uint8_t)((int)hq[i] + 128);
                if (xparams) { xparams[0] = rm0.xs; xparams[1] = (float)(rm0.za + 128); }
            }
            return CS_OK;
        }
        const int epi = epilogue == 0 ? SH_OUT_F32 : epilogue == 1 ? SH_OUT_SPLIT_GELU : epilogue == 2 ? SH_OUT_F32_RESID : SH_OUT_SPLIT;
        if (epi == SH_OUT_SPLIT_GELU || epi == SH_OUT_SPLIT) CS_HIP(hipMalloc(&sC, c_n * 4));
        if (a_split & 4) {  // the few-rows kernel: its "pairs" are the one (lo, hi) in the slot (the words are the floats' bits)
            if (dAcc) CS_HIP(hipMemset(dAcc, 0, c_n * 4));
            CS_TRY(launch_gemm_q8_skinny(epi, (a_split & 1) ? Q8_SRC_SPLIT : Q8_SRC_F32, (a_split & 1) ? (const void*)sA : (const void*)dA,
                                         reinterpret_cast<const float*>(dRange), 1, dWq, dCm, dR, dC, sC, M, N, K, dF, nullptr, nullptr, nullptr));
        } else if (a_split & 16) {  // the slab kernel (acc is not reported)
            if (dAcc) CS_HIP(hipMemset(dAcc, 0, c_n * 4));
            CS_TRY(launch_gemm_q8_slab_split(dA, dRange, dWq, dCmT, sC, M, N, K, dF, nullptr));
        } else if (a_split & 8) {  // the products that quantise their own rows on the way in (row-block kernel; acc is not reported)
            if (dAcc) CS_HIP(hipMemset(dAcc, 0, c_n * 4));
            CS_TRY(launch_gemm_q8_from_source(epi, (a_split & 1) ? Q8_SRC_SPLIT : Q8_SRC_F32, (a_split & 1) ? (const void*)sA : (const void*)dA, dRange,
                                              dWq, dCm, dB, dR, dC, sC, M, N, K, dF, nullptr));
        } else
        CS_TRY(launch_gemm_q8(epi, dXq, dRm, dWq, dCm, dB, dR, dC, sC, M, N, K, dF, nullptr, dAcc));
        CS_HIP(hipDeviceSynchronize());
        uint32_t flags[2] = {0, 0};
        CS_HIP(hipMemcpy(flags, dF, 8, hipMemcpyDeviceToHost));
        if (flags[1]) return fail(CS_ERR_BAD_ARG, "cs_debug_gemm_q8: W is not a quantised matrix for these column scales (flag %u)", flags[1]);
        if (sC) {
            std::vector<_Float16> hs(c_n * 2);
            CS_HIP(hipMemcpy(hs.data(), sC, c_n * 4, hipMemcpyDeviceToHost));
            const size_t nch = N / 32;
            for (size_t m = 0; m < M; ++m)
                for (size_t n = 0; n < N; ++n) {
                    const _Float16* line = hs.data() + (m * nch + n / 32) * 64;
                    C[m * N + n] = (float)line[n % 32] + (float)line[32 + n % 32] * (1.0f / 2048.0f);
                }
        } else {
            CS_HIP(hipMemcpy(C, dC, c_n * 4, hipMemcpyDeviceToHost));
        }
        if (acc_out) CS_HIP(hipMemcpy(acc_out, dAcc, c_n * 4, hipMemcpyDeviceToHost));
        if (xq_out || xparams) {
            std::vector<int8_t> hq(a_n);
            Q8RowMeta rm0;
            CS_HIP(hipMemcpy(hq.data(), dXq, a_n, hipMemcpyDeviceToHost));
            CS_HIP(hipMemcpy(&rm0, dRm, sizeof(rm0), hipMemcpyDeviceToHost));
            if (xq_out) for (size_t i = 0; i < a_n; ++i) xq_out[i] = (uint8_t)((int)hq[i] + 128);
            if (xparams) { xparams[0] = rm0.xs; xparams[1] = (float)(rm0.za + 128); }
        }
        return CS_OK;
    };
    const int32_t st = run();
    for (void* p : {(void*)dA, (void*)dW, (void*)dS, (void*)dB, (void*)dR, (void*)dC, (void*)sA, (void*)sC, (void*)dXq, (void*)dWq,
                    (void*)dRm, (void*)dCm, (void*)dF, (void*)dRange, (void*)dAcc, (void*)dCmT})
        if (p) (void)hipFree(p);
    return st;
}

// Diagnostics: the row-block products over a tensor of SEVERAL quantisation units (queued calls in one device batch):
// row_slot [M] as launch_q8_quantize takes it.  epilogue 4 (f32 source -> split store), 2 (split source, + residual) or
// 5 (FFN-up: GELU, quantised again per unit).  row_params [M][4] = per row (x_scale, x_zero_point, out_scale,
// out_zero_point) — the last two only for epilogue 5, where rowsums [M] receives each output row's sum of uint8 values.
int32_t cs_debug_gemm_q8_units(int32_t device, int32_t epilogue, const float* A, const float* W, const float* wscale,
                               const float* bias, const float* resid, float* C, uint32_t M, uint32_t N, uint32_t K,
                               const uint32_t* row_slot, uint32_t units, float* row_params, int32_t* rowsums) {
    if (!A || !W || !wscale || !bias || !C || !row_slot || (epilogue == 2 && !resid)) return fail(CS_ERR_BAD_ARG, "null buffer");
    if (epilogue != 2 && epilogue != 4 && epilogue != 5) return fail(CS_ERR_BAD_ARG, "unknown epilogue %d", epilogue);
    if (M == 0 || units == 0 || N % 128 || !q8_rows_from_source(forward_knobs(), M, K))
        return fail(CS_ERR_UNSUPPORTED, "cs_debug_gemm_q8_units: M=%u N=%u K=%u is not a row-block product", M, N, K);
    for (uint32_t m = 0; m < M; ++m)
        if ((row_slot[m] & 0x7fffffffu) >= units || (m && (row_slot[m] & 0x7fffffffu) < (row_slot[m - 1] & 0x7fffffffu)))
            return fail(CS_ERR_BAD_ARG, "row_slot[%u]: units must be consecutive runs of rows, in order", m);
    int ndev = 0;
    CS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(CS_ERR_HIP, "HIP device %d not available (%d visible)", device, ndev);
    DeviceGuard g(device);
    const size_t a_n = (size_t)M * K, w_n = (size_t)N * K, c_n = (size_t)M * N;
    float *dA = nullptr, *dW = nullptr, *dS = nullptr, *dB = nullptr, *dR = nullptr, *dC = nullptr;
    _Float16 *sA = nullptr, *sC = nullptr;
    int8_t *dXq = nullptr, *dWq = nullptr, *dOut = nullptr;
    Q8RowMeta *dRm = nullptr, *dRm2 = nullptr;
    Q8ColMeta* dCm = nullptr;
    uint32_t *dF = nullptr, *dRange = nullptr, *dRange2 = nullptr, *dSlot = nullptr;
    auto run = [&]() -> int32_t {
        const size_t rbytes = (size_t)units * Q8_RANGE_WORDS * 4;
        CS_HIP(hipMalloc(&dA, a_n * 4)); CS_HIP(hipMalloc(&dW, w_n * 4)); CS_HIP(hipMalloc(&dS, (size_t)N * 4));
        CS_HIP(hipMalloc(&dB, (size_t)N * 4)); CS_HIP(hipMalloc(&dC, c_n * 4)); CS_HIP(hipMalloc(&dF, 16));
        CS_HIP(hipMalloc(&dXq, a_n)); CS_HIP(hipMalloc(&dWq, w_n)); CS_HIP(hipMalloc(&dRm, (size_t)M * sizeof(Q8RowMeta)));
        CS_HIP(hipMalloc(&dCm, (size_t)N * sizeof(Q8ColMeta))); CS_HIP(hipMalloc(&dRange, rbytes)); CS_HIP(hipMalloc(&dRange2, rbytes));
        CS_HIP(hipMalloc(&dSlot, (size_t)M * 4));
        CS_HIP(hipMemcpy(dA, A, a_n * 4, hipMemcpyHostToDevice));
        CS_HIP(hipMemcpy(dW, W, w_n * 4, hipMemcpyHostToDevice));
        CS_HIP(hipMemcpy(dS, wscale, (size_t)N * 4, hipMemcpyHostToDevice));
        CS_HIP(hipMemcpy(dB, bias, (size_t)N * 4, hipMemcpyHostToDevice));
        CS_HIP(hipMemcpy(dSlot, row_slot, (size_t)M * 4, hipMemcpyHostToDevice));
        CS_HIP(hipMemset(dF, 0, 16));
        CS_HIP(hipMemset(dRange, 0, rbytes));
        CS_HIP(hipMemset(dRange2, 0, rbytes));
        CS_TRY(launch_q8_pack_weight(dW, dS, dB, N, K, dWq, dCm, dF + 1, nullptr));
        // the units' ranges by a pass over the tensor (the quantised rows this also writes only serve row_params)
        if (epilogue == 2) {
            CS_HIP(hipMalloc(&sA, a_n * 4));
            CS_HIP(hipMalloc(&dR, c_n * 4));
            CS_HIP(hipMemcpy(dR, resid, c_n * 4, hipMemcpyHostToDevice));
            CS_TRY(launch_split_rows(dA, sA, M, K, dF, nullptr));
            CS_TRY(launch_q8_quantize(Q8_SRC_SPLIT, sA, M, K, dRange, dSlot, dXq, dRm, nullptr));
            CS_TRY(launch_gemm_q8_from_source(SH_OUT_F32_RESID, Q8_SRC_SPLIT, sA, dRange, dWq, dCm, dB, dR, dC, nullptr, M, N, K, dF, nullptr, dSlot));
        } else {
            CS_TRY(launch_q8_quantize(Q8_SRC_F32, dA, M, K, dRange, dSlot, dXq, dRm, nullptr));
            if (epilogue == 4) {
                CS_HIP(hipMalloc(&sC, c_n * 4));
                CS_TRY(launch_gemm_q8_from_source(SH_OUT_SPLIT, Q8_SRC_F32, dA, dRange, dWq, dCm, dB, nullptr, nullptr, sC, M, N, K, dF, nullptr, dSlot));
            } else {
                CS_HIP(hipMalloc(&dOut, c_n));
                CS_HIP(hipMalloc(&dRm2, (size_t)M * sizeof(Q8RowMeta)));
                CS_TRY(launch_gemm_q8_gelu_requant_from_source(dA, dRange, dWq, dCm, dB, M, N, K, dRange2, dOut, dRm2, nullptr, dSlot));
            }
        }
        CS_HIP(hipDeviceSynchronize());
        uint32_t flags[2] = {0, 0};
        CS_HIP(hipMemcpy(flags, dF, 8, hipMemcpyDeviceToHost));
        if (flags[1]) return fail(CS_ERR_BAD_ARG, "cs_debug_gemm_q8_units: W is not a quantised matrix for these column scales (flag %u)", flags[1]);
        std::vector<Q8RowMeta> hr(M), hr2;
        CS_HIP(hipMemcpy(hr.data(), dRm, (size_t)M * sizeof(Q8RowMeta), hipMemcpyDeviceToHost));
        if (epilogue == 5) {
            std::vector<int8_t> ho(c_n);
            hr2.resize(M);
            CS_HIP(hipMemcpy(ho.data(), dOut, c_n, hipMemcpyDeviceToHost));
            CS_HIP(hipMemcpy(hr2.data(), dRm2, (size_t)M * sizeof(Q8RowMeta), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < c_n; ++i) C[i] = (float)((int)ho[i] + 128);
            if (rowsums) for (size_t m = 0; m < M; ++m) rowsums[m] = hr2[m].rowsum + 128 * (int32_t)N;
        } else if (sC) {
            std::vector<_Float16> hs(c_n * 2);
            CS_HIP(hipMemcpy(hs.data(), sC, c_n * 4, hipMemcpyDeviceToHost));
            const size_t nch = N / 32;
            for (size_t m = 0; m < M; ++m)
                for (size_t n = 0; n < N; ++n) {
                    const _Float16* line = hs.data() + (m * nch + n / 32) * 64;
                    C[m * N + n] = (float)line[n % 32] + (float)line[32 + n % 32] * (1.0f / 2048.0f);
                }
        } else {
            CS_HIP(hipMemcpy(C, dC, c_n * 4, hipMemcpyDeviceToHost));
        }
        if (row_params)
            for (size_t m = 0; m < M; ++m) {
                row_params[4 * m] = hr[m].xs;
                row_params[4 * m + 1] = (float)(hr[m].za + 128);
                row_params[4 * m + 2] = epilogue == 5 ? hr2[m].xs : 0.0f;
                row_params[4 * m + 3] = epilogue == 5 ? (float)(hr2[m].za + 128) : 0.0f;
            }
        return CS_OK;
    };
    const int32_t st = run();
    for (void* p : {(void*)dA, (void*)dW, (void*)dS, (void*)dB, (void*)dR, (void*)dC, (void*)sA, (void*)sC, (void*)dXq, (void*)dWq,
                    (void*)dOut, (void*)dRm, (void*)dRm2, (void*)dCm, (void*)dF, (void*)dRange, (void*)dRange2, (void*)dSlot})
        if (p) (void)hipFree(p);
    return st;
}

// Diagnostics: the attention kernels (E3) alone on host buffers — launch_attention_sh2 as the encoder calls it, or (proj_w
// given) attention inside the out-projection, launch_sp_attn_proj.  Buffers hold exactly B * L token rows (the kernels
// clamp their reads to the last one).  Contract in include/codesearch_gpu_diag.h.
int32_t cs_debug_attention(int32_t device, const float* qkv, const int32_t* mask, uint32_t B, uint32_t L, uint32_t H,
                           uint32_t heads, const float* alibi_slopes, uint32_t window, const uint32_t* seq_unit,
                           const uint32_t* unit_len, uint32_t units, const float* proj_w, const float* proj_bias,
                           const float* proj_resid, float* out, float* range_pairs_out, uint32_t range_pairs_cap,
                           uint32_t* range_pairs, uint32_t* range_flag) {
    if (!qkv || !mask || !out) return fail(CS_ERR_BAD_ARG, "null buffer");
    if (B == 0 || L == 0 || H == 0 || heads == 0) return fail(CS_ERR_BAD_ARG, "cs_debug_attention needs B, L, H, heads > 0");
    if (H % heads || (H / heads != 32 && H / heads != 64))
        return fail(CS_ERR_UNSUPPORTED, "head_dim %u not supported (32 or 64)", H / heads);
    if (L > 8192 || (uint64_t)B * L > (1u << 20)) return fail(CS_ERR_UNSUPPORTED, "cs_debug_attention: L <= 8192, B * L <= 2^20");
    if ((units != 0) != (seq_unit != nullptr) || (units != 0) != (unit_len != nullptr))
        return fail(CS_ERR_BAD_ARG, "seq_unit, unit_len and units go together");
    for (uint32_t b = 0; b < B && units; ++b)
        if (seq_unit[b] >= units) return fail(CS_ERR_BAD_ARG, "seq_unit[%u] = %u: only %u units", b, seq_unit[b], units);
    if ((range_pairs_out != nullptr) != (range_pairs != nullptr) || (range_pairs_out && range_pairs_cap == 0))
        return fail(CS_ERR_BAD_ARG, "range_pairs_out, its capacity and range_pairs go together");
    const uint32_t T = B * L;
    if (!proj_w != !proj_bias || !proj_w != !proj_resid) return fail(CS_ERR_BAD_ARG, "proj_w, proj_bias and proj_resid go together");
    if (proj_w) {
        if (alibi_slopes || window || units || range_pairs_out)
            return fail(CS_ERR_BAD_ARG, "attention inside the out-projection takes no ALiBi, window, units or range pairs");
        if (!sp_attn_proj_supported(H, heads, T, L))
            return fail(CS_ERR_UNSUPPORTED, "attention + out-projection in one launch: %u rows of %u tokens, hidden %u, %u heads not built", T, L, H, heads);
    }
    int ndev = 0;
    CS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(CS_ERR_HIP, "HIP device %d not available (%d visible)", device, ndev);
    DeviceGuard g(device);
    const size_t q_n = (size_t)T * 3 * H, c_n = (size_t)T * H;
    // the most pairs a launch writes: one head per block (launch_attention_sh2)
    const size_t pair_cap = (size_t)heads * B * ((L + 127) / 128) * 4;
    float *dQ = nullptr, *dW = nullptr, *dB = nullptr, *dR = nullptr, *dC = nullptr, *dAl = nullptr, *dRp = nullptr;
    _Float16 *sQ = nullptr, *sW = nullptr, *sC = nullptr;
    int32_t* dM = nullptr;
    uint32_t *dF = nullptr, *dSu = nullptr, *dUl = nullptr;
    auto run = [&]() -> int32_t {
        CS_HIP(hipMalloc(&dQ, q_n * 4)); CS_HIP(hipMalloc(&sQ, q_n * 4)); CS_HIP(hipMalloc(&dM, (size_t)T * 4)); CS_HIP(hipMalloc(&dF, 4));
        CS_HIP(hipMemcpy(dQ, qkv, q_n * 4, hipMemcpyHostToDevice));
        CS_HIP(hipMemcpy(dM, mask, (size_t)T * 4, hipMemcpyHostToDevice));
        CS_HIP(hipMemset(dF, 0, 4));
        CS_TRY(launch_split_rows(dQ, sQ, T, 3 * H, dF, nullptr));
        if (proj_w) {
            CS_HIP(hipMalloc(&dW, (size_t)H * H * 4)); CS_HIP(hipMalloc(&sW, (size_t)H * H * 4)); CS_HIP(hipMalloc(&dB, (size_t)H * 4));
            CS_HIP(hipMalloc(&dR, c_n * 4)); CS_HIP(hipMalloc(&dC, c_n * 4));
            CS_HIP(hipMemcpy(dW, proj_w, (size_t)H * H * 4, hipMemcpyHostToDevice));
            CS_HIP(hipMemcpy(dB, proj_bias, (size_t)H * 4, hipMemcpyHostToDevice));
            CS_HIP(hipMemcpy(dR, proj_resid, c_n * 4, hipMemcpyHostToDevice));
            CS_TRY(launch_split_rows(dW, sW, H, H, dF, nullptr));
            CS_TRY(launch_sp_attn_proj(sQ, dM, sW, dB, dR, dC, T, L, H, heads, dF, nullptr));
            CS_HIP(hipDeviceSynchronize());
            CS_HIP(hipMemcpy(out, dC, c_n * 4, hipMemcpyDeviceToHost));
            if (range_flag) CS_HIP(hipMemcpy(range_flag, dF, 4, hipMemcpyDeviceToHost));
            return CS_OK;
        }
        CS_HIP(hipMalloc(&sC, c_n * 4));
        CS_HIP(hipMemset(sC, 0, c_n * 4));
        if (alibi_slopes) {  // [2][heads]: the slopes, then the slopes times log2 e in f32 (embedder.hip)
            std::vector<float> sl(2 * (size_t)heads);
            for (uint32_t i = 0; i < heads; ++i) { sl[i] = alibi_slopes[i]; sl[heads + i] = sl[i] * 1.4426950408889634f; }
            CS_HIP(hipMalloc(&dAl, sl.size() * 4));
            CS_HIP(hipMemcpy(dAl, sl.data(), sl.size() * 4, hipMemcpyHostToDevice));
        }
        if (units) {
            CS_HIP(hipMalloc(&dSu, (size_t)B * 4)); CS_HIP(hipMalloc(&dUl, (size_t)units * 4));
            CS_HIP(hipMemcpy(dSu, seq_unit, (size_t)B * 4, hipMemcpyHostToDevice));
            CS_HIP(hipMemcpy(dUl, unit_len, (size_t)units * 4, hipMemcpyHostToDevice));
        }
        if (range_pairs_out) {
            CS_HIP(hipMalloc(&dRp, pair_cap * 8));
            CS_HIP(hipMemset(dRp, 0, pair_cap * 8));
        }
        uint32_t pairs = 0;
        CS_TRY(launch_attention_sh2(sQ, dM, sC, dF, B, L, H, heads, nullptr, dRp, range_pairs_out ? &pairs : nullptr, dSu, dUl, dAl, window));
        CS_HIP(hipDeviceSynchronize());
        if (range_pairs_out) {
            *range_pairs = pairs;
            if (pairs > pair_cap) return fail(CS_ERR_HIP, "attention reported %u range pairs, more than one per wave (%zu)", pairs, pair_cap);
            if (pairs > range_pairs_cap) return fail(CS_ERR_BAD_ARG, "range_pairs_out holds %u pairs, the launch wrote %u", range_pairs_cap, pairs);
            CS_HIP(hipMemcpy(range_pairs_out, dRp, (size_t)pairs * 8, hipMemcpyDeviceToHost));
        }
        std::vector<_Float16> hs(c_n * 2);
        CS_HIP(hipMemcpy(hs.data(), sC, c_n * 4, hipMemcpyDeviceToHost));
        const size_t nch = H / 32;
        for (size_t m = 0; m < T; ++m)
            for (size_t n = 0; n < H; ++n) {
                const _Float16* line = hs.data() + (m * nch + n / 32) * 64;
                out[m * H + n] = (float)line[n % 32] + (float)line[32 + n % 32] * (1.0f / 2048.0f);
            }
        if (range_flag) CS_HIP(hipMemcpy(range_flag, dF, 4, hipMemcpyDeviceToHost));
        return CS_OK;
    };
    const int32_t st = run();
    if (st != CS_OK) (void)hipDeviceSynchronize();
    for (void* p : {(void*)dQ, (void*)dW, (void*)dB, (void*)dR, (void*)dC, (void*)dAl, (void*)dRp, (void*)sQ, (void*)sW, (void*)sC,
                    (void*)dM, (void*)dF, (void*)dSu, (void*)dUl})
        if (p) (void)hipFree(p);
    return st;
}

}  // extern "C"

namespace {

// The device buffers of one diagnostic call: freed together when the call returns, after the device has gone idle.
struct DiagBufs {
    std::vector<void*> owned;
    ~DiagBufs() {
        (void)hipDeviceSynchronize();
        for (void* q : owned) (void)hipFree(q);
    }
    template <class T>
    int32_t get(T** out, size_t bytes, const void* host = nullptr) {
        void* q = nullptr;
        CS_HIP(hipMalloc(&q, bytes ? bytes : 4));
        owned.push_back(q);
        if (host && bytes) CS_HIP(hipMemcpy(q, host, bytes, hipMemcpyHostToDevice));
        *out = static_cast<T*>(q);
        return CS_OK;
    }
};

int32_t diag_device(int32_t device) {
    int ndev = 0;
    CS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(CS_ERR_HIP, "HIP device %d not available (%d visible)", device, ndev);
    return CS_OK;
}

// a split tensor [rows][N/32][64] on the device -> f32 [rows][N] on the host, hi + lo / 2048
int32_t diag_read_split(const _Float16* d_split, size_t rows, size_t N, float* out) {
    std::vector<_Float16> hs(rows * N * 2);
    CS_HIP(hipMemcpy(hs.data(), d_split, rows * N * 4, hipMemcpyDeviceToHost));
    const size_t nch = N / 32;
    for (size_t m = 0; m < rows; ++m)
        for (size_t n = 0; n < N; ++n) {
            const _Float16* line = hs.data() + (m * nch + n / 32) * 64;
            out[m * N + n] = (float)line[n % 32] + (float)line[32 + n % 32] * (1.0f / 2048.0f);
        }
    return CS_OK;
}

}  // namespace

extern "C" {

// Diagnostics: the row kernels of encoder.hip alone on host buffers — launch_row_kernel as the embedder calls it.  Contract
// in include/codesearch_gpu_diag.h.
int32_t cs_debug_rows(int32_t device, int32_t which, uint32_t H, uint32_t T, uint32_t L, uint32_t B, float eps, int32_t pooling,
                      const int32_t* ids, const float* word, const float* pos, const float* type_table, const int32_t* types,
                      uint32_t ntypes, uint32_t vocab, const float* x, const int32_t* mask, const float* parts, uint32_t nparts,
                      const float* bias, const float* gamma, const float* beta, int32_t range_mode, float* out, float* out_split,
                      float* src_after, float* range_out, uint32_t* range_flag) {
    if (which < 0 || which > 4) return fail(CS_ERR_BAD_ARG, "cs_debug_rows: which = %d (0 embeddings, 1 LayerNorm, 2 pooling, 3 slab sum, 4 LayerNorm of a source)", which);
    if (!out || H == 0) return fail(CS_ERR_BAD_ARG, "cs_debug_rows: null output or H = 0");
    if (which == 2) {
        if (!x || !mask || B == 0 || L == 0) return fail(CS_ERR_BAD_ARG, "cs_debug_rows: pooling needs x, mask, B > 0 and L > 0");
        if (pooling != CS_POOL_CLS && pooling != CS_POOL_MEAN) return fail(CS_ERR_BAD_ARG, "cs_debug_rows: unknown pooling %d", pooling);
        if (out_split || src_after || range_mode) return fail(CS_ERR_BAD_ARG, "cs_debug_rows: pooling writes f32 rows only");
        T = B * L;
    } else {
        if (T == 0 || !gamma || !beta) return fail(CS_ERR_BAD_ARG, "cs_debug_rows: needs T > 0, gamma and beta");
        if (which == 0 && (!ids || !word || !type_table || vocab == 0 || ntypes == 0 || L == 0))
            return fail(CS_ERR_BAD_ARG, "cs_debug_rows: the embedding kernel needs ids, the word and type tables, vocab, ntypes and L > 0");
        if (which != 0 && !x) return fail(CS_ERR_BAD_ARG, "cs_debug_rows: null input rows");
        if (which == 3 && (!parts || !bias || nparts == 0)) return fail(CS_ERR_BAD_ARG, "cs_debug_rows: the slab sum needs parts, bias and nparts > 0");
        if (range_mode < 0 || range_mode > 2 || (range_mode != 0) != (range_out != nullptr))
            return fail(CS_ERR_BAD_ARG, "cs_debug_rows: range_mode (1 per block, 2 per row) and range_out go together");
        if (range_mode && which != 0 && which != 1) return fail(CS_ERR_BAD_ARG, "cs_debug_rows: only kernels 0 and 1 report ranges");
        if (src_after && which != 4) return fail(CS_ERR_BAD_ARG, "cs_debug_rows: src_after belongs to kernel 4");
    }
    if ((uint64_t)T * H > (1ull << 28)) return fail(CS_ERR_UNSUPPORTED, "cs_debug_rows: T * H <= 2^28");
    CS_TRY(diag_device(device));
    DeviceGuard g(device);
    DiagBufs bufs;
    const size_t row_n = (size_t)T * H;
    EncoderLaunch a;
    float *dX = nullptr, *dSrc = nullptr, *dOut = nullptr, *dRange = nullptr;
    _Float16* dXs = nullptr;
    uint32_t* dF = nullptr;
    CS_TRY(bufs.get(&dF, 4));
    CS_HIP(hipMemset(dF, 0, 4));
    a.flag = dF;
    a.eps = eps;
    a.T = T; a.L = L; a.B = B;
    if (which == 2) {
        int32_t* dM = nullptr;
        CS_TRY(bufs.get(&dX, row_n * 4, x));
        CS_TRY(bufs.get(&dM, (size_t)T * 4, mask));
        CS_TRY(bufs.get(&dOut, (size_t)B * H * 4));
        CS_HIP(hipMemset(dOut, 0xff, (size_t)B * H * 4));
        a.x = dX; a.mask = dM; a.out = dOut; a.pooling = pooling;
        CS_TRY(launch_row_kernel(2, a, H, nullptr));
        CS_HIP(hipDeviceSynchronize());
        CS_HIP(hipMemcpy(out, dOut, (size_t)B * H * 4, hipMemcpyDeviceToHost));
        if (range_flag) CS_HIP(hipMemcpy(range_flag, dF, 4, hipMemcpyDeviceToHost));
        return CS_OK;
    }
    float *dG = nullptr, *dB = nullptr;
    CS_TRY(bufs.get(&dG, (size_t)H * 4, gamma));
    CS_TRY(bufs.get(&dB, (size_t)H * 4, beta));
    a.g = dG; a.b = dB;
    if (which == 0) {
        int32_t *dIds = nullptr, *dTypes = nullptr;
        float *dWord = nullptr, *dPos = nullptr, *dType = nullptr;
        CS_TRY(bufs.get(&dIds, (size_t)T * 4, ids));
        CS_TRY(bufs.get(&dWord, (size_t)vocab * H * 4, word));
        CS_TRY(bufs.get(&dType, (size_t)ntypes * H * 4, type_table));
        if (pos) CS_TRY(bufs.get(&dPos, (size_t)L * H * 4, pos));
        if (types) CS_TRY(bufs.get(&dTypes, (size_t)T * 4, types));
        CS_TRY(bufs.get(&dX, row_n * 4));
        CS_HIP(hipMemset(dX, 0xff, row_n * 4));
        a.ids = dIds; a.word = dWord; a.pos = dPos; a.type0 = dType; a.types = dTypes; a.ntypes = ntypes; a.vocab = vocab;
    } else if (which == 4) {
        CS_TRY(bufs.get(&dSrc, row_n * 4, x));
        CS_TRY(bufs.get(&dX, row_n * 4));
        CS_HIP(hipMemset(dX, 0xff, row_n * 4));
        a.src = dSrc;
    } else {
        CS_TRY(bufs.get(&dX, row_n * 4, x));
        if (which == 3) {
            float *dParts = nullptr, *dBias = nullptr;
            CS_TRY(bufs.get(&dParts, (size_t)nparts * row_n * 4, parts));
            CS_TRY(bufs.get(&dBias, (size_t)H * 4, bias));
            a.parts = dParts; a.nparts = nparts; a.bias = dBias;
        }
    }
    a.x = dX;
    if (out_split) {
        if (H % 32) return fail(CS_ERR_UNSUPPORTED, "cs_debug_rows: the split form needs H %% 32 == 0");
        CS_TRY(bufs.get(&dXs, row_n * 4));
        CS_HIP(hipMemset(dXs, 0xff, row_n * 4));
        a.xs = dXs;
    }
    const size_t range_pairs = range_mode == 2 ? T : (T + 3) / 4;
    if (range_mode) {  // unwritten pairs come back as NaN
        CS_TRY(bufs.get(&dRange, range_pairs * 8));
        CS_HIP(hipMemset(dRange, 0xff, range_pairs * 8));
        a.range_out = dRange;
        a.range_rows = range_mode == 2;
    }
    CS_TRY(launch_row_kernel(which, a, H, nullptr));
    CS_HIP(hipDeviceSynchronize());
    CS_HIP(hipMemcpy(out, dX, row_n * 4, hipMemcpyDeviceToHost));
    if (out_split) CS_TRY(diag_read_split(dXs, T, H, out_split));
    if (src_after) CS_HIP(hipMemcpy(src_after, dSrc, row_n * 4, hipMemcpyDeviceToHost));
    if (range_mode) CS_HIP(hipMemcpy(range_out, dRange, range_pairs * 8, hipMemcpyDeviceToHost));
    if (range_flag) CS_HIP(hipMemcpy(range_flag, dF, 4, hipMemcpyDeviceToHost));
    return CS_OK;
}

// Diagnostics: the element-wise kernels of nomic.hip alone on host buffers — the rotary map (op 0), the feed-forward gate
// (op 1) and the query / key LayerNorm (op 2), each in its split and its f32 form.  Contract in include/codesearch_gpu_diag.h.
int32_t cs_debug_elementwise(int32_t device, int32_t op, int32_t split, uint32_t T, uint32_t L, uint32_t H, uint32_t heads,
                             uint32_t I, int32_t gelu_gate, float eps, const float* a, const float* b, const float* table,
                             float* out, uint32_t* flags) {
    if (op < 0 || op > 2) return fail(CS_ERR_BAD_ARG, "cs_debug_elementwise: op = %d (0 rotary map, 1 gate, 2 query / key LayerNorm)", op);
    if (!a || !out || T == 0) return fail(CS_ERR_BAD_ARG, "cs_debug_elementwise: null buffer or T = 0");
    if (op == 1 ? I == 0 : H == 0) return fail(CS_ERR_BAD_ARG, "cs_debug_elementwise: zero width");
    if (op != 1 && !table) return fail(CS_ERR_BAD_ARG, "cs_debug_elementwise: the rotary map needs its (cos, sin) table, the LayerNorm its four vectors");
    if (op == 0 && (L == 0 || heads == 0 || H % heads)) return fail(CS_ERR_BAD_ARG, "cs_debug_elementwise: the rotary map needs L > 0 and heads dividing H");
    if (op == 1 && !split && (!b || I % 4)) return fail(CS_ERR_BAD_ARG, "cs_debug_elementwise: the f32 gate needs the gate matrix and I %% 4 == 0");
    const size_t width = op == 1 ? (split ? 2 * (size_t)I : (size_t)I) : 3 * (size_t)H;  // of the input rows
    const size_t out_w = op == 1 ? (size_t)I : width;
    if ((uint64_t)T * width > (1ull << 28)) return fail(CS_ERR_UNSUPPORTED, "cs_debug_elementwise: T * row width <= 2^28");
    CS_TRY(diag_device(device));
    DeviceGuard g(device);
    DiagBufs bufs;
    float *dA = nullptr, *dB = nullptr, *dT = nullptr;
    _Float16 *sA = nullptr, *sO = nullptr;
    uint32_t* dF = nullptr;  // [0] the kernel's flag, [1] the input split's
    CS_TRY(bufs.get(&dF, 8));
    CS_HIP(hipMemset(dF, 0, 8));
    CS_TRY(bufs.get(&dA, (size_t)T * width * 4, a));
    if (op == 0) CS_TRY(bufs.get(&dT, (size_t)L * (H / heads / 2) * 8, table));
    if (op == 2) CS_TRY(bufs.get(&dT, (size_t)4 * H * 4, table));
    if (split) {
        CS_TRY(bufs.get(&sA, (size_t)T * width * 4));
        CS_HIP(hipMemset(sA, 0, (size_t)T * width * 4));
        // (a width the split form cannot hold goes to the launcher unsplit: its refusal is the answer)
        if (width % 32 == 0) CS_TRY(launch_split_rows(dA, sA, T, (uint32_t)width, dF + 1, nullptr));
    }
    if (op == 0) {
        if (split) CS_TRY(launch_rope_split(sA, reinterpret_cast<const float2*>(dT), T, L, H, heads, dF, nullptr));
        else CS_TRY(launch_rope_f32(dA, reinterpret_cast<const float2*>(dT), T, L, H, heads, nullptr));
    } else if (op == 1) {
        if (split) {
            CS_TRY(bufs.get(&sO, (size_t)T * I * 4));
            CS_HIP(hipMemset(sO, 0xff, (size_t)T * I * 4));
            CS_TRY(launch_swiglu_split(sA, sO, T, I, dF, nullptr, gelu_gate != 0));
        } else {
            CS_TRY(bufs.get(&dB, (size_t)T * I * 4, b));
            CS_TRY(launch_swiglu_f32(dA, dB, T, I, nullptr, gelu_gate != 0));
        }
    } else {
        if (split) CS_TRY(launch_qk_layernorm_split(sA, dT, eps, T, H, dF, nullptr));
        else CS_TRY(launch_qk_layernorm_f32(dA, dT, eps, T, H, nullptr));
    }
    CS_HIP(hipDeviceSynchronize());
    if (split) CS_TRY(diag_read_split(sO ? sO : sA, T, out_w, out));
    else CS_HIP(hipMemcpy(out, dA, (size_t)T * out_w * 4, hipMemcpyDeviceToHost));
    if (flags) CS_HIP(hipMemcpy(flags, dF, 8, hipMemcpyDeviceToHost));
    return CS_OK;
}

// Diagnostics: the CLS tail's own kernels (cls_tail.hip) alone on host buffers: the one-query attention and the gather of
// the CLS rows.  Contract in include/codesearch_gpu_diag.h.
int32_t cs_debug_attention_cls(int32_t device, const float* qkv, const int32_t* mask, uint32_t B, uint32_t L, uint32_t H,
                               uint32_t heads, float* out, uint32_t* flags, const float* gather_src, float* x_cls,
                               uint16_t* xs_cls) {
    if ((qkv != nullptr) != (mask != nullptr) || (qkv != nullptr) != (out != nullptr))
        return fail(CS_ERR_BAD_ARG, "cs_debug_attention_cls: qkv, mask and out go together");
    if ((gather_src != nullptr) != (x_cls != nullptr) || (gather_src != nullptr) != (xs_cls != nullptr))
        return fail(CS_ERR_BAD_ARG, "cs_debug_attention_cls: gather_src, x_cls and xs_cls go together");
    if (!qkv && !gather_src) return fail(CS_ERR_BAD_ARG, "cs_debug_attention_cls: nothing to run");
    if (B == 0 || L == 0 || H == 0 || H % 32) return fail(CS_ERR_BAD_ARG, "cs_debug_attention_cls needs B, L > 0 and H a multiple of 32");
    if ((uint64_t)B * L > (1u << 20)) return fail(CS_ERR_UNSUPPORTED, "cs_debug_attention_cls: B * L <= 2^20");
    CS_TRY(diag_device(device));
    DeviceGuard g(device);
    DiagBufs bufs;
    const size_t T = (size_t)B * L;
    uint32_t* dF = nullptr;  // [0] the kernel's flag, [1] the input split's
    CS_TRY(bufs.get(&dF, 8));
    CS_HIP(hipMemset(dF, 0, 8));
    if (qkv) {
        float* dQ = nullptr;
        _Float16 *sQ = nullptr, *kvs = nullptr, *q_cls = nullptr, *ctxs = nullptr;
        int32_t* dM = nullptr;
        const size_t rowb = (size_t)3 * H * 4;  // bytes of a qkv row, f32 or split
        CS_TRY(bufs.get(&dQ, T * rowb, qkv));
        CS_TRY(bufs.get(&dM, T * 4, mask));
        CS_TRY(bufs.get(&sQ, T * rowb));
        CS_TRY(bufs.get(&kvs, T * (size_t)2 * H * 4));
        CS_TRY(bufs.get(&q_cls, (size_t)B * H * 4));
        CS_TRY(bufs.get(&ctxs, (size_t)B * H * 4));
        CS_HIP(hipMemset(ctxs, 0xff, (size_t)B * H * 4));
        CS_TRY(launch_split_rows(dQ, sQ, T, 3 * H, dF + 1, nullptr));
        // kvs [T][2H/32][64]: per token the K lines, then the V lines; q_cls [B][H/32][64]: the Q lines of the rows b * L
        CS_HIP(hipMemcpy2D(kvs, (size_t)2 * H * 4, reinterpret_cast<const char*>(sQ) + (size_t)H * 4, rowb, (size_t)2 * H * 4, T, hipMemcpyDeviceToDevice));
        CS_HIP(hipMemcpy2D(q_cls, (size_t)H * 4, sQ, (size_t)L * rowb, (size_t)H * 4, B, hipMemcpyDeviceToDevice));
        CS_TRY(launch_attention_cls(q_cls, kvs, dM, ctxs, dF, B, L, H, heads, nullptr));
        CS_HIP(hipDeviceSynchronize());
        CS_TRY(diag_read_split(ctxs, B, H, out));
    }
    if (gather_src) {
        float *dX = nullptr, *dXc = nullptr;
        _Float16 *sX = nullptr, *sXc = nullptr;
        CS_TRY(bufs.get(&dX, T * H * 4, gather_src));
        CS_TRY(bufs.get(&sX, T * H * 4));
        CS_TRY(bufs.get(&dXc, (size_t)B * H * 4));
        CS_TRY(bufs.get(&sXc, (size_t)B * H * 4));
        CS_HIP(hipMemset(dXc, 0xff, (size_t)B * H * 4));
        CS_HIP(hipMemset(sXc, 0xff, (size_t)B * H * 4));
        CS_TRY(launch_split_rows(dX, sX, T, H, dF + 1, nullptr));
        CS_TRY(launch_gather_cls(sX, dXc, sXc, B, L, H, nullptr));
        CS_HIP(hipDeviceSynchronize());
        CS_HIP(hipMemcpy(x_cls, dXc, (size_t)B * H * 4, hipMemcpyDeviceToHost));
        CS_HIP(hipMemcpy(xs_cls, sXc, (size_t)B * H * 4, hipMemcpyDeviceToHost));
    }
    if (flags) CS_HIP(hipMemcpy(flags, dF, 8, hipMemcpyDeviceToHost));
    return CS_OK;
}

// Diagnostics: the exact-f32 attention kernels of encoder.hip (attention_kernel<false>, attention64_kernel) alone on host
// buffers — launch_attention as the f32 forward and every re-run after a raised range flag call it.
int32_t cs_debug_attention_f32(int32_t device, const float* qkv, const int32_t* mask, uint32_t B, uint32_t L, uint32_t H,
                               uint32_t heads, const float* alibi_slopes, uint32_t window, float* out) {
    if (!qkv || !mask || !out) return fail(CS_ERR_BAD_ARG, "null buffer");
    if (B == 0 || L == 0 || H == 0 || heads == 0) return fail(CS_ERR_BAD_ARG, "cs_debug_attention_f32 needs B, L, H, heads > 0");
    if (L > 512 || (uint64_t)B * L > (1u << 20)) return fail(CS_ERR_UNSUPPORTED, "cs_debug_attention_f32: L <= 512, B * L <= 2^20");
    CS_TRY(diag_device(device));
    DeviceGuard g(device);
    DiagBufs bufs;
    const size_t T = (size_t)B * L;
    float *dQ = nullptr, *dC = nullptr, *dAl = nullptr;
    int32_t* dM = nullptr;
    CS_TRY(bufs.get(&dQ, T * 3 * H * 4, qkv));
    CS_TRY(bufs.get(&dM, T * 4, mask));
    CS_TRY(bufs.get(&dC, T * H * 4));
    CS_HIP(hipMemset(dC, 0xff, T * H * 4));
    if (alibi_slopes) CS_TRY(bufs.get(&dAl, (size_t)heads * 4, alibi_slopes));
    CS_TRY(launch_attention(dQ, dM, dC, B, L, H, heads, nullptr, dAl, window));
    CS_HIP(hipDeviceSynchronize());
    CS_HIP(hipMemcpy(out, dC, T * H * 4, hipMemcpyDeviceToHost));
    return CS_OK;
}

// Diagnostics: the dense kernels of the small path (small_path.hip) alone on host buffers — launch_sp_ln_gemm (op 0) and
// launch_sp_partial (op 1) as Slice::run_small calls them, the route (narrow or wide form) chosen by the launcher.  Every
// input holds exactly T rows (the kernels clamp their reads to row T - 1); every output is followed by kSpGuardRows rows of a
// bit pattern that must come back unchanged.  Contract in include/codesearch_gpu_diag.h.
constexpr uint32_t kSpGuardRows = 16, kSpGuardWord = 0xA5A5A5A5u;

int32_t cs_debug_small_path(int32_t device, int32_t op, int32_t epi, int32_t pro, uint32_t H, uint32_t T, uint32_t N, uint32_t L,
                            float eps, const float* gamma, const float* beta, const float* rows, const float* parts,
                            const float* parts_bias, const float* x, const int32_t* ids, const float* word, const float* pos,
                            const float* type_table, const int32_t* types, uint32_t ntypes, uint32_t vocab, const float* W,
                            const float* bias, float* xout, float* cs_out, float* x_after, float* parts_out, uint32_t* flags,
                            uint32_t* guard_changed) {
    if (op != 0 && op != 1) return fail(CS_ERR_BAD_ARG, "cs_debug_small_path: op = %d (0 LayerNorm + product, 1 FFN-down K slices)", op);
    if (H != 384 && H != 768 && H != 1024) return fail(CS_ERR_UNSUPPORTED, "hidden size %u not supported (384/768/1024)", H);
    if (T == 0 || T > SP_MAX_ROWS || N == 0 || N % 32) return fail(CS_ERR_BAD_ARG, "cs_debug_small_path needs 1 <= T <= %u and N a positive multiple of 32", SP_MAX_ROWS);
    if (!W || !guard_changed) return fail(CS_ERR_BAD_ARG, "cs_debug_small_path: null weights or guard counter");
    if (op == 0) {
        if (epi != 0 && epi != 1) return fail(CS_ERR_BAD_ARG, "cs_debug_small_path: epi = %d (0 split, 1 GELU -> split)", epi);
        if (pro < 0 || pro > 2) return fail(CS_ERR_BAD_ARG, "cs_debug_small_path: pro = %d (0 rows, 1 slab sum, 2 embedding gather)", pro);
        if (!gamma || !beta || !bias || !xout || !cs_out) return fail(CS_ERR_BAD_ARG, "cs_debug_small_path: op 0 needs gamma, beta, bias, xout and cs_out");
        if (pro == 0 && !rows) return fail(CS_ERR_BAD_ARG, "cs_debug_small_path: prologue 0 needs its rows");
        if (pro == 1 && (!parts || !parts_bias || !x)) return fail(CS_ERR_BAD_ARG, "cs_debug_small_path: prologue 1 needs parts, parts_bias and x");
        if (pro == 2 && (!ids || !word || !pos || !type_table || vocab == 0 || ntypes == 0 || L == 0))
            return fail(CS_ERR_BAD_ARG, "cs_debug_small_path: prologue 2 needs ids, the word, position and type tables, vocab, ntypes and L > 0");
        if (x_after && pro != 1) return fail(CS_ERR_BAD_ARG, "cs_debug_small_path: x_after belongs to prologue 1");
    } else if (!rows || !parts_out) {
        return fail(CS_ERR_BAD_ARG, "cs_debug_small_path: op 1 needs its rows and parts_out");
    }
    CS_TRY(diag_device(device));
    DeviceGuard g(device);
    DiagBufs bufs;
    const uint32_t K = op == 0 ? H : 4 * H;
    const size_t row_n = (size_t)T * H, w_n = (size_t)N * K;
    uint32_t* dF = nullptr;  // [0] the kernel's flag, [1] that of the operands' split
    float* dW = nullptr;
    _Float16* sW = nullptr;
    CS_TRY(bufs.get(&dF, 8));
    CS_HIP(hipMemset(dF, 0, 8));
    CS_TRY(bufs.get(&dW, w_n * 4, W));
    CS_TRY(bufs.get(&sW, w_n * 4));
    CS_TRY(launch_split_rows(dW, sW, N, K, dF + 1, nullptr));
    // an output of `rows` rows of `row_bytes` each, followed by the guard rows
    std::vector<std::pair<const char*, size_t>> guards;
    auto guarded = [&](auto** out, size_t rows_, size_t row_bytes) -> int32_t {
        const size_t body = rows_ * row_bytes, tail = (size_t)kSpGuardRows * row_bytes;
        CS_TRY(bufs.get(out, body + tail));
        CS_HIP(hipMemset(*out, 0xff, body));  // an element the launch does not write comes back as NaN
        CS_HIP(hipMemset(reinterpret_cast<char*>(*out) + body, 0xA5, tail));
        guards.emplace_back(reinterpret_cast<const char*>(*out) + body, tail);
        return CS_OK;
    };
    auto count_guards = [&]() -> int32_t {
        uint32_t changed = 0;
        for (const auto& gd : guards) {
            std::vector<uint32_t> hw(gd.second / 4);
            CS_HIP(hipMemcpy(hw.data(), gd.first, gd.second, hipMemcpyDeviceToHost));
            for (uint32_t w : hw) changed += w != kSpGuardWord;
        }
        *guard_changed = changed;
        return CS_OK;
    };
    if (op == 1) {
        float *dA = nullptr, *dParts = nullptr;
        _Float16* sA = nullptr;
        CS_TRY(bufs.get(&dA, (size_t)T * K * 4, rows));
        CS_TRY(bufs.get(&sA, (size_t)T * K * 4));
        CS_TRY(launch_split_rows(dA, sA, T, K, dF + 1, nullptr));
        CS_TRY(guarded(&dParts, (size_t)4 * T, (size_t)N * 4));  // [4][T][N]: the guard rows follow slab 3's row T - 1
        CS_TRY(launch_sp_partial(sA, sW, dParts, T, N, H, nullptr));
        CS_HIP(hipDeviceSynchronize());
        CS_HIP(hipMemcpy(parts_out, dParts, (size_t)4 * T * N * 4, hipMemcpyDeviceToHost));
        if (flags) CS_HIP(hipMemcpy(flags, dF, 8, hipMemcpyDeviceToHost));
        return count_guards();
    }
    SpLnGemmArgs a{};
    float *dG = nullptr, *dBe = nullptr, *dBias = nullptr, *dXout = nullptr, *dX = nullptr;
    _Float16* dCs = nullptr;
    CS_TRY(bufs.get(&dG, (size_t)H * 4, gamma));
    CS_TRY(bufs.get(&dBe, (size_t)H * 4, beta));
    CS_TRY(bufs.get(&dBias, (size_t)N * 4, bias));
    if (pro == 0) {
        float* dY = nullptr;
        CS_TRY(bufs.get(&dY, row_n * 4, rows));
        a.Y = dY;
    } else if (pro == 1) {
        float *dParts = nullptr, *dPb = nullptr;
        CS_TRY(bufs.get(&dParts, 4 * row_n * 4, parts));  // [4][T][H], slab stride T
        CS_TRY(bufs.get(&dPb, (size_t)H * 4, parts_bias));
        CS_TRY(bufs.get(&dX, row_n * 4, x));
        a.parts = dParts; a.parts_bias = dPb; a.X = dX;
    } else {
        int32_t *dIds = nullptr, *dTypes = nullptr;
        float *dWord = nullptr, *dPos = nullptr, *dType = nullptr;
        CS_TRY(bufs.get(&dIds, (size_t)T * 4, ids));
        CS_TRY(bufs.get(&dWord, (size_t)vocab * H * 4, word));
        CS_TRY(bufs.get(&dPos, (size_t)L * H * 4, pos));
        CS_TRY(bufs.get(&dType, (size_t)ntypes * H * 4, type_table));
        if (types) CS_TRY(bufs.get(&dTypes, (size_t)T * 4, types));
        a.ids = dIds; a.word = dWord; a.pos = dPos; a.type0 = dType; a.types = dTypes; a.ntypes = ntypes; a.vocab = vocab;
    }
    CS_TRY(guarded(&dXout, T, (size_t)H * 4));  // never the buffer X is read from, as in the embedder
    CS_TRY(guarded(&dCs, T, (size_t)N * 4));
    a.L = L; a.ln_g = dG; a.ln_b = dBe; a.eps = eps; a.Xout = dXout; a.W = sW; a.bias = dBias; a.Cs = dCs; a.T = T; a.N = N; a.flag = dF;
    CS_TRY(launch_sp_ln_gemm(epi ? SH_OUT_SPLIT_GELU : SH_OUT_SPLIT, pro, a, H, nullptr));
    CS_HIP(hipDeviceSynchronize());
    CS_HIP(hipMemcpy(xout, dXout, row_n * 4, hipMemcpyDeviceToHost));
    CS_TRY(diag_read_split(dCs, T, N, cs_out));
    if (x_after) CS_HIP(hipMemcpy(x_after, dX, row_n * 4, hipMemcpyDeviceToHost));
    if (flags) CS_HIP(hipMemcpy(flags, dF, 8, hipMemcpyDeviceToHost));
    return count_guards();
}

// Diagnostics: device time of one dense layer on synthetic operands already in HBM (no PCIe, no allocation inside the
// timed region).  mode as cs_debug_gemm (0 f32 MFMA, 1 split-f16 128 x 128 / skinny kernels, 2 split-f16 wide kernel);
// epilogue 0 f32 store, 1 GELU -> split store, 2 + residual, 3 LayerNorm-fused (mode 2, N = 384), 4 bias -> split store
// (the QKV projection).  `ablation` (mode 2, epilogue 4 only): 1 no LDS-DMA, 2 no MFMA, 3 DMAs issued at the step start.
int32_t cs_debug_gemm_time(int32_t device, int32_t mode, int32_t epilogue, uint32_t M, uint32_t N, uint32_t K,
                           uint32_t iters, int32_t ablation, double* ms_per_launch) {
    if (!ms_per_launch || iters == 0 || M == 0 || N % 128 || K % 32 || K == 0) return fail(CS_ERR_BAD_ARG, "bad arguments");
    int ndev = 0;
    CS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(CS_ERR_HIP, "HIP device %d not available (%d visible)", device, ndev);
    DeviceGuard g(device);
    const size_t a_n = (size_t)M * K, w_n = (size_t)N * K, c_n = (size_t)M * N;
    float *dA = nullptr, *dW = nullptr, *dB = nullptr, *dR = nullptr, *dC = nullptr;
    _Float16 *sA = nullptr, *sW = nullptr, *sC = nullptr;
    uint32_t* dF = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int32_t {
        CS_HIP(hipMalloc(&dA, a_n * 4)); CS_HIP(hipMalloc(&dW, w_n * 4)); CS_HIP(hipMalloc(&dB, (size_t)N * 4));
        CS_HIP(hipMalloc(&dC, c_n * 4)); CS_HIP(hipMalloc(&dR, c_n * 4)); CS_HIP(hipMalloc(&dF, 4));
        CS_HIP(hipMalloc(&sA, a_n * 4)); CS_HIP(hipMalloc(&sW, w_n * 4)); CS_HIP(hipMalloc(&sC, c_n * 4));
        // operands from the counter-based generator: unit-scale activations, weights / 20
        CS_TRY(launch_synth_fill(dA, M, K, 11, 0, nullptr));
        CS_TRY(launch_synth_fill(dW, N, K, 12, 0, nullptr));
        CS_TRY(launch_synth_fill(dR, M, N, 13, 0, nullptr));
        if (cs_lab_env("CS_DEBUG_GEMM_ZERO")) {  // all-zero operands: what the clock (DVFS), not the schedule, is worth
            CS_HIP(hipMemset(dA, 0, a_n * 4)); CS_HIP(hipMemset(dW, 0, w_n * 4)); CS_HIP(hipMemset(dR, 0, c_n * 4));
        }
        CS_HIP(hipMemset(dB, 0, (size_t)N * 4));
        CS_HIP(hipMemset(dF, 0, 4));
        CS_TRY(launch_split_rows(dA, sA, M, K, dF, nullptr));
        CS_TRY(launch_split_rows(dW, sW, N, K, dF, nullptr));
        CS_HIP(hipEventCreate(&e0)); CS_HIP(hipEventCreate(&e1));
        auto once = [&]() -> int32_t {
            if (mode == CS_GEMM_F32)
                return launch_gemm(epilogue == 1 ? GEMM_GELU : epilogue == 2 ? GEMM_RESID : GEMM_BIAS, dA, dW, dB, dR, dC, M, N, K, nullptr);
            if (epilogue == 3) return launch_gemm_wide_ln(sA, sW, dB, dR, dB, dB, 1e-12f, dR, sC, M, K, dF, nullptr);
            const int epi = epilogue == 0 ? SH_OUT_F32 : epilogue == 1 ? SH_OUT_SPLIT_GELU : epilogue == 2 ? SH_OUT_F32_RESID : SH_OUT_SPLIT;
            if (mode == 2) return launch_gemm_wide(epi, sA, sW, dB, dR, dC, sC, M, N, K, dF, nullptr, 0);
            return launch_gemm_split(epi, sA, sW, dB, dR, dC, sC, M, N, K, dF, nullptr);
        };
        // ablation >= 100: DMA schedule ablation - 100 of the product kernel (gemm_wide.hip gw_dma_slot), any epilogue
        // ablation 192 / 384: that block shape of the product kernel, any epilogue
        // ablation 3192 / 3384: that block shape with the main loop on the 32 x 32 x 16 MFMA (gemm_wide32.hip); 1192 / 1384:
        // the 16 x 16 x 32 form whatever CS_GEMM_WIDE_MFMA says
        if (mode == 2 && (ablation == 3192 || ablation == 3384 || ablation == 1192 || ablation == 1384)) {
            cs::g_gemm_wide_mfma = ablation >= 3000 ? 32 : 16;
            ablation %= 1000;
        }
        cs::g_gemm_wide_shape = (mode == 2 && (ablation == 192 || ablation == 384 || ablation == 256)) ? ablation : 0;  // (256: the 256 x 192 block)
        cs::g_gemm_wide_ablation = (mode == 2 && epilogue == 4 && ablation < 100) ? ablation : 0;
        for (int i = 0; i < 3; ++i) CS_TRY(once());
        CS_HIP(hipEventRecord(e0, nullptr));
        for (uint32_t i = 0; i < iters; ++i) CS_TRY(once());
        CS_HIP(hipEventRecord(e1, nullptr));
        CS_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        CS_HIP(hipEventElapsedTime(&ms, e0, e1));
        *ms_per_launch = (double)ms / iters;
        if (cs::g_gemm_wide_ablation == 7)  // stamped build: the clock the blocks of the LAST launch ran at
        {
            double mc = 0.0, ec = 0.0;
            const double ghz = cs::gemm_wide_read_clock_ghz(&mc, &ec);
            fprintf(stderr, "gemm_wide in-kernel clock: %.3f GHz (median over blocks, last of %u launches, %.1f us each); per tile: "
                            "k loop %.0f cycles, epilogue %.0f cycles\n", ghz, iters, (double)ms / iters * 1e3, mc, ec);
        }
        return CS_OK;
    };
    const int32_t st = run();
    cs::g_gemm_wide_ablation = 0;
    cs::g_gemm_wide_shape = 0;
    cs::g_gemm_wide_mfma = 0;
    (void)hipDeviceSynchronize();
    for (void* p : {(void*)dA, (void*)dW, (void*)dB, (void*)dR, (void*)dC, (void*)sA, (void*)sW, (void*)sC, (void*)dF})
        if (p) (void)hipFree(p);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return st;
}

// Diagnostics: the wide kernel (gemm_wide.hip, gemm_wide32.hip) alone on host buffers, every block shape, MFMA form and
// epilogue — launch_gemm_wide / launch_gemm_wide_ln as the encoder calls them, the block chosen by gemm_wide_route and
// reported in *block_out.  Every output is followed by kSpGuardRows guard rows.  Contract in include/codesearch_gpu_diag.h.
int32_t cs_debug_gemm_wide(int32_t device, int32_t epi, int32_t shape, int32_t mfma, const float* A, const float* W,
                           const float* bias, const float* resid, float* C, uint32_t M, uint32_t N, uint32_t K,
                           int32_t* block_out, uint32_t* guard_changed, uint32_t* range_flag) {
    if (!A || !W || !bias || !C || !block_out || !guard_changed) return fail(CS_ERR_BAD_ARG, "cs_debug_gemm_wide: null buffer");
    if (epi < 0 || epi > 7) return fail(CS_ERR_BAD_ARG, "cs_debug_gemm_wide: epi = %d (0 f32, 1 GELU -> split, 2 + resid, 3 split, 4 SwiGLU, 5 GEGLU, 6 / 7 LayerNorm)", epi);
    if ((epi == 2 || epi >= 6) && !resid) return fail(CS_ERR_BAD_ARG, "cs_debug_gemm_wide: epilogue %d needs a residual", epi);
    if (shape != 0 && shape != 192 && shape != 384 && shape != 256) return fail(CS_ERR_BAD_ARG, "cs_debug_gemm_wide: shape = %d (0, 192, 384, 256)", shape);
    if (mfma != 0 && mfma != 16 && mfma != 32) return fail(CS_ERR_BAD_ARG, "cs_debug_gemm_wide: mfma = %d (0, 16, 32)", mfma);
    if (M == 0 || !gemm_wide_supported(N, K)) return fail(CS_ERR_UNSUPPORTED, "cs_debug_gemm_wide needs M > 0, N %% 192 == 0 and K %% 32 == 0 (M=%u N=%u K=%u)", M, N, K);
    const bool gated = epi == 4 || epi == 5, ln = epi >= 6;
    if (gated && N % 64) return fail(CS_ERR_UNSUPPORTED, "cs_debug_gemm_wide: the gated epilogues need N %% 64 == 0 (N=%u)", N);
    if (ln && N != 384) return fail(CS_ERR_UNSUPPORTED, "cs_debug_gemm_wide: the LayerNorm epilogue needs N = 384");
    CS_TRY(diag_device(device));
    DeviceGuard g(device);
    DiagBufs bufs;
    const int kernel_epi = epi == 0 ? SH_OUT_F32 : epi == 1 ? SH_OUT_SPLIT_GELU : epi == 2 ? SH_OUT_F32_RESID : epi == 3 ? SH_OUT_SPLIT
                         : epi == 4 ? GW_OUT_SWIGLU : epi == 5 ? GW_OUT_GEGLU : GW_OUT_LN;
    struct Overrides {  // the launcher's diagnostic overrides, as cs_debug_gemm_time sets them; reset on every exit path
        Overrides(int s, int m) { cs::g_gemm_wide_shape = s; cs::g_gemm_wide_mfma = m; }
        ~Overrides() { cs::g_gemm_wide_shape = 0; cs::g_gemm_wide_mfma = 0; }
    } overrides(shape, mfma);
    const GwRoute route = gemm_wide_route(kernel_epi, N, 0);
    if (mfma && (mfma == 32) != route.mfma32) return fail(CS_ERR_UNSUPPORTED, "cs_debug_gemm_wide: epilogue %d is not built on the 32 x 32 x 16 form", epi);
    *block_out = route.block;
    const size_t a_n = (size_t)M * K, w_n = (size_t)N * K, c_n = (size_t)M * N;
    const size_t out_w = gated ? N / 2 : N;  // columns of the output
    uint32_t* dF = nullptr;  // [0] the kernel's flag, [1] that of the operands' split, [2] scratch of the weight range check
    float *dA = nullptr, *dW = nullptr, *dB = nullptr, *dR = nullptr, *dC = nullptr;
    _Float16 *sA = nullptr, *sW = nullptr, *sC = nullptr;
    CS_TRY(bufs.get(&dF, 16));
    CS_HIP(hipMemset(dF, 0, 16));
    CS_TRY(bufs.get(&dA, a_n * 4, A));
    CS_TRY(bufs.get(&dW, w_n * 4, W));
    CS_TRY(bufs.get(&dB, (size_t)N * 4, bias));
    CS_TRY(bufs.get(&sA, a_n * 4));
    CS_TRY(bufs.get(&sW, w_n * 4));
    CS_TRY(launch_split_rows(dA, sA, M, K, dF + 1, nullptr));
    CS_TRY(launch_split_rows(dW, sW, N, K, dF + 1, nullptr));
    bool fits = false;
    CS_TRY(sh_weights_fit_wide(sW, (uint64_t)w_n * 2, dF + 2, &fits, nullptr));
    if (!fits) return fail(CS_ERR_UNSUPPORTED, "cs_debug_gemm_wide: the wide kernel needs |w| <= 31.98");
    // an output of M rows of `row_bytes` each, followed by the guard rows (cs_debug_small_path)
    std::vector<std::pair<const char*, size_t>> guards;
    auto guarded = [&](auto** out, size_t row_bytes) -> int32_t {
        const size_t body = (size_t)M * row_bytes, tail = (size_t)kSpGuardRows * row_bytes;
        CS_TRY(bufs.get(out, body + tail));
        CS_HIP(hipMemset(*out, 0xff, body));  // an element the launch does not write comes back as NaN
        CS_HIP(hipMemset(reinterpret_cast<char*>(*out) + body, 0xA5, tail));
        guards.emplace_back(reinterpret_cast<const char*>(*out) + body, tail);
        return CS_OK;
    };
    if (epi == 2) CS_TRY(bufs.get(&dR, c_n * 4, resid));
    if (ln) {  // read and (epilogue 6) overwritten in place: an output like the others
        CS_TRY(guarded(&dR, (size_t)N * 4));
        CS_HIP(hipMemcpy(dR, resid, c_n * 4, hipMemcpyHostToDevice));
    }
    if (epi == 0 || epi == 2) CS_TRY(guarded(&dC, (size_t)N * 4));
    else CS_TRY(guarded(&sC, out_w * 4));
    if (ln) CS_TRY(diag_wide_ln(epi == 7, sA, sW, dB, dR, sC, bias, M, N, K, dF));
    else CS_TRY(launch_gemm_wide(kernel_epi, sA, sW, dB, dR, dC, sC, M, N, K, dF, nullptr, 0));
    CS_HIP(hipDeviceSynchronize());
    if (sC) CS_TRY(diag_read_split(sC, M, out_w, C));
    else CS_HIP(hipMemcpy(C, dC, c_n * 4, hipMemcpyDeviceToHost));
    if (range_flag) CS_HIP(hipMemcpy(range_flag, dF, 4, hipMemcpyDeviceToHost));
    uint32_t changed = 0;
    for (const auto& gd : guards) {
        std::vector<uint32_t> hw(gd.second / 4);
        CS_HIP(hipMemcpy(hw.data(), gd.first, gd.second, hipMemcpyDeviceToHost));
        for (uint32_t w : hw) changed += w != kSpGuardWord;
    }
    *guard_changed = changed;
    return CS_OK;
}

// Diagnostics: the LayerNorm-fused quantised product alone on host buffers, from either production source, at any M —
// launch_gemm_q8_ln as the forward calls it (embedder_forward.hip: out-proj from the split context, FFN-down from the s8 rows
// FFN-up left).  X is followed by CS_DEBUG_Q8_LN_GUARD_ROWS guard rows (a whole row group of the kernel: a store that forgot
// `row < M` lands there).  Contract in include/codesearch_gpu_diag.h.
int32_t cs_debug_gemm_q8_ln(int32_t device, int32_t source, int32_t flags, const float* A, const float* W, const float* wscale,
                            const float* bias, const float* gamma, const float* beta, float eps, const float* resid, uint32_t M,
                            uint32_t K, float* out, float* pairs, uint32_t pairs_cap, uint32_t* out_pairs, uint32_t* slot,
                            uint8_t* xq, float* xparams) {
    if (!A || !W || !wscale || !bias || !gamma || !beta || !resid || !out || !out_pairs || !slot) return fail(CS_ERR_BAD_ARG, "cs_debug_gemm_q8_ln: null buffer");
    if ((source != 0 && source != 1) || (flags & ~3)) return fail(CS_ERR_BAD_ARG, "cs_debug_gemm_q8_ln: source = %d (0 split, 1 prequant), flags = %d (1 stage-major weight, 2 range slot)", source, flags);
    if (M == 0 || (K != 384 && K != 1536) || (source == 0 && K != 384))
        return fail(CS_ERR_UNSUPPORTED, "cs_debug_gemm_q8_ln needs M > 0 and K = 384 (either source) or 1536 (prequant) (M=%u K=%u)", M, K);
    const bool stage_major = flags & 1, slot_mode = flags & 2;
    const uint32_t N = QN_N, pairs_room = (M + 127) / 128 * 8;  // eight pairs per 128-row group (the four-wave form, four per 64 rows, never leaves more)
    if (!slot_mode && (!pairs || pairs_cap < pairs_room)) return fail(CS_ERR_BAD_ARG, "cs_debug_gemm_q8_ln: pairs needs room for %u", pairs_room);
    CS_TRY(diag_device(device));
    DeviceGuard g(device);
    DiagBufs bufs;
    const size_t a_n = (size_t)M * K, w_n = (size_t)N * K, x_n = (size_t)M * N, guard_n = (size_t)CS_DEBUG_Q8_LN_GUARD_ROWS * N;
    float *dA = nullptr, *dW = nullptr, *dS = nullptr, *dB = nullptr, *dG = nullptr, *dBe = nullptr, *dX = nullptr, *dPairs = nullptr;
    _Float16* sA = nullptr;
    int8_t *dXq = nullptr, *dWq = nullptr, *dWst = nullptr;
    Q8RowMeta* dRm = nullptr;
    Q8ColMeta* dCm = nullptr;
    uint32_t *dF = nullptr, *dRanges = nullptr;  // dRanges: slot 0 the fused kernel's input range, 1 the separate pass's, 2 the output's
    CS_TRY(bufs.get(&dF, 16));
    CS_HIP(hipMemset(dF, 0, 16));
    CS_TRY(bufs.get(&dRanges, 3 * Q8_RANGE_WORDS * 4));
    CS_HIP(hipMemset(dRanges, 0, 3 * Q8_RANGE_WORDS * 4));
    CS_TRY(bufs.get(&dA, a_n * 4, A));
    CS_TRY(bufs.get(&dW, w_n * 4, W));
    CS_TRY(bufs.get(&dS, (size_t)N * 4, wscale));
    CS_TRY(bufs.get(&dB, (size_t)N * 4, bias));
    CS_TRY(bufs.get(&dG, (size_t)N * 4, gamma));
    CS_TRY(bufs.get(&dBe, (size_t)N * 4, beta));
    CS_TRY(bufs.get(&dWq, w_n));
    CS_TRY(bufs.get(&dCm, (size_t)N * sizeof(Q8ColMeta)));
    CS_TRY(bufs.get(&dXq, a_n));
    CS_TRY(bufs.get(&dRm, (size_t)M * sizeof(Q8RowMeta)));
    CS_TRY(bufs.get(&dX, (x_n + guard_n) * 4));
    CS_HIP(hipMemcpy(dX, resid, x_n * 4, hipMemcpyHostToDevice));
    {
        const std::vector<uint32_t> pattern(guard_n, CS_DEBUG_Q8_LN_GUARD_WORD);
        CS_HIP(hipMemcpy(dX + x_n, pattern.data(), guard_n * 4, hipMemcpyHostToDevice));
    }
    CS_TRY(bufs.get(&dPairs, (size_t)pairs_room * 8));
    CS_HIP(hipMemset(dPairs, 0xff, (size_t)pairs_room * 8));  // a pair the launch does not write comes back as NaN
    CS_TRY(launch_q8_pack_weight(dW, dS, dB, N, K, dWq, dCm, dF + 1, nullptr));
    CS_HIP(hipDeviceSynchronize());
    uint32_t bad = 0;
    CS_HIP(hipMemcpy(&bad, dF + 1, 4, hipMemcpyDeviceToHost));
    if (bad) return fail(CS_ERR_BAD_ARG, "cs_debug_gemm_q8_ln: W is not a quantised matrix for these column scales (flag %u)", bad);
    const int8_t* w_used = dWq;
    if (stage_major) {
        CS_TRY(bufs.get(&dWst, w_n));
        CS_TRY(launch_q8_stage_major(dWq, N, K, dWst, nullptr));
        w_used = dWst;
    }
    uint32_t *in_range = dRanges, *sep_range = dRanges + Q8_RANGE_WORDS, *out_slot = dRanges + 2 * Q8_RANGE_WORDS;
    uint32_t n_pairs = 0;
    if (source == 0) {
        CS_TRY(bufs.get(&sA, a_n * 4));
        CS_TRY(launch_split_rows(dA, sA, M, K, dF, nullptr));
        CS_TRY(launch_q8_range(Q8_SRC_SPLIT, sA, M, K, in_range, nullptr));
        CS_TRY(launch_q8_quantize(Q8_SRC_SPLIT, sA, M, K, sep_range, nullptr, dXq, dRm, nullptr));  // (for xq / xparams only)
        CS_TRY(launch_gemm_q8_ln(Q8_SRC_SPLIT, sA, nullptr, in_range, w_used, dCm, dX, dG, dBe, eps, M, K, dPairs, &n_pairs, nullptr,
                                 slot_mode ? out_slot : nullptr, stage_major));
    } else {
        CS_TRY(launch_q8_quantize(Q8_SRC_F32, dA, M, K, sep_range, nullptr, dXq, dRm, nullptr));
        CS_TRY(launch_gemm_q8_ln(Q8_SRC_PREQUANT, dXq, dRm, nullptr, w_used, dCm, dX, dG, dBe, eps, M, K, dPairs, &n_pairs, nullptr,
                                 slot_mode ? out_slot : nullptr, stage_major));
    }
    if (!slot_mode) {
        if (n_pairs == 0 || n_pairs > pairs_room) return fail(CS_ERR_HIP, "cs_debug_gemm_q8_ln: the launcher reported %u pairs (room for %u)", n_pairs, pairs_room);
        CS_TRY(launch_q8_range(Q8_SRC_F32, dX, M, N, out_slot, nullptr, dPairs, n_pairs));
    }
    CS_HIP(hipDeviceSynchronize());
    *out_pairs = n_pairs;
    CS_HIP(hipMemcpy(out, dX, (x_n + guard_n) * 4, hipMemcpyDeviceToHost));
    CS_HIP(hipMemcpy(slot, out_slot, 8, hipMemcpyDeviceToHost));
    if (!slot_mode) CS_HIP(hipMemcpy(pairs, dPairs, (size_t)pairs_room * 8, hipMemcpyDeviceToHost));
    if (xq) {
        std::vector<int8_t> hq(a_n);
        CS_HIP(hipMemcpy(hq.data(), dXq, a_n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < a_n; ++i) xq[i] = (uint8_t)((int)hq[i] + 128);
    }
    if (xparams) {
        Q8RowMeta rm0;
        CS_HIP(hipMemcpy(&rm0, dRm, sizeof(rm0), hipMemcpyDeviceToHost));
        xparams[0] = rm0.xs;
        xparams[1] = (float)(rm0.za + 128);
    }
    return CS_OK;
}

// Diagnostics: launch_q8_row_slots and launch_q8_range_units alone.  Contract in include/codesearch_gpu_diag.h.
int32_t cs_debug_q8_unit_ranges(int32_t device, const uint32_t* seq_unit, const uint32_t* unit_len, uint32_t B, uint32_t units,
                                uint32_t L, const float* pairs, uint32_t pairs_per_seq, int32_t pairs_are_rows, uint32_t* row_slot,
                                uint32_t* slots) {
    if (!seq_unit || !unit_len || (!pairs) != (!slots) || (!row_slot && !slots)) return fail(CS_ERR_BAD_ARG, "cs_debug_q8_unit_ranges: null buffer");
    if (B == 0 || units == 0 || L == 0 || (pairs && pairs_per_seq == 0)) return fail(CS_ERR_BAD_ARG, "cs_debug_q8_unit_ranges needs B, units, L, pairs_per_seq > 0");
    if (pairs && pairs_are_rows && pairs_per_seq != L) return fail(CS_ERR_BAD_ARG, "cs_debug_q8_unit_ranges: row pairs come L = %u per sequence (pairs_per_seq = %u)", L, pairs_per_seq);
    for (uint32_t b = 0; b < B; ++b)
        if (seq_unit[b] >= units || (b && seq_unit[b] < seq_unit[b - 1]))
            return fail(CS_ERR_BAD_ARG, "seq_unit[%u]: units must be consecutive runs of sequences, in order", b);
    CS_TRY(diag_device(device));
    DeviceGuard g(device);
    DiagBufs bufs;
    uint32_t *dSu = nullptr, *dUl = nullptr, *dRs = nullptr, *dRange = nullptr;
    float* dP = nullptr;
    CS_TRY(bufs.get(&dSu, (size_t)B * 4, seq_unit));
    CS_TRY(bufs.get(&dUl, (size_t)units * 4, unit_len));
    if (row_slot) {
        const size_t T = (size_t)B * L;
        CS_TRY(bufs.get(&dRs, T * 4));
        CS_HIP(hipMemset(dRs, 0xA5, T * 4));
        CS_TRY(launch_q8_row_slots(dSu, dUl, (uint32_t)T, L, dRs, nullptr));
        CS_HIP(hipDeviceSynchronize());
        CS_HIP(hipMemcpy(row_slot, dRs, T * 4, hipMemcpyDeviceToHost));
    }
    if (slots) {
        const size_t rbytes = (size_t)units * Q8_RANGE_WORDS * 4;
        CS_TRY(bufs.get(&dP, (size_t)B * pairs_per_seq * 8, pairs));
        CS_TRY(bufs.get(&dRange, rbytes));
        CS_HIP(hipMemset(dRange, 0xA5, rbytes));  // (the kernel writes words 0, 1: it must not depend on what they held)
        CS_TRY(launch_q8_range_units(dP, pairs_per_seq, pairs_are_rows != 0, dSu, dUl, B, units, dRange, nullptr));
        CS_HIP(hipDeviceSynchronize());
        std::vector<uint32_t> hr((size_t)units * Q8_RANGE_WORDS);
        CS_HIP(hipMemcpy(hr.data(), dRange, rbytes, hipMemcpyDeviceToHost));
        for (uint32_t u = 0; u < units; ++u) { slots[2 * u] = hr[(size_t)u * Q8_RANGE_WORDS]; slots[2 * u + 1] = hr[(size_t)u * Q8_RANGE_WORDS + 1]; }
    }
    return CS_OK;
}

// Diagnostics: one filter phase alone on host buffers — the copies built, the queries prepared and the phase launched by the
// launchers the index and launch_scan_split call.  Contract in include/codesearch_gpu_diag.h.
int32_t cs_debug_filter(int32_t device, uint32_t dim, const float* corpus, uint64_t n_rows, const float* queries, uint32_t nq,
                        const float* tau, const uint32_t* dead, const float* mu_in, int32_t kernel, uint32_t nqt, uint64_t row_lo,
                        uint64_t row_hi, uint32_t cap, uint32_t grid, uint64_t tail_lo, uint64_t tail_hi, float* norms_out,
                        float* mu_out, uint16_t* f16_out, int8_t* q8_out, float* tmeta_out, uint16_t* qunit_out, int8_t* q8q_out,
                        int8_t* q8q_hi_out, int8_t* q8q_lo_out, float* qmeta_out, float* qmag_out, uint32_t* cnt_out,
                        uint32_t* cand_out, uint32_t* guard_changed) {
    using K = FilterKernel;
    if (!corpus || !queries || !tau || !cnt_out || !cand_out || !guard_changed) return fail(CS_ERR_BAD_ARG, "cs_debug_filter: null buffer");
    if (!split_scan_supported(dim)) return fail(CS_ERR_UNSUPPORTED, "cs_debug_filter: dim 384 / 768 / 1024, got %u", dim);
    if (n_rows == 0 || n_rows > (1u << 20) || nq == 0 || nq > 4096 || cap == 0 || cap > (1u << 16))
        return fail(CS_ERR_BAD_ARG, "cs_debug_filter needs 1 <= n_rows <= 2^20, 1 <= nq <= 4,096, 1 <= cap <= 65,536");
    if (kernel < (int32_t)K::None || kernel > (int32_t)K::F16Tile128) return fail(CS_ERR_BAD_ARG, "cs_debug_filter: kernel = %d", kernel);
    const K kern = (K)kernel;
    const bool i8 = kern == K::Q8Tile256 || kern == K::Q8Rq || kern == K::Q8Rq1 || kern == K::Q8Rw || kern == K::Q8Rw2;
    const bool tiles256 = kern == K::Q8Tile256 || kern == K::F16Tile256;
    const uint64_t q8_rows = n_rows / 128 * 128;  // complete tiles only
    if (kern != K::None && (row_hi <= row_lo || row_hi > (i8 ? q8_rows : n_rows)))
        return fail(CS_ERR_BAD_ARG, "cs_debug_filter: rows [%llu, %llu) of %llu stored (int8: %llu in complete tiles)",
                    (unsigned long long)row_lo, (unsigned long long)row_hi, (unsigned long long)n_rows, (unsigned long long)q8_rows);
    if (tail_hi < tail_lo || tail_hi > n_rows || tail_hi - tail_lo >= 128)
        return fail(CS_ERR_BAD_ARG, "cs_debug_filter: the tail is fewer than 128 stored rows");
    CS_TRY(diag_device(device));
    DeviceGuard g(device);
    DiagBufs bufs;
    // both copies in whole tiles, an even number of them (index.hip: the 256-row kernels read whole pairs) and one pair
    // more, for a row_lo on an odd tile
    const size_t tiles = ((size_t)n_rows + 255) / 256 * 2 + 2, kq8 = (size_t)dim * 128, pad_q = CS_DEBUG_FILTER_CNT_PAD;
    const size_t q_n = (size_t)nq * dim, cnt_words = (nq + pad_q) * kCntStride, cand_slots = ((size_t)nq + 1) * cap;
    float *dC = nullptr, *dN = nullptr, *dMu = nullptr, *dQ = nullptr, *dTau = nullptr, *dQmag = nullptr;
    _Float16 *dSplit = nullptr, *dQs = nullptr;
    int8_t *dQ8 = nullptr, *dQ8q = nullptr, *dQhi = nullptr;
    float4 *dTm = nullptr, *dQm = nullptr;
    uint32_t *dDead = nullptr, *dCnt = nullptr, *dOv = nullptr;
    uint64_t *dCand = nullptr, *dCarry = nullptr;
    CS_TRY(bufs.get(&dC, (size_t)n_rows * dim * 4, corpus));
    CS_TRY(bufs.get(&dN, tiles * 128 * 4));
    CS_HIP(hipMemset(dN, 0, tiles * 128 * 4));
    CS_TRY(bufs.get(&dMu, (size_t)dim * 4));
    CS_TRY(bufs.get(&dQ, q_n * 4, queries));
    CS_TRY(bufs.get(&dTau, (size_t)nq * 4));
    CS_TRY(bufs.get(&dQmag, (size_t)nq * 4));
    CS_TRY(bufs.get(&dSplit, tiles * kq8 * 2));
    CS_HIP(hipMemset(dSplit, 0, tiles * kq8 * 2));
    CS_TRY(bufs.get(&dQ8, tiles * kq8));
    CS_HIP(hipMemset(dQ8, 0, tiles * kq8));
    CS_TRY(bufs.get(&dTm, tiles * sizeof(float4)));
    CS_HIP(hipMemset(dTm, 0, tiles * sizeof(float4)));
    CS_TRY(bufs.get(&dQs, q_n * 2));
    CS_TRY(bufs.get(&dQ8q, q_n));
    CS_TRY(bufs.get(&dQhi, 2 * q_n));
    CS_TRY(bufs.get(&dQm, (size_t)4 * nq * sizeof(float4)));
    CS_HIP(hipMemset(dQm, 0, (size_t)4 * nq * sizeof(float4)));
    if (dead) CS_TRY(bufs.get(&dDead, (tiles * 128 / 32) * 4));
    if (dead) {
        CS_HIP(hipMemset(dDead, 0xff, (tiles * 128 / 32) * 4));  // rows that are not stored are blocked
        CS_HIP(hipMemcpy(dDead, dead, (size_t)((n_rows + 31) / 32) * 4, hipMemcpyHostToDevice));
    }
    CS_TRY(bufs.get(&dCnt, cnt_words * 4));
    CS_TRY(bufs.get(&dOv, 16));
    CS_HIP(hipMemset(dOv, 0, 16));
    CS_TRY(bufs.get(&dCand, cand_slots * 8));
    CS_TRY(bufs.get(&dCarry, 8));

    // 1, 2: the norms and the copies, as cs_index_build makes them
    CS_TRY(launch_row_norms(dC, 0, n_rows, dim, dN, nullptr));
    CS_TRY(launch_corpus_split(dC, dN, dSplit, 0, n_rows, dim, nullptr));
    if (mu_in) CS_HIP(hipMemcpy(dMu, mu_in, (size_t)dim * 4, hipMemcpyHostToDevice));
    else CS_TRY(launch_unit_mean(dC, dN, n_rows, dim, dMu, nullptr));
    if (q8_rows) CS_TRY(launch_corpus_q8(dC, dN, dQ8, dTm, 0, q8_rows / 128, dim, dMu, nullptr));
    // 3: the queries, both planes
    BatchedState st;
    st.d_cand = dCand; st.d_cnt = dCnt; st.d_tau = dTau; st.d_carry = dCarry; st.d_overflow = dOv;
    SplitQueryWs qw;
    qw.d_qsplit = dQs; qw.d_qmag = dQmag; qw.d_q8q = dQ8q; qw.d_qmeta = dQm; qw.d_q8q_hi = dQhi; qw.d_q8q_lo = dQhi + q_n;
    CS_TRY(launch_prep_queries(dim, st, qw, dQ, nq, 0, 0, dMu, true, true, nullptr));
    CS_HIP(hipDeviceSynchronize());
    // 4: the caller's tau; zeroed counters (word 0 of a line) between pattern words; pattern in every candidate slot
    CS_HIP(hipMemcpy(dTau, tau, (size_t)nq * 4, hipMemcpyHostToDevice));
    {
        std::vector<uint32_t> hc(cnt_words, CS_DEBUG_FILTER_GUARD_WORD);
        for (size_t q = 0; q < nq + pad_q; ++q) hc[q * kCntStride] = 0;
        CS_HIP(hipMemcpy(dCnt, hc.data(), cnt_words * 4, hipMemcpyHostToDevice));
        const std::vector<uint32_t> pattern(cand_slots * 2, CS_DEBUG_FILTER_GUARD_WORD);
        CS_HIP(hipMemcpy(dCand, pattern.data(), cand_slots * 8, hipMemcpyHostToDevice));
    }
    // 5: one phase, filled by hand; grid 0 = plan_filter's rule for the kernel
    FilterPhase ph;
    ph.kernel = kern;
    ph.nqt = nqt;
    ph.lo = row_lo;
    ph.hi = ph.filter_hi = row_hi;
    ph.tail_lo = tail_lo;
    ph.tail_hi = tail_hi;
    if (kern != K::None) {
        const int cus = cu_count(), cus8 = cus >= 8 ? cus / 8 * 8 : 256;
        const uint64_t rows = row_hi - row_lo;
        if (tiles256) {
            ph.slots = filter_grid_slots((uint32_t)((rows + 255) / 256), (nq + 255) / 256);
            if (grid % 8) return fail(CS_ERR_BAD_ARG, "cs_debug_filter: a persistent tile kernel's grid is a multiple of 8 (%u)", grid);
            ph.grid = grid ? grid : std::min<uint32_t>(ph.slots, kern == K::Q8Tile256 ? (uint32_t)cus8 : ((uint32_t)cus + 7) / 8 * 8);
        } else if (kern == K::F16Tile128) {
            ph.grid = filter_grid_slots((uint32_t)((rows + 127) / 128), (nq + 127) / 128);  // a block per tile
            if (grid && grid < ph.grid) return fail(CS_ERR_BAD_ARG, "cs_debug_filter: the 128 x 128 kernel needs a block per tile slot (%u < %u)", grid, ph.grid);
            if (grid) ph.grid = grid;
        } else {
            if (nqt == 0 || nqt > 8) return fail(CS_ERR_BAD_ARG, "cs_debug_filter: nqt = %u", nqt);
            ph.qtiles = (nq + 32 * nqt - 1) / (32 * nqt);
            const uint64_t groups = (kern == K::Q8Rq || kern == K::Q8Rq1) ? (rows / 128 + 1) / 2 : (rows + 127) / 128;
            ph.grid = grid ? grid : filter_resident_grid(groups, ph.qtiles, cus8);
        }
        if (ph.grid > 65536) return fail(CS_ERR_BAD_ARG, "cs_debug_filter: grid = %u", ph.grid);
    }
    Q8View q8;
    q8.d_q8 = dQ8; q8.d_tmeta = dTm; q8.d_mu = dMu; q8.rows = q8_rows;
    bool sub_ok = false;
    CS_TRY(sh_denorm_selftest(&sub_ok, nullptr));
    FilterOperands op;
    op.st = &st; op.qw = &qw; op.d_split = dSplit; op.q8 = &q8; op.d_dead = dDead;
    op.nq = nq; op.cap = cap; op.margin = filter_margin(dim, sub_ok); op.nt_stream = filter_knobs().nt; op.stream = nullptr;
    CS_TRY(launch_filter_phase(dim, ph, op));
    CS_HIP(hipGetLastError());
    CS_HIP(hipDeviceSynchronize());

    if (norms_out) CS_HIP(hipMemcpy(norms_out, dN, (size_t)n_rows * 4, hipMemcpyDeviceToHost));
    if (mu_out) CS_HIP(hipMemcpy(mu_out, dMu, (size_t)dim * 4, hipMemcpyDeviceToHost));
    if (f16_out) {  // [tile][dim / 64][128 rows][64] -> [n_rows][dim]
        std::vector<uint16_t> h(tiles * kq8);
        CS_HIP(hipMemcpy(h.data(), dSplit, tiles * kq8 * 2, hipMemcpyDeviceToHost));
        const size_t kc = dim / 64;
        for (size_t r = 0; r < n_rows; ++r)
            for (size_t c = 0; c < kc; ++c)
                memcpy(f16_out + r * dim + c * 64, h.data() + (((r >> 7) * kc + c) * 128 + (r & 127)) * 64, 128);
    }
    if (q8_out) {   // [tile][dim / 128][128 rows][128] -> [q8_rows][dim]
        std::vector<int8_t> h(tiles * kq8);
        CS_HIP(hipMemcpy(h.data(), dQ8, tiles * kq8, hipMemcpyDeviceToHost));
        const size_t kc = dim / 128;
        for (size_t r = 0; r < q8_rows; ++r)
            for (size_t c = 0; c < kc; ++c)
                memcpy(q8_out + r * dim + c * 128, h.data() + (((r >> 7) * kc + c) * 128 + (r & 127)) * 128, 128);
    }
    if (tmeta_out && q8_rows) CS_HIP(hipMemcpy(tmeta_out, dTm, (size_t)(q8_rows / 128) * sizeof(float4), hipMemcpyDeviceToHost));
    if (qunit_out) CS_HIP(hipMemcpy(qunit_out, dQs, q_n * 2, hipMemcpyDeviceToHost));
    if (q8q_out) CS_HIP(hipMemcpy(q8q_out, dQ8q, q_n, hipMemcpyDeviceToHost));
    if (q8q_hi_out) CS_HIP(hipMemcpy(q8q_hi_out, dQhi, q_n, hipMemcpyDeviceToHost));
    if (q8q_lo_out) CS_HIP(hipMemcpy(q8q_lo_out, dQhi + q_n, q_n, hipMemcpyDeviceToHost));
    if (qmeta_out) CS_HIP(hipMemcpy(qmeta_out, dQm, (size_t)4 * nq * sizeof(float4), hipMemcpyDeviceToHost));
    if (qmag_out) CS_HIP(hipMemcpy(qmag_out, dQmag, (size_t)nq * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> hc(cnt_words), hcand(cand_slots * 2);
    CS_HIP(hipMemcpy(hc.data(), dCnt, cnt_words * 4, hipMemcpyDeviceToHost));
    CS_HIP(hipMemcpy(hcand.data(), dCand, cand_slots * 8, hipMemcpyDeviceToHost));
    uint32_t changed = 0;
    for (size_t i = 0; i < cnt_words; ++i) {
        if (i % kCntStride == 0) cnt_out[i / kCntStride] = hc[i];
        else changed += hc[i] != CS_DEBUG_FILTER_GUARD_WORD;
    }
    for (size_t q = 0; q <= nq; ++q) {  // (query nq: the spare query's slots)
        const size_t used = q < nq ? std::min<size_t>(hc[q * kCntStride], cap) : 0;
        for (size_t i = 0; i < cap; ++i) {
            const size_t s = q * cap + i;
            if (q < nq) cand_out[s] = hcand[2 * s];
            changed += hcand[2 * s + 1] != CS_DEBUG_FILTER_GUARD_WORD;  // a filter writes the low word of a slot only
            if (i >= used) changed += hcand[2 * s] != CS_DEBUG_FILTER_GUARD_WORD;
        }
    }
    *guard_changed = changed;
    return CS_OK;
}

}  // extern "C"
