"""Reference, error bound and input families of the operator test of the LayerNorm-fused quantised product
(gemm_q8_ln_kernel, csrc/gemm_q8.hip; tests/test_gpu_q8_ln.py, tests/test_q8_ln_bar.py), and the numpy statements of the ONNX
quantisers every quantised test shares (tests/test_gpu_quantized.py imports them from here).  Pure numpy: nothing here
touches the library under test.

One call of the kernel is  X <- LayerNorm(MatMulInteger(x_q, W_q) * (x_scale * W_scale) + bias + X).  Its reference has four
steps.
  (a) The activation bytes: dynamic_quantize(A) — of A after the split round trip for the "split" source (out-proj takes the
      attention context in split-f16 form).  The separate quantising pass returns the same bytes (asserted first by the GPU
      test), so what is left to disagree belongs to the fused kernel.
  (b) The integer product acc = (q - x_zp) . d^T as a float64 BLAS product: every operand is an integer below 2^8, a sum of K
      <= 1536 products stays below 2^27, far below 2^53 — exact in any order (integer_product asserts it).
  (c) The row before the LayerNorm, in float32 in the kernel's stated order:
          v = ((f32(acc) * (x_scale * W_scale)) + bias) + resid
      __fmul_rn / __fadd_rn and one plain add of their result: nothing there can be contracted, and the F32_RESID epilogue
      of the row-block kernel — the same operations — is asserted bit for bit by tests/test_gpu_quantized.py.  v is therefore
      taken as EXACT (no ev term).  The integer half cannot overflow the 24-bit operands of v_mad_i32_i24:
          |rowsum - K za| = |sum (q - x_zp)| <= 1536 * 255 < 393,216 = 1536 * 256,   |colsum| <= 1536 * 128 = 196,608,
      |zw| <= 255 + 128, |za| <= 128: all below 2^23; the "extreme" family reaches rowsum - K za = 1536 * 254 and column
      sums of 1536 * 127 with both zero points at an end of their range.
  (d) rows_ref.layernorm_ref(v, gamma, beta, eps, counts=(99, 100)), no margin factor.  The counts, from the kernel: a lane
      holds 96 of a row's 384 values (columns 16 j + 4 g + r) and adds them serially — the first add is to 0 and exact: 95
      roundings — two butterfly steps follow (xor 16, xor 32), then the constant 1 / 384 rounded to f32 and the product with
      it: c_sum = 95 + 2 + 2 = 99.  The squares: 96 fma, the two steps, 1 / 384 and its product: c_q = 100.  (The compiler
      may contract qv * (1 / 384) + eps and the last product with the add of beta into fused multiply-adds: one rounding
      less each, inside the bound's 2.5 u and 3 u terms either way.)
"""
import functools

import numpy as np

from tests import rows_ref as R

N = 384                      # the kernel's width (QN_N)
LN_COUNTS = (99, 100)
GUARD_ROWS = 128             # CS_DEBUG_Q8_LN_GUARD_ROWS
GUARD_WORD = 0xA5A5A5A5      # CS_DEBUG_Q8_LN_GUARD_WORD
SOURCES = (("split", 384), ("prequant", 384), ("prequant", 1536))
FAMILIES = ("normal", "offset", "outlier", "zero", "extreme", "ties")
WEIGHT_KINDS = {"per-channel unsigned": (True, True), "per-channel signed": (True, False), "per-tensor unsigned": (False, True)}


# ---- the ONNX quantisers ---------------------------------------------------------------------------------------------------

def quantize_matrix(W, per_channel, unsigned):
    """onnxruntime's weight quantisation of one [N, K] matrix -> (dequantised W, integers q - zp, scale [N])."""
    W = np.asarray(W, np.float32)
    axis = 1 if per_channel else None
    lo = np.minimum(W.min(axis=axis, keepdims=True), np.float32(0))
    hi = np.maximum(W.max(axis=axis, keepdims=True), np.float32(0))
    if unsigned:
        scale = ((hi - lo) / np.float32(255)).astype(np.float32)
        zp = np.clip(np.rint(-lo / scale), 0, 255)
        q = np.clip(np.rint(W / scale) + zp, 0, 255)
    else:
        scale = (np.maximum(np.abs(lo), np.abs(hi)) / np.float32(127)).astype(np.float32)
        zp = np.zeros_like(scale)
        q = np.clip(np.rint(W / scale), -127, 127)
    d = (q - zp).astype(np.int64)
    sc = np.broadcast_to(scale.reshape(-1), (W.shape[0],)).astype(np.float32) if per_channel \
        else np.full(W.shape[0], scale.reshape(-1)[0], np.float32)
    return (d.astype(np.float32) * sc[:, None]).astype(np.float32), d, sc


def dynamic_quantize(x):
    """ONNX DynamicQuantizeLinear (opset 11), float32 arithmetic -> (uint8 tensor, scale, zero point)."""
    x = np.asarray(x, np.float32)
    lo = np.minimum(np.float32(0), x.min())
    hi = np.maximum(np.float32(0), x.max())
    scale = np.float32(1) if hi == lo else np.float32((hi - lo) / np.float32(255))
    zp = np.float32(np.rint(np.clip(np.float32(0) - np.float32(lo / scale), 0, 255)))
    q = np.clip(np.rint((x / scale).astype(np.float32)) + zp, 0, 255).astype(np.uint8)
    return q, scale, int(zp)


def split_round_trip(A):
    """What an f32 value becomes on its way through the split-f16 hand-over: hi + lo / 2048."""
    A = np.asarray(A, np.float32)
    hi = A.astype(np.float16)
    lo = ((A - hi.astype(np.float32)) * np.float32(2048)).astype(np.float16)
    return (hi.astype(np.float32) + lo.astype(np.float32) * np.float32(1 / 2048)).astype(np.float32)


# ---- the reference of one call ---------------------------------------------------------------------------------------------

def integer_product(q, xz, d):
    """MatMulInteger: sum_k (q - x_zp) d as a float64 BLAS product -> int64 [M, N], exact."""
    a = q.astype(np.float64) - float(xz)
    dd = np.asarray(d, np.float64)
    assert np.abs(a).max(initial=0.0) * np.abs(dd).max(initial=0.0) * a.shape[1] < 2.0 ** 53   # every partial sum is an exact integer
    acc = a @ dd.T
    assert np.array_equal(acc, np.rint(acc))
    return acc.astype(np.int64)


def pre_ln_rows(acc, xs, sc, bias, resid):
    """v = ((f32(acc) * (x_scale * W_scale)) + bias) + resid, one f32 rounding per operation, the kernel's order."""
    scale = (np.float32(xs) * np.asarray(sc, np.float32)).astype(np.float32)
    y = (np.asarray(acc).astype(np.float32) * scale[None, :]).astype(np.float32)
    y = (y + np.asarray(bias, np.float32)[None, :]).astype(np.float32)
    return (y + np.asarray(resid, np.float32)).astype(np.float32)


def source_activations(case, source):
    """The values the kernel's quantiser sees: A itself, or A after the split round trip."""
    return split_round_trip(case["A"]) if source == "split" else case["A"]


def quantized(case, source):
    """-> (q uint8 [M, K], x_scale, x_zp, acc int64 [M, N])"""
    q, xs, xz = dynamic_quantize(source_activations(case, source))
    return q, xs, xz, integer_product(q, xz, case["d"])


def reference(case, source, eps, quant=None):
    """-> dict(q, xs, xz, acc, v, ref, bound): ref / bound float64 [M, N]."""
    q, xs, xz, acc = quant if quant is not None else quantized(case, source)
    v = pre_ln_rows(acc, xs, case["sc"], case["bias"], case["resid"])
    ref, bound = R.layernorm_ref(v, case["gamma"], case["beta"], eps, counts=LN_COUNTS)
    return {"q": q, "xs": xs, "xz": xz, "acc": acc, "v": v, "ref": ref, "bound": bound}


def kernel_order_f32(v, gamma, beta, eps):
    """The LayerNorm in plain float32 in gemm_q8_ln_kernel's own order: lane g of a row's four lanes owns the columns
    16 j + 4 g + r (j = 0..23, r = 0..3) and walks them in that order; serial sums, then the butterfly steps xor 16 and
    xor 32 (lane g meets g ^ 1, then g ^ 2); mean = sum * f32(1 / 384); the squares of v - mean by fma; inv = 1 /
    sqrt(qv * f32(1 / 384) + eps); ((v - mean) * inv) * gamma + beta."""
    v = np.asarray(v, np.float32)
    g32, b32 = np.asarray(gamma, np.float32), np.asarray(beta, np.float32)
    cols = np.array([[16 * j + 4 * g + r for j in range(24) for r in range(4)] for g in range(4)])   # [4, 96]
    lanes = v[:, cols]                                                                                  # [T, 4, 96]
    rn = np.float32(1.0 / N)

    def butterfly(s):
        s = (s + s[:, [1, 0, 3, 2]]).astype(np.float32)
        return (s + s[:, [2, 3, 0, 1]]).astype(np.float32)

    s = np.zeros(lanes.shape[:2], np.float32)
    for i in range(96):
        s = (s + lanes[:, :, i]).astype(np.float32)
    mean = (butterfly(s) * rn).astype(np.float32)
    d = (lanes - mean[:, :, None]).astype(np.float32)
    qv = np.zeros(lanes.shape[:2], np.float32)
    for i in range(96):   # fma: the product of two f32 is exact in float64, one rounding of the sum
        qv = (d[:, :, i].astype(np.float64) ** 2 + qv.astype(np.float64)).astype(np.float32)
    var = (butterfly(qv) * rn).astype(np.float32)
    inv = (np.float32(1.0) / np.sqrt((var + np.float32(eps)).astype(np.float32))).astype(np.float32)
    o = (((d * inv[:, :, None]).astype(np.float32) * g32[cols][None]).astype(np.float32) + b32[cols][None]).astype(np.float32)
    out = np.empty_like(v)
    out[:, cols] = o
    return out


# ---- input families --------------------------------------------------------------------------------------------------------

def make_weight(family, K, kind, rng):
    per_channel, unsigned = WEIGHT_KINDS[kind]
    if family == "extreme":
        # a third of the columns all-positive, a third all-negative, a third mixed, every magnitude near the column's
        # largest: column sums and the weights' zero points at an end of their range
        mag = (0.05 * rng.uniform(0.8, 1.0, size=(N, K)))
        sign = np.where(rng.random((N, K)) < 0.5, -1.0, 1.0)
        third = np.arange(N) % 3
        sign[third == 0] = 1.0
        sign[third == 1] = -1.0
        Wf = (mag * sign).astype(np.float32)
        Wf[third == 0, 0] = 0.05
        Wf[third == 1, 0] = -0.05
    else:
        Wf = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    return quantize_matrix(Wf, per_channel, unsigned)


@functools.lru_cache(maxsize=None)
def make_case(family, M, K, kind, seed=0):
    """One call's operands: A [M, K], W [384, K] (dequantised) with its integers d and column scales sc, bias, gamma, beta,
    resid [M, 384].  The families:
      normal    rows at scales 0.3 / 1 / 4 and one outlier of 9.5 that sets the range, as in real activations
      offset    the same, the residual rows_ref.make_rows("offset"): a common offset of 100 with a spread of 0.01
      outlier   the same, the residual rows_ref.make_rows("outlier"): one column of 1e3 per row
      zero      all-zero activations (x_scale 1, zero point 0), a constant bias and a residual constant per row: the
                variance is 0 and the output is beta
      extreme   rows wholly at the tensor's maximum 7.96875 or its minimum -0.03125 (x_scale 8 / 255, zero point 1: every
                byte 255 or 0, sum (q - x_zp) = 254 K or -K), weights as make_weight builds them
      ties      multiples of 1 / 64 in [-2, 5.96875] with both ends planted: x_scale is exactly 2^-5 and x / x_scale a
                multiple of 0.5 — half the values on a rounding tie; exact in split form"""
    rng = np.random.default_rng([FAMILIES.index(family), M, K, sorted(WEIGHT_KINDS).index(kind), seed])
    if family == "zero":
        A = np.zeros((M, K), np.float32)
    elif family == "extreme":
        top = rng.random(M) < 0.5
        top[0] = True
        if M > 1:
            top[-1] = False
        A = np.where(top[:, None], np.float32(7.96875), np.float32(-0.03125)) * np.ones((1, K), np.float32)
        if M == 1:
            A[0, K // 2:] = np.float32(-0.03125)
    elif family == "ties":
        A = (rng.integers(-128, 383, size=(M, K)) / 64.0).astype(np.float32)
        A.reshape(-1)[rng.choice(M * K, 2, replace=False)] = (-2.0, 5.96875)
        assert dynamic_quantize(A)[1] == np.float32(2.0 ** -5) and np.array_equal(split_round_trip(A), A)
    else:
        A = (rng.standard_normal((M, K)) * rng.choice([0.3, 1.0, 4.0], size=(M, 1))).astype(np.float32)
        A[rng.integers(0, M), rng.integers(0, K)] = 9.5
    W, d, sc = make_weight(family, K, kind, rng)
    gamma, beta = R.make_gamma_beta(N, int(rng.integers(1 << 30)))
    if family == "zero":
        bias = np.full(N, 0.375, np.float32)
        resid = np.repeat((rng.standard_normal((M, 1)) * 3.0).astype(np.float32), N, axis=1)
    else:
        bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
        resid = R.make_rows(family if family in ("offset", "outlier") else "normal", M, N, int(rng.integers(1 << 30)))
    case = {"A": np.ascontiguousarray(A, np.float32), "W": np.ascontiguousarray(W), "d": d, "sc": np.ascontiguousarray(sc),
            "bias": bias, "gamma": gamma, "beta": beta, "resid": np.ascontiguousarray(resid, np.float32)}
    for a in case.values():
        a.setflags(write=False)   # shared among the tests that need it, left unchanged
    return case


# ---- the (lo, hi) hand-over to the next quantisation -----------------------------------------------------------------------

def range_pair(rows):
    """(min(0, .), max(0, .)) over f32 values -> uint32 [2], the bits the kernel leaves (an empty set: (+0, +0))."""
    rows = np.asarray(rows, np.float32)
    lo = np.minimum(np.float32(0), rows.min()) if rows.size else np.float32(0)
    hi = np.maximum(np.float32(0), rows.max()) if rows.size else np.float32(0)
    return np.array([lo, hi], np.float32).view(np.uint32)


def unit_row_slots(seq_unit, unit_len, L):
    """launch_q8_row_slots: row (b, t) -> its unit, bit 31 set where t lies beyond the unit's own padded length."""
    su = np.repeat(np.asarray(seq_unit, np.uint32), L)
    t = np.tile(np.arange(L, dtype=np.uint32), len(seq_unit))
    return (su | np.where(t >= np.asarray(unit_len, np.uint32)[su], np.uint32(0x80000000), np.uint32(0))).astype(np.uint32)


def unit_ranges(pairs, pps, pairs_are_rows, seq_unit, unit_len, units):
    """launch_q8_range_units: per unit the range_pair of its sequences' pairs (row pairs: positions below its own length)."""
    pairs = np.asarray(pairs, np.float32).reshape(len(seq_unit), pps, 2)
    out = np.zeros((units, 2), np.uint32)
    for u in range(units):
        mine = pairs[np.asarray(seq_unit) == u]
        if pairs_are_rows:
            mine = mine[:, :unit_len[u]]
        out[u, 0] = range_pair(mine[..., 0])[0]
        out[u, 1] = range_pair(mine[..., 1])[1]
    return out
