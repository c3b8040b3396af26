"""Float64 references, error bounds and a float32 emulation for the operator tests of the persistent wide dense-layer
kernel (codesearch_amd/csrc/gemm_wide.hip, gemm_wide32.hip; tests/test_gpu_gemm_wide.py, tests/test_gemm_wide_bar.py).
Pure numpy (torch only for erf on large float64 arrays): nothing here touches the library under test, nothing a kernel
returns enters a bound, and no factor sits on a bound.

The product.  Every k-chunk's three MFMAs (w_hi 2^11 x a_hi, w_lo' x a_hi, w_hi x a_lo') add into ONE f32 accumulator that
starts at bias * 2^11; the epilogue multiplies by 2^-11 (exact).  Its bound is small_path_ref.product_ref's, unchanged:

    d = PRODUCT_BAR sum_k |a_k| |w_nk|  +  u (sum_w |p_w| + |p0 + p1| + |p2 + p3| + |acc| + |acc + bias_n|)

PRODUCT_BAR = 6e-7 per product is the project's bar of the split-f16 product (the activation's split 2^-22, the dropped
lo x lo term 2^-22, the MFMA's f32 accumulation); the u terms were written for the small path's four partial sums and are
kept as they stand: the wide kernel has fewer roundings outside the MFMA (none: bias and products share the accumulator),
so the bound is the same bar, not a wider one.

Epilogues (u = 2^-24; A, W and the bias go through rows_ref.split_roundtrip first, so the kernel sees exactly the values the
reference takes as exact):
  0  f32                 d
  1  GELU -> split       small_path_ref.ln_gemm_ref's GELU form: GELU_SLOPE d + GELU_CA u |gelu(p)| + GELU_CB u |p| + 2^-126
                         + split_bound(gelu(p))
  2  + resid, f32        d + u |p + resid|                    (the one f32 add of the epilogue)
  3  split               d + split_bound(p)
  4  SwiGLU, 5 GEGLU     v = A Wv^T + bv, g = A Wg^T + bg, out = v act(g); with d_v, d_g the two product bounds
                             |act(g)| d_v + |v| slope d_g + slope d_v d_g + gate + split_bound(out)
                         slope = max |act'|: GELU_SLOPE = 1.13, SILU_SLOPE = 1.0998 (at g = 2.3994); the cross term is the
                         second order of the same expansion.  `gate` is rows_ref.gate_ref's bound of the activation's own
                         evaluation: |v| (GELU_CA u |a| + GELU_CB u |g|) + 2^-126 max(1, |v|) for the GELU, and for the silu
                             |v| (SILU_W_CA + SILU_W_CG |g|) u |silu(g)| + 2^-126 max(1, |v|)              (see below)
  6 / 7  LayerNorm       the bar of tests/test_gpu_gemm_split.py test_wide_gemm_with_fused_layernorm, unchanged: 1e-5
                         absolute on unit-scale rows, 2e-6 between the two residual forms.

Activation constants.  gw_erf_fast and gw_silu (gemm_wide.hpp) are fast forms: a degree-9 polynomial, the hardware's exp2 and
reciprocal.  Their float32 emulation below (gelu_fast, silu_fast: correctly rounded exp2 and reciprocal, 0.5 ulp each),
on 2,000,001 points of [-6, 6] against math.erf / float64 exp:
  erf-GELU   err / (GELU_CA u |gelu| + GELU_CB u |g|) <= 0.301 (at g = 1.18): rows_ref's constants hold with more than the
             2x margin, and are kept as they stand.
  silu       relative error up to 8.96 u (at g = -5.63) > rows_ref.SILU_CA = 5: gw_silu forms exp2(g * -log2 e), and the
             rounding of that product (and of the constant) is a RELATIVE error 2 u of the exponent, i.e. 2 u |g| of the
             exponential (ln 2 * log2 e = 1), which expf(-g) on an exact argument does not have.  That part is analytic:
             SILU_W_CG = 2.  The rest, max (err / (u |silu|) - 2 |g|), measured 2.69; SILU_W_CA = 5.5 is that with the 2x
             margin.  The margin is what covers the hardware: the about 1 ulp of v_exp_f32 and v_rcp_f32 is an ASSUMPTION
             taken from the kernel's own comment (gemm_wide.hpp gw_silu), against the emulation's 0.5 ulp each.
tests/test_gemm_wide_bar.py re-measures both on a grid and asserts the margins.
"""
import math

import numpy as np

from tests import rows_ref as R
from tests import small_path_ref as S

U = R.U
GELU_SLOPE = S.GELU_SLOPE
SILU_SLOPE = 1.0998          # max |silu'(x)| = 1.09984 (at x = 2.3994), carried to four places
SILU_W_CG = 2.0              # analytic: the exponent's two roundings (see above)
SILU_W_CA = 5.5              # 2 x 2.69, measured on the float32 emulation (hardware exp2 / rcp at about 1 ulp: assumed)
LN_BAR, LN_FORMS_BAR = 1e-5, 2e-6

EPI_F32, EPI_GELU, EPI_RESID, EPI_SPLIT, EPI_SWIGLU, EPI_GEGLU, EPI_LN, EPI_LN_SPLIT = range(8)
EPI_NAMES = ("f32", "GELU -> split", "+ resid", "split", "SwiGLU", "GEGLU", "LayerNorm", "LayerNorm, split residual")
GATED = (EPI_SWIGLU, EPI_GEGLU)
SPLIT_STORES = (EPI_GELU, EPI_SPLIT, EPI_SWIGLU, EPI_GEGLU)


# ---- operands ------------------------------------------------------------------------------------------------------------

def column_scale(N):
    """A scale that differs in every column, in [0.75, 1.25): the columns' signature — a column slip moves a value by
    percents, not by a rounding."""
    return 0.75 + 0.5 * np.modf(np.arange(N) * 0.6180339887498949)[0]


def make_operands(M, N, K, seed, resid=False):
    """A [M, K] unit-scale rows, W [N, K] of about 1 / sqrt(K) and a bias, the last two with the per-column signature; all
    through split_roundtrip.  resid: a unit-scale f32 residual [M, N] as well."""
    rng = np.random.default_rng(seed)
    a = R.split_roundtrip(rng.standard_normal((M, K)).astype(np.float32))
    sc = column_scale(N)
    w = (rng.standard_normal((N, K)) / math.sqrt(K) * sc[:, None]).astype(np.float32)
    bias = ((0.2 * np.sin(np.arange(N) * 0.23) + 0.1 * rng.standard_normal(N)) * sc).astype(np.float32)
    out = [a, R.split_roundtrip(w), R.split_roundtrip(bias)]
    if resid:
        out.append(rng.standard_normal((M, N)).astype(np.float32))
    return out


def pack_gated(wv, wg, bv, bg):
    """Value and gate rows [I, K] (and biases [I]) -> W [2I, K], bias [2I] in the interleaved order GW_OUT_SWIGLU reads:
    16 value rows, then their 16 gate rows — rows_ref.pack_gate_input's grouping, applied to W's rows."""
    w = np.ascontiguousarray(R.pack_gate_input(np.ascontiguousarray(wv.T), np.ascontiguousarray(wg.T)).T)
    return w, R.pack_gate_input(bv[None, :], bg[None, :])[0]


def unpack_gated(raw):
    """[.., 2I] in the interleaved order -> (value [.., I], gate [.., I])."""
    g = raw.reshape(raw.shape[:-1] + (raw.shape[-1] // 32, 2, 16))
    return g[..., 0, :].reshape(raw.shape[:-1] + (-1,)), g[..., 1, :].reshape(raw.shape[:-1] + (-1,))


# ---- float64 references --------------------------------------------------------------------------------------------------

def erf64(x):
    """erf in float64: math.erf up to 10^6 elements, torch.special.erf on float64 CPU tensors beyond."""
    x = np.asarray(x, np.float64)
    if x.size <= 1_000_000:
        return R._erf64(x)
    import torch

    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def act64(g, gelu):
    g = np.asarray(g, np.float64)
    if gelu:
        return 0.5 * g * (1.0 + erf64(g / math.sqrt(2.0)))
    return R.act64(g, False)


def plain_ref(epi, pre, d, resid=None):
    """(ref, bound) of epilogues 0 - 3 from the product's (pre, d) = small_path_ref.product_ref(A, W, bias)."""
    if epi == EPI_F32:
        return pre, d
    if epi == EPI_RESID:
        ref = pre + R.f64(resid)
        return ref, d + U * np.abs(ref)
    if epi == EPI_SPLIT:
        return pre, d + R.split_bound(pre)
    assert epi == EPI_GELU
    ref = act64(pre, True)
    return ref, GELU_SLOPE * d + R.GELU_CA * U * np.abs(ref) + R.GELU_CB * U * np.abs(pre) + R.UNDERFLOW + R.split_bound(ref)


def gated_ref(epi, v, dv, g, dg):
    """(ref, bound) of the gated epilogues from the two products' (v, d_v), (g, d_g)."""
    gelu = epi == EPI_GEGLU
    a = act64(g, gelu)
    ref = v * a
    slope = GELU_SLOPE if gelu else SILU_SLOPE
    floor = R.UNDERFLOW * np.maximum(1.0, np.abs(v))
    if gelu:   # rows_ref.gate_ref's bound
        gate = np.abs(v) * (R.GELU_CA * U * np.abs(a) + R.GELU_CB * U * np.abs(g)) + floor
    else:      # its silu form with the fast silu's constants
        gate = np.abs(v) * (SILU_W_CA + SILU_W_CG * np.abs(g)) * U * np.abs(a) + floor
    return ref, np.abs(a) * dv + np.abs(v) * slope * dg + slope * dv * dg + gate + R.split_bound(ref)


def reference(epi, a, w, bias, resid=None, products=None):
    """(ref, bound) of one launch of epilogues 0 - 5.  W / bias of the gated ones in the interleaved order.  products: the
    product_ref results of an earlier call on the same operands (shared between the epilogues of a shape)."""
    if epi in GATED:
        if products is None:
            wv, wg = unpack_gated(np.ascontiguousarray(w.T))
            bv, bg = unpack_gated(bias)
            products = S.product_ref(a, np.ascontiguousarray(wv.T), bv) + S.product_ref(a, np.ascontiguousarray(wg.T), bg)
        return gated_ref(epi, *products)
    if products is None:
        products = S.product_ref(a, w, bias)
    return plain_ref(epi, *products, resid=resid)


def layernorm_ref(a, w, bias, resid):
    """Epilogues 6 / 7: LayerNorm(A W^T + bias + resid) with gamma = bias + 1, beta = -bias, eps 1e-12, in float64."""
    v = R.f64(a) @ R.f64(w).T + R.f64(bias) + R.f64(resid)
    mu = v.mean(axis=1, keepdims=True)
    var = ((v - mu) ** 2).mean(axis=1, keepdims=True)
    return (v - mu) / np.sqrt(var + 1e-12) * (R.f64(bias) + 1.0) - R.f64(bias)


# ---- a float32 emulation of the kernel's arithmetic (tests/test_gemm_wide_bar.py) ----------------------------------------

_ERF_POLY = (7.569788067485206e-07, -1.6365151168429293e-05, 0.00015192339196801186, -0.0007679605041630566,
             0.002005203627049923, 0.0003252939786761999, -0.028044508770108223, 0.1484302133321762, 0.9184240698814392,
             1.6279078722000122)


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(np.float32)   # one rounding


def erf_fast(x):
    """gw_erf_fast in float32 numpy (exp2 correctly rounded)."""
    x = np.asarray(x, np.float32)
    t = np.minimum(np.abs(x), np.float32(4.0))
    q = np.full_like(t, np.float32(_ERF_POLY[0]))
    for c in _ERF_POLY[1:]:
        q = _fma(q, t, np.float32(c))
    e = np.float32(1.0) - np.exp2((-(q * t)).astype(np.float64)).astype(np.float32)
    return np.copysign(e, x)


def gelu_fast(v, tanh_gelu=False):
    """gw_gelu in float32 numpy; tanh_gelu: the perturbation."""
    v = np.asarray(v, np.float32)
    if tanh_gelu:
        return R.act64(v, True, tanh_gelu=True).astype(np.float32)
    return (np.float32(0.5) * v) * (np.float32(1.0) + erf_fast(v * np.float32(0.70710678118654752440)))


def silu_fast(v):
    """gw_silu in float32 numpy (exp2 and the reciprocal correctly rounded)."""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore"):
        e = np.exp2((v * np.float32(-1.44269504088896340736)).astype(np.float64)).astype(np.float32)
        return v * (1.0 / (np.float32(1.0) + e).astype(np.float64)).astype(np.float32)


def kc_order(nt, ntiles, kchunks, wrap=True):
    """The k-chunks in the order n-tile nt of ntiles walks them (split_f16.hpp sh_kc_rot).  wrap = False (perturbation): the
    walk does not wrap, so the chunks before the rotation are never read."""
    stride = max(kchunks // ntiles, 1)
    rot = (nt * stride) % kchunks
    return [(rot + i) % kchunks for i in range(kchunks)] if wrap else list(range(rot, kchunks))


def emulate_raw(a, w, bias, bn=384, lo_terms=True, wrap=True):
    """The raw projection A W^T + bias as the kernel forms it, in float32 numpy: one accumulator per output on the scale
    2^11 that starts at bias * 2^11, per k-chunk (in the n-tile's rotated order) the products (w_hi 2^11) a_hi, w_lo' a_hi,
    w_hi a_lo' added in f32, the result times 2^-11.  bn: the block's columns (384 | 192).  -> f32 [M, N]."""
    ah, al = (p.astype(np.float32) for p in R.split_planes(a))
    wh, wl = (p.astype(np.float32) for p in R.split_planes(w))
    M, K = ah.shape
    N = wh.shape[0]
    out = np.empty((M, N), np.float32)
    ntiles = N // bn
    for nt in range(ntiles):
        n = slice(nt * bn, (nt + 1) * bn)
        acc = np.broadcast_to(np.asarray(bias, np.float32)[n] * np.float32(2048.0), (M, bn)).astype(np.float32)
        for kc in kc_order(nt, ntiles, K // 32, wrap):
            k = slice(32 * kc, 32 * kc + 32)
            acc = acc + S._f32_dot(ah[:, k], wh[n, k] * np.float32(2048.0))
            if lo_terms:
                acc = acc + S._f32_dot(ah[:, k], wl[n, k])
                acc = acc + S._f32_dot(al[:, k], wh[n, k])
        out[:, n] = acc * np.float32(2.0 ** -11)
    return out


def emulate_epilogue(epi, raw, resid=None, tanh_gelu=False, swap_gate=False):
    """What the launch returns, read back (split stores as hi + lo / 2048), from the raw projection."""
    if epi == EPI_F32:
        return raw
    if epi == EPI_RESID:
        return raw + np.asarray(resid, np.float32)
    if epi == EPI_SPLIT:
        return R.unsplit(*R.split_planes(raw))
    if epi == EPI_GELU:
        return R.unsplit(*R.split_planes(gelu_fast(raw, tanh_gelu)))
    v, g = unpack_gated(raw)
    if swap_gate:
        v, g = g, v
    o = v * (gelu_fast(g, tanh_gelu) if epi == EPI_GEGLU else silu_fast(g))
    return R.unsplit(*R.split_planes(o.astype(np.float32)))


def emulate(epi, a, w, bias, resid=None, bn=384, **kw):
    epi_kw = {k: kw.pop(k) for k in ("tanh_gelu", "swap_gate") if k in kw}
    return emulate_epilogue(epi, emulate_raw(a, w, bias, bn, **kw), resid, **epi_kw)
