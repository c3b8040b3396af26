"""Float64 references, error bounds and a float32 emulation for the operator tests of the small path's dense kernels
(codesearch_amd/csrc/small_path.hip: sp_ln_gemm_kernel, sp_partial_kernel; tests/test_gpu_small_path.py,
tests/test_small_path_bar.py).  Pure numpy: nothing here touches the library under test, and no factor sits on a bound.

A launch of sp_ln_gemm_kernel is checked in two stages, so that the bounds do not compound:

  stage 1   Xout, the normalised f32 rows, against tests/rows_ref.py's LayerNorm reference and bound, unchanged (the rows a
            prologue forms as a rounded sum carry rows_ref.ordered_sum's ev).
  stage 2   Cs against the float64 product of the values Xout actually holds — f32, taken as exact: stage 1 has checked them
            on their own, and the blocks that do not write Xout recompute them, so a block that normalised another row or
            column fails here.  Weights and bias are rounded with rows_ref.split_roundtrip first: the kernel then sees
            exactly the values the reference takes as exact.

The product (both kernels; u = 2^-24).  A 16 x 16 tile's K range is cut into 32-k chunks; wave w = 0..3 (the wide form: the
w-th of a wave's four partial sums) takes chunks w, w + 4, ...; its partial sum is
    p_w = fma(xx_w, 2^-11, hh_w),   hh_w = sum x_hi w_hi,  xx_w = sum (x_hi w_lo + x_lo w_hi)   (f32 inside the MFMA)
and the tile is ((p0 + p1) + (p2 + p3)) [+ bias].  Bound of the pre-activation acc + bias of column n:

    PRODUCT_BAR sum_k |x_k| |w_nk|  +  u (sum_w |p_w| + |p0 + p1| + |p2 + p3| + |acc| + |acc + bias_n|)

  PRODUCT_BAR = 6e-7   the project's per-product bar of the split-f16 product (tests/attention_ref.py, split_f16.hpp: the
                       activation's own split 2^-22, the dropped lo x lo term 2^-22, the MFMA's f32 accumulation).
  the u terms          every f32 rounding outside the MFMA, each at u times the magnitude of ITS result, taken from the
                       float64 reference: the fma that joins a wave's two sums (four of them), the adds p0 + p1 and p2 + p3,
                       the add of the two pairs and the add of the bias.  A term's path passes FOUR of them (fma, pair,
                       pair of pairs, bias), not the two a bare "(w0 + w1) + (w2 + w3) + bias" suggests; sp_partial_kernel
                       has no bias: three on a path, the last |acc + bias| term is dropped and acc is the slab.
Epilogue "split":  + split_bound(ref) (2^-22 |ref|, 2^-36 under 2^-14).
Epilogue "GELU -> split":  |gelu'| <= 1.13 carries the pre-activation bound d through the activation, the activation's own
    evaluation costs rows_ref's erf-GELU bound GELU_CA u |gelu(g)| + GELU_CB u |g| + 2^-126 (sh_erf_fast's 1.2e-7 on erf is
    2 u, inside the 9 u the bound grants 1 + erf), then the output's split bound:
        1.13 d + GELU_CA u |gelu(g)| + GELU_CB u |g| + 2^-126 + split_bound(gelu(g)).
sp_partial_kernel, per slab ks:  PRODUCT_BAR sum_{k in slice ks} |a_k| |w_nk| + u (sum_w |p_w| + |p0 + p1| + |p2 + p3| + |slab|);
    A and W both pass split_roundtrip first.
"""
import math

import numpy as np

from tests import rows_ref as R
from tests.attention_ref import PRODUCT_BAR

U = R.U
GELU_SLOPE = 1.13   # max |gelu'(x)| = 1.1290 (at x = sqrt 2)
EPI_SPLIT, EPI_GELU = 0, 1


def wave_chunks(K):
    """[4] lists of 32-k chunk indices of a K range: wave w takes chunks w, w + 4, ..."""
    n = K // 32
    return [list(range(w, n, 4)) for w in range(4)]


def _wave_cols(K, w):
    # (a K range of fewer than four chunks leaves a wave none: its partial sum is an exact 0)
    return np.concatenate([np.arange(32 * c, 32 * c + 32) for c in wave_chunks(K)[w]] or [np.arange(0)])


_W64 = {}   # id(w) -> (w, its four waves' columns in float64, |w| in float64): the tests reuse a few weight matrices


def _weights64(w):
    hit = _W64.get(id(w))
    if hit is None or hit[0] is not w:
        if len(_W64) >= 8:
            _W64.clear()
        w64 = R.f64(w)
        hit = (w, [np.ascontiguousarray(w64[:, _wave_cols(w64.shape[1], wv)].T) for wv in range(4)], np.ascontiguousarray(np.abs(w64).T))
        _W64[id(w)] = hit
    return hit[1], hit[2]


def product_ref(x, w, bias=None):
    """x [T, K], w [N, K] (f32, taken as exact), bias [N] or None -> (acc (+ bias) [T, N] float64, bound) of the tile sum
    described above."""
    x = R.f64(x)
    K = x.shape[1]
    w_waves, w_abs = _weights64(w)
    parts = [x[:, _wave_cols(K, wv)] @ w_waves[wv] for wv in range(4)]
    s01, s23 = parts[0] + parts[1], parts[2] + parts[3]
    acc = s01 + s23
    rounding = sum(np.abs(p) for p in parts) + np.abs(s01) + np.abs(s23) + np.abs(acc)
    ref = acc
    if bias is not None:
        ref = acc + R.f64(bias)[None, :]
        rounding = rounding + np.abs(ref)
    bound = PRODUCT_BAR * (np.abs(x) @ w_abs) + U * rounding
    return ref, bound


def ln_gemm_ref(xout, w, bias, epi):
    """Stage 2 of one sp_ln_gemm launch: xout [T, H] the f32 rows the kernel returned, w [N, H] and bias [N] already through
    split_roundtrip -> (ref [T, N], bound) of Cs read back as hi + lo / 2048."""
    pre, d = product_ref(xout, w, bias)
    if epi == EPI_SPLIT:
        return pre, d + R.split_bound(pre)
    ref = R.act64(pre, True)
    bound = GELU_SLOPE * d + R.GELU_CA * U * np.abs(ref) + R.GELU_CB * U * np.abs(pre) + R.UNDERFLOW + R.split_bound(ref)
    return ref, bound


def partial_ref(a, w, H):
    """a [T, 4H], w [N, 4H] (through split_roundtrip) -> (slabs [4, T, N], bound): slab ks = the product over the K range
    [ks H, (ks + 1) H)."""
    refs, bounds = zip(*(product_ref(a[:, ks * H:(ks + 1) * H], _k_slice(w, ks, H)) for ks in range(4)))
    return np.stack(refs), np.stack(bounds)


_SLICES = {}   # (id(w), ks) -> (w, its K range ks): so that _weights64 meets the same object again


def _k_slice(w, ks, H):
    hit = _SLICES.get((id(w), ks))
    if hit is None or hit[0] is not w:
        if len(_SLICES) >= 32:
            _SLICES.clear()
        hit = (w, w[:, ks * H:(ks + 1) * H])
        _SLICES[(id(w), ks)] = hit
    return hit[1]


# ---- the prologues' rows -------------------------------------------------------------------------------------------------

def slab_sum_terms(parts, parts_bias, x):
    """The terms of prologue 1 in the kernel's order: ((p0 + p1 + p2 + p3) + bias) + residual."""
    return list(parts) + [np.broadcast_to(parts_bias, x.shape), x]


def prologue_ref(pro, g, b, eps, rows=None, parts=None, parts_bias=None, x=None, ids=None, word=None, pos=None, type_table=None,
                 types=None, L=1):
    """Stage 1: (ref, bound) of Xout for prologue 0 (LayerNorm of rows), 1 (of the slab sum) or 2 (of the embedding gather)."""
    if pro == 0:
        return R.layernorm_ref(rows, g, b, eps)
    if pro == 1:
        s, ev = R.ordered_sum(slab_sum_terms(parts, parts_bias, x))
    else:
        s, ev = R.ordered_sum(R.embed_rows(ids, word, pos, type_table, types, L))
    return R.layernorm_ref(s, g, b, eps, ev=ev)


# ---- a float32 emulation of the split arithmetic (tests/test_small_path_bar.py) ------------------------------------------------

def _f32_dot(a, b):
    return np.einsum("tk,nk->tn", a, b, dtype=np.float32)


def emulate_product(x, w, bias=None, drop_lo_hi_chunk=None, lo_scale=2.0 ** -11, pairs=True):
    """The kernels' product in float32 numpy: split_planes of both operands, per 32-k chunk the three products hi x hi,
    hi x lo, lo x hi accumulated in f32, a wave's two sums joined by one fma, the four waves' sums added
    (p0 + p1) + (p2 + p3), then the bias.  -> f32 [T, N].
    Perturbations: drop_lo_hi_chunk = c: chunk c loses its x_lo x w_hi product; lo_scale: the weight of the cross terms;
    pairs = False: the four sums added ((p0 + p1) + p2) + p3."""
    xh, xl = (p.astype(np.float32) for p in R.split_planes(x))
    wh, wl = (p.astype(np.float32) for p in R.split_planes(w))
    K = xh.shape[1]
    p = []
    for wv in range(4):
        hh = np.zeros((xh.shape[0], wh.shape[0]), np.float32)
        xx = np.zeros_like(hh)
        for c in wave_chunks(K)[wv]:
            k = slice(32 * c, 32 * c + 32)
            hh = hh + _f32_dot(xh[:, k], wh[:, k])
            xx = xx + _f32_dot(xh[:, k], wl[:, k])
            if c != drop_lo_hi_chunk:
                xx = xx + _f32_dot(xl[:, k], wh[:, k])
        p.append((xx.astype(np.float64) * lo_scale + hh.astype(np.float64)).astype(np.float32))   # one rounding: the fma
    o = (p[0] + p[1]) + (p[2] + p[3]) if pairs else ((p[0] + p[1]) + p[2]) + p[3]
    if bias is not None:
        o = o + np.asarray(bias, np.float32)[None, :]
    return o.astype(np.float32)


def gelu_f32(v, tanh_gelu=False):
    """The activation in float32 numpy (erf rounded to f32); tanh_gelu: the perturbation."""
    v = np.asarray(v, np.float32)
    if tanh_gelu:
        return R.act64(v, True, tanh_gelu=True).astype(np.float32)
    e = R._erf64((v * np.float32(0.70710678118654752440)).astype(np.float64)).astype(np.float32)
    return (np.float32(0.5) * v * (np.float32(1.0) + e)).astype(np.float32)


def emulate_ln_gemm(xout, w, bias, epi, tanh_gelu=False, **kw):
    """Cs of one launch as hi + lo / 2048 read back, from the f32 rows xout."""
    o = emulate_product(xout, w, bias, **kw)
    if epi == EPI_GELU:
        o = gelu_f32(o, tanh_gelu)
    return R.unsplit(*R.split_planes(o))


def emulate_partial(a, w, H, slab_of_chunk=None, **kw):
    """The four slabs.  slab_of_chunk (perturbation): {(ks, chunk within the slice): other slab} moves a chunk's products
    into another slab."""
    a, w = np.asarray(a, np.float32), np.asarray(w, np.float32)
    slabs = [emulate_product(a[:, ks * H:(ks + 1) * H], w[:, ks * H:(ks + 1) * H], **kw) for ks in range(4)]
    for (ks, c), to in (slab_of_chunk or {}).items():
        k = slice(ks * H + 32 * c, ks * H + 32 * c + 32)
        moved = emulate_product(a[:, k], w[:, k])
        slabs[ks] = slabs[ks] - moved
        slabs[to] = slabs[to] + moved
    return np.stack(slabs)


# ---- operands ------------------------------------------------------------------------------------------------------------

def make_weights(N, K, seed):
    """W [N, K] of about 1 / sqrt(K) (unit-variance rows give unit-scale products) and a bias that differs in every column,
    both through split_roundtrip."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((N, K)) / math.sqrt(K)).astype(np.float32)
    bias = (0.2 * np.sin(np.arange(N) * 0.23) + 0.1 * rng.standard_normal(N)).astype(np.float32)
    return R.split_roundtrip(w), R.split_roundtrip(bias)


def integer_weights(N, K, seed, quarters=1):
    """Small-integer W [N, K], asymmetric in n and in k, with another pattern in each of `quarters` K ranges, and an integer
    bias: every product and partial sum is exact in f16 x f16 -> f32."""
    rng = np.random.default_rng(seed)
    w = rng.integers(-3, 4, (N, K)).astype(np.float32)
    q = K // quarters
    for i in range(quarters):
        w[:, i * q] += (np.arange(N) % 7).astype(np.float32)            # asymmetric in n
        w[:, i * q + 1 + i] += np.float32(i + 1)                          # the quarter's own mark
        w[i::4, i * q:(i + 1) * q] *= np.float32(2.0)                     # and its own row pattern
    w[:, 5] += np.float32(2.0)                                            # asymmetric in k
    return w, (np.arange(N) % 11 - 5).astype(np.float32)
