"""Float64 references, error bounds and input families of the operator tests of the encoder's row kernels, the element-wise
kernels of the Nomic / Jina families and the CLS tail (tests/test_gpu_rows.py, tests/test_gpu_attention_cls.py,
tests/test_rows_bar.py).  Pure numpy: nothing here touches the library under test.

Every reference takes f32 inputs as exact, evaluates the operation in float64 and returns (ref, bound): a per-element bound
formed from the reference's own quantities only.  u = 2^-24 is the cost of one f32 operation (round to nearest); the
kernels are built with -fno-fast-math, so division and square root are correctly rounded and cost u each.  No margin factor
sits on top of any bound.

Wave reductions (encoder_rows.hpp wave_sum): a lane adds its NPL = H / 64 values serially (NPL - 1 roundings: the first add
is to 0 and exact), then 6 butterfly steps; every term passes NPL + 5 roundings.

LayerNorm family (ln_row_core: embed_ln, layernorm, layernorm_to, layernorm_sum; nomic.hip qk_layernorm_kernel)
    dmean   = c_sum u mean|v|                 c_sum = NPL + 7: NPL + 5 roundings of the sum, the constant 1 / H rounded to f32,
                                              the product with it.  qk_layernorm: a lane adds pairs (1), then four pair sums
                                              per round of 512 columns (4 R, R = ceil(H / 512)), 6 butterfly steps, one
                                              division by H: c_sum = 4 R + 8.
    d       = v - mean, var = mean(d^2), inv = 1 / sqrt(var + eps)
    rel_inv = ( (c_q + 2) u var + dmean^2 ) / (2 (var + eps)) + 2.5 u
                                              c_q = NPL + 8: NPL fma + 6 butterfly steps on the squares, 1 / H and its product;
                                              + 2: each d carries its own rounding u |d|, twice in the square; the common
                                              shift dmean moves the sum of squares by H dmean^2 only (sum d = 0); 2.5 u: the
                                              add of eps (halved by the root), the root, the division.  qk_layernorm: two
                                              squares and their add, 4 R accumulations, 6 steps, the division: c_q = 4 R + 9.
    |got - ref| <= (dmean + u (|v| + |mean|)) inv |g| + |d inv g| (rel_inv + 3 u) + u |b|
                                              3 u: the two products and the final add.
  An input that is itself a rounded sum (embed_ln: (word + type) + pos; layernorm_sum: ((p0 + p1 + ..) + bias) + resid) has
  the error ev = u * (sum of the magnitudes of the partial sums in the kernel's order, evaluated in float64); it enters as
  dmean += mean(ev), the first bracket += ev, rel_inv += mean(|d| ev) / (var + eps).

Pooling (pool_normalize_kernel, mean_pool_normalize_kernel)
    dv      = (n - 1) u sum|x| / n + u |v|    n valid rows: in either kernel a term passes at most n - 1 inexact adds (an add
                                              of 0 is exact; each inexact add on a term's path joins at least one more row);
                                              u |v|: the division by n.  CLS pooling: dv = 0.
    out = v / (N + 1e-12), N = |v|_2:   rel_den = sum(|v| dv) / N^2 + ((NPL + 6) / 2 + 2) u    (the squares' fma chain and
                                              butterfly, halved by the root; the root; the add of 1e-12)
    |got - ref| <= dv / (N + 1e-12) + |out| (rel_den + u)

Rotary map     |got - ref| <= 3 u (|x1 c| + |x2 s|): two products and one add.
Gate           silu(g) = g / (1 + exp(-g)): nothing cancels (both terms positive), every step is relative:
                   |got - ref| <= |v| c_a u |silu(g)| + 2^-126 max(1, |v|),   c_a = 2 * 1 + 3
               (expf: 1 ulp = 2 u at worst, HIP math API reference, single-precision table; the add of 1, the division, the
               product with v; 2^-126: results under the f32 normal range — expf(104) is inf and silu(-104) = -7e-44 comes
               back as 0).  This is the erf-GELU's form below with c_b = 0: the silu has no cancelling term.
               erf-GELU 0.5 g (1 + erf(g / sqrt 2)): 1 + erf cancels for negative g, its error is absolute:
                   |got - ref| <= |v| (c_a u |gelu(g)| + c_b u |g|) + 2^-126 max(1, |v|),   c_a = 3,  c_b = 4 + 0.5
               (erff: 4 ulp (same table) = 8 u |erf| <= 8 u; its argument g * rn(1 / sqrt 2) carries 2 u, worth
               2 u max(x erf'(x)) = 0.97 u <= u; together 9 u on (1 + erf), times 0.5 |g|; c_a: the add of 1 and two products).
Split-form outputs add 2^-22 |x| (split_f16.hpp), 2^-36 absolutely under 2^-14.
"""
import math

import numpy as np

U = 2.0 ** -24
SPLIT_REL = 2.0 ** -22
SPLIT_ABS = 2.0 ** -36
ULP_EXPF = 1.0
ULP_ERFF = 4.0
SILU_CA = 2.0 * ULP_EXPF + 3.0
GELU_CA = 3.0
GELU_CB = ULP_ERFF + 0.5
UNDERFLOW = 2.0 ** -126
F16_MAX = 65504.0


def f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


# ---- the split-f16 format in numpy ---------------------------------------------------------------------------------------

def split_planes(x):
    """f32 -> (hi, lo) float16 planes as sh_split forms them: hi = rn_f16(x), lo = rn_f16((x - hi) * 2048)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16)
        lo = ((x - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi, lo


def unsplit(hi, lo):
    return hi.astype(np.float32) + lo.astype(np.float32) * np.float32(1.0 / 2048.0)   # exact in f32


def split_roundtrip(x):
    """The nearest f32 values the split form holds exactly: y with hi + lo / 2048 of split(y) equal to y.  Inputs of the
    split kernels are passed through this first, so that the kernel sees exactly the values the reference takes as exact.
    (One pass almost always suffices; where lo's rounding carries into hi's last place a second one settles it.)"""
    y = np.asarray(x, np.float32)
    for _ in range(4):
        y2 = unsplit(*split_planes(y))
        if np.array_equal(y2, y):
            return y
        y = y2
    raise AssertionError("the split form's round trip did not settle")


def split_lines(x):
    """[rows, K] f32 -> the split tensor's 16-bit words [rows][K / 32][64]: per 32 columns one 128-byte line, 32 hi then 32 lo."""
    hi, lo = split_planes(x)
    rows, K = hi.shape
    lines = np.concatenate([hi.reshape(rows, K // 32, 32), lo.reshape(rows, K // 32, 32)], axis=2)
    return np.ascontiguousarray(lines).view(np.uint16)


def split_bound(ref):
    return np.maximum(SPLIT_REL * np.abs(ref), SPLIT_ABS)


def worst(got, ref, bound):
    """max |got - ref| / bound (inf for a value that is not finite; 0 / 0 counts as 0)."""
    g = np.asarray(got, np.float64)
    if not np.isfinite(g).all():
        return math.inf
    err = np.abs(g - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


# ---- LayerNorm family ----------------------------------------------------------------------------------------------------

def ln_counts(H):
    npl = H // 64
    return npl + 7, npl + 8


def qk_counts(H):
    r = (H + 511) // 512
    return 4 * r + 8, 4 * r + 9


def layernorm_ref(v, g, b, eps, ev=None, counts=None, var_ddof=0, eps_outside=False):
    """LayerNorm of rows v [T, H] (float64, or f32 taken as exact).  ev: the absolute error bound of v when v is itself a
    rounded sum.  counts = (c_sum, c_q), default: the row kernels'.  The last two arguments are perturbations
    (tests/test_rows_bar.py).  -> (ref, bound)."""
    v = np.asarray(v, np.float64)
    g, b = f64(g), f64(b)
    H = v.shape[-1]
    c_sum, c_q = counts or ln_counts(H)
    eps = float(np.float32(eps))
    mean = v.mean(axis=-1, keepdims=True)
    d = v - mean
    var = (d * d).sum(axis=-1, keepdims=True) / (H - var_ddof)
    inv = 1.0 / (np.sqrt(var) + eps) if eps_outside else 1.0 / np.sqrt(var + eps)
    ref = d * inv * g + b
    ev = np.zeros_like(v) if ev is None else np.asarray(ev, np.float64)
    dmean = c_sum * U * np.abs(v).mean(axis=-1, keepdims=True) + ev.mean(axis=-1, keepdims=True)
    rel_inv = ((c_q + 2) * U * var + dmean ** 2) / (2.0 * (var + eps)) + 2.5 * U + (np.abs(d) * ev).mean(axis=-1, keepdims=True) / (var + eps)
    bound = (dmean + ev + U * (np.abs(v) + np.abs(mean))) * inv * np.abs(g) + np.abs(d * inv * g) * (rel_inv + 3 * U) + U * np.abs(b)
    return ref, bound


def layernorm_f32(v, g, b, eps, one_pass=False):
    """The same in plain float32 numpy (two passes).  one_pass (perturbation): var = E[x^2] - mean^2, which cancels in f32."""
    v = np.asarray(v, np.float32)
    H = np.float32(v.shape[-1])
    mean = v.sum(axis=-1, keepdims=True, dtype=np.float32) / H
    d = v - mean
    if one_pass:
        var = (v * v).sum(axis=-1, keepdims=True, dtype=np.float32) / H - mean * mean
    else:
        var = (d * d).sum(axis=-1, keepdims=True, dtype=np.float32) / H
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = np.float32(1.0) / np.sqrt(var + np.float32(eps))
    return (d * inv * np.asarray(g, np.float32) + np.asarray(b, np.float32)).astype(np.float32)


def ordered_sum(terms):
    """((t0 + t1) + t2) + ... in float64 -> (sum, ev): ev = u * sum of the partial sums' magnitudes, the rounding of the same
    chain in f32."""
    acc = f64(terms[0])
    ev = np.zeros_like(acc)
    for t in terms[1:]:
        acc = acc + f64(t)
        ev = ev + U * np.abs(acc)
    return acc, ev


def embed_rows(ids, word, pos, type_table, types, L, t_mod=True, clamp_type=True):
    """The rows embed_ln_kernel normalises, (word + type) + pos, as the three f32 terms [T, H].  An id outside the table
    reads row 0, a type id beyond the table its last row; token t takes position t % L.  t_mod / clamp_type = False: the
    perturbations."""
    ids = np.asarray(ids, np.int64)
    T = ids.size
    vocab = word.shape[0]
    ids = np.where((ids < 0) | (ids >= vocab), 0, ids)
    terms = [word[ids]]
    nt = type_table.shape[0]
    if types is None:
        terms.append(np.broadcast_to(type_table[0], terms[0].shape))
    else:
        ty = np.asarray(types, np.int64)
        ty = np.where((ty < 0) | (ty >= nt), nt - 1, ty) if clamp_type else ty % nt
        terms.append(type_table[ty])
    if pos is not None:
        t = np.arange(T)
        terms.append(pos[t % L] if t_mod else pos[np.minimum(t, pos.shape[0] - 1)])
    return terms


# ---- pooling -------------------------------------------------------------------------------------------------------------

def pool_ref(x, mask, B, L, mean_pool, count_mask=None):
    """x [B*L, H], mask [B, L] -> (ref [B, H], bound).  count_mask (perturbation): the mask whose tokens are summed and
    counted instead."""
    H = x.shape[-1]
    npl = H // 64
    x = f64(x).reshape(B, L, H)
    if not mean_pool:
        v = x[:, 0]
        dv = np.zeros_like(v)
    else:
        m = (np.asarray(mask if count_mask is None else count_mask).reshape(B, L) != 0).astype(np.float64)
        n = m.sum(axis=1, keepdims=True)
        nn = np.maximum(n, 1e-9)
        v = (x * m[:, :, None]).sum(axis=1) / nn
        dv = np.maximum(n - 1, 0) * U * (np.abs(x) * m[:, :, None]).sum(axis=1) / nn + U * np.abs(v)
    N = np.sqrt((v * v).sum(axis=-1, keepdims=True))
    ref = v / (N + 1e-12)
    N2 = np.where(N > 0, N * N, 1.0)
    rel_den = (np.abs(v) * dv).sum(axis=-1, keepdims=True) / N2 + ((npl + 6) / 2.0 + 2.0) * U
    bound = dv / (N + 1e-12) + np.abs(ref) * (rel_den + U)
    return ref, bound


def pool_f32(x, mask, B, L, mean_pool):
    H = x.shape[-1]
    x = np.asarray(x, np.float32).reshape(B, L, H)
    if not mean_pool:
        v = x[:, 0]
    else:
        m = (np.asarray(mask).reshape(B, L) != 0).astype(np.float32)
        n = np.maximum(m.sum(axis=1, keepdims=True, dtype=np.float32), np.float32(1e-9))
        v = (x * m[:, :, None]).sum(axis=1, dtype=np.float32) / n
    N = np.sqrt((v * v).sum(axis=-1, keepdims=True, dtype=np.float32))
    return (v / (N + np.float32(1e-12))).astype(np.float32)


# ---- rotary map ----------------------------------------------------------------------------------------------------------

def rope_table(L, dh, base=10000.0, seed=None):
    """[L, dh / 2, 2] f32 (cos, sin) of distinct angles: pos * base^(-2 i / dh), as the module builds its cache."""
    i = np.arange(dh // 2)
    ang = np.arange(L)[:, None] * (base ** (-2.0 * i / dh))[None, :] + 0.25
    return np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang)], axis=-1).astype(np.float32))


def rope_ref(qkv, table, T, L, H, heads, t_mod=True, interleaved=False, sin_sign=1.0):
    """qkv [T, 3H] -> (ref, bound) of the whole tensor: Q and K rotated (the half split: x1 = the head's first dh / 2
    columns, x2 = the rest), V as it is (bound 0)."""
    dh = H // heads
    half = dh // 2
    x = f64(qkv).reshape(T, 3, heads, dh).copy()
    t = np.arange(T)
    tab = f64(table)[t % L if t_mod else np.minimum(t, L - 1)]           # [T, half, 2]
    c, s = tab[:, None, None, :, 0], tab[:, None, None, :, 1] * sin_sign
    qk = x[:, :2]
    if interleaved:
        x1, x2 = qk[..., 0::2], qk[..., 1::2]
    else:
        x1, x2 = qk[..., :half], qk[..., half:]
    o1, o2 = x1 * c - x2 * s, x2 * c + x1 * s
    b1 = 3 * U * (np.abs(x1 * c) + np.abs(x2 * s))
    b2 = 3 * U * (np.abs(x2 * c) + np.abs(x1 * s))
    ref, bound = x.copy(), np.zeros_like(x)
    if interleaved:
        ref[:, :2, :, 0::2], ref[:, :2, :, 1::2] = o1, o2
        bound[:, :2, :, 0::2], bound[:, :2, :, 1::2] = b1, b2
    else:
        ref[:, :2, :, :half], ref[:, :2, :, half:] = o1, o2
        bound[:, :2, :, :half], bound[:, :2, :, half:] = b1, b2
    return ref.reshape(T, 3 * H), bound.reshape(T, 3 * H)


def rope_f32(qkv, table, T, L, H, heads):
    dh = H // heads
    half = dh // 2
    x = np.asarray(qkv, np.float32).reshape(T, 3, heads, dh).copy()
    tab = np.asarray(table, np.float32)[np.arange(T) % L]
    c, s = tab[:, None, None, :, 0], tab[:, None, None, :, 1]
    x1, x2 = x[:, :2, :, :half].copy(), x[:, :2, :, half:].copy()
    x[:, :2, :, :half] = x1 * c - x2 * s
    x[:, :2, :, half:] = x2 * c + x1 * s
    return x.reshape(T, 3 * H)


# ---- feed-forward gate ---------------------------------------------------------------------------------------------------

def _erf64(x):
    return np.vectorize(math.erf, otypes=[np.float64])(x)


def act64(g, gelu, tanh_gelu=False):
    g = np.asarray(g, np.float64)
    if not gelu:
        with np.errstate(over="ignore"):
            return g / (1.0 + np.exp(-g))
    if tanh_gelu:
        return 0.5 * g * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (g + 0.044715 * g ** 3)))
    return 0.5 * g * (1.0 + _erf64(g / math.sqrt(2.0)))


def gate_ref(value, gate, gelu, swapped=False, tanh_gelu=False):
    """value * act(gate) -> (ref, bound); act = silu or the erf-GELU."""
    v, g = f64(value), f64(gate)
    if swapped:
        v, g = g, v
    a = act64(g, gelu, tanh_gelu)
    ref = v * a
    floor = UNDERFLOW * np.maximum(1.0, np.abs(v))
    if gelu:
        bound = np.abs(v) * (GELU_CA * U * np.abs(a) + GELU_CB * U * np.abs(g)) + floor
    else:
        bound = np.abs(v) * SILU_CA * U * np.abs(a) + floor
    return ref, bound


def gate_f32(value, gate, gelu):
    v, g = np.asarray(value, np.float32), np.asarray(gate, np.float32)
    if gelu:
        e = _erf64((g * np.float32(0.70710678118654752440)).astype(np.float64)).astype(np.float32)   # erf rounded to f32
        return (v * (np.float32(0.5) * g * (np.float32(1.0) + e))).astype(np.float32)
    with np.errstate(over="ignore"):
        return (v * (g / (np.float32(1.0) + np.exp(-g)))).astype(np.float32)


def pack_gate_input(value, gate):
    """Logical value [T, I] and gate [T, I] -> the f32 matrix [T, 2I] whose split form the gate kernel reads: columns in
    groups of 32 = 16 values | their 16 gates (the row order of the up projection's interleaved weight).  Split, a group
    is one 128-byte line: 16 hi of the values | 16 hi of the gates | 16 lo of the values | 16 lo of the gates."""
    T, I = value.shape
    assert I % 16 == 0
    out = np.empty((T, I // 16, 2, 16), np.float32)
    out[:, :, 0] = np.asarray(value, np.float32).reshape(T, I // 16, 16)
    out[:, :, 1] = np.asarray(gate, np.float32).reshape(T, I // 16, 16)
    return np.ascontiguousarray(out.reshape(T, 2 * I))


# ---- query / key LayerNorm -----------------------------------------------------------------------------------------------

def qk_layernorm_ref(qkv, ln, eps, T, H, swap_gamma=False):
    """qkv [T, 3H], ln = gamma_q | beta_q | gamma_k | beta_k [4, H] -> (ref, bound) of the whole tensor (V: as it is,
    bound 0).  swap_gamma (perturbation): the query's gamma on the key."""
    x = f64(qkv).reshape(T, 3, H)
    ln = np.asarray(ln, np.float32).reshape(4, H)
    ref, bound = x.copy(), np.zeros_like(x)
    for w in range(2):
        gam = ln[0] if (w == 1 and swap_gamma) else ln[2 * w]
        ref[:, w], bound[:, w] = layernorm_ref(x[:, w], gam, ln[2 * w + 1], eps, counts=qk_counts(H))
    return ref.reshape(T, 3 * H), bound.reshape(T, 3 * H)


def qk_layernorm_f32(qkv, ln, eps, T, H):
    x = np.asarray(qkv, np.float32).reshape(T, 3, H).copy()
    ln = np.asarray(ln, np.float32).reshape(4, H)
    for w in range(2):
        x[:, w] = layernorm_f32(x[:, w], ln[2 * w], ln[2 * w + 1], eps)
    return x.reshape(T, 3 * H)


# ---- row families of the LayerNorm tests -----------------------------------------------------------------------------------

ROW_FAMILIES = ("normal", "offset", "outlier", "constant", "tiny")


def make_rows(family, T, H, seed):
    """f32 rows [T, H]:
      normal    N(0, 1)
      offset    a common offset of 100 with a spread of 0.01 (a residual stream with a large mean)
      outlier   N(0, 1) with one column of 1e3 per row (a BERT outlier dimension)
      constant  every column of a row equal (var = 0: the output is beta)
      tiny      values of about 1e-20"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, H))
    if family == "offset":
        x = 100.0 + 0.01 * x
    elif family == "outlier":
        x[np.arange(T), rng.integers(0, H, T)] = 1e3
    elif family == "constant":
        x = np.repeat(rng.standard_normal((T, 1)) * 3.0, H, axis=1)
    elif family == "tiny":
        x = x * 1e-20
    elif family != "normal":
        raise ValueError(family)
    return np.ascontiguousarray(x.astype(np.float32))


def make_gamma_beta(H, seed):
    """gamma and beta that differ in every column."""
    rng = np.random.default_rng(seed)
    g = (1.0 + 0.5 * np.sin(np.arange(H) * 0.37) + 0.05 * rng.standard_normal(H)).astype(np.float32)
    b = (0.3 * np.cos(np.arange(H) * 0.11) + np.arange(H) / H + 0.05 * rng.standard_normal(H)).astype(np.float32)
    return g, b
