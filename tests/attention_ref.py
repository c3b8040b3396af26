"""Float64 reference, error bound and input families of the attention operator tests (tests/test_gpu_attention.py,
tests/test_attention_bar.py).  Pure numpy: nothing here touches the library under test.

The operator (codesearch_amd/csrc/attention_shx_body.hpp), in the exp2 domain as the kernel states it:

    t_ij = (log2 e / sqrt(dh)) q_i . k_j  -  slope_h log2 e |i - j|
    key j visible to query i:  mask[j] != 0, and |i - j| <= window when a window is set
    p_ij = 2^(t_ij - max_i) / sum over visible j,    o_i = sum_j p_ij v_j

The bar is a first-order error bound per output element, formed from the reference's own quantities only:

    dt_ij    = 6e-7 (log2 e / sqrt(dh)) sum_d |q_id| |k_jd|  +  2^-23 (2 |t_ij| + |max_i| + |alibi term|)
    r_ij     = ln 2 dt_ij + 2^-20
    bound_id = sum_j p_ij r_ij |v_jd|  +  |o_id| sum_j p_ij r_ij  +  2^-20 sum_j p_ij |v_jd|  +  L 2^-35 max |v|

Where each constant comes from:
  6e-7     the split-f16 product's per-product bar (split_f16.hpp: "<= ~3 * 2^-22 |a w|"), as asserted on the dense layers in
           tests/test_gpu_gemm_split.py; the score product is the same three-MFMA sum (attention_shx_body.hpp compute_s).
  2^-23    two f32 roundings at 2^-24 each on t (the fma h2 * scale + mask, with scale_log2e and slope * log2 e themselves
           rounded to f32: launch_attention_sh2, embedder.hip) and one on t - m (finish_tile, d2 = p2 - m2v); the ALiBi term
           is one more fma on the mask word.
  ln 2     d(2^x) = ln 2 2^x dx.
  2^-20    in r: the hardware exp2 (v_exp_f32, 1 ulp = 2^-23) and the probability's two round-toward-zero f16 planes — the
           high plane leaves a residual below 2^-10 E, the residual's own f16 leaves below 2^-10 of that (comment "Probabilities
           travel as E = 2^11 e", attention_shx_body.hpp).
  2^-20    on sum p |v|: the dropped v_lo P_lo'' product (2^-11 * 2^-10 = 2^-21 of the term) plus the store's split
           (sh_split: 2^-22) and the f32 roundings of the accumulation's final scale — together below 2^-20.
  L 2^-35  E = 2^11 e is cut at the f16 subnormal spacing 2^-24, i.e. e at 2^-35 absolutely; the row sum is >= 1 in these units
           because the running reference m never exceeds the row's maximum (it may lag it by up to CS_ATTN_LAZY_RESCALE = 4),
           so each of at most L keys adds at most 2^-35 |v| after the division.
"""
import math

import numpy as np

LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
PRODUCT_BAR = 6e-7


def split_qkv(qkv, B, L, H, heads):
    """[B*L, 3H] (a row = Q heads | K heads | V heads) -> q, k, v as [B, heads, L, dh], same dtype."""
    dh = H // heads
    x = qkv.reshape(B, L, 3, heads, dh)
    return tuple(np.ascontiguousarray(x[:, :, i].transpose(0, 2, 1, 3)) for i in range(3))


def visibility(mask, L, window):
    """[B, 1, L, L] bool: key j visible to query i."""
    idx = np.arange(L)
    dist = np.abs(idx[:, None] - idx[None, :])
    vis = (np.asarray(mask).reshape(-1, L) != 0)[:, None, None, :]
    if window:
        vis = vis & (dist <= window)[None, None]
    return np.broadcast_to(vis, (vis.shape[0], 1, L, L)), dist


def attention_ref(qkv, mask, B, L, H, heads, slopes=None, window=0, key_mask=None, scale_dh=None, want_bound=True):
    """Float64 attention of f32 inputs.  Returns (out [B*L, H], bound [B*L, H] or None, valid [B*L] bool).
    key_mask (default: mask) decides which keys are visible; `valid` (which query rows are compared) always comes from
    mask.  scale_dh: the head width the scale 1 / sqrt(dh) is taken for (default: the real one).  Both exist for the
    perturbation test only."""
    dh = H // heads
    q, k, v = split_qkv(np.asarray(qkv, np.float32).astype(np.float64), B, L, H, heads)
    scale = LOG2E / math.sqrt(scale_dh or dh)
    vis, dist = visibility(mask if key_mask is None else key_mask, L, window)
    s = np.einsum("bhid,bhjd->bhij", q, k) * scale
    if slopes is not None:
        alibi = (np.asarray(slopes, np.float32).astype(np.float64) * LOG2E)[None, :, None, None] * dist[None, None]
    else:
        alibi = np.zeros((1, 1, L, L))
    t = s - alibi
    tm = np.where(vis, t, -np.inf)
    mx = tm.max(axis=-1, keepdims=True)
    seen = np.isfinite(mx)                      # a query with no visible key (padded rows only) gets p = 0
    mx = np.where(seen, mx, 0.0)
    e = np.where(vis, np.exp2(tm - mx), 0.0)
    den = e.sum(axis=-1, keepdims=True)
    p = e / np.where(den > 0, den, 1.0)
    o = p @ v
    out = o.transpose(0, 2, 1, 3).reshape(B * L, H)
    valid = np.asarray(mask).reshape(B * L) != 0
    if not want_bound:
        return out, None, valid
    sabs = np.einsum("bhid,bhjd->bhij", np.abs(q), np.abs(k)) * scale
    dt = PRODUCT_BAR * sabs + 2.0 ** -23 * (2.0 * np.abs(t) + np.abs(mx) + np.abs(alibi))
    pr = p * (LN2 * dt + 2.0 ** -20)
    av = np.abs(v)
    vmax = np.where(vis.any(axis=2)[..., None], av, 0.0).max(axis=(2, 3), keepdims=True)  # over the keys some query sees
    bound = pr @ av + np.abs(o) * pr.sum(axis=-1, keepdims=True) + 2.0 ** -20 * (p @ av) + L * 2.0 ** -35 * vmax
    return out, bound.transpose(0, 2, 1, 3).reshape(B * L, H), valid


def attention_f32(qkv, mask, B, L, H, heads, slopes=None, window=0):
    """The same operator evaluated in plain float32 numpy (what an unfused f32 implementation gives): a sanity check that
    the bar is one a correct single-precision evaluation meets."""
    dh = H // heads
    q, k, v = split_qkv(np.asarray(qkv, np.float32), B, L, H, heads)
    vis, dist = visibility(mask, L, window)
    t = np.einsum("bhid,bhjd->bhij", q, k) * np.float32(LOG2E / math.sqrt(dh))
    if slopes is not None:
        t = t - (np.asarray(slopes, np.float32) * np.float32(LOG2E))[None, :, None, None] * dist[None, None].astype(np.float32)
    tm = np.where(vis, t, np.float32(-np.inf))
    mx = tm.max(axis=-1, keepdims=True)
    mx = np.where(np.isfinite(mx), mx, np.float32(0))
    e = np.where(vis, np.exp2(tm - mx), np.float32(0)).astype(np.float32)
    den = e.sum(axis=-1, keepdims=True)
    o = (e @ v) / np.where(den > 0, den, np.float32(1))
    return o.transpose(0, 2, 1, 3).reshape(B * L, H).astype(np.float32)


def worst_ratio(got, ref, bound, valid):
    """max over valid query rows of |got - ref| / bound (inf when a compared value is not finite)."""
    g = np.asarray(got, np.float64)[valid]
    if not np.isfinite(g).all():
        return math.inf
    return float((np.abs(g - ref[valid]) / bound[valid]).max()) if valid.any() else 0.0


# ---- masks ---------------------------------------------------------------------------------------------------------------

def mask_from_lens(lens, L):
    m = np.zeros((len(lens), L), np.int32)
    for b, n in enumerate(lens):
        m[b, :n] = 1
    return m


def holes_mask(L, seed):
    """Valid positions with interior holes: position 0 and the last one stay valid, about a third of the rest is masked."""
    rng = np.random.default_rng(seed)
    m = (rng.random(L) > 0.35).astype(np.int32)
    m[0] = 1
    m[L - 1] = 1
    return m


def tile_end(L):
    """The largest valid length that ends exactly on a 32-key tile (L itself below 32)."""
    return L // 32 * 32 if L >= 32 else L


# ---- score families ------------------------------------------------------------------------------------------------------

FLAT_FAMILIES = ("unit", "narrow", "vbig")
PEAKY_FAMILIES = ("wide", "ramp3.9", "ramp4.1", "dominant_first", "dominant_last")
FAMILIES = FLAT_FAMILIES + PEAKY_FAMILIES


def make_qkv(family, B, L, H, heads, seed, mask=None):
    """f32 qkv [B*L, 3H] of one score family:
      unit            q, k, v unit normal (scores of about +-1.4 in the log2 domain)
      narrow          q x 0.02: near-uniform probabilities, the query's scaled low plane in the f16 subnormals
      vbig            unit scores, v uniform in +-60,000: just inside the f16 range
      wide            q x 14: log2-domain scores of about +-60
      ramp<g>         the score rises by g per 32-key tile (+- 0.05): g = 3.9 stays inside the lazy rescale's lag of
                      CS_ATTN_LAZY_RESCALE = 4, g = 4.1 moves the reference at every tile
      dominant_first  one key, at the first slot of the second tile (or slot 0), outweighs the rest by ~2^20
      dominant_last   the same at each sequence's last valid slot (needs mask)"""
    dh = H // heads
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, L, 3, heads, dh))
    scale = LOG2E / math.sqrt(dh)
    if family == "narrow":
        x[:, :, 0] *= 0.02
    elif family == "vbig":
        x[:, :, 2] = rng.uniform(-60000.0, 60000.0, (B, L, heads, dh))
    elif family == "wide":
        x[:, :, 0] *= 14.0
    elif family.startswith("ramp"):
        g = float(family[4:])
        x[:, :, 0] *= 0.02
        x[:, :, 0, :, 0] = 4.0
        x[:, :, 1, :, 0] = (g * (np.arange(L) // 32) / (scale * 4.0))[None, :, None]
    elif family.startswith("dominant"):
        x[:, :, 0, :, 0] = 3.0
        for b in range(B):
            if family == "dominant_first":
                j = 32 if L > 32 else 0
            else:
                j = int(np.flatnonzero(np.asarray(mask).reshape(B, L)[b])[-1])
            x[b, j, 1, :, 0] = 20.0 / (scale * 3.0)
    elif family != "unit":
        raise ValueError(family)
    return np.ascontiguousarray(x.reshape(B * L, 3 * H).astype(np.float32))


def jina_slopes(heads):
    """JinaBert's ALiBi slopes as cs_embedder_create forms them (embedder.hip): for 12 heads 2^-1 .. 2^-8 and
    2^-0.5, 2^-1.5, 2^-2.5, 2^-3.5."""
    closest = 1
    while closest * 2 <= heads:
        closest *= 2

    def slope(n, i):
        start = 2.0 ** (-8.0 / n)
        return start * start ** i
    return np.array([slope(closest, i) if i < closest else slope(2 * closest, 2 * (i - closest)) for i in range(heads)], np.float32)


def geometric_slopes(heads):
    """heads slopes from 1 down to 2^-8, evenly spaced in the exponent."""
    return np.array([2.0 ** (-8.0 * i / (heads - 1)) for i in range(heads)], np.float32)


def heads_per_block(L, heads, dh):
    """launch_attention_sh2: head_dim 32 packs 4 heads into a block up to 32 tokens, 2 up to 64, halved until it divides
    the head count; head_dim 64 never packs."""
    if dh != 32:
        return 1
    Lp = (L + 31) // 32 * 32
    hb = 4 if Lp <= 32 else (2 if Lp <= 64 else 1)
    while heads % hb:
        hb //= 2
    return hb
