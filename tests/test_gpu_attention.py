"""Unit parity of the attention kernels (attention_shx_kernel, its body attention_shx_body.hpp, and the
attention inside the out-projection, sp_attn_proj_kernel) through cs_debug_attention, against float64 numpy.

Reference, bar and the source of every constant in it: tests/attention_ref.py (module docstring).  In short,

    t_ij = (log2 e / sqrt(dh)) q_i . k_j - slope_h log2 e |i - j|,   p = 2^(t - max) / sum over visible keys,   o = p v
    |got - ref| <= sum_j p r |v| + |o| sum_j p r + 2^-20 sum_j p |v| + L 2^-35 max |v|,
    r = ln 2 (6e-7 (log2 e / sqrt(dh)) sum_d |q||k| + 2^-23 (2 |t| + |max| + |alibi|)) + 2^-20

on every query row with mask != 0; nothing the kernel returns enters the bound.  tests/test_attention_bar.py shows on the
CPU that this bar bites (a lost edge key, a window off by one, ... leave it by 10^3 - 4 10^5 x) and that a plain float32
evaluation meets it at 0.01 - 0.15; the kernels measure 0.01 - 0.18 (DESIGN.md §4.0 has the table per family).  Every test prints its worst err / bound; DESIGN.md §4.0 and
profiles/attention_operator_parity.log record them.  Needs an MI355X."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import attention_ref as R

pytestmark = pytest.mark.gpu

# (heads, head width): heads-per-block 4 / 2 / 1 by length; the `while (heads % hb)` fallback 4 -> 2; hb 1; the 64-wide kernel
LAYOUTS = [(4, 32), (6, 32), (3, 32), (2, 64)]
LENGTHS = [1, 31, 32, 33, 64, 65, 127, 128, 129, 257, 512]


def run_attention(lib, qkv, mask, B, L, H, heads, slopes=None, window=0, units=None, proj=None, want_pairs=False):
    """-> (out [B*L, H] f32, flag, pairs [n, 2] f32 or None)."""
    from codesearch_amd import _lib

    f32p, u32p, i32p = _lib.f32p, _lib.u32p, _lib.i32p
    qkv = np.ascontiguousarray(qkv, np.float32)
    mask = np.ascontiguousarray(mask, np.int32)
    assert qkv.shape == (B * L, 3 * H) and mask.size == B * L
    out = np.full((B * L, H), np.nan, np.float32)
    flag, npairs = C.c_uint32(0), C.c_uint32(0)
    sl = None if slopes is None else np.ascontiguousarray(slopes, np.float32)
    su = ul = None
    if units is not None:
        su, ul = (np.ascontiguousarray(a, np.uint32) for a in units)
    cap = heads * B * ((L + 127) // 128) * 4
    pairs = np.zeros((cap, 2), np.float32) if want_pairs else None
    w = b = r = None
    if proj is not None:
        w, b, r = (np.ascontiguousarray(a, np.float32) for a in proj)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    _lib.check_diag(lib.cs_debug_attention(0, ptr(qkv, f32p), ptr(mask, i32p), B, L, H, heads, ptr(sl, f32p), window, ptr(su, u32p),
                                           ptr(ul, u32p), 0 if ul is None else len(ul), ptr(w, f32p), ptr(b, f32p), ptr(r, f32p),
                                           ptr(out, f32p), ptr(pairs, f32p), cap if want_pairs else 0,
                                           C.byref(npairs) if want_pairs else None, C.byref(flag)))
    return out, int(flag.value), (pairs[:npairs.value] if want_pairs else None)


def check(lib, what, qkv, mask, B, L, H, heads, slopes=None, window=0):
    """One launch against the float64 reference: flag 0, every output finite, valid rows inside the bound.  Returns the
    worst err / bound."""
    got, flag, _ = run_attention(lib, qkv, mask, B, L, H, heads, slopes=slopes, window=window)
    ref, bound, valid = R.attention_ref(qkv, mask, B, L, H, heads, slopes=slopes, window=window)
    ratio = R.worst_ratio(got, ref, bound, valid)
    print(f"attention {what}: heads {heads} x {H // heads}, B {B}, L {L}, window {window}: flag {flag}, "
          f"finite {bool(np.isfinite(got).all())}, worst err/bound = {ratio:.3f}")
    assert flag == 0, what
    assert np.isfinite(got).all(), what
    assert ratio <= 1.0, (what, ratio)
    return ratio


def lens_mask_sets(L, seed):
    """The two batches of three masks every shape runs: (a full row, valid length 1, interior holes) and (a valid length
    ending exactly on a 32-key tile, one past it, interior holes ending short of L)."""
    a = np.stack([R.mask_from_lens([L], L)[0], R.mask_from_lens([1], L)[0], R.holes_mask(L, seed)])
    te = R.tile_end(L)
    short = R.holes_mask(L, seed + 1)
    short[max(1, (2 * L) // 3):] = 0
    b = np.stack([R.mask_from_lens([te], L)[0], R.mask_from_lens([min(L, te + 1)], L)[0], short])
    return a, b


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("heads,dh", LAYOUTS)
def test_shapes_and_masks_against_float64(diag_lib, heads, dh, L):
    H, B = heads * dh, 3
    for i, mask in enumerate(lens_mask_sets(L, 100 + L)):
        qkv = R.make_qkv("unit", B, L, H, heads, 1000 * heads + 10 * L + i)
        check(diag_lib, f"shapes[{'ab'[i]}]", qkv, mask, B, L, H, heads)


@pytest.mark.parametrize("L", [129, 512])
@pytest.mark.parametrize("heads,dh", [(4, 32), (2, 64)])
@pytest.mark.parametrize("family", [f for f in R.FAMILIES if f != "unit"])
def test_score_families_against_float64(diag_lib, family, heads, dh, L):
    H, B = heads * dh, 3
    mask = np.stack([R.mask_from_lens([L], L)[0], R.mask_from_lens([R.tile_end(L) // 2 + 1], L)[0], R.holes_mask(L, 5 + L)])
    qkv = R.make_qkv(family, B, L, H, heads, 77 + L + heads, mask)
    check(diag_lib, family, qkv, mask, B, L, H, heads)


def test_a_value_beyond_the_f16_range_raises_the_flag(diag_lib):
    heads, dh, B, L = 4, 32, 2, 65
    H = heads * dh
    qkv = R.make_qkv("unit", B, L, H, heads, 9)
    mask = R.mask_from_lens([L, 40], L)
    assert run_attention(diag_lib, qkv, mask, B, L, H, heads)[1] == 0
    qkv[L + 3, 2 * H + 17] = 70000.0   # one |v| > 65,504 (a valid key of the second sequence)
    assert run_attention(diag_lib, qkv, mask, B, L, H, heads)[1] == 1


def test_a_sequence_masked_entirely_is_finite_and_leaves_the_others_alone(diag_lib):
    for heads, dh, L in ((4, 32, 33), (4, 32, 129), (2, 64, 129)):
        H = heads * dh
        qkv = R.make_qkv("unit", 3, L, H, heads, 31 + L)
        mask = np.stack([R.mask_from_lens([L], L)[0], np.zeros(L, np.int32), R.holes_mask(L, 3)])
        got3, flag3, _ = run_attention(diag_lib, qkv, mask, 3, L, H, heads)
        keep = np.r_[0:L, 2 * L:3 * L]
        got2, flag2, _ = run_attention(diag_lib, qkv[keep], mask[[0, 2]], 2, L, H, heads)
        assert flag3 == 0 and flag2 == 0
        assert np.isfinite(got3).all()
        assert np.array_equal(got3[keep], got2)
        ref, bound, valid = R.attention_ref(qkv, mask, 3, L, H, heads)
        assert not valid[L:2 * L].any() and R.worst_ratio(got3, ref, bound, valid) <= 1.0


# ---- ModernBERT's local window (POS = 2) -----------------------------------------------------------------------------------

WINDOWS = [(100, 16), (200, 16), (300, 16), (512, 8), (512, 64), (512, 1)]


@pytest.mark.parametrize("heads,dh", [(4, 32), (2, 64)])
@pytest.mark.parametrize("L,window", WINDOWS)
def test_window_full_masks(diag_lib, L, window, heads, dh):
    H, B = heads * dh, 2
    qkv = R.make_qkv("unit", B, L, H, heads, L + window)
    check(diag_lib, "window, full", qkv, R.mask_from_lens([L, L], L), B, L, H, heads, window=window)


@pytest.mark.parametrize("heads,dh", [(4, 32), (2, 64)])
@pytest.mark.parametrize("L,window", WINDOWS)
def test_window_ragged_masks_with_query_tiles_that_see_no_key(diag_lib, L, window, heads, dh):
    """A short row beside a full one: its padded query rows from 32 ntiles + window on belong to 32-query tiles (and, from
    L = 300 on, whole 128-query blocks) that can see no key tile at all — the kernel walks nothing for them.  They must
    come back finite (zeros) and must not raise the range flag: a raised flag sends the whole mini-batch of an embedder
    to the exact-f32 kernels."""
    H, B = heads * dh, 3
    lens = [L, 5, min(L, 40)]
    mask = R.mask_from_lens(lens, L)
    if L >= 200:
        mask[2, 9] = 0   # and an interior hole in the third row
    qkv = R.make_qkv("unit", B, L, H, heads, 3 * L + window)
    check(diag_lib, "window, ragged", qkv, mask, B, L, H, heads, window=window)
    if L >= 100:   # rows of sequence 1 whose 32-query tile sees no key tile: stored as zeros
        got = run_attention(diag_lib, qkv, mask, B, L, H, heads, window=window)[0]
        first_blind = ((32 + window + 31) // 32 + 1) * 32
        assert first_blind < L and not got[L + first_blind:2 * L].any()


# ---- JinaBert's ALiBi (POS = 1) ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [129, 512])
@pytest.mark.parametrize("dh", [32, 64])
@pytest.mark.parametrize("slopes", ["jina", "geometric"])
def test_alibi_against_float64(diag_lib, slopes, dh, L):
    heads, B = 12, 2
    H = heads * dh
    sl = R.jina_slopes(heads) if slopes == "jina" else R.geometric_slopes(heads)   # 2^-0.5 .. 2^-8 | 1 .. 2^-8
    mask = np.stack([R.mask_from_lens([L], L)[0], R.holes_mask(L, L)])
    mask[1, (3 * L) // 4:] = 0
    qkv = R.make_qkv("unit", B, L, H, heads, L + dh)
    check(diag_lib, f"alibi {slopes}", qkv, mask, B, L, H, heads, slopes=sl)


def test_refusals(diag_lib):
    from codesearch_amd import _lib

    heads, dh, B, L = 4, 32, 1, 40
    H = heads * dh
    qkv = R.make_qkv("unit", B, L, H, heads, 1)
    mask = R.mask_from_lens([L], L)
    with pytest.raises(_lib.CsError) as e:   # the launcher's own refusal comes through
        run_attention(diag_lib, qkv, mask, B, L, H, heads, slopes=R.jina_slopes(heads), window=8)
    assert e.value.code == _lib.CS_ERR_BAD_ARG and "ALiBi and a local window" in str(e.value)
    with pytest.raises(_lib.CsError) as e:   # head width 16
        run_attention(diag_lib, qkv, mask, B, L, H, 8)
    assert e.value.code == _lib.CS_ERR_UNSUPPORTED
    with pytest.raises(_lib.CsError) as e:   # a unit index beyond the units
        run_attention(diag_lib, qkv, mask, B, L, H, heads, units=([1], [L]))
    assert e.value.code == _lib.CS_ERR_BAD_ARG
    w = np.zeros((H, H), np.float32)
    with pytest.raises(_lib.CsError) as e:   # attention inside the out-projection is built for 384 / 12 heads, L <= 32
        run_attention(diag_lib, qkv, mask, B, L, H, heads, proj=(w, np.zeros(H, np.float32), np.zeros((B * L, H), np.float32)))
    assert e.value.code == _lib.CS_ERR_UNSUPPORTED
    f32p = _lib.f32p
    out = np.zeros((B * L, H), np.float32)   # a bias without its weight: the three projection buffers go together
    st = diag_lib.cs_debug_attention(0, qkv.ctypes.data_as(f32p), mask.ctypes.data_as(_lib.i32p), B, L, H, heads, None, 0, None, None, 0,
                                     None, out.ctypes.data_as(f32p), None, out.ctypes.data_as(f32p), None, 0, None, None)
    assert st == _lib.CS_ERR_BAD_ARG


# ---- the range pairs the quantised path reads ----------------------------------------------------------------------------

@pytest.mark.parametrize("heads,dh,L", [(4, 32, 31), (6, 32, 31), (4, 32, 64), (3, 32, 64), (4, 32, 129), (2, 64, 129), (4, 32, 300)])
def test_range_pairs_fold_to_the_stored_extremes(diag_lib, heads, dh, L):
    H, B = heads * dh, 3
    mask = np.stack([R.mask_from_lens([L], L)[0], R.mask_from_lens([max(1, L // 3)], L)[0], R.holes_mask(L, 11)])
    qkv = R.make_qkv("unit", B, L, H, heads, 400 + L)
    got, flag, pairs = run_attention(diag_lib, qkv, mask, B, L, H, heads, want_pairs=True)
    plain = run_attention(diag_lib, qkv, mask, B, L, H, heads)[0]
    assert flag == 0 and np.array_equal(got, plain)
    assert len(pairs) == (heads // R.heads_per_block(L, heads, dh)) * B * ((L + 127) // 128) * 4
    assert pairs[:, 0].min() == min(0.0, got.min()) and pairs[:, 1].max() == max(0.0, got.max())
    assert (pairs[:, 0] <= 0).all() and (pairs[:, 1] >= 0).all()
    # two quantisation units of different padded lengths in one batch: query rows at or beyond the unit's length stay out
    unit_len = [L, max(1, (2 * L) // 5)]
    seq_unit = [0, 1, 1]
    got_u, _, pairs_u = run_attention(diag_lib, qkv, mask, B, L, H, heads, units=(seq_unit, unit_len), want_pairs=True)
    assert np.array_equal(got_u, plain) and len(pairs_u) == len(pairs)
    inside = np.concatenate([got[b * L:b * L + unit_len[seq_unit[b]]].ravel() for b in range(B)])
    assert pairs_u[:, 0].min() == min(0.0, inside.min()) and pairs_u[:, 1].max() == max(0.0, inside.max())
    per_seq = len(pairs) // B   # ... and per sequence, as launch_q8_range_units folds them
    for b in range(B):
        rows = got[b * L:b * L + unit_len[seq_unit[b]]]
        pb = pairs_u[b * per_seq:(b + 1) * per_seq]
        assert pb[:, 0].min() == min(0.0, rows.min()) and pb[:, 1].max() == max(0.0, rows.max())


# ---- attention inside the out-projection (sp_attn_proj_kernel) -------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 3, 16, 17, 24, 32])   # a 16-row tile's sequences span <= 32 rows up to L = 16, 64 beyond
def test_attention_inside_the_out_projection(diag_lib, L):
    """Reference: the attention reference, then @ W^T + bias + resid in float64.  Bar: the attention bound pushed through
    |W|, plus the dense layers' own bar (tests/test_gpu_gemm_split.py): 6e-7 (sum |ctx||w| + |bias| + |resid|)."""
    heads, H = 12, 384
    worst = 0.0
    for B in sorted({1, max(1, 96 // L), 192 // L}):   # T = B L up to 192, with and without a partial 16-row tile
        T = B * L
        rng = np.random.default_rng(50 * L + B)
        lens = rng.integers(1, L + 1, B)
        lens[0] = L
        mask = R.mask_from_lens(lens, L)
        if L >= 16 and B > 1:
            mask[1] = R.holes_mask(L, L)
        qkv = R.make_qkv("unit", B, L, H, heads, 60 * L + B)
        W = (rng.standard_normal((H, H)) * 0.05).astype(np.float32)
        bias = (rng.standard_normal(H) * 0.1).astype(np.float32)
        resid = rng.standard_normal((T, H)).astype(np.float32)
        got, flag, _ = run_attention(diag_lib, qkv, mask, B, L, H, heads, proj=(W, bias, resid))
        ctx, cbound, valid = R.attention_ref(qkv, mask, B, L, H, heads)
        W64 = W.astype(np.float64)
        ref = ctx @ W64.T + bias.astype(np.float64) + resid.astype(np.float64)
        bound = cbound @ np.abs(W64).T + R.PRODUCT_BAR * (np.abs(ctx) @ np.abs(W64).T + np.abs(bias) + np.abs(resid))
        ratio = R.worst_ratio(got, ref, bound, valid)
        worst = max(worst, ratio)
        assert flag == 0 and np.isfinite(got).all()
        assert ratio <= 1.0, (L, B, ratio)
    print(f"attention inside the out-projection: L {L}: worst err/bound = {worst:.3f}")
