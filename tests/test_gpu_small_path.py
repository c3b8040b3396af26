"""Unit parity of the small path's dense kernels (csrc/small_path.hip: sp_ln_gemm_kernel — LayerNorm, the slab sum or the
embedding gather as the prologue of the QKV / FFN-up product, narrow and wide form — and sp_partial_kernel, FFN-down as four K
slices) through cs_debug_small_path, against float64 numpy.

Every launch is checked in two stages (tests/small_path_ref.py, module docstring): Xout against the LayerNorm reference and
bound of tests/rows_ref.py, then Cs against the float64 product of the f32 rows Xout actually holds.  Every comparison
asserts a finite output, the range flag 0 (unless the test is about the flag), the guard rows behind row T - 1 untouched and
err / bound <= 1 with no factor on the bound; every test prints its worst err / bound (DESIGN.md §4.0,
profiles/small_path_operator_parity.log).  tests/test_small_path_bar.py shows on the CPU that these bars bite.
Needs an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import rows_ref as R
from tests import small_path_ref as S
from tests.test_gpu_rows import BIAS_SCALE, run_rows

pytestmark = pytest.mark.gpu

HIDDEN = [384, 768, 1024]
# partial last 16-row tiles, a 4-row wave group that straddles T, the last narrow (127) and the first wide size (128) at 384,
# SP_MAX_ROWS; the larger widths have one form only
ROWS = {384: [1, 15, 16, 17, 33, 127, 128, 130, 199, 256], 768: [1, 17, 130, 256], 1024: [1, 17, 130, 256]}
SMALL_T = 33
# prologue 2: T = B * L for L in {1, 5, 32}
EMBED_ROWS = {384: [(1, 1), (15, 5), (16, 1), (17, 1), (33, 1), (35, 5), (64, 32), (127, 1), (128, 32), (130, 5), (199, 1), (256, 32)],
              768: [(1, 1), (17, 1), (130, 5), (256, 32)], 1024: [(1, 1), (17, 1), (130, 5), (256, 32)]}
EPS = [1e-12, 1e-5]
VOCAB, NTYPES = 40, 2


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, np.int32)


def run_ln_gemm(lib, epi, pro, H, T, N, g, b, W, bias, eps=1e-12, L=1, rows=None, parts=None, parts_bias=None, x=None, ids=None,
                word=None, pos=None, type_table=None, types=None):
    """One launch_sp_ln_gemm -> dict(xout, cs, x_after, flag, in_flag, guard)."""
    from codesearch_amd import _lib

    f32p, i32p = _lib.f32p, _lib.i32p
    g, b, W, bias, rows, parts, parts_bias, x, word, pos, type_table = (_f32(a) for a in (g, b, W, bias, rows, parts, parts_bias, x, word, pos, type_table))
    ids, types = _i32(ids), _i32(types)
    assert W.shape == (N, H) and bias.shape == (N,)
    assert rows is None or rows.shape == (T, H)
    assert parts is None or (parts.shape == (4, T, H) and x.shape == (T, H))
    assert ids is None or (ids.shape == (T,) and pos.shape == (L, H) and T % L == 0)
    xout = np.full((T, H), np.nan, np.float32)
    cs = np.full((T, N), np.nan, np.float32)
    x_after = np.full((T, H), np.nan, np.float32) if pro == 1 else None
    flags = (C.c_uint32 * 2)(7, 7)
    guard = C.c_uint32(7)
    _lib.check_diag(lib.cs_debug_small_path(
        0, 0, epi, pro, H, T, N, L, eps, _ptr(g, f32p), _ptr(b, f32p), _ptr(rows, f32p), _ptr(parts, f32p), _ptr(parts_bias, f32p),
        _ptr(x, f32p), _ptr(ids, i32p), _ptr(word, f32p), _ptr(pos, f32p), _ptr(type_table, f32p), _ptr(types, i32p),
        0 if type_table is None else type_table.shape[0], 0 if word is None else word.shape[0], _ptr(W, f32p), _ptr(bias, f32p),
        _ptr(xout, f32p), _ptr(cs, f32p), _ptr(x_after, f32p), None, flags, C.byref(guard)))
    if pro == 1:
        assert np.array_equal(x_after.view(np.uint32), x.view(np.uint32)), "the slab-sum prologue changed its residual"
    return dict(xout=xout, cs=cs, x_after=x_after, flag=int(flags[0]), in_flag=int(flags[1]), guard=int(guard.value))


def run_partial(lib, H, T, N, A, W):
    """One launch_sp_partial -> dict(parts [4, T, N], flag, in_flag, guard)."""
    from codesearch_amd import _lib

    f32p = _lib.f32p
    A, W = _f32(A), _f32(W)
    assert A.shape == (T, 4 * H) and W.shape == (N, 4 * H)
    parts = np.full((4, T, N), np.nan, np.float32)
    flags = (C.c_uint32 * 2)(7, 7)
    guard = C.c_uint32(7)
    _lib.check_diag(lib.cs_debug_small_path(0, 1, 0, 0, H, T, N, 1, 0.0, None, None, _ptr(A, f32p), None, None, None, None, None, None, None,
                                            None, 0, 0, _ptr(W, f32p), None, None, None, None, _ptr(parts, f32p), flags, C.byref(guard)))
    return dict(parts=parts, flag=int(flags[0]), in_flag=int(flags[1]), guard=int(guard.value))


@functools.lru_cache(maxsize=None)
def weights(N, K, seed=0):
    return S.make_weights(N, K, 100 + seed)


def settle(what, r, stage1, W, bias, epi, want_flag=0):
    """The shared checks of one sp_ln_gemm launch -> (stage 1 ratio, stage 2 ratio)."""
    assert r["guard"] == 0, (what, "guard words changed", r["guard"])
    assert (r["flag"], r["in_flag"]) == (want_flag, 0), (what, r["flag"], r["in_flag"])
    assert np.isfinite(r["xout"]).all() and np.isfinite(r["cs"]).all(), what
    r1 = R.worst(r["xout"], *stage1)
    assert r1 <= 1.0, (what, "Xout", r1)
    r2 = R.worst(r["cs"], *S.ln_gemm_ref(r["xout"], W, bias, epi))
    assert r2 <= 1.0, (what, "Cs", r2)
    return r1, r2


def settle_partial(what, r, A, W, H):
    assert r["guard"] == 0, (what, "guard words changed", r["guard"])
    assert (r["flag"], r["in_flag"]) == (0, 0), what
    assert np.isfinite(r["parts"]).all(), what
    ratio = R.worst(r["parts"], *S.partial_ref(A, W, H))
    assert ratio <= 1.0, (what, ratio)
    return ratio


# ---- inputs of the three prologues -----------------------------------------------------------------------------------------

def slab_inputs(family, T, H, seed):
    """Four slabs, their bias and the residual whose sum has the family's character."""
    rng = np.random.default_rng(seed)
    terms = [R.make_rows(family, T, H, seed + 7 * s) / np.float32(5) for s in range(5)]
    pb = np.full(H, 0.25, np.float32) if family == "constant" else (rng.standard_normal(H) * BIAS_SCALE[family]).astype(np.float32)
    return dict(parts=np.stack(terms[:4]), parts_bias=pb, x=terms[4])


def embed_inputs(family, T, L, H, seed, type_mode):
    """ids with the table's ends and an id beyond it; types null (0), given (1) or given with one beyond the table (2)."""
    rng = np.random.default_rng(seed)
    word = R.make_rows(family, VOCAB, H, seed) * np.float32(0.5)
    pos = R.make_rows(family, L, H, seed + 1) * np.float32(0.25)
    tab = R.make_rows(family, NTYPES, H, seed + 2) * np.float32(0.25)
    ids = rng.integers(0, VOCAB, T)
    ids[0] = 0
    ids[T - 1] = VOCAB - 1 if T > 1 else 0
    if T > 2:
        ids[T // 2] = VOCAB + 3
    types = None
    if type_mode:
        types = rng.integers(0, NTYPES, T)
        if type_mode == 2:
            types[T - 1] = NTYPES + 1
    return dict(ids=ids, word=word, pos=pos, type_table=tab, types=types, L=L)


def prologue_inputs(pro, family, T, H, seed, L=1, type_mode=0):
    if pro == 0:
        return dict(rows=R.make_rows(family, T, H, seed))
    if pro == 1:
        return slab_inputs(family, T, H, seed)
    return embed_inputs(family, T, L, H, seed, type_mode)


def products(H, T):
    """(epi, N) as the embedder uses them; at H = 384 from the first wide size on also N = 96, no multiple of 64: the launcher
    must stay on the narrow form there."""
    out = [(S.EPI_SPLIT, 3 * H), (S.EPI_GELU, 4 * H)]
    if H == 384 and T >= 128:
        out.append((S.EPI_SPLIT, 96))
    return out


# ---- op 0 against float64 -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", HIDDEN)
@pytest.mark.parametrize("pro", [0, 1, 2])
def test_ln_gemm_against_float64(diag_lib, pro, H):
    g, b = R.make_gamma_beta(H, H + pro)
    worst1, worst2, launches = {}, {}, 0
    cases = [(T, 1) for T in ROWS[H]] if pro != 2 else EMBED_ROWS[H]
    for ci, (T, L) in enumerate(cases):
        families = R.ROW_FAMILIES if T <= SMALL_T else (R.ROW_FAMILIES[ci % len(R.ROW_FAMILIES)],)
        for fi, family in enumerate(families):
            seed = 1000 * pro + 10 * T + fi
            inp = prologue_inputs(pro, family, T, H, seed, L=L, type_mode=(ci + fi) % 3)
            for eps in EPS:
                stage1 = S.prologue_ref(pro, g, b, eps, **inp)
                for epi, N in products(H, T):
                    W, bias = weights(N, H, epi)
                    r = run_ln_gemm(diag_lib, epi, pro, H, T, N, g, b, W, bias, eps=eps, **inp)
                    r1, r2 = settle((pro, H, T, L, family, eps, epi, N), r, stage1, W, bias, epi)
                    worst1[family] = max(worst1.get(family, 0.0), r1)
                    key = "GELU" if epi else "split"
                    worst2[key] = max(worst2.get(key, 0.0), r2)
                    launches += 1
    print(f"sp_ln_gemm prologue {pro} H {H}: {launches} launches, worst err/bound Xout " + ", ".join(f"{k} {v:.3f}" for k, v in worst1.items())
          + "; Cs " + ", ".join(f"{k} {v:.3f}" for k, v in worst2.items()))


# ---- op 1 against float64 -------------------------------------------------------------------------------------------------

MID_FAMILIES = ("normal", "wide", "outlier", "big")


def ffn_mid(family, T, H, seed):
    """A [T, 4H] in split form, of the character FFN-down reads:
      normal    the GELU of N(0, 1)
      wide      the GELU of N(0, 3): values up to about 12, and a third of them the tiny outputs of deep negative inputs
      outlier   normal with one column of 1e3 per row
      big       uniform in +-60,000: just inside the f16 range
    (The product's bar is relative.  A value under 2^-14 carries the format's absolute 2^-36 instead (split_f16.hpp), which
    the bar does not grant: these families keep such values a minority of every K slice, as activations do.)"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((T, 4 * H))
    if family == "wide":
        v = v * 3.0
    if family == "big":
        a = rng.uniform(-60000.0, 60000.0, (T, 4 * H))
    else:
        a = R.act64(v.astype(np.float32), True)
    if family == "outlier":
        a[np.arange(T), rng.integers(0, 4 * H, T)] = 1e3
    return R.split_roundtrip(a.astype(np.float32))


@pytest.mark.parametrize("H", HIDDEN)
def test_partial_against_float64(diag_lib, H):
    worst, launches = {}, 0
    for ci, T in enumerate(ROWS[H]):
        families = MID_FAMILIES if T <= SMALL_T else (MID_FAMILIES[ci % len(MID_FAMILIES)],)
        for fi, family in enumerate(families):
            A = ffn_mid(family, T, H, 50 * T + fi)
            for N in ([H, 96] if (H == 384 and T >= 128) else [H]):
                W, _ = weights(N, 4 * H)
                r = run_partial(diag_lib, H, T, N, A, W)
                worst[family] = max(worst.get(family, 0.0), settle_partial((H, T, N, family), r, A, W, H))
                launches += 1
    print(f"sp_partial H {H}: {launches} launches, worst err/bound per slab " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---- exactness and mapping ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", HIDDEN)
def test_ln_gemm_is_exact_on_integer_rows_and_weights(diag_lib, H):
    """gamma = 0 makes every normalised row equal beta, here small integers; with integer weights asymmetric in n and k every
    product and partial sum is exact: Xout is beta and Cs the integer result, bit for bit, for every prologue."""
    beta = ((np.arange(H) % 7) - 3).astype(np.float32)
    for T in ([17, 130, 256] if H == 384 else [17, 130]):
        for N in ([3 * H, 96] if H == 384 else [3 * H]):
            W, bias = S.integer_weights(N, H, H + N)
            want = (beta.astype(np.int64)[None, :] @ W.astype(np.int64).T + bias.astype(np.int64)).astype(np.float32)
            for pro in (0, 1, 2):
                inp = prologue_inputs(pro, "normal", T, H, 7 + pro, L=1, type_mode=1)
                r = run_ln_gemm(diag_lib, S.EPI_SPLIT, pro, H, T, N, np.zeros(H, np.float32), beta, W, bias, **inp)
                what = (H, T, N, pro)
                assert r["guard"] == 0 and (r["flag"], r["in_flag"]) == (0, 0), what
                assert np.array_equal(r["xout"], np.broadcast_to(beta, (T, H))), what
                assert np.array_equal(r["cs"], np.broadcast_to(want, (T, N))), what
    # rows that differ: alternating +-1 with eps = 0 normalise to rn(+-g + b) exactly (tests/test_gpu_rows.py); integer g, b
    T, N = 37, 3 * H
    W, bias = S.integer_weights(N, H, 3 * H)
    pm = np.where((np.arange(H)[None, :] + np.arange(T)[:, None]) % 2 == 0, 1.0, -1.0).astype(np.float32)
    g, b = ((np.arange(H) % 3) + 1).astype(np.float32), ((np.arange(H) % 5) - 2).astype(np.float32)
    rows = (pm * g[None, :] + b[None, :]).astype(np.float32)
    r = run_ln_gemm(diag_lib, S.EPI_SPLIT, 0, H, T, N, g, b, W, bias, eps=0.0, rows=pm)
    assert r["guard"] == 0 and r["flag"] == 0 and np.array_equal(r["xout"], rows)
    assert np.array_equal(r["cs"], (rows.astype(np.int64) @ W.astype(np.int64).T + bias.astype(np.int64)).astype(np.float32))
    print(f"sp_ln_gemm exact cases H {H}: bit for bit")


@pytest.mark.parametrize("H", HIDDEN)
def test_partial_slabs_are_exact_on_integers_each_in_its_own_k_range(diag_lib, H):
    """Integer A and W with another weight pattern in each K quarter: slab ks must be the integer product over
    [ks H, (ks + 1) H) bit for bit.  (The sum of the slabs would not see a chunk put into the wrong slab.)"""
    for T in ([17, 130, 256] if H == 384 else [17, 130]):
        for N in ([H, 96] if H == 384 else [H]):
            A = np.random.default_rng(T + N).integers(-4, 5, (T, 4 * H)).astype(np.float32)
            W, _ = S.integer_weights(N, 4 * H, H + T, quarters=4)
            r = run_partial(diag_lib, H, T, N, A, W)
            assert r["guard"] == 0 and (r["flag"], r["in_flag"]) == (0, 0), (H, T, N)
            want = np.stack([(A[:, k * H:(k + 1) * H].astype(np.int64) @ W[:, k * H:(k + 1) * H].astype(np.int64).T).astype(np.float32) for k in range(4)])
            assert len({want[k].tobytes() for k in range(4)}) == 4
            for ks in range(4):
                assert np.array_equal(r["parts"][ks], want[ks]), (H, T, N, ks)
    print(f"sp_partial exact slabs H {H}: bit for bit")


# ---- the wide form against the narrow form -----------------------------------------------------------------------------------

def test_the_wide_form_gives_the_narrow_forms_bits(diag_lib):
    """H = 384: T = 144 takes the wide form (a block = 16 x 64), T = 112 the narrow one (16 x 16).  Rows are independent, so
    the first 112 rows of Xout, Cs and parts must be equal bit for bit."""
    H, TW, TN, L = 384, 144, 112, 16
    g, b = R.make_gamma_beta(H, 31)

    def first(inp):
        out = {}
        for k, v in inp.items():
            if k == "parts":
                out[k] = np.ascontiguousarray(v[:, :TN])        # the slab stride follows T
            elif k in ("rows", "x", "ids", "types") and v is not None:
                out[k] = v[:TN]
            else:
                out[k] = v
        return out

    for pro in (0, 1, 2):
        inp = prologue_inputs(pro, "normal", TW, H, 40 + pro, L=L, type_mode=1)
        for epi, N in ((S.EPI_SPLIT, 3 * H), (S.EPI_GELU, 4 * H)):
            W, bias = weights(N, H, epi)
            wide = run_ln_gemm(diag_lib, epi, pro, H, TW, N, g, b, W, bias, **inp)
            narrow = run_ln_gemm(diag_lib, epi, pro, H, TN, N, g, b, W, bias, **first(inp))
            for r in (wide, narrow):
                assert r["guard"] == 0 and (r["flag"], r["in_flag"]) == (0, 0) and np.isfinite(r["cs"]).all()
            assert np.array_equal(wide["xout"][:TN].view(np.uint32), narrow["xout"].view(np.uint32)), (pro, epi, "Xout")
            assert np.array_equal(wide["cs"][:TN].view(np.uint32), narrow["cs"].view(np.uint32)), (pro, epi, "Cs")
    A = ffn_mid("normal", TW, H, 60)
    W, _ = weights(H, 4 * H)
    wide, narrow = run_partial(diag_lib, H, TW, H, A, W), run_partial(diag_lib, H, TN, H, A[:TN], W)
    assert wide["guard"] == 0 and narrow["guard"] == 0
    assert np.array_equal(wide["parts"][:, :TN].view(np.uint32), narrow["parts"].view(np.uint32))
    print("wide form against narrow form, H 384, T 144 / 112: bit for bit (3 prologues x 2 epilogues, FFN-down)")


# ---- the prologues against the row kernels ---------------------------------------------------------------------------------

@pytest.mark.parametrize("H", HIDDEN)
def test_the_prologues_give_the_row_kernels_bits(diag_lib, H):
    """ln_rows_core<NPL, 4> is "per row exactly ln_row_core's operations in its order", prologue 1 "the arithmetic of
    layernorm_sum_kernel": Xout of prologues 0, 1 and 2 equals the f32 rows of layernorm_kernel, layernorm_sum_kernel (4
    slabs) and embed_ln_kernel on the same inputs, bit for bit."""
    g, b = R.make_gamma_beta(H, 77)
    W, bias = weights(96, H)
    for T, L in ((5, 5), (130, 5)):
        for fi, family in enumerate(R.ROW_FAMILIES):
            for eps in EPS:
                for pro, which in ((0, 1), (1, 3), (2, 0)):
                    inp = prologue_inputs(pro, family, T, H, 900 + fi + pro, L=L, type_mode=2)
                    r = run_ln_gemm(diag_lib, S.EPI_SPLIT, pro, H, T, 96, g, b, W, bias, eps=eps, **inp)
                    if pro == 0:
                        k = run_rows(diag_lib, 1, H, T=T, eps=eps, x=inp["rows"], g=g, b=b)
                    elif pro == 1:
                        k = run_rows(diag_lib, 3, H, T=T, eps=eps, x=inp["x"], parts=inp["parts"], bias=inp["parts_bias"], g=g, b=b)
                    else:
                        k = run_rows(diag_lib, 0, H, T=T, L=L, eps=eps, ids=inp["ids"], word=inp["word"], pos=inp["pos"],
                                     type_table=inp["type_table"], types=inp["types"], g=g, b=b)
                    assert r["guard"] == 0 and r["flag"] == 0 and k["flag"] == 0
                    same = r["xout"].view(np.uint32) == k["out"].view(np.uint32)
                    assert same.all(), (H, T, family, eps, pro, int((~same).sum()), "values differ from the row kernel's")
    print(f"prologues 0 / 1 / 2 against layernorm / layernorm_sum / embed_ln, H {H}: bit for bit")


# ---- the range flag -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [17, 130])    # the narrow and the wide form
def test_range_flag(diag_lib, T):
    """A gamma that pushes one normalised value past 65,504 raises the flag, a bias that pushes one GELU output past it raises
    it from the epilogue's split, a NaN in Y raises it; the same inputs without the offending value leave it 0.
    The prologue's split alone: a value past 65,504 becomes an infinite hi plane, whose products are infinite or NaN, so the
    epilogue's split reports it too — except in (65,504, 65,520), where hi rounds to 65,504 and hi + lo / 2048 still holds the
    value.  gamma = 0 and beta = 65,510 put exactly that into every row: with zero weights Cs is finite (zero), and only the
    prologue's split can have raised the flag."""
    H = 384
    N = 4 * H
    rows = R.make_rows("normal", T, H, 5)
    g0, b = R.make_gamma_beta(H, 6)
    W, bias0 = np.zeros((N, H), np.float32), np.zeros(N, np.float32)
    for scale, want in ((1e6, 1), (1e3, 0)):
        g = g0.copy()
        g[77] = scale
        r = run_ln_gemm(diag_lib, S.EPI_SPLIT, 0, H, T, N, g, b, W, bias0, rows=rows)
        assert np.isfinite(r["xout"]).all() and (np.abs(r["xout"]).max() > R.F16_MAX) == bool(want)
        assert r["guard"] == 0 and (r["flag"], r["in_flag"]) == (want, 0), ("gamma", scale, r["flag"])
        if not want:
            assert not r["cs"].any()
    for value, want in ((65510.0, 1), (65504.0, 0)):
        g, bb = g0.copy(), b.copy()
        g[77], bb[77] = 0.0, value
        r = run_ln_gemm(diag_lib, S.EPI_SPLIT, 0, H, T, N, g, bb, W, bias0, rows=rows)
        assert np.array_equal(r["xout"][:, 77], np.full(T, value, np.float32))
        assert np.isfinite(r["cs"]).all() and not r["cs"].any(), "the product of a value inside the hi plane's range left it"
        assert r["guard"] == 0 and (r["flag"], r["in_flag"]) == (want, 0), ("the prologue's split alone", value, r["flag"])
    for value, want in ((7e4, 1), (6e4, 0)):
        bias = bias0.copy()
        bias[N - 3] = value
        r = run_ln_gemm(diag_lib, S.EPI_GELU, 0, H, T, N, g0, b, W, bias, rows=rows)
        assert r["guard"] == 0 and (r["flag"], r["in_flag"]) == (want, 0), ("bias", value, r["flag"])
        assert np.abs(r["xout"]).max() < R.F16_MAX
        if not want:
            assert np.allclose(r["cs"][:, N - 3], value, rtol=1e-6, atol=0.0)
    bad = rows.copy()
    bad[T - 1, 5] = np.nan
    for y, want in ((bad, 1), (rows, 0)):
        r = run_ln_gemm(diag_lib, S.EPI_SPLIT, 0, H, T, N, g0, b, W, bias0, rows=y)
        assert r["guard"] == 0 and (r["flag"], r["in_flag"]) == (want, 0), ("NaN", want, r["flag"])
        assert np.isfinite(r["xout"][:T - 1]).all() and np.isnan(r["xout"][T - 1]).all() == bool(want)



# ---- a feed-forward block as the embedder chains it ----------------------------------------------------------------------

@pytest.mark.parametrize("T", [17, 130])
def test_ffn_block_chain(diag_lib, T):
    """LayerNorm + FFN-up (GELU, N = 4H), FFN-down as four K slices on its output, then the slab-sum LayerNorm in front of the
    next QKV product: every launch inside its own bound, each computed from what the launch before it produced."""
    H = 384
    y = R.make_rows("normal", T, H, 300 + T)
    g1, b1 = R.make_gamma_beta(H, 301)
    g2, b2 = R.make_gamma_beta(H, 302)
    w_up, b_up = weights(4 * H, H, S.EPI_GELU)
    w_down, _ = weights(H, 4 * H)
    b_down = weights(H, H, 3)[1]
    w_qkv, b_qkv = weights(3 * H, H, S.EPI_SPLIT)
    up = run_ln_gemm(diag_lib, S.EPI_GELU, 0, H, T, 4 * H, g1, b1, w_up, b_up, rows=y)
    r_up = settle(("FFN-up", T), up, S.prologue_ref(0, g1, b1, 1e-12, rows=y), w_up, b_up, S.EPI_GELU)
    mid = R.split_roundtrip(up["cs"])            # hi + lo / 2048 as read back: the values the next launch's split holds
    down = run_partial(diag_lib, H, T, H, mid, w_down)
    r_down = settle_partial(("FFN-down", T), down, mid, w_down, H)
    nxt = run_ln_gemm(diag_lib, S.EPI_SPLIT, 1, H, T, 3 * H, g2, b2, w_qkv, b_qkv, parts=down["parts"], parts_bias=b_down, x=up["xout"])
    stage1 = S.prologue_ref(1, g2, b2, 1e-12, parts=down["parts"], parts_bias=b_down, x=up["xout"])
    r_next = settle(("slab sum + QKV", T), nxt, stage1, w_qkv, b_qkv, S.EPI_SPLIT)
    print(f"FFN block H 384 T {T}: worst err/bound FFN-up Xout {r_up[0]:.3f} Cs {r_up[1]:.3f}, FFN-down slabs {r_down:.3f}, "
          f"slab sum Xout {r_next[0]:.3f}, QKV Cs {r_next[1]:.3f}")
