"""Unit parity of the encoder's row kernels (encoder.hip: embed_ln, layernorm, layernorm_to, layernorm_sum, pool_normalize,
mean_pool_normalize) and of the element-wise kernels of nomic.hip (rotary map, feed-forward gate, query / key LayerNorm, each
in its split and its f32 form) through cs_debug_rows / cs_debug_elementwise, against float64 numpy.

References, bounds and the source of every constant: tests/rows_ref.py (module docstring).  Every comparison asserts the
range flag 0 (unless the test is about the flag), a finite output and err / bound <= 1 with no factor on the bound, and
every test prints its worst err / bound; DESIGN.md §4.0 and profiles/rows_operator_parity.log record them.
tests/test_rows_bar.py shows on the CPU that these bars bite.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

from tests import attention_ref as A
from tests import rows_ref as R

pytestmark = pytest.mark.gpu

HIDDEN = [384, 768, 1024]
LN_ROWS = [1, 3, 4, 5, 1023]     # four rows per block: partial last blocks
EPS = [1e-12, 1e-5]
POOL_CLS, POOL_MEAN = 0, 1


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, np.int32)


def run_rows(lib, which, H, T=0, L=1, B=0, eps=1e-12, pooling=POOL_CLS, ids=None, word=None, pos=None, type_table=None, types=None,
             x=None, mask=None, parts=None, bias=None, g=None, b=None, range_mode=0, want_split=True):
    """-> dict(out, split, src_after, ranges, flag)."""
    from codesearch_amd import _lib

    f32p, i32p = _lib.f32p, _lib.i32p
    ids, types, mask = _i32(ids), _i32(types), _i32(mask)
    word, pos, type_table, x, parts, bias, g, b = (_f32(a) for a in (word, pos, type_table, x, parts, bias, g, b))
    rows = B if which == 2 else T
    out = np.full((rows, H), np.nan, np.float32)
    split = np.full((rows, H), np.nan, np.float32) if (want_split and which != 2) else None
    src_after = np.full((T, H), np.nan, np.float32) if which == 4 else None
    ranges = None
    if range_mode:
        ranges = np.full((T if range_mode == 2 else (T + 3) // 4, 2), np.nan, np.float32)
    flag = C.c_uint32(0)
    _lib.check_diag(lib.cs_debug_rows(
        0, which, H, T, L, B, eps, pooling, _ptr(ids, i32p), _ptr(word, f32p), _ptr(pos, f32p), _ptr(type_table, f32p),
        _ptr(types, i32p), 0 if type_table is None else type_table.shape[0], 0 if word is None else word.shape[0],
        _ptr(x, f32p), _ptr(mask, i32p), _ptr(parts, f32p), 0 if parts is None else parts.shape[0], _ptr(bias, f32p),
        _ptr(g, f32p), _ptr(b, f32p), range_mode, _ptr(out, f32p), _ptr(split, f32p), _ptr(src_after, f32p), _ptr(ranges, f32p),
        C.byref(flag)))
    return dict(out=out, split=split, src_after=src_after, ranges=ranges, flag=int(flag.value))


def run_elementwise(lib, op, split, T, a, b=None, table=None, L=1, H=0, heads=1, I=0, gelu=False, eps=1e-12):
    """-> (out, kernel flag, input-split flag)."""
    from codesearch_amd import _lib

    f32p = _lib.f32p
    a, b, table = _f32(a), _f32(b), _f32(table)
    out = np.full((T, I if op == 1 else 3 * H), np.nan, np.float32)
    flags = (C.c_uint32 * 2)(0, 0)
    _lib.check_diag(lib.cs_debug_elementwise(0, op, int(split), T, L, H, heads, I, int(gelu), eps, _ptr(a, f32p), _ptr(b, f32p),
                                             _ptr(table, f32p), _ptr(out, f32p), flags))
    return out, int(flags[0]), int(flags[1])


def settle(what, r, ref, bound):
    """The shared checks of one LayerNorm-family launch: flag 0, finite, f32 rows inside the bound, the split form equal to
    the f32 rows within the format's 2^-22 (2^-36 under 2^-14).  Returns err / bound of the f32 rows."""
    assert r["flag"] == 0, what
    assert np.isfinite(r["out"]).all() and np.isfinite(r["split"]).all(), what
    ratio = R.worst(r["out"], ref, bound)
    assert ratio <= 1.0, (what, ratio)
    out64 = r["out"].astype(np.float64)
    sratio = R.worst(r["split"], out64, R.split_bound(out64))
    assert sratio <= 1.0, (what, "split form", sratio)
    return ratio


# ---- LayerNorm kernels (which = 1, 3, 4) ----------------------------------------------------------------------------------

BIAS_SCALE = {"normal": 0.1, "offset": 0.001, "outlier": 0.1, "tiny": 1e-21}


def sum_inputs(family, T, H, nparts, seed):
    """Slabs, bias and residual whose sum has the family's character (constant rows: every term constant along the row)."""
    rng = np.random.default_rng(seed)
    n = nparts + 1
    terms = [R.make_rows(family, T, H, seed + 7 * s) / np.float32(n) for s in range(n)]
    bias = np.full(H, 0.25, np.float32) if family == "constant" else (rng.standard_normal(H) * BIAS_SCALE[family]).astype(np.float32)
    return np.stack(terms[:nparts]), bias, terms[nparts]


def ln_launch(lib, which, H, T, eps, g, b, v=None, parts=None, bias=None, resid=None, **kw):
    """-> (result, ref, bound) of one launch of kernel 1, 3 or 4."""
    if which == 3:
        r = run_rows(lib, 3, H, T=T, eps=eps, x=resid, parts=parts, bias=bias, g=g, b=b, **kw)
        s, ev = R.ordered_sum(list(parts) + [np.broadcast_to(bias, resid.shape), resid])
        ref, bound = R.layernorm_ref(s, g, b, eps, ev=ev)
    else:
        r = run_rows(lib, which, H, T=T, eps=eps, x=v, g=g, b=b, **kw)
        ref, bound = R.layernorm_ref(v, g, b, eps)
        if which == 4:
            assert np.array_equal(r["src_after"].view(np.uint32), v.view(np.uint32)), "layernorm_to changed its source"
    return r, ref, bound


@pytest.mark.parametrize("H", HIDDEN)
@pytest.mark.parametrize("which", [1, 3, 4])
def test_layernorm_kernels_against_float64(diag_lib, which, H):
    g, b = R.make_gamma_beta(H, H + which)
    worst = {}
    for T in LN_ROWS:
        for fi, family in enumerate(R.ROW_FAMILIES):
            for eps in EPS:
                seed = 1000 * which + 10 * T + fi
                if which != 3:
                    v = R.make_rows(family, T, H, seed)
                    r, ref, bound = ln_launch(diag_lib, which, H, T, eps, g, b, v=v)
                    ratio = settle((which, H, T, family, eps), r, ref, bound)
                    worst[family] = max(worst.get(family, 0.0), ratio)
                    continue
                for nparts in ((1, 2, 4) if T <= 5 else ((1, 2, 4)[fi % 3],)):
                    parts, bias, resid = sum_inputs(family, T, H, nparts, seed)
                    r, ref, bound = ln_launch(diag_lib, 3, H, T, eps, g, b, parts=parts, bias=bias, resid=resid)
                    ratio = settle((which, H, T, family, eps, nparts), r, ref, bound)
                    worst[family] = max(worst.get(family, 0.0), ratio)
    name = {1: "layernorm", 3: "layernorm_sum", 4: "layernorm_to"}[which]
    print(f"{name} H {H}: worst err/bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def exact_inputs(which, H, T, v):
    """The inputs that make kernel `which` normalise exactly the rows v (v's entries are sums of two equal halves)."""
    if which == 3:
        half = (v * np.float32(0.5)).astype(np.float32)
        return dict(parts=np.stack([half * np.float32(0.5), half * np.float32(0.5)]), bias=np.zeros(H, np.float32), resid=half)
    return dict(v=v)


@pytest.mark.parametrize("H", HIDDEN)
@pytest.mark.parametrize("which", [1, 3, 4])
def test_layernorm_exact_cases_catch_mapping_slips(diag_lib, which, H):
    """gamma = 0, beta = the column index: the output is beta, bit for bit.  Rows of alternating +-1 with eps = 0: the mean
    is 0, the variance 1 (H times rn(1 / H) rounds to 1 for 384, 768 and 1024) and the output rn(+-g + b), bit for bit."""
    T = 5
    cols = np.arange(H, dtype=np.float32)
    v = R.make_rows("normal", T, H, 77 + H)
    r, _, _ = ln_launch(diag_lib, which, H, T, 1e-12, np.zeros(H, np.float32), cols, **exact_inputs(which, H, T, v))
    assert r["flag"] == 0 and np.array_equal(r["out"], np.broadcast_to(cols, (T, H))) and np.array_equal(r["split"], r["out"])
    g, b = R.make_gamma_beta(H, 5 + H)
    pm = np.where((np.arange(H)[None, :] + np.arange(T)[:, None]) % 2 == 0, 1.0, -1.0).astype(np.float32)
    r, _, _ = ln_launch(diag_lib, which, H, T, 0.0, g, b, **exact_inputs(which, H, T, pm))
    expect = pm * g[None, :] + b[None, :]
    assert r["flag"] == 0 and np.array_equal(r["out"].view(np.uint32), expect.astype(np.float32).view(np.uint32))
    print(f"exact cases, kernel {which} H {H}: bit for bit")


@pytest.mark.parametrize("which", [0, 1, 3, 4])
def test_layernorm_range_flag(diag_lib, which):
    """A gamma that pushes an output past 65,504 raises the flag of the split store; the same data scaled into range does not."""
    H, T = 384, 5
    v = R.make_rows("normal", T, H, 3)
    _, b = R.make_gamma_beta(H, 4)
    for gscale, want in ((1e5, 1), (1e3, 0)):
        g = np.full(H, gscale, np.float32)
        if which == 0:
            r = run_rows(diag_lib, 0, H, T=T, L=T, ids=np.arange(T), word=v, type_table=np.zeros((1, H), np.float32), g=g, b=b)
        else:
            r, _, _ = ln_launch(diag_lib, which, H, T, 1e-12, g, b, **exact_inputs(which, H, T, v))
        assert np.isfinite(r["out"]).all() and (np.abs(r["out"]).max() > R.F16_MAX) == bool(want)
        assert r["flag"] == want, (which, gscale, r["flag"])


@pytest.mark.parametrize("H", HIDDEN)
@pytest.mark.parametrize("which", [0, 1])
def test_range_pairs_equal_the_rows_extremes_exactly(diag_lib, which, H):
    """range_out, per block of four rows and per row: the min / max of the returned f32 rows with zero included, exactly;
    rows at or beyond T add nothing but the zero."""
    g, b = R.make_gamma_beta(H, 9)
    for T in (1, 5, 1023):
        v = R.make_rows("normal", T, H, 30 + T)
        v[0] = np.abs(v[0]) + 1.0           # a row whose normalised values ...
        gg, bb = g, b
        if T == 5:
            gg, bb = np.abs(g), np.full(H, 8.0, np.float32)   # ... here all stay positive: the pair's lo is the included zero
        for mode in (1, 2):
            if which == 0:
                r = run_rows(diag_lib, 0, H, T=T, L=T, ids=np.arange(T), word=v, type_table=np.zeros((1, H), np.float32), g=gg, b=bb,
                             range_mode=mode)
            else:
                r = run_rows(diag_lib, 1, H, T=T, x=v, g=gg, b=bb, range_mode=mode)
            out, pairs = r["out"], r["ranges"]
            assert r["flag"] == 0 and np.isfinite(pairs).all()
            if mode == 2:
                lo, hi = np.minimum(out.min(axis=1), 0), np.maximum(out.max(axis=1), 0)
            else:
                pad = np.zeros(((T + 3) // 4 * 4, H), np.float32)
                pad[:T] = out
                blocks = pad.reshape(-1, 4 * H)
                lo, hi = np.minimum(blocks.min(axis=1), 0), np.maximum(blocks.max(axis=1), 0)
            assert np.array_equal(pairs[:, 0], lo) and np.array_equal(pairs[:, 1], hi), (which, H, T, mode)
            if T == 5:
                assert (pairs[:, 0] == 0).all()
    print(f"range pairs, kernel {which} H {H}: exact in both modes")


# ---- embed_ln (which = 0) -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", HIDDEN)
@pytest.mark.parametrize("L", [1, 5, 33])
def test_embed_ln_against_float64(diag_lib, H, L):
    B, vocab, ntypes = 3, 40, 2
    T = B * L
    rng = np.random.default_rng(H + L)
    word = rng.standard_normal((vocab, H)).astype(np.float32)
    pos = rng.standard_normal((L, H)).astype(np.float32)
    tab = rng.standard_normal((ntypes, H)).astype(np.float32)
    ids = rng.integers(0, vocab, T)
    ids[0], ids[T - 1], ids[T // 2] = 0, vocab - 1, vocab + 3      # the table's ends, and an id outside it: row 0
    types = rng.integers(0, ntypes, T)
    types[T - 1] = ntypes + 1                                       # beyond the table: its last row
    g, b = R.make_gamma_beta(H, 12)
    worst = 0.0
    for use_pos in (False, True):
        for ty, table in ((None, tab[:1]), (None, tab), (types, tab)):   # (no type ids: row 0, also of a two-row table)
            p = pos if use_pos else None
            r = run_rows(diag_lib, 0, H, T=T, L=L, ids=ids, word=word, pos=p, type_table=table, types=ty, g=g, b=b)
            s, ev = R.ordered_sum(R.embed_rows(ids, word, p, table, ty, L))   # (word + type) + position
            ref, bound = R.layernorm_ref(s, g, b, 1e-12, ev=ev)
            worst = max(worst, settle(("embed_ln", H, L, use_pos, ty is not None), r, ref, bound))
    # bit for bit: gamma = 0, beta = the column index; rows of +-1 from the word table alone with eps = 0
    cols = np.arange(H, dtype=np.float32)
    r = run_rows(diag_lib, 0, H, T=T, L=L, ids=ids, word=word, pos=pos, type_table=tab, types=types, g=np.zeros(H, np.float32), b=cols)
    assert r["flag"] == 0 and np.array_equal(r["out"], np.broadcast_to(cols, (T, H)))
    pm = np.where((np.arange(H)[None, :] + np.arange(vocab)[:, None]) % 2 == 0, 1.0, -1.0).astype(np.float32)
    r = run_rows(diag_lib, 0, H, T=T, L=L, eps=0.0, ids=ids, word=pm, type_table=np.zeros((1, H), np.float32), g=g, b=b)
    rows = pm[np.where(ids >= vocab, 0, ids)]
    assert np.array_equal(r["out"].view(np.uint32), (rows * g[None, :] + b[None, :]).astype(np.float32).view(np.uint32))
    print(f"embed_ln H {H} L {L}: worst err/bound = {worst:.3f}")


# ---- pooling --------------------------------------------------------------------------------------------------------------

def pool_masks(B, L, shift, seed):
    """B rows cycling through: full, one valid token, interior holes, all zero — starting at kind `shift`."""
    kinds = [A.mask_from_lens([L], L)[0], A.mask_from_lens([1], L)[0], A.holes_mask(L, seed), np.zeros(L, np.int32)]
    return np.stack([kinds[(shift + i) % 4] for i in range(B)])


@pytest.mark.parametrize("L", [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 512])   # the kernels switch at 16; 64 per wave, 256 per round
@pytest.mark.parametrize("H", HIDDEN)
def test_pooling_against_float64(diag_lib, H, L):
    worst = {POOL_CLS: 0.0, POOL_MEAN: 0.0}
    for B in (1, 3, 5):
        x = (np.random.default_rng(H + 7 * L + B).standard_normal((B * L, H)) + 0.5).astype(np.float32)
        for shift in range(4):
            mask = pool_masks(B, L, shift, L + shift)
            for pooling in (POOL_CLS, POOL_MEAN):
                r = run_rows(diag_lib, 2, H, L=L, B=B, pooling=pooling, x=x, mask=mask)
                ref, bound = R.pool_ref(x, mask, B, L, pooling == POOL_MEAN)
                what = (H, L, B, shift, pooling)
                assert r["flag"] == 0 and np.isfinite(r["out"]).all(), what
                ratio = R.worst(r["out"], ref, bound)
                assert ratio <= 1.0, (what, ratio)
                worst[pooling] = max(worst[pooling], ratio)
                # rows that pool something have norm 1 within the bound; an all-zero mask gives a zero row under mean pooling
                live = (mask != 0).any(axis=1) | (pooling == POOL_CLS)
                norm = np.linalg.norm(r["out"].astype(np.float64), axis=1)
                ref_norm = np.linalg.norm(ref, axis=1)
                assert (np.abs(norm - ref_norm) <= np.linalg.norm(bound, axis=1))[live].all(), what
                assert (np.abs(ref_norm - 1.0) <= 1e-11)[live].all(), what
                assert not r["out"][~live].any(), what
    print(f"pooling H {H} L {L}: worst err/bound CLS {worst[POOL_CLS]:.3f}, mean {worst[POOL_MEAN]:.3f}")


@pytest.mark.parametrize("L", [15, 64])
def test_an_all_zero_mask_pools_to_zero_and_leaves_the_other_rows_their_bits(diag_lib, L):
    H, B = 384, 3
    x = np.random.default_rng(L).standard_normal((B * L, H)).astype(np.float32)
    full, holes = A.mask_from_lens([L], L)[0], A.holes_mask(L, 2)
    a = run_rows(diag_lib, 2, H, L=L, B=B, pooling=POOL_MEAN, x=x, mask=np.stack([full, np.zeros(L, np.int32), holes]))["out"]
    c = run_rows(diag_lib, 2, H, L=L, B=B, pooling=POOL_MEAN, x=x, mask=np.stack([full, full, holes]))["out"]
    assert np.isfinite(a).all() and not a[1].any() and c[1].any()
    assert np.array_equal(a[[0, 2]].view(np.uint32), c[[0, 2]].view(np.uint32))


# ---- rotary map -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("heads", [3, 12])
@pytest.mark.parametrize("dh", [32, 64])
def test_rope_against_float64(diag_lib, dh, heads, split):
    H, B = heads * dh, 3
    worst = 0.0
    for L in (1, 7, 64):
        T = B * L
        qkv = np.random.default_rng(dh + heads + L).standard_normal((T, 3 * H)).astype(np.float32)
        if split:
            qkv = R.split_roundtrip(qkv)
        table = R.rope_table(L, dh)          # L rows of distinct angles
        got, flag, in_flag = run_elementwise(diag_lib, 0, split, T, qkv, table=table, L=L, H=H, heads=heads)
        ref, bound = R.rope_ref(qkv, table, T, L, H, heads)
        if split:
            bound[:, :2 * H] += R.split_bound(ref[:, :2 * H])
        assert flag == 0 and in_flag == 0 and np.isfinite(got).all()
        ratio = R.worst(got[:, :2 * H], ref[:, :2 * H], bound[:, :2 * H])
        assert ratio <= 1.0, (dh, heads, split, L, ratio)
        assert np.array_equal(got[:, 2 * H:].view(np.uint32), qkv[:, 2 * H:].view(np.uint32)), "the rotary map touched V"
        worst = max(worst, ratio)
    print(f"rotary map {'split' if split else 'f32'} dh {dh} heads {heads}: worst err/bound = {worst:.3f}")


def test_rope_range_flag(diag_lib):
    """x1 = x2 = 50,000 turned by 45 degrees: x2 cos + x1 sin = 70,711 leaves the f16 range; a tenth of it does not."""
    dh, heads, L = 32, 3, 2
    H, T = heads * dh, 2
    table = np.empty((L, dh // 2, 2), np.float32)
    table[...] = np.float32(np.sqrt(0.5))
    for value, want in ((50000.0, 1), (5000.0, 0)):
        qkv = np.zeros((T, 3 * H), np.float32)
        qkv[1, H + dh + 3] = qkv[1, H + dh + dh // 2 + 3] = value        # K, head 1, pair 3
        got, flag, in_flag = run_elementwise(diag_lib, 0, True, T, qkv, table=table, L=L, H=H, heads=heads)
        assert (flag, in_flag) == (want, 0), (value, flag, in_flag)


# ---- feed-forward gate ----------------------------------------------------------------------------------------------------

GATE_POINTS = np.array([-104, -88, -30, -8, -3, 0, 3, 30, 90], np.float32)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("gelu", [False, True])
def test_gate_against_float64(diag_lib, gelu, split):
    worst = 0.0
    for T in (1, 5, 257):
        for I in (32, 96, 1536):
            rng = np.random.default_rng(T + I)
            gate = (rng.standard_normal((T, I)) * 2.0).astype(np.float32)
            gate[0, :GATE_POINTS.size] = GATE_POINTS
            value = rng.standard_normal((T, I)).astype(np.float32)      # both signs
            if split:
                value, gate = R.split_roundtrip(value), R.split_roundtrip(gate)
                got, flag, in_flag = run_elementwise(diag_lib, 1, True, T, R.pack_gate_input(value, gate), I=I, gelu=gelu)
            else:
                got, flag, in_flag = run_elementwise(diag_lib, 1, False, T, value, b=gate, I=I, gelu=gelu)
            ref, bound = R.gate_ref(value, gate, gelu)
            if split:
                bound = bound + R.split_bound(ref)
            assert flag == 0 and in_flag == 0 and np.isfinite(got).all()
            ratio = R.worst(got, ref, bound)
            assert ratio <= 1.0, (gelu, split, T, I, ratio)
            worst = max(worst, ratio)
    print(f"gate {'erf-GELU' if gelu else 'silu'} {'split' if split else 'f32'}: worst err/bound = {worst:.3f}")


@pytest.mark.parametrize("gelu", [False, True])
def test_gate_range_flag(diag_lib, gelu):
    """60,000 x act(3) = 171,000 (silu) / 179,000 (erf-GELU) leaves the f16 range; 6,000 x act(3) does not."""
    T, I = 2, 32
    for v, want in ((60000.0, 1), (6000.0, 0)):
        value, gate = np.ones((T, I), np.float32), np.full((T, I), 3.0, np.float32)
        value[1, 17] = v
        got, flag, in_flag = run_elementwise(diag_lib, 1, True, T, R.pack_gate_input(value, gate), I=I, gelu=gelu)
        assert (flag, in_flag) == (want, 0), (gelu, v, flag, in_flag)


# ---- query / key LayerNorm ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("H", [96, 384, 768, 1024])    # 96, 384, 768: the c < H guards of a width that is no multiple of 512
def test_qk_layernorm_against_float64(diag_lib, H, split):
    rng = np.random.default_rng(H)
    ln = np.stack([R.make_gamma_beta(H, 1)[0], R.make_gamma_beta(H, 2)[1], R.make_gamma_beta(H, 3)[0] * 0.7, R.make_gamma_beta(H, 4)[1] - 0.2]).astype(np.float32)
    assert len({ln[i].tobytes() for i in range(4)}) == 4
    worst = {}
    for T in (1, 2, 3, 7):
        for fi, family in enumerate(R.ROW_FAMILIES):
            qkv = np.concatenate([R.make_rows(family, T, H, 10 * T + fi), R.make_rows(family, T, H, 10 * T + fi + 100),
                                  rng.standard_normal((T, H)).astype(np.float32)], axis=1)
            if split:
                qkv = R.split_roundtrip(qkv)
            for eps in EPS:
                got, flag, in_flag = run_elementwise(diag_lib, 2, split, T, qkv, table=ln, H=H, eps=eps)
                ref, bound = R.qk_layernorm_ref(qkv, ln, eps, T, H)
                if split:
                    bound[:, :2 * H] += R.split_bound(ref[:, :2 * H])
                assert flag == 0 and in_flag == 0 and np.isfinite(got).all()
                ratio = R.worst(got[:, :2 * H], ref[:, :2 * H], bound[:, :2 * H])
                assert ratio <= 1.0, (H, split, T, family, eps, ratio)
                assert np.array_equal(got[:, 2 * H:].view(np.uint32), qkv[:, 2 * H:].view(np.uint32)), "the query / key LayerNorm touched V"
                worst[family] = max(worst.get(family, 0.0), ratio)
    print(f"query / key LayerNorm {'split' if split else 'f32'} H {H}: worst err/bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("H", [1056, 100])
def test_qk_layernorm_refuses_widths_it_is_not_built_for(diag_lib, H, split):
    from codesearch_amd import _lib

    T = 2
    qkv = np.zeros((T, 3 * H), np.float32)
    with pytest.raises(_lib.CsError) as e:
        run_elementwise(diag_lib, 2, split, T, qkv, table=np.ones((4, H), np.float32), H=H)
    assert e.value.code == _lib.CS_ERR_UNSUPPORTED and f"query / key LayerNorm: hidden size {H} not supported" in str(e.value)
