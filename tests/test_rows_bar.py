"""The bars of the row-kernel operator tests must bite (CPU only; the bars themselves: tests/rows_ref.py).

tests/test_gpu_rows.py and tests/test_gpu_attention_cls.py accept a kernel when |got - ref| <= bound.  Two things are shown
here for every operation, on the same input families the GPU tests use:
  (a) a plain float32 numpy evaluation — which is correct — stays inside the bound on every family, so the bar is not one
      that only a float64 implementation could meet;
  (b) the reference perturbed the way a kernel goes wrong leaves the bound on at least one family; the factor by which it
      leaves is printed.
Nothing a kernel returns enters a bound, so nothing here needs a GPU."""
import numpy as np
import pytest

from tests import attention_ref as A
from tests import rows_ref as R

T, H = 5, 384
EPS = (1e-12, 1e-5)


def ln_case(family, seed=3):
    v = R.make_rows(family, T, H, seed)
    g, b = R.make_gamma_beta(H, seed + 1)
    return v, g, b


def report(what, found):
    print(f"{what}: " + ", ".join(f"{k} {v:.3g}x" for k, v in found.items()))
    best = max(found.values())
    assert best > 1.0, (what, found)


# ---- (a) float32 evaluations meet the bars -------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("family", R.ROW_FAMILIES)
def test_float32_layernorm_meets_the_bar(family, eps):
    v, g, b = ln_case(family)
    ref, bound = R.layernorm_ref(v, g, b, eps)
    ratio = R.worst(R.layernorm_f32(v, g, b, eps), ref, bound)
    print(f"LayerNorm {family} eps {eps:g}: float32 numpy err/bound = {ratio:.3f}")
    assert ratio <= 1.0
    # the input as a rounded sum (layernorm_sum, embed_ln): the f32 sum in the kernel's order, then the f32 LayerNorm
    rng = np.random.default_rng(9)
    parts = [v * 0.5, v * 0.25 + rng.standard_normal(v.shape).astype(np.float32) * 0.01, rng.standard_normal(H).astype(np.float32) * 0.1, v * 0.25]
    parts = [np.broadcast_to(p, v.shape).astype(np.float32) for p in parts]
    s64, ev = R.ordered_sum(parts)
    s32 = parts[0]
    for p in parts[1:]:
        s32 = s32 + p
    ref, bound = R.layernorm_ref(s64, g, b, eps, ev=ev)
    ratio = R.worst(R.layernorm_f32(s32, g, b, eps), ref, bound)
    print(f"LayerNorm of a sum, {family} eps {eps:g}: float32 numpy err/bound = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("family", R.ROW_FAMILIES)
def test_float32_qk_layernorm_meets_the_bar(family):
    Hq = 96
    rng = np.random.default_rng(4)
    qkv = np.concatenate([R.make_rows(family, T, Hq, 5), R.make_rows(family, T, Hq, 6), R.make_rows("normal", T, Hq, 7)], axis=1)
    ln = rng.standard_normal((4, Hq)).astype(np.float32)
    for eps in EPS:
        ref, bound = R.qk_layernorm_ref(qkv, ln, eps, T, Hq)
        ratio = R.worst(R.qk_layernorm_f32(qkv, ln, eps, T, Hq), ref, bound)
        print(f"query / key LayerNorm {family} eps {eps:g}: float32 numpy err/bound = {ratio:.3f}")
        assert ratio <= 1.0
        assert np.array_equal(ref[:, 2 * Hq:], qkv[:, 2 * Hq:].astype(np.float64)) and not bound[:, 2 * Hq:].any()


def pool_case(L, B=3, seed=11):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B * L, H)) + 0.5).astype(np.float32)
    mask = np.stack([A.mask_from_lens([L], L)[0], A.mask_from_lens([max(1, L // 2)], L)[0], A.holes_mask(L, seed)])
    return x, mask, B


@pytest.mark.parametrize("L", [1, 15, 65])
def test_float32_pooling_meets_the_bar(L):
    x, mask, B = pool_case(L)
    for mean_pool in (False, True):
        ref, bound = R.pool_ref(x, mask, B, L, mean_pool)
        ratio = R.worst(R.pool_f32(x, mask, B, L, mean_pool), ref, bound)
        print(f"pooling {'mean' if mean_pool else 'CLS'} L {L}: float32 numpy err/bound = {ratio:.3f}")
        assert ratio <= 1.0


def rope_case(dh, L=7, B=3, heads=3, seed=13):
    Hh = heads * dh
    qkv = np.random.default_rng(seed).standard_normal((B * L, 3 * Hh)).astype(np.float32)
    return qkv, R.rope_table(L, dh), B * L, L, Hh, heads


@pytest.mark.parametrize("dh", [32, 64])
def test_float32_rope_meets_the_bar(dh):
    qkv, table, Tt, L, Hh, heads = rope_case(dh)
    ref, bound = R.rope_ref(qkv, table, Tt, L, Hh, heads)
    ratio = R.worst(R.rope_f32(qkv, table, Tt, L, Hh, heads), ref, bound)
    print(f"rotary map dh {dh}: float32 numpy err/bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert not bound[:, 2 * Hh:].any()


GATE_POINTS = np.array([-104, -88, -30, -8, -3, 0, 3, 30, 90], np.float32)


def gate_case(seed=17, I=96):
    rng = np.random.default_rng(seed)
    gate = (rng.standard_normal((T, I)) * 2.0).astype(np.float32)
    gate[0, :GATE_POINTS.size] = GATE_POINTS
    value = rng.standard_normal((T, I)).astype(np.float32)
    return value, gate


@pytest.mark.parametrize("gelu", [False, True])
def test_float32_gate_meets_the_bar(gelu):
    value, gate = gate_case()
    ref, bound = R.gate_ref(value, gate, gelu)
    ratio = R.worst(R.gate_f32(value, gate, gelu), ref, bound)
    print(f"gate {'erf-GELU' if gelu else 'silu'}: float32 numpy err/bound = {ratio:.3f}")
    assert ratio <= 1.0


def cls_rows(B, L):
    return np.arange(B) * L


@pytest.mark.parametrize("family", A.FAMILIES)
def test_float32_cls_attention_meets_the_bar(family):
    B, L, heads, Hh = 2, 129, 4, 128
    mask = A.mask_from_lens([L, L - 37], L)
    qkv = A.make_qkv(family, B, L, Hh, heads, 7, mask)
    ref, bound, _ = A.attention_ref(qkv, mask, B, L, Hh, heads)
    got = A.attention_f32(qkv, mask, B, L, Hh, heads)
    rows = cls_rows(B, L)
    ratio = R.worst(got[rows], ref[rows], bound[rows])
    print(f"CLS attention {family}: float32 numpy err/bound = {ratio:.3f}")
    assert ratio <= 1.0


# ---- (b) perturbed references leave the bars -----------------------------------------------------------------------------

def test_perturbed_layernorms_leave_the_bound():
    one_pass, ddof, eps_out, shifted = {}, {}, {}, {}
    for family in R.ROW_FAMILIES:
        v, g, b = ln_case(family)
        ref, bound = R.layernorm_ref(v, g, b, 1e-5)
        one_pass[family] = R.worst(R.layernorm_f32(v, g, b, 1e-5, one_pass=True), ref, bound)
        ddof[family] = R.worst(R.layernorm_ref(v, g, b, 1e-5, var_ddof=1)[0], ref, bound)
        eps_out[family] = R.worst(R.layernorm_ref(v, g, b, 1e-5, eps_outside=True)[0], ref, bound)
        shifted[family] = R.worst(R.layernorm_ref(v, np.roll(g, 2), np.roll(b, 2), 1e-5)[0], ref, bound)
    report("one-pass variance E[x^2] - mean^2 in f32", one_pass)
    report("variance over H - 1", ddof)
    report("eps added outside the square root", eps_out)
    report("gamma and beta shifted by one column pair", shifted)


def test_perturbed_embeddings_leave_the_bound():
    rng = np.random.default_rng(21)
    vocab, ntypes, B, L = 50, 2, 3, 5
    word = rng.standard_normal((vocab, H)).astype(np.float32)
    pos = rng.standard_normal((B * L, H)).astype(np.float32)       # (B * L rows, so that position t exists for the perturbation)
    types_tab = rng.standard_normal((ntypes, H)).astype(np.float32)
    ids = rng.integers(0, vocab, B * L)
    types = rng.integers(0, ntypes, B * L)
    types[3] = 2                                                     # beyond the table: clamped to its last row
    g, b = R.make_gamma_beta(H, 22)
    s, ev = R.ordered_sum(R.embed_rows(ids, word, pos, types_tab, types, L))
    ref, bound = R.layernorm_ref(s, g, b, 1e-12, ev=ev)
    p1 = R.layernorm_ref(R.ordered_sum(R.embed_rows(ids, word, pos, types_tab, types, L, t_mod=False))[0], g, b, 1e-12)[0]
    p2 = R.layernorm_ref(R.ordered_sum(R.embed_rows(ids, word, pos, types_tab, types, L, clamp_type=False))[0], g, b, 1e-12)[0]
    report("position t instead of t % L", {"embeddings": R.worst(p1, ref, bound)})
    report("type row not clamped", {"embeddings": R.worst(p2, ref, bound)})


def test_perturbed_pooling_leaves_the_bound():
    counted, dropped = {}, {}
    for L in (15, 65):
        x, mask, B = pool_case(L)
        ref, bound = R.pool_ref(x, mask, B, L, True)
        more = mask.copy()
        more[1, np.flatnonzero(mask[1] == 0)[0]] = 1                 # one masked token counted
        less = mask.copy()
        for bb in range(B):
            less[bb, np.flatnonzero(mask[bb])[-1]] = 0               # the last valid token dropped
        counted[f"L {L}"] = R.worst(R.pool_ref(x, mask, B, L, True, count_mask=more)[0], ref, bound)
        dropped[f"L {L}"] = R.worst(R.pool_ref(x, mask, B, L, True, count_mask=less)[0], ref, bound)
    report("pooled mean counting one masked token", counted)
    report("pooled mean dropping the last valid token", dropped)


def test_perturbed_rope_leaves_the_bound():
    inter, sign, tpos = {}, {}, {}
    for dh in (32, 64):
        qkv, table, Tt, L, Hh, heads = rope_case(dh)
        ref, bound = R.rope_ref(qkv, table, Tt, L, Hh, heads)
        inter[f"dh {dh}"] = R.worst(R.rope_ref(qkv, table, Tt, L, Hh, heads, interleaved=True)[0], ref, bound)
        sign[f"dh {dh}"] = R.worst(R.rope_ref(qkv, table, Tt, L, Hh, heads, sin_sign=-1.0)[0], ref, bound)
        tpos[f"dh {dh}"] = R.worst(R.rope_ref(qkv, table, Tt, L, Hh, heads, t_mod=False)[0], ref, bound)
    report("interleaved rotary pairing instead of the half split", inter)
    report("sin with the wrong sign", sign)
    report("rotary position t instead of t % L", tpos)


def test_perturbed_gates_leave_the_bound():
    value, gate = gate_case()
    swapped, tanh = {}, {}
    for gelu in (False, True):
        ref, bound = R.gate_ref(value, gate, gelu)
        swapped["erf-GELU" if gelu else "silu"] = R.worst(R.gate_ref(value, gate, gelu, swapped=True)[0], ref, bound)
    ref, bound = R.gate_ref(value, gate, True)
    tanh["erf-GELU"] = R.worst(R.gate_ref(value, gate, True, tanh_gelu=True)[0], ref, bound)
    report("value and gate swapped", swapped)
    report("tanh-GELU in place of erf-GELU", tanh)


def test_perturbed_qk_layernorm_leaves_the_bound():
    Hq = 96
    rng = np.random.default_rng(4)
    found = {}
    for family in R.ROW_FAMILIES:
        qkv = np.concatenate([R.make_rows(family, T, Hq, 5), R.make_rows(family, T, Hq, 6), R.make_rows("normal", T, Hq, 7)], axis=1)
        ln = rng.standard_normal((4, Hq)).astype(np.float32)
        ref, bound = R.qk_layernorm_ref(qkv, ln, 1e-5, T, Hq)
        found[family] = R.worst(R.qk_layernorm_ref(qkv, ln, 1e-5, T, Hq, swap_gamma=True)[0], ref, bound)
    report("the query's gamma applied to the key", found)


def test_cls_attention_missing_the_last_key_of_a_pass_leaves_the_bound():
    B, heads, Hh = 2, 4, 128     # head width 32: a pass covers 8 keys
    found = {}
    for family in A.FLAT_FAMILIES:
        for L in (9, 129):
            mask = A.mask_from_lens([L, max(8, L - 37)], L)
            qkv = A.make_qkv(family, B, L, Hh, heads, 7, mask)
            ref, bound, _ = A.attention_ref(qkv, mask, B, L, Hh, heads)
            lost = mask.copy()
            lost[:, 7] = 0                                          # key 7: the last key of the first pass
            pert, _, _ = A.attention_ref(qkv, mask, B, L, Hh, heads, key_mask=lost, want_bound=False)
            rows = cls_rows(B, L)
            found[f"{family} L {L}"] = R.worst(pert[rows], ref[rows], bound[rows])
    report("CLS attention missing the last key of a pass", found)
