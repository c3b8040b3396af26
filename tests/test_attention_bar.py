"""The attention operator test's bar must bite (CPU only; the bar itself: tests/attention_ref.py).

tests/test_gpu_attention.py accepts the kernel when |got - ref| <= bound.  Here the REFERENCE is perturbed the way a kernel
goes wrong — a key lost or gained at an edge, a window off by one, slopes of two heads exchanged, the mask off by one, the
scale of the other head width — and the perturbed output must leave the bound by at least 100 x on some valid row, for
every flat-score family.  The peaky families (wide, ramp, dominant) are left out on purpose: where one key carries all of
the probability, a dropped or added far key can carry none, and no bar that a correct kernel passes could notice it.

The other direction: a plain float32 numpy evaluation of the operator, which is correct, must stay inside the bound on every
family — so the bar is not one that only a float64 implementation could meet."""
import numpy as np
import pytest

from tests import attention_ref as R

B, HEADS, H = 2, 4, 128   # head width 32 (the perturbed scale is that of width 64)
BITE = 100.0


def case(family, L, seed=7):
    lens = [L, L - 37]                     # a full row and a ragged one (its last valid key is an interior position)
    mask = R.mask_from_lens(lens, L)
    return R.make_qkv(family, B, L, H, HEADS, seed, mask), mask, lens


def bite(qkv, mask, L, ref_kw, pert_kw):
    ref, bound, valid = R.attention_ref(qkv, mask, B, L, H, HEADS, **ref_kw)
    pert, _, _ = R.attention_ref(qkv, mask, B, L, H, HEADS, want_bound=False, **pert_kw)
    return R.worst_ratio(pert, ref, bound, valid)


@pytest.mark.parametrize("L", [129, 300])
@pytest.mark.parametrize("family", R.FLAT_FAMILIES)
def test_perturbed_references_leave_the_bound(family, L):
    qkv, mask, lens = case(family, L)
    dropped = mask.copy()
    for b, n in enumerate(lens):
        dropped[b, n - 1] = 0                                  # last valid key dropped
    shifted = np.roll(mask, 1, axis=1)                          # mask shifted by one: key 0 lost (full row: key L - 1 wraps in)
    shifted[:, 0] = 0
    jina = R.jina_slopes(HEADS)
    swapped = jina.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    w = 16
    found = {
        "last valid key dropped": bite(qkv, mask, L, {}, {"key_mask": dropped}),
        "mask shifted by one": bite(qkv, mask, L, {}, {"key_mask": shifted}),
        "scale of the other head width": bite(qkv, mask, L, {}, {"scale_dh": 64}),
        "window widened by one": bite(qkv, mask, L, {"window": w}, {"window": w + 1}),
        "window narrowed by one": bite(qkv, mask, L, {"window": w}, {"window": w - 1}),
        "last valid key dropped, window": bite(qkv, mask, L, {"window": w}, {"window": w, "key_mask": dropped}),
        "slopes of two heads swapped": bite(qkv, mask, L, {"slopes": jina}, {"slopes": swapped}),
        "last valid key dropped, ALiBi": bite(qkv, mask, L, {"slopes": jina}, {"slopes": jina, "key_mask": dropped}),
    }
    print(f"{family} L={L}: " + ", ".join(f"{k} {v:.3g}x" for k, v in found.items()))
    for what, ratio in found.items():
        assert ratio >= BITE, (family, L, what, ratio)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_a_float32_evaluation_meets_the_bar(family):
    L = 129
    qkv, mask, _ = case(family, L)
    for kw in ({}, {"window": 16}, {"slopes": R.geometric_slopes(HEADS)}):
        ref, bound, valid = R.attention_ref(qkv, mask, B, L, H, HEADS, **kw)
        got = R.attention_f32(qkv, mask, B, L, H, HEADS, **kw)
        ratio = R.worst_ratio(got, ref, bound, valid)
        print(f"{family} {kw and list(kw)[0] or 'plain'}: float32 numpy err/bound = {ratio:.3f}")
        assert ratio <= 1.0, (family, kw, ratio)
