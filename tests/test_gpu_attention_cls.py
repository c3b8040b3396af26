"""Unit parity of the CLS tail's kernels (cls_tail.hip: attention_cls_kernel, gather_cls_kernel) through
cs_debug_attention_cls, and of the exact-f32 attention kernels (encoder.hip: attention_kernel<false>, attention64_kernel)
through cs_debug_attention_f32, against the float64 attention of tests/attention_ref.py — reference and bound unchanged.

The CLS attention answers one query per sequence, row b * L; only those rows are compared.  Its inputs are first passed
through the split form's round trip (tests/rows_ref.py split_roundtrip), so that the kernel reads exactly the values the
reference takes as exact.  The f32 kernels go through the `check` function of tests/test_gpu_attention.py itself, handed
an object whose cs_debug_attention is cs_debug_attention_f32.  Every test prints its worst err / bound; DESIGN.md §4.0 and
profiles/rows_operator_parity.log record them.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

from tests import attention_ref as A
from tests import rows_ref as R
from tests import test_gpu_attention as TA

pytestmark = pytest.mark.gpu

CLS_LAYOUTS = [(4, 32), (12, 32), (3, 32), (2, 64)]
# a pass covers 8 keys (head width 32) or 4 (64), an iteration four passes: lengths around 8, 16, 32 and their multiples
CLS_LENGTHS = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 129, 257, 511, 512]


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def run_cls(lib, qkv, mask, B, L, H, heads):
    """-> (out [B, H], the kernel's flag, the input split's flag)."""
    from codesearch_amd import _lib

    qkv = np.ascontiguousarray(qkv, np.float32)
    mask = np.ascontiguousarray(mask, np.int32)
    assert qkv.shape == (B * L, 3 * H) and mask.size == B * L
    out = np.full((B, H), np.nan, np.float32)
    flags = (C.c_uint32 * 2)(0, 0)
    _lib.check_diag(lib.cs_debug_attention_cls(0, _ptr(qkv, _lib.f32p), _ptr(mask, _lib.i32p), B, L, H, heads, _ptr(out, _lib.f32p), flags,
                                               None, None, None))
    return out, int(flags[0]), int(flags[1])


def check_cls(lib, what, qkv, mask, B, L, H, heads):
    got, flag, in_flag = run_cls(lib, qkv, mask, B, L, H, heads)
    ref, bound, valid = A.attention_ref(qkv, mask, B, L, H, heads)
    rows = np.arange(B) * L
    assert valid[rows].all()
    ratio = R.worst(got, ref[rows], bound[rows])
    print(f"CLS attention {what}: heads {heads} x {H // heads}, B {B}, L {L}: flags {flag} {in_flag}, "
          f"finite {bool(np.isfinite(got).all())}, worst err/bound = {ratio:.3f}")
    assert flag == 0 and in_flag == 0, what
    assert np.isfinite(got).all(), what
    assert ratio <= 1.0, (what, ratio)
    return ratio


@pytest.mark.parametrize("L", CLS_LENGTHS)
@pytest.mark.parametrize("heads,dh", CLS_LAYOUTS)
def test_cls_attention_shapes_and_masks_against_float64(diag_lib, heads, dh, L):
    H, B = heads * dh, 3
    for i, mask in enumerate(TA.lens_mask_sets(L, 100 + L)):
        qkv = R.split_roundtrip(A.make_qkv("unit", B, L, H, heads, 1000 * heads + 10 * L + i))
        check_cls(diag_lib, f"shapes[{'ab'[i]}]", qkv, mask, B, L, H, heads)


@pytest.mark.parametrize("L", [129, 512])
@pytest.mark.parametrize("heads,dh", [(4, 32), (2, 64)])
@pytest.mark.parametrize("family", A.FAMILIES)
def test_cls_attention_score_families_against_float64(diag_lib, family, heads, dh, L):
    H, B = heads * dh, 3
    mask = np.stack([A.mask_from_lens([L], L)[0], A.mask_from_lens([A.tile_end(L) // 2 + 1], L)[0], A.holes_mask(L, 5 + L)])
    qkv = R.split_roundtrip(A.make_qkv(family, B, L, H, heads, 77 + L + heads, mask))
    check_cls(diag_lib, family, qkv, mask, B, L, H, heads)


@pytest.mark.parametrize("heads,dh", [(4, 32), (2, 64)])
def test_cls_attention_range_flag_follows_the_mask(diag_lib, heads, dh):
    """One |v| > 65,504 (infinite in the split form) on a valid key raises the kernel's flag; on a masked key it does not, and
    the output stays finite and inside the bound: a key of probability 0 is left out of P V, not multiplied by 0."""
    B, L = 2, 41
    H = heads * dh
    qkv = R.split_roundtrip(A.make_qkv("unit", B, L, H, heads, 9))
    mask = A.mask_from_lens([L, 30], L)
    assert run_cls(diag_lib, qkv, mask, B, L, H, heads)[1:] == (0, 0)
    on_valid = qkv.copy()
    on_valid[L + 3, 2 * H + 17] = 70000.0      # V of a valid key of the second sequence
    assert run_cls(diag_lib, on_valid, mask, B, L, H, heads)[1:] == (1, 1)
    on_masked = qkv.copy()
    on_masked[L + 35, 2 * H + 17] = 70000.0    # V of a masked key of the second sequence
    got, flag, in_flag = run_cls(diag_lib, on_masked, mask, B, L, H, heads)
    assert (flag, in_flag) == (0, 1) and np.isfinite(got).all()
    ref, bound, _ = A.attention_ref(qkv, mask, B, L, H, heads)
    rows = np.arange(B) * L
    assert R.worst(got, ref[rows], bound[rows]) <= 1.0


def test_cls_attention_of_a_sequence_masked_entirely_is_finite_and_leaves_the_others_alone(diag_lib):
    for heads, dh, L in ((4, 32, 33), (12, 32, 129), (2, 64, 129)):
        H = heads * dh
        qkv = R.split_roundtrip(A.make_qkv("unit", 3, L, H, heads, 31 + L))
        mask = np.stack([A.mask_from_lens([L], L)[0], np.zeros(L, np.int32), A.holes_mask(L, 3)])
        got3, flag3, _ = run_cls(diag_lib, qkv, mask, 3, L, H, heads)
        keep = np.r_[0:L, 2 * L:3 * L]
        got2, flag2, _ = run_cls(diag_lib, qkv[keep], mask[[0, 2]], 2, L, H, heads)
        assert flag3 == 0 and flag2 == 0
        assert np.isfinite(got3).all()
        assert np.array_equal(got3[[0, 2]].view(np.uint32), got2.view(np.uint32))
        ref, bound, _ = A.attention_ref(qkv, mask, 3, L, H, heads)
        assert R.worst(got3[[0, 2]], ref[[0, 2 * L]], bound[[0, 2 * L]]) <= 1.0


def test_cls_attention_refusals(diag_lib):
    from codesearch_amd import _lib

    heads, dh, B = 4, 32, 2
    H = heads * dh
    with pytest.raises(_lib.CsError) as e:      # L = 0
        run_cls(diag_lib, np.zeros((0, 3 * H), np.float32), np.zeros(0, np.int32), B, 0, H, heads)
    assert e.value.code == _lib.CS_ERR_BAD_ARG
    L = 513
    with pytest.raises(_lib.CsError) as e:      # the launcher's own refusal: p_s holds 512 scores
        run_cls(diag_lib, np.zeros((B * L, 3 * H), np.float32), np.ones(B * L, np.int32), B, L, H, heads)
    assert e.value.code == _lib.CS_ERR_UNSUPPORTED and "CLS attention" in str(e.value) and "513" in str(e.value)
    with pytest.raises(_lib.CsError) as e:      # head width 16
        run_cls(diag_lib, np.zeros((B * 8, 3 * H), np.float32), np.ones(B * 8, np.int32), B, 8, H, 8)
    assert e.value.code == _lib.CS_ERR_UNSUPPORTED


@pytest.mark.parametrize("L", [1, 40])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("H", [384, 1024])
def test_gather_cls_copies_the_cls_rows_exactly(diag_lib, H, B, L):
    from codesearch_amd import _lib

    x = R.split_roundtrip(np.random.default_rng(H + B + L).standard_normal((B * L, H)).astype(np.float32) * 3.0)
    x_cls = np.full((B, H), np.nan, np.float32)
    xs_cls = np.zeros((B, H // 32, 64), np.uint16)
    flags = (C.c_uint32 * 2)(0, 0)
    _lib.check_diag(diag_lib.cs_debug_attention_cls(0, None, None, B, L, H, 1, None, flags, _ptr(x, _lib.f32p), _ptr(x_cls, _lib.f32p),
                                                    _ptr(xs_cls, C.POINTER(C.c_uint16))))
    rows = x[np.arange(B) * L]
    assert (flags[0], flags[1]) == (0, 0)
    assert np.array_equal(x_cls.view(np.uint32), rows.view(np.uint32))      # hi + lo / 2048 of row b * L
    assert np.array_equal(xs_cls, R.split_lines(rows))                       # the source lines' bytes


# ---- the exact-f32 attention kernels --------------------------------------------------------------------------------------

class F32Attention:
    """Stands in for the diagnostic library in tests/test_gpu_attention.py's run_attention / check: its cs_debug_attention
    is cs_debug_attention_f32 (no units, pairs or projection; the range flag stays 0 — the f32 kernels have none)."""

    def __init__(self, lib):
        self.lib = lib

    def cs_debug_attention(self, device, qkv, mask, B, L, H, heads, slopes, window, seq_unit, unit_len, units, w, b, r, out, pairs, cap,
                           npairs, flag):
        assert seq_unit is None and unit_len is None and w is None and pairs is None
        return self.lib.cs_debug_attention_f32(device, qkv, mask, B, L, H, heads, slopes, window, out)


@pytest.fixture
def f32_attention(diag_lib):
    return F32Attention(diag_lib)


@pytest.mark.parametrize("L", [1, 32, 33, 128, 129, 512])
@pytest.mark.parametrize("heads,dh", TA.LAYOUTS)
def test_f32_attention_shapes_and_masks_against_float64(f32_attention, heads, dh, L):
    H, B = heads * dh, 3
    for i, mask in enumerate(TA.lens_mask_sets(L, 100 + L)):
        qkv = A.make_qkv("unit", B, L, H, heads, 1000 * heads + 10 * L + i)
        TA.check(f32_attention, f"f32 shapes[{'ab'[i]}]", qkv, mask, B, L, H, heads)


@pytest.mark.parametrize("heads,dh", [(4, 32), (2, 64)])
def test_f32_attention_window_and_alibi_against_float64(f32_attention, heads, dh):
    H, B, L = heads * dh, 3, 200
    mask = A.mask_from_lens([L, 5, 40], L)
    mask[2, 9] = 0
    qkv = A.make_qkv("unit", B, L, H, heads, 3 * L)
    TA.check(f32_attention, "f32 window, ragged", qkv, mask, B, L, H, heads, window=16)
    TA.check(f32_attention, "f32 window, full", qkv, A.mask_from_lens([L] * B, L), B, L, H, heads, window=16)
    hole = np.stack([A.mask_from_lens([L], L)[0], A.holes_mask(L, L), A.mask_from_lens([(3 * L) // 4], L)[0]])
    TA.check(f32_attention, "f32 alibi", qkv, hole, B, L, H, heads, slopes=A.geometric_slopes(heads))


def test_f32_attention_of_a_sequence_masked_entirely_is_finite_and_leaves_the_others_alone(f32_attention):
    for heads, dh, L in ((4, 32, 33), (4, 32, 129), (2, 64, 129)):
        H = heads * dh
        qkv = A.make_qkv("unit", 3, L, H, heads, 31 + L)
        mask = np.stack([A.mask_from_lens([L], L)[0], np.zeros(L, np.int32), A.holes_mask(L, 3)])
        got3, _, _ = TA.run_attention(f32_attention, qkv, mask, 3, L, H, heads)
        keep = np.r_[0:L, 2 * L:3 * L]
        got2, _, _ = TA.run_attention(f32_attention, qkv[keep], mask[[0, 2]], 2, L, H, heads)
        assert np.isfinite(got3).all()
        assert np.array_equal(got3[keep], got2)
        ref, bound, valid = A.attention_ref(qkv, mask, 3, L, H, heads)
        ratio = A.worst_ratio(got3, ref, bound, valid)
        print(f"f32 attention, a sequence masked entirely: heads {heads} x {dh}, L {L}: worst err/bound = {ratio:.3f}")
        assert not valid[L:2 * L].any() and ratio <= 1.0
