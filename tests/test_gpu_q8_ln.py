"""The LayerNorm-fused quantised product (gemm_q8_ln_kernel, csrc/gemm_q8.hip) and the unit bookkeeping kernels next to it,
each alone through cs_debug_gemm_q8_ln / cs_debug_q8_unit_ranges, against numpy (tests/q8_ln_ref.py: float64 reference and
derived bound; tests/test_q8_ln_bar.py shows that the bound bites and that a correct float32 evaluation meets it).

Every launch asserts: the separate quantising pass holds the reference's bytes and parameters exactly; the output rows are
finite and inside the bound; every guard row behind row M still holds the sentinel; and the range hand-over — the (lo, hi)
pair of each 16 rows bit for bit over the RETURNED rows below M, (0, 0) from a wave wholly past M, the reduced (or directly
widened) slot the same over the whole tensor."""
import ctypes as C
import functools

import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd._lib import f32p, u32p
from tests import q8_ln_ref as Q
from tests import rows_ref as R

pytestmark = pytest.mark.gpu

EPS = (1e-12, 1e-5)
KINDS = tuple(Q.WEIGHT_KINDS)
STAGE_MAJOR, SLOT = 1, 2


def run_ln(lib, case, source, eps, flags=0):
    M, K = case["A"].shape
    out = np.empty((M + Q.GUARD_ROWS, Q.N), np.float32)
    cap = (M + 127) // 128 * 8
    pairs = np.empty((cap, 2), np.float32)
    n_pairs = C.c_uint32(0xffffffff)
    slot = np.empty(2, np.uint32)
    xq = np.empty((M, K), np.uint8)
    xp = np.empty(2, np.float32)
    p = lambda a: a.ctypes.data_as(f32p)
    _lib.check_diag(lib.cs_debug_gemm_q8_ln(0, 0 if source == "split" else 1, flags, p(case["A"]), p(case["W"]), p(case["sc"]),
                                            p(case["bias"]), p(case["gamma"]), p(case["beta"]), eps, p(case["resid"]), M, K,
                                            p(out), p(pairs), cap, C.byref(n_pairs), slot.ctypes.data_as(u32p),
                                            xq.ctypes.data_as(C.POINTER(C.c_uint8)), p(xp)))
    return {"rows": out[:M], "guard": out[M:].view(np.uint32), "pairs": pairs.view(np.uint32), "n_pairs": n_pairs.value,
            "slot": slot, "xq": xq, "xp": xp}


@functools.lru_cache(maxsize=None)
def reference(family, M, K, kind, source, eps):
    """Computed once per call shape, shared by the tests that need it (the integer product once for both eps)."""
    return Q.reference(Q.make_case(family, M, K, kind), source, eps, quantized(family, M, K, kind, source))


@functools.lru_cache(maxsize=None)
def quantized(family, M, K, kind, source):
    return Q.quantized(Q.make_case(family, M, K, kind), source)


def check(got, ref, M, slot_mode=False, waves=8):
    """The five assertions of one launch -> worst err / bound."""
    assert got["xp"][0] == ref["xs"] and int(got["xp"][1]) == ref["xz"]
    assert np.array_equal(got["xq"], ref["q"])                                   # the separate pass: the reference's bytes
    rows = got["rows"]
    assert np.isfinite(rows).all()
    ratio = R.worst(rows, ref["ref"], ref["bound"])
    assert ratio <= 1.0, ratio
    assert (got["guard"] == Q.GUARD_WORD).all(), np.argwhere(got["guard"] != Q.GUARD_WORD)[:4]
    whole = Q.range_pair(rows)
    if slot_mode:
        assert got["n_pairs"] == 0
    else:
        rg = 16 * waves
        n = (M + rg - 1) // rg * waves
        assert got["n_pairs"] == n
        want = np.stack([Q.range_pair(rows[16 * i:min(16 * i + 16, M)]) if 16 * i < M else np.zeros(2, np.uint32) for i in range(n)])
        assert np.array_equal(got["pairs"][:n], want), np.argwhere(got["pairs"][:n] != want)[:4]
        assert (got["pairs"][n:] == 0xffffffff).all()                            # nothing written behind the reported pairs
    assert np.array_equal(got["slot"], whole), (got["slot"], whole)
    return ratio


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("source,K", Q.SOURCES)
@pytest.mark.parametrize("M", [1, 15, 16, 17, 127, 128, 129, 293])
def test_small_shapes_meet_the_bound(diag_lib, M, source, K, eps):
    """One row, a wave's 16 rows and one either side, a block's 128 and one either side, three groups with a ragged last one:
    waves wholly past M, lanes past M inside a wave.  The weight in the order the forward streams it (stage-major)."""
    kind = KINDS[(M + K // 384) % 3]
    got = run_ln(diag_lib, Q.make_case("normal", M, K, kind), source, eps, STAGE_MAJOR)
    ratio = check(got, reference("normal", M, K, kind, source, eps), M)
    print(f"q8 LayerNorm product M {M} {source} K {K} {kind} eps {eps:g}: err/bound = {ratio:.3f}")


@pytest.mark.parametrize("source,K", Q.SOURCES)
@pytest.mark.parametrize("family", Q.FAMILIES)
def test_every_family_meets_the_bound(diag_lib, family, source, K):
    M = 293
    for kind in KINDS:
        worst = 0.0
        for eps in EPS:
            got = run_ln(diag_lib, Q.make_case(family, M, K, kind), source, eps, STAGE_MAJOR)
            worst = max(worst, check(got, reference(family, M, K, kind, source, eps), M))
        print(f"q8 LayerNorm product {family} {source} K {K} {kind}: worst err/bound = {worst:.3f}")


@pytest.mark.parametrize("source,K", Q.SOURCES)
def test_weight_order_and_range_form_leave_the_same_bits(diag_lib, source, K):
    """Row-major against stage-major weight (launch_q8_stage_major's order is the one the kernel streams), pairs against the
    slot the kernel widens itself: the same output bytes, and each form's own hand-over."""
    M, kind, eps = 293, KINDS[0], 1e-12
    case, ref = Q.make_case("normal", M, K, kind), reference("normal", M, K, kind, source, eps)
    base = run_ln(diag_lib, case, source, eps, 0)
    worst = check(base, ref, M)
    for flags in (STAGE_MAJOR, SLOT, STAGE_MAJOR | SLOT):
        got = run_ln(diag_lib, case, source, eps, flags)
        worst = max(worst, check(got, ref, M, slot_mode=bool(flags & SLOT)))
        assert got["rows"].tobytes() == base["rows"].tobytes(), flags
        if not flags & SLOT:
            assert got["pairs"].tobytes() == base["pairs"].tobytes()
    print(f"q8 LayerNorm product, both weight orders and range forms, {source} K {K}: worst err/bound = {worst:.3f}")


@pytest.mark.parametrize("source,K", Q.SOURCES)
def test_a_block_walks_three_groups(diag_lib, monkeypatch, source, K):
    """CS_Q8_LN_MAX_BLOCKS=1: one block takes the three row groups of M = 293 one after the other — the weight ring restarts
    in the slots the previous group's last stages left, the (lo, hi) words of LDS are used again (slot mode).  The uncapped
    launch's bytes, inside the bound."""
    M, kind, eps = 293, KINDS[1], 1e-5
    case, ref = Q.make_case("normal", M, K, kind), reference("normal", M, K, kind, source, eps)
    for flags in (STAGE_MAJOR, SLOT):
        monkeypatch.delenv("CS_Q8_LN_MAX_BLOCKS", raising=False)
        free = run_ln(diag_lib, case, source, eps, flags)
        monkeypatch.setenv("CS_Q8_LN_MAX_BLOCKS", "1")
        capped = run_ln(diag_lib, case, source, eps, flags)
        ratio = check(capped, ref, M, slot_mode=bool(flags & SLOT))
        check(free, ref, M, slot_mode=bool(flags & SLOT))
        assert capped["rows"].tobytes() == free["rows"].tobytes()
        assert capped["pairs"].tobytes() == free["pairs"].tobytes() or flags & SLOT
        print(f"q8 LayerNorm product, three groups in one block, {source} K {K} flags {flags}: err/bound = {ratio:.3f}")


def test_production_grid(diag_lib):
    """M = 33,000, above 128 rows x 256 CUs: the grid the forward launches, where two blocks walk a second group."""
    M, K, kind, eps = 33000, 384, KINDS[2], 1e-12
    case = Q.make_case("normal", M, K, kind)
    for source in ("split", "prequant"):
        ratio = check(run_ln(diag_lib, case, source, eps, STAGE_MAJOR), reference("normal", M, K, kind, source, eps), M)
        print(f"q8 LayerNorm product M {M} {source} K {K} {kind}: err/bound = {ratio:.3f}")


@pytest.mark.parametrize("source,K", Q.SOURCES)
def test_four_wave_variant_leaves_the_same_bits(diag_lib, monkeypatch, source, K):
    """CS_Q8_LN_WAVES=4 (64-row blocks, a three-stage ring, gamma / beta from global memory): the arithmetic of a row is the
    same, so the eight-wave form's bytes, and ceil(M / 64) * 4 pairs."""
    M, kind, eps = 293, KINDS[0], 1e-12
    case, ref = Q.make_case("normal", M, K, kind), reference("normal", M, K, kind, source, eps)
    monkeypatch.delenv("CS_Q8_LN_WAVES", raising=False)
    eight = run_ln(diag_lib, case, source, eps, STAGE_MAJOR)
    monkeypatch.setenv("CS_Q8_LN_WAVES", "4")
    four = run_ln(diag_lib, case, source, eps, STAGE_MAJOR)
    ratio = check(four, ref, M, waves=4)
    assert four["rows"].tobytes() == eight["rows"].tobytes()
    assert four["n_pairs"] == (M + 63) // 64 * 4
    print(f"q8 LayerNorm product, four waves, {source} K {K}: err/bound = {ratio:.3f}")


def test_a_weight_off_its_grid_is_refused(diag_lib):
    case = dict(Q.make_case("normal", 16, 384, KINDS[0]))
    W = case["W"].copy()
    W[5, 7] += 0.4 * case["sc"][5]
    case["W"] = W
    with pytest.raises(_lib.CsError, match="not a quantised matrix"):
        run_ln(diag_lib, case, "prequant", 1e-12)


# ---- the unit bookkeeping of queued batches ----------------------------------------------------------------------------------

def run_units(lib, seq_unit, unit_len, L, pairs=None, pps=0, rows=False, want_slots=True):
    B, U = len(seq_unit), len(unit_len)
    su, ul = np.ascontiguousarray(seq_unit, np.uint32), np.ascontiguousarray(unit_len, np.uint32)
    row_slot = np.empty(B * L, np.uint32)
    slots = np.empty((U, 2), np.uint32)
    pr = None if pairs is None else np.ascontiguousarray(pairs, np.float32)
    _lib.check_diag(lib.cs_debug_q8_unit_ranges(0, su.ctypes.data_as(u32p), ul.ctypes.data_as(u32p), B, U, L,
                                                None if pr is None else pr.ctypes.data_as(f32p), pps, int(rows),
                                                row_slot.ctypes.data_as(u32p), None if pr is None else slots.ctypes.data_as(u32p)))
    return row_slot, slots


@pytest.mark.parametrize("L", [1, 37, 128])
def test_row_slots_against_numpy(diag_lib, L):
    """q8_row_slot_kernel: every own length from 1 to L, units whose own length is L included; 300 sequences, so the rows
    span many blocks of 256 threads and end inside one."""
    rng = np.random.default_rng(L)
    unit_len = sorted({1, max(1, L // 3), max(1, L - 1), L}) + [L, 1]
    counts = rng.multinomial(300 - len(unit_len), np.ones(len(unit_len)) / len(unit_len)) + 1
    seq_unit = np.repeat(np.arange(len(unit_len)), counts)
    row_slot, _ = run_units(diag_lib, seq_unit, unit_len, L)
    assert np.array_equal(row_slot, Q.unit_row_slots(seq_unit, unit_len, L))


@pytest.mark.parametrize("rows", [True, False])
def test_unit_ranges_against_numpy(diag_lib, rows):
    """q8_range_reduce_units_kernel, B = 300 sequences over 7 units (the search for a unit's first and last sequence strides
    past the block's 256 threads): unit 3 owns no sequence — (0, 0); unit 1's positions beyond its own length hold the
    batch's most extreme pairs — they must not widen it (row pairs); unit 5's pairs are all positive — lo stays +0."""
    rng = np.random.default_rng(11 + rows)
    L = 37
    pps = L if rows else 5
    unit_len = [L, 9, 20, 12, L, 30, 1]
    counts = [40, 30, 100, 0, 90, 25, 15]
    seq_unit = np.repeat(np.arange(7), counts)
    B = len(seq_unit)
    assert B == 300
    v = rng.standard_normal((B, pps, 2)).astype(np.float32) * rng.choice([0.5, 2.0, 6.0], size=7)[seq_unit][:, None, None].astype(np.float32)
    pairs = np.stack([np.minimum(v.min(axis=2), 0), np.maximum(v.max(axis=2), 0)], axis=2).astype(np.float32)
    pairs[seq_unit == 5, :, 0] = 0.0
    pairs[seq_unit == 5, :, 1] = np.abs(v[seq_unit == 5, :, 1]) + np.float32(0.25)
    if rows:
        pairs[seq_unit == 1, unit_len[1]:] = (-1.0e4, 1.0e4)
    _, slots = run_units(diag_lib, seq_unit, unit_len, L, pairs, pps, rows)
    want = Q.unit_ranges(pairs, pps, rows, seq_unit, unit_len, 7)
    assert np.array_equal(slots, want), (slots, want)
    assert not slots[3].any() and slots[5, 0] == 0
    if rows:
        assert slots[1].view(np.float32)[1] < 100.0
