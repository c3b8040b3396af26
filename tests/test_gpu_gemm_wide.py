"""The persistent wide dense-layer kernel alone against float64: every block shape (128 x 384, 128 x 192, the diagnostic
256 x 192), both MFMA forms (gemm_wide.hip, gemm_wide32.hip) and every epilogue, through cs_debug_gemm_wide.

References and bounds: tests/gemm_wide_ref.py (the bounds are formed from the float64 reference alone; that they bite is
shown on the CPU in tests/test_gemm_wide_bar.py).  Every case asserts the block the launch reports, that no guard word
behind an output changed, that no live element stayed unwritten (NaN), and err <= bound everywhere.  The err/bound ratio
of every case is printed (pytest -s).

Shapes (M, N, K) and what each is there for:
  (1, 384, 32)            one k-chunk, one row: prefetch and double buffer with nothing to prefetch
  (129, 1152, 96)         one full tile + 1 row: with 2 m-tiles, 6 of every 8 slots are invalid (next_valid); 3 k-chunks
                          against 3 (384) and 6 (192) n-tiles: both branches of sh_kc_rot
  (130, 192 | 576, 64)    N only the 192-column blocks take
  (5, 3840 | 4224, 32)    the largest N whose bias the 128 x 384 block keeps in LDS, and the first it hands to 128 x 192
  (130, 6144, 768)        NomicBert's up projection
  (130, 2304, 768), (130, 768, 3072), (130, 3072, 1024)   hidden 768 / 1024
  (130, 1024, 4096)       hidden 1024's FFN-down: N = 1024 is no multiple of 192 — the wide kernel does not take it, and the
                          entry point must say so (test_unsupported_width_is_refused)
  (255 | 256 | 257, 384, 64)   the 256-row block's edges
  persistent loop         more tiles than resident blocks, last m-tile partial (test_persistent_loop; sizes from the
                          device's CU count)
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import gemm_wide_ref as G
from tests import rows_ref as R
from tests import small_path_ref as S

pytestmark = pytest.mark.gpu

TABLE = [(1, 384, 32), (129, 1152, 96), (130, 192, 64), (130, 576, 64), (5, 3840, 32), (5, 4224, 32), (130, 6144, 768),
         (130, 2304, 768), (130, 768, 3072), (130, 3072, 1024), (255, 384, 64), (256, 384, 64), (257, 384, 64)]
FIRST_ROWS = TABLE[:4]            # the table's first three rows (the third holds two widths)
EDGES_256 = TABLE[10:]
GATED_N = (192, 384, 1152, 6144)  # the widths the gated epilogues run on
PLAIN, GATED, LN = (0, 1, 2, 3), G.GATED, (G.EPI_LN, G.EPI_LN_SPLIT)
# (block, mfma): the product kernels, then the diagnostic-only forms
PRODUCT_FORMS = ((384, 16), (192, 16))
DIAG_FORMS = ((384, 32), (192, 32), (256, 16))


def accepts(block, N):
    """The widths a block takes (gemm_wide.hpp gemm_wide_route; GW_PARAM_FLOATS = 4096: the bias the 384 block keeps in LDS)."""
    return N % 384 == 0 and N <= 4096 if block == 384 else N % 192 == 0


def epilogues(block, mfma, N):
    epis = list(PLAIN)
    if mfma == 16 and N in GATED_N:
        epis += GATED                      # (the gated epilogues are not built on the 32 x 32 x 16 form)
    if block == 384 and N == 384:
        epis += LN                         # whole rows in one block
    return epis


def table_cases():
    cases = []
    for block, mfma in PRODUCT_FORMS + DIAG_FORMS:
        product = (block, mfma) in PRODUCT_FORMS
        shapes = TABLE if product else FIRST_ROWS + (EDGES_256 if block == 256 else [])
        for M, N, K in shapes:
            if accepts(block, N):
                cases += [(M, N, K, block, mfma, epi) for epi in epilogues(block, mfma, N)]
    return sorted(cases)   # by shape: a shape's reference is computed once (shape_data)


def case_id(c):
    return "-".join(str(v) for v in c) if isinstance(c, tuple) else str(c)


class ShapeData:
    """The operands of one shape and, computed once and shared by its cases, the float64 products with their bounds."""

    def __init__(self, M, N, K):
        self.a, self.w, self.bias, self.resid = G.make_operands(M, N, K, M * 7 + N * 3 + K, resid=True)
        if N % 64 == 0:   # the same rows as value rows | gate rows, in the interleaved order
            self.wg, self.bg = G.pack_gated(self.w[:N // 2], self.w[N // 2:], self.bias[:N // 2], self.bias[N // 2:])
        self._plain = self._gated = self._ln = None

    def operands(self, epi):
        return (self.a, self.wg, self.bg) if epi in GATED else (self.a, self.w, self.bias)

    def reference(self, epi):
        if epi in LN:
            if self._ln is None:
                self._ln = G.layernorm_ref(self.a, self.w, self.bias, self.resid)
            return self._ln, G.LN_BAR
        if epi in GATED:
            if self._gated is None:
                h = self.w.shape[0] // 2
                self._gated = (S.product_ref(self.a, np.ascontiguousarray(self.w[:h]), self.bias[:h])
                               + S.product_ref(self.a, np.ascontiguousarray(self.w[h:]), self.bias[h:]))
            return G.gated_ref(epi, *self._gated)
        if self._plain is None:
            self._plain = S.product_ref(self.a, self.w, self.bias)
        return G.plain_ref(epi, *self._plain, resid=self.resid)


@functools.lru_cache(maxsize=2)
def shape_data(M, N, K):
    return ShapeData(M, N, K)


def run_wide(lib, epi, shape, mfma, a, w, bias, resid=None):
    """-> (out [M, N] or [M, N / 2], the block that ran, changed guard words, the kernel's range flag)"""
    from codesearch_amd import _lib

    M, K = a.shape
    N = w.shape[0]
    out = np.empty((M, N // 2 if epi in GATED else N), np.float32)
    block, guard, flag = C.c_int32(0), C.c_uint32(12345), C.c_uint32(0)
    f32p = _lib.f32p
    a, w, bias = (np.ascontiguousarray(x, np.float32) for x in (a, w, bias))
    resid = None if resid is None else np.ascontiguousarray(resid, np.float32)
    _lib.check_diag(lib.cs_debug_gemm_wide(0, epi, shape, mfma, a.ctypes.data_as(f32p), w.ctypes.data_as(f32p),
                                           bias.ctypes.data_as(f32p), resid.ctypes.data_as(f32p) if resid is not None else None,
                                           out.ctypes.data_as(f32p), M, N, K, C.byref(block), C.byref(guard), C.byref(flag)))
    return out, int(block.value), int(guard.value), int(flag.value)


def check(lib, d, block, mfma, epi, shape=None):
    """One launch on the operands of d against its float64 reference; -> the output."""
    a, w, bias = d.operands(epi)
    resid = d.resid if epi in (G.EPI_RESID,) + LN else None
    got, ran, guard, flag = run_wide(lib, epi, block if shape is None else shape, mfma, a, w, bias, resid)
    assert ran == block, f"asked for the {block} block, the launch ran on {ran}"
    assert guard == 0, f"{guard} guard words behind the output changed"
    assert not np.isnan(got).any(), f"{int(np.isnan(got).sum())} live elements were not written"
    ref, bound = d.reference(epi)
    ratio = R.worst(got, ref, bound)
    print(f"RATIO block {block} mfma {mfma or 16} epi {epi} ({G.EPI_NAMES[epi]}) M {a.shape[0]} N {w.shape[0]} K {a.shape[1]}: "
          f"err/bound = {ratio:.4f}")
    assert flag == 0
    assert ratio <= 1.0
    return got


@pytest.mark.parametrize("case", table_cases(), ids=case_id)
def test_wide_gemm_against_float64(diag_lib, case):
    M, N, K, block, mfma, epi = case
    d = shape_data(M, N, K)
    got = check(diag_lib, d, block, mfma, epi)
    if epi == G.EPI_LN_SPLIT:   # the two residual forms of the LayerNorm epilogue against each other
        other = check(diag_lib, d, block, mfma, G.EPI_LN)
        assert R.worst(got, other.astype(np.float64), G.LN_FORMS_BAR) <= 1.0


def persistent_shape(block, cus):
    """The smallest (M, N, K) whose tiles overflow the resident blocks of a persistent grid, last m-tile partial: -> the
    shape, ceil8(mtiles) * ntiles and the resident blocks (gemm_wide.hip gemm_wide_launch: whole XCD octets of CUs, two
    blocks per CU for the 128 x 192 block)."""
    resident = cus // 8 * 8 * (2 if block == 192 else 1)
    N, bn, bm, short = {192: (6144, 192, 128, 5), 384: (1536, 384, 128, 5), 256: (1536, 192, 256, 3)}[block]
    ntiles = N // bn
    octets = resident // ntiles // 8 + 1            # of m-tiles: ceil8(mtiles) = 8 * octets is the first to overflow
    mtiles = 8 * octets - 7                         # the smallest mtiles of that octet count
    return (mtiles * bm - short, N, 64), 8 * octets * ntiles, resident


@pytest.mark.parametrize("block,mfma", PRODUCT_FORMS + DIAG_FORMS, ids=case_id)
def test_persistent_loop(diag_lib, block, mfma):
    """ceil8(mtiles) * ntiles > resident blocks: blocks walk on to a second tile, whose first stage was prefetched under the
    first tile's epilogue; the last m-tile is partial.  Every epilogue of the form on one shape."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    (M, N, K), slots, resident = persistent_shape(block, cus)
    assert slots > resident and M % (256 if block == 256 else 128) != 0
    assert M * N * K < 1e9   # the float64 reference stays a product of under 10^9 multiply-adds
    d = shape_data(M, N, K)
    for epi in PLAIN + (GATED if mfma == 16 else ()):
        check(diag_lib, d, block, mfma, epi)
    if block == 384:   # the LayerNorm epilogue's own: N = 384 is one n-tile, so one m-tile more than the resident blocks
        mtiles = cus // 8 * 8 + 1
        d = shape_data(mtiles * 128 - 5, 384, 32)
        got = [check(diag_lib, d, block, mfma, epi) for epi in LN]
        assert R.worst(got[1], got[0].astype(np.float64), G.LN_FORMS_BAR) <= 1.0


@pytest.mark.parametrize("N", [384, 576, 4224])
def test_shape_zero_takes_the_documented_default(diag_lib, N):
    """shape = 0: the 128 x 192 block for the bias -> split store (the QKV projection), otherwise 128 x 384 where N allows."""
    d = shape_data(5, N, 32)
    for epi in PLAIN + GATED:
        want = 192 if epi == G.EPI_SPLIT or not accepts(384, N) else 384
        check(diag_lib, d, want, 0, epi, shape=0)


def test_unsupported_width_is_refused(diag_lib):
    """(130, 1024, 4096), hidden 1024's FFN-down: 1024 is no multiple of 192, so no block of the wide kernel takes it; a
    384 block asked for at a width it cannot take shows in the reported block."""
    from codesearch_amd import _lib

    a, w, bias = G.make_operands(130, 1024, 4096, 1)
    with pytest.raises(_lib.CsError) as e:
        run_wide(diag_lib, 0, 0, 0, a, w, bias)
    assert e.value.code == _lib.CS_ERR_UNSUPPORTED
    d = shape_data(5, 4224, 32)
    _, ran, guard, _ = run_wide(diag_lib, 0, 384, 0, *d.operands(0))
    assert ran == 192 and guard == 0


# ---- exactness -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def integer_operands():
    M, N, K = 129, 1152, 96
    w, bias = S.integer_weights(N, K, 7)
    a = np.random.default_rng(9).integers(-4, 5, (M, K)).astype(np.float32)
    a[:, 3] += (np.arange(M) % 5).astype(np.float32)              # asymmetric in m
    resid = np.random.default_rng(10).integers(-9, 10, (M, N)).astype(np.float32)
    return a, w, bias, resid


@pytest.mark.parametrize("w31", [False, True], ids=["small", "w31"])
@pytest.mark.parametrize("epi", [G.EPI_F32, G.EPI_RESID, G.EPI_SPLIT])
@pytest.mark.parametrize("block,mfma", PRODUCT_FORMS + DIAG_FORMS, ids=case_id)
def test_integer_operands_bit_for_bit(diag_lib, block, mfma, epi, w31):
    """Small integers, asymmetric in m, n and k: every product and partial sum is exact on the scaled accumulator, so the
    f32 stores and the split store return the integer result bit for bit.  w31: one weight of 31, whose hi part times 2^11
    is the largest the f16 fragment holds."""
    a, w, bias, resid = integer_operands()
    if w31:
        w = w.copy()
        w[5, 7] = 31.0
    want = (a.astype(np.int64) @ w.astype(np.int64).T + bias.astype(np.int64)).astype(np.float32)
    if epi == G.EPI_RESID:
        want = want + resid
    got, ran, guard, flag = run_wide(diag_lib, epi, block, mfma, a, w, bias, resid if epi == G.EPI_RESID else None)
    assert ran == block and guard == 0 and flag == 0
    assert np.array_equal(got, want)


# ---- range flag ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("epi", G.SPLIT_STORES)
@pytest.mark.parametrize("block", [384, 192, 256])
def test_range_flag(diag_lib, block, epi):
    """One output beyond 65,504 in the last live row of a partial tile raises the kernel's flag; the same rows scaled down
    by ten do not."""
    M, N, K = 130, 384, 32
    a, w, bias = (x.copy() for x in G.make_operands(M, N, K, 77))
    w[:, 0] = 0.0                      # k = 0 reaches one output only
    a[M - 1, 0] = 3.0e4                # f16-representable
    if epi in GATED:                   # gated column 100: value 9e4, gate exactly 3
        vrow, grow = 32 * (100 // 16) + 100 % 16, 32 * (100 // 16) + 16 + 100 % 16
        w[vrow, 0] = 3.0
        w[grow, :] = 0.0
        w[grow, 0] = 1.0e-4
        bias[grow] = 0.0
    else:
        w[200, 0] = 3.0                # output (129, 200) = 9e4 + O(1)
    w = R.split_roundtrip(w)
    got, ran, guard, flag = run_wide(diag_lib, epi, block, 0, a, w, bias)
    assert ran == block and guard == 0
    assert flag == 1
    got, ran, guard, flag = run_wide(diag_lib, epi, block, 0, a * np.float32(0.1), w, bias)
    assert ran == block and guard == 0 and not np.isnan(got).any()
    assert flag == 0
