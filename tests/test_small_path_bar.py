"""The bars of the small path's operator tests must bite (CPU only; the bars themselves: tests/small_path_ref.py).

tests/test_gpu_small_path.py accepts a launch when |got - ref| <= bound in both stages.  Shown here, on the row families the
GPU tests use:
  (a) a plain numpy emulation of the split arithmetic — split_planes of both operands, the three-term product, f32
      accumulation, the kernels' order of adds — stays inside every new bound on every family: a correct kernel can meet them;
  (b) the emulation perturbed the way a kernel goes wrong leaves the bound on at least one family; the factor is printed.
Stage 1 (Xout against the LayerNorm bound) is tests/rows_ref.py's bar, shown to bite in tests/test_rows_bar.py.
Nothing a kernel returns enters a bound, so nothing here needs a GPU."""
import numpy as np
import pytest

from tests import rows_ref as R
from tests import small_path_ref as S
from tests.test_rows_bar import report

T, H = 21, 384           # two 16-row tiles, the second with five live rows
N_QKV, N_UP = 96, 128    # enough columns for every column slip below; the bounds do not depend on N
EPS = 1e-12


def xout_of(family, seed=3, shift_gb=False):
    """The f32 rows a correct prologue hands the product: the float32 LayerNorm of the family's rows."""
    v = R.make_rows(family, T, H, seed)
    g, b = R.make_gamma_beta(H, seed + 1)
    if shift_gb:
        g, b = np.roll(g, 2), np.roll(b, 2)
    return R.layernorm_f32(v, g, b, EPS)


def ffn_mid(family, seed=5):
    """A [T, 4H] as FFN-down reads it: the GELU of a unit-scale product of the family's rows, in split form."""
    w, bias = S.make_weights(4 * H, H, seed)
    return R.split_roundtrip(S.emulate_ln_gemm(xout_of(family, seed), w, bias, S.EPI_GELU))


# ---- (a) the emulation meets the bars ------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", R.ROW_FAMILIES)
def test_split_emulation_meets_every_bar(family):
    x = xout_of(family)
    for epi, N in ((S.EPI_SPLIT, N_QKV), (S.EPI_GELU, N_UP)):
        w, bias = S.make_weights(N, H, 11 + epi)
        ref, bound = S.ln_gemm_ref(x, w, bias, epi)
        ratio = R.worst(S.emulate_ln_gemm(x, w, bias, epi), ref, bound)
        print(f"LayerNorm product, {'GELU -> split' if epi else 'split'}, {family}: float32 emulation err/bound = {ratio:.3f}")
        assert ratio <= 1.0
    a = ffn_mid(family)
    w, _ = S.make_weights(N_QKV, 4 * H, 13)
    ref, bound = S.partial_ref(a, w, H)
    ratio = R.worst(S.emulate_partial(a, w, H), ref, bound)
    print(f"FFN-down K slices, {family}: float32 emulation err/bound = {ratio:.3f}")
    assert ratio <= 1.0


def test_integer_operands_are_exact_in_the_emulation():
    """What the GPU tests' bit-for-bit cases rest on: small integers pass the split arithmetic exactly."""
    w, bias = S.integer_weights(N_QKV, H, 7)
    x = np.broadcast_to(((np.arange(H) % 7) - 3).astype(np.float32), (T, H))
    want = (x.astype(np.int64) @ w.astype(np.int64).T + bias.astype(np.int64)).astype(np.float32)
    assert np.array_equal(S.emulate_ln_gemm(x, w, bias, S.EPI_SPLIT), want)
    w4, _ = S.integer_weights(N_QKV, 4 * H, 8, quarters=4)
    a = np.random.default_rng(9).integers(-4, 5, (T, 4 * H)).astype(np.float32)
    slabs = S.emulate_partial(a, w4, H)
    for ks in range(4):
        k = slice(ks * H, (ks + 1) * H)
        assert np.array_equal(slabs[ks], (a[:, k].astype(np.int64) @ w4[:, k].astype(np.int64).T).astype(np.float32))
    assert len({slabs[ks].tobytes() for ks in range(4)}) == 4


# ---- (b) perturbed emulations leave the bars -----------------------------------------------------------------------------

def test_perturbed_products_leave_the_bound():
    w, bias = S.make_weights(N_QKV, H, 11)
    dropped, scaled, next_bias, shifted, last_row = {}, {}, {}, {}, {}
    for family in R.ROW_FAMILIES:
        x = xout_of(family)
        ref, bound = S.ln_gemm_ref(x, w, bias, S.EPI_SPLIT)
        dropped[family] = R.worst(S.emulate_ln_gemm(x, w, bias, S.EPI_SPLIT, drop_lo_hi_chunk=5), ref, bound)
        scaled[family] = R.worst(S.emulate_ln_gemm(x, w, bias, S.EPI_SPLIT, lo_scale=2.0 ** -10), ref, bound)
        next_bias[family] = R.worst(S.emulate_ln_gemm(x, w, np.roll(bias, -1), S.EPI_SPLIT), ref, bound)
        # a block that is not the one writing Xout applies gamma / beta a column pair off: Xout is right, its tile is not
        shifted[family] = R.worst(S.emulate_ln_gemm(xout_of(family, shift_gb=True), w, bias, S.EPI_SPLIT), ref, bound)
        clamped = x.copy()
        clamped[16] = x[T - 1]                                  # the last tile's first row read as row T - 1
        last_row[family] = R.worst(S.emulate_ln_gemm(clamped, w, bias, S.EPI_SPLIT), ref, bound)
    report("one k-chunk's lo x hi term dropped", dropped)
    report("the lo x hi terms scaled by 2^-10 instead of 2^-11", scaled)
    report("the bias of column n + 1", next_bias)
    report("gamma / beta shifted by a column pair in a block that does not write Xout", shifted)
    report("row T - 1 in place of the last tile's first row", last_row)


def test_tanh_gelu_leaves_the_bound():
    w, bias = S.make_weights(N_UP, H, 12)
    found = {}
    for family in R.ROW_FAMILIES:
        x = xout_of(family)
        ref, bound = S.ln_gemm_ref(x, w, bias, S.EPI_GELU)
        found[family] = R.worst(S.emulate_ln_gemm(x, w, bias, S.EPI_GELU, tanh_gelu=True), ref, bound)
    report("tanh-GELU in place of erf-GELU", found)


def test_perturbed_k_slices_leave_the_bound():
    w, _ = S.make_weights(N_QKV, 4 * H, 13)
    moved, dropped = {}, {}
    for family in R.ROW_FAMILIES:
        a = ffn_mid(family)
        ref, bound = S.partial_ref(a, w, H)
        moved[family] = R.worst(S.emulate_partial(a, w, H, slab_of_chunk={(1, 2): 2}), ref, bound)
        dropped[family] = R.worst(S.emulate_partial(a, w, H, drop_lo_hi_chunk=5), ref, bound)
        # the SUM of the slabs does not see a chunk in the wrong slab: only the per-slab check does
        total = S.emulate_partial(a, w, H, slab_of_chunk={(1, 2): 2}).astype(np.float64).sum(axis=0)
        assert R.worst(total, ref.sum(axis=0), bound.sum(axis=0)) <= 1.0
    report("a chunk of slab 1 added into slab 2", moved)
    report("one k-chunk's lo x hi term dropped in every slab", dropped)


def test_pairwise_slab_sum_breaks_bit_equality_only():
    """Slabs summed (p0 + p1) + (p2 + p3) instead of ((p0 + p1) + p2) + p3: an equally good rounding, so it stays inside
    the float64 bound — what catches it is the bit-for-bit comparison of Xout with layernorm_sum_kernel's rows."""
    rng = np.random.default_rng(17)
    parts = [rng.standard_normal((T, H)).astype(np.float32) for _ in range(4)]
    pb = (rng.standard_normal(H) * 0.1).astype(np.float32)
    x = R.make_rows("normal", T, H, 18)
    g, b = R.make_gamma_beta(H, 19)
    chain = ((((parts[0] + parts[1]) + parts[2]) + parts[3]) + pb) + x
    pairs = (((parts[0] + parts[1]) + (parts[2] + parts[3])) + pb) + x
    ref, bound = S.prologue_ref(1, g, b, EPS, parts=np.stack(parts), parts_bias=pb, x=x)
    out_chain, out_pairs = R.layernorm_f32(chain, g, b, EPS), R.layernorm_f32(pairs, g, b, EPS)
    r_chain, r_pairs = R.worst(out_chain, ref, bound), R.worst(out_pairs, ref, bound)
    differing = int((out_chain.view(np.uint32) != out_pairs.view(np.uint32)).sum())
    print(f"slabs summed (p0 + p1) + (p2 + p3): err/bound = {r_pairs:.3f} (in order: {r_chain:.3f}), {differing} of {out_chain.size} values differ in their bits")
    assert r_chain <= 1.0 and differing > 0
