"""The bars of the wide GEMM's operator tests must bite (CPU only; the bars themselves: tests/gemm_wide_ref.py).

tests/test_gpu_gemm_wide.py accepts a launch when |got - ref| <= bound.  Shown here, on operands from the generator the GPU
tests use (gemm_wide_ref.make_operands: unit-scale rows, weights and bias with a per-column signature):
  (a) a float32 numpy emulation of the kernel's arithmetic — the three-term product on ONE accumulator scaled by 2^11 that
      starts at bias * 2^11, the k-chunks in the n-tile's rotated order, the epilogue arithmetic as written (gw_erf_fast's
      polynomial, exp2, the reciprocal) — stays inside every bound: a correct kernel can meet them;
  (b) the emulation perturbed the way this kernel can go wrong leaves the bound; every factor is printed and is above 1;
  (c) the activation constants of the bounds keep their 2x margin over the emulated fast forms on a grid of [-6, 6].
Nothing a kernel returns enters a bound, so nothing here needs a GPU."""
import math

import numpy as np
import pytest

from tests import gemm_wide_ref as G
from tests import rows_ref as R
from tests import small_path_ref as S

M, N, K = 140, 1152, 96      # two m-tiles (row 131 exists), three 384-column n-tiles over three k-chunks: rotations 0, 1, 2
I = N // 2                   # gated width: twelve waves' 48 columns
PLAIN = (G.EPI_F32, G.EPI_GELU, G.EPI_RESID, G.EPI_SPLIT)


def operands(gated, seed=21):
    a, w, bias, resid = G.make_operands(M, N, K, seed, resid=True)
    if gated:   # the generator's rows taken as value rows | gate rows, packed in the interleaved order
        w, bias = G.pack_gated(w[:I], w[I:], bias[:I], bias[I:])
    return a, w, bias, resid


def bars(epi):
    a, w, bias, resid = operands(epi in G.GATED)
    ref, bound = G.reference(epi, a, w, bias, resid)
    return a, w, bias, resid, ref, bound


def report(what, found):
    print(f"{what}: " + ", ".join(f"{G.EPI_NAMES[e]} {v:.3g}x" for e, v in found.items()))
    assert all(v > 1.0 for v in found.values()), (what, found)


# ---- (a) the emulation meets the bars ------------------------------------------------------------------------------------

@pytest.mark.parametrize("epi", range(6))
def test_emulation_meets_every_bar(epi):
    a, w, bias, resid, ref, bound = bars(epi)
    for bn in (384, 192):
        ratio = R.worst(G.emulate(epi, a, w, bias, resid, bn=bn), ref, bound)
        print(f"{G.EPI_NAMES[epi]}, {bn}-column tiles: float32 emulation err/bound = {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("k", [32, 768, 4096])
def test_emulation_meets_the_bars_at_every_k(k):
    """One k-chunk, and the K of the hidden-768 / 1024 layers: the bound grows with sum |a| |w| as the accumulation does."""
    a, w, bias, resid = G.make_operands(33, 384, k, k, resid=True)
    wg, bg = G.pack_gated(w[:192], w[192:], bias[:192], bias[192:])
    for epi in range(6):
        ww, bb = (wg, bg) if epi in G.GATED else (w, bias)
        ref, bound = G.reference(epi, a, ww, bb, resid)
        ratio = R.worst(G.emulate(epi, a, ww, bb, resid), ref, bound)
        print(f"K = {k}, {G.EPI_NAMES[epi]}: float32 emulation err/bound = {ratio:.3f}")
        assert ratio <= 1.0


def test_integer_operands_are_exact_in_the_emulation():
    """What the GPU tests' bit-for-bit cases rest on: small integers (|w| up to 31) pass the scaled accumulator exactly."""
    w, bias = S.integer_weights(N, K, 7)
    w[5, 7] = 31.0
    a = np.random.default_rng(9).integers(-4, 5, (M, K)).astype(np.float32)
    resid = np.random.default_rng(10).integers(-9, 10, (M, N)).astype(np.float32)
    want = (a.astype(np.int64) @ w.astype(np.int64).T + bias.astype(np.int64)).astype(np.float32)
    assert np.abs(w).max() == 31.0
    assert np.array_equal(G.emulate(G.EPI_F32, a, w, bias), want)
    assert np.array_equal(G.emulate(G.EPI_SPLIT, a, w, bias), want)
    assert np.array_equal(G.emulate(G.EPI_RESID, a, w, bias, resid), want + resid)


# ---- (b) perturbed emulations leave the bars -----------------------------------------------------------------------------

def test_gate_mapping_slips_leave_the_bound():
    swapped, group, flat_bias, piece, half_line, stride, stride_even = {}, {}, {}, {}, {}, {}, {}
    for epi in G.GATED:
        a, w, bias, _, ref, bound = bars(epi)
        good = G.emulate(epi, a, w, bias)
        swapped[epi] = R.worst(G.emulate(epi, a, w, bias, swap_gate=True), ref, bound)
        group[epi] = R.worst(np.roll(good, 16, axis=1), ref, bound)
        bv, bg = G.unpack_gated(bias)
        flat_bias[epi] = R.worst(G.emulate(epi, a, w, np.concatenate([bv, bg])), ref, bound)
        got = good.copy()   # wave 1 owns gated columns 48 .. 95: its pieces 2 and 3 change places
        got[:, 64:72], got[:, 72:80] = good[:, 72:80], good[:, 64:72]
        piece[epi] = R.worst(got, ref, bound)
        got = good.copy()   # the line of columns 32 .. 63 is wave 0's second half line and wave 1's first: wave 0 writes both
        got[:, 48:64] = good[:, 32:48]
        half_line[epi] = R.worst(got, ref, bound)
        # destination stride N / 32 chunks instead of N / 64: row m lands where row 2 m belongs, odd rows stay unwritten
        got = np.full_like(good, np.nan)
        got[0::2] = good[:(M + 1) // 2]
        stride[epi] = R.worst(got, ref, bound)
        stride_even[epi] = R.worst(got[2::2], ref[2::2], bound[2::2])
    report("value and gate swapped", swapped)
    report("the 16-groups off by one group", group)
    report("the bias left un-interleaved", flat_bias)
    report("an 8-column piece shifted inside a wave's 48 gated columns", piece)
    report("the half line two waves share written by one of them", half_line)
    report("destination stride N / 32 instead of N / 64 (unwritten rows: NaN)", stride)
    report("destination stride N / 32 instead of N / 64, the rows it does write", stride_even)


def test_product_slips_leave_the_bound():
    dropped, no_lo, next_tile = {}, {}, {}
    for epi in range(6):
        a, w, bias, resid, ref, bound = bars(epi)
        good = G.emulate(epi, a, w, bias, resid)
        dropped[epi] = R.worst(G.emulate(epi, a, w, bias, resid, wrap=False), ref, bound)
        no_lo[epi] = R.worst(G.emulate(epi, a, w, bias, resid, lo_terms=False), ref, bound)
        got = good.copy()
        got[3] = good[131] if epi != G.EPI_RESID else good[131] - resid[131] + resid[3]   # the product of row 128 + 3
        next_tile[epi] = R.worst(got, ref, bound)
    report("k-chunks dropped: the rotated walk does not wrap", dropped)
    report("the lo terms dropped", no_lo)
    report("a row of the next m-tile", next_tile)


def test_tanh_gelu_leaves_the_bound():
    found = {}
    for epi in (G.EPI_GELU, G.EPI_GEGLU):
        a, w, bias, resid, ref, bound = bars(epi)
        found[epi] = R.worst(G.emulate(epi, a, w, bias, resid, tanh_gelu=True), ref, bound)
    report("tanh-GELU in place of erf-GELU", found)


# ---- (c) the activation constants ----------------------------------------------------------------------------------------

def test_activation_constants_keep_their_margin():
    g = np.linspace(-6.0, 6.0, 200_001).astype(np.float32)
    g64 = g.astype(np.float64)
    nz = np.abs(g64) > 1e-6
    gel = G.act64(g64, True)
    err = np.abs(G.gelu_fast(g).astype(np.float64) - gel)
    ratio = (err / (R.GELU_CA * G.U * np.abs(gel) + R.GELU_CB * G.U * np.abs(g64) + R.UNDERFLOW)).max()
    print(f"gw_gelu emulated: err / (GELU_CA u |gelu| + GELU_CB u |g|) = {ratio:.3f} (2x margin: <= 0.5)")
    assert ratio <= 0.5
    sil = G.act64(g64, False)
    rel = np.abs(G.silu_fast(g).astype(np.float64) - sil)[nz] / (G.U * np.abs(sil[nz]))
    rest = (rel - G.SILU_W_CG * np.abs(g64[nz])).max()
    print(f"gw_silu emulated: relative error up to {rel.max():.2f} u (rows_ref.SILU_CA = {R.SILU_CA}); beyond {G.SILU_W_CG} |g| u: "
          f"{rest:.2f} u (SILU_W_CA = {G.SILU_W_CA})")
    assert 2.0 * rest <= G.SILU_W_CA
    # and the slopes the bounds carry a product's error through
    x = np.linspace(-8.0, 8.0, 400_001)
    s = 1.0 / (1.0 + np.exp(-x))
    assert round(float((s * (1.0 + x * (1.0 - s))).max()), 4) == G.SILU_SLOPE   # 1.09984, carried to four places
    dgelu = 0.5 * (1.0 + R._erf64(x[::8] / math.sqrt(2.0))) + x[::8] * np.exp(-0.5 * x[::8] ** 2) / math.sqrt(2.0 * math.pi)
    assert np.abs(dgelu).max() <= G.GELU_SLOPE
