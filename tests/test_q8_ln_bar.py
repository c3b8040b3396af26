"""The bar of the LayerNorm-fused quantised product's operator test must bite (CPU only; the bar itself: tests/q8_ln_ref.py).

tests/test_gpu_q8_ln.py accepts gemm_q8_ln_kernel when |got - ref| <= bound.  Shown here, on the input families that test
uses:
  (a) a plain float32 numpy evaluation in the kernel's own order — which is correct — stays inside the bound on every
      family, weight form, K and eps, so the bar is not one that only a float64 implementation could meet;
  (b) the reference perturbed the way this kernel can go wrong — a flipped activation bit, a zero-point correction off by
      one, a column-metadata tile taken from its neighbour, a last K stage never multiplied, a weight fragment read before it
      landed — leaves the bound; the factor by which it leaves is printed.
Nothing a kernel returns enters a bound, so nothing here needs a GPU."""
import numpy as np
import pytest

from tests import q8_ln_ref as Q
from tests import rows_ref as R

T = 7
EPS = (1e-12, 1e-5)
KS = (384, 1536)


def sources_of(K):
    return [s for s, k in Q.SOURCES if k == K]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("family", Q.FAMILIES)
def test_float32_in_the_kernels_order_meets_the_bar(family, K):
    worst = 0.0
    for kind in Q.WEIGHT_KINDS:
        case = Q.make_case(family, T, K, kind)
        for source in sources_of(K):
            quant = Q.quantized(case, source)
            for eps in EPS:
                ref = Q.reference(case, source, eps, quant)
                got = Q.kernel_order_f32(ref["v"], case["gamma"], case["beta"], eps)
                ratio = R.worst(got, ref["ref"], ref["bound"])
                print(f"q8 LayerNorm product {family} K {K} {source} {kind} eps {eps:g}: float32 in the kernel's order err/bound = {ratio:.3f}")
                assert ratio <= 1.0
                worst = max(worst, ratio)
                if family == "zero":   # variance 0: the reference IS beta
                    assert np.array_equal(ref["ref"], np.broadcast_to(case["beta"].astype(np.float64), ref["ref"].shape))
    print(f"q8 LayerNorm product {family} K {K}: worst err/bound = {worst:.3f}")


def test_the_families_reach_what_they_claim():
    for K in KS:
        case = Q.make_case("extreme", T, K, "per-channel unsigned")
        q, xs, xz, acc = Q.quantized(case, "prequant")
        assert set(np.unique(q)) == {0, 255} and xz == 1
        rows = (q.astype(np.int64) - xz).sum(axis=1)
        assert rows.max() == 254 * K and rows.min() == -K and np.abs(rows).max() < 2 ** 23
        d = case["d"]
        assert d[0::3].min() >= 0 and d[1::3].max() <= 0 and d[2::3].min() < 0 < d[2::3].max()
        assert np.abs(acc).max() < 2 ** 31
        # the kernel's stored forms: b = d - (dmin + 128) in [-128, 127], column sums below 2^23 in magnitude
        b = d - (d.min(axis=1, keepdims=True) + 128)
        assert b.min() >= -128 and b.max() <= 127 and np.abs(b.sum(axis=1)).max() <= 128 * K < 2 ** 23
        assert np.abs(b.sum(axis=1)).max() > 100 * K                     # near the widest
        case = Q.make_case("ties", T, K, "per-channel unsigned")
        q, xs, xz, _ = Q.quantized(case, "prequant")
        assert xs == np.float32(2.0 ** -5) and xz == 64
        t = case["A"].astype(np.float64) * 32.0
        assert 0.4 < (np.abs(t - np.floor(t) - 0.5) == 0).mean() < 0.6    # half the values sit on a rounding tie
        case = Q.make_case("zero", T, K, "per-tensor unsigned")
        q, xs, xz, acc = Q.quantized(case, "prequant")
        assert xs == 1 and xz == 0 and not q.any() and not acc.any()


@pytest.mark.parametrize("K", KS)
def test_perturbed_references_leave_the_bound(K):
    """Each on the normal family, 7 rows, per-channel weights (a per-tensor weight has one scale: its tiles cannot differ)."""
    found = {}
    for kind in ("per-channel unsigned", "per-channel signed"):
        case = Q.make_case("normal", T, K, kind)
        source = sources_of(K)[0]
        q, xs, xz, acc = Q.quantized(case, source)
        base = Q.reference(case, source, 1e-5, (q, xs, xz, acc))

        def factor(q_=q, xz_=xz, d_=case["d"], sc_=case["sc"], acc_=None):
            acc2 = Q.integer_product(q_, xz_, d_) if acc_ is None else acc_
            v = Q.pre_ln_rows(acc2, xs, sc_, case["bias"], case["resid"])
            pert = R.layernorm_ref(v, case["gamma"], case["beta"], 1e-5, counts=Q.LN_COUNTS)[0]
            return R.worst(pert, base["ref"], base["bound"])

        q1 = q.copy()
        q1[3, 17] ^= 1
        sc1 = case["sc"].copy()
        sc1[16:32] = case["sc"][32:48]
        d1 = case["d"].copy()
        d1[100, K - 1] += 1
        a = q.astype(np.float64) - xz
        short = (a[:, :K - 64] @ case["d"][:, :K - 64].astype(np.float64).T).astype(np.int64)
        found[kind] = {"one activation byte flipped in its lowest bit": factor(q_=q1),
                       "the activations' zero point off by one": factor(xz_=xz + 1),
                       "one 16-column tile's scales taken from its neighbour": factor(sc_=sc1),
                       "the last 64-column K stage never multiplied": factor(acc_=short),
                       "one weight integer off by one": factor(d_=d1)}
    for what in found["per-channel unsigned"]:
        line = {kind: found[kind][what] for kind in found}
        print(f"K {K}, {what}: " + ", ".join(f"{k} {v:.3g}x" for k, v in line.items()))
        assert min(line.values()) > 1.0, (what, line)
