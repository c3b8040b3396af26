"""The bar of the filter kernels' operator test must bite (CPU only; the rules themselves: tests/filter_ref.py).

tests/test_gpu_filter_kernels.py accepts a kernel's candidate set when it holds every *must* pair and no *must not* pair.
Shown here, from the f32 inputs alone:
  (a) in every case that test runs, the pairs left *free* are at most 0.1 % of all pairs and fewer than a tenth of the *must*
      pairs — the rules decide practically every pair;
  (b) a plain float32 numpy evaluation in the kernels' own order — the integer product, the f32 line of q8_threshold and >;
      f32 accumulation in 16-wide k steps and !(score <= tau - margin) — which is correct, violates nothing: the bar is not one
      that only a float64 implementation could meet;
  (c) that evaluation perturbed the way these kernels can go wrong violates at least one pair; the counts are printed.
Nothing a kernel returns enters a rule, so nothing here needs a GPU."""
import functools

import numpy as np
import pytest

from tests import filter_ref as R

DIMS = (384, 768, 1024)


@functools.lru_cache(maxsize=4)
def _restated(family, dim, n, nq, mu_random):
    case = R.Case(dim, R.Q8_RW, 1, family=family, span=n - R.ROW_LO - R.BEHIND, nq=nq, mu_random=mu_random)
    return R.Restated(case.rows(), case.queries(), mu=case.mu_in())


def _hits(case, Rs, tau):
    """The set a correct kernel returns, by float32 numpy in the kernel's order."""
    live = case.live()
    if case.int8:
        hits = np.zeros((case.n, case.nq), bool)
        hits[:Rs.a.shape[0]] = R.kernel_hits_q8(Rs.product(case.two_planes), R.q8_line32(Rs, tau, case.two_planes))
    else:
        with np.errstate(invalid="ignore"):
            hits = ~(R.f16_scores32(Rs) <= (tau - R.filter_margin(case.dim)).astype(np.float32)[None, :])
    hits[:case.lo] = False
    hits[case.hi:] = False
    hits[~live] = False
    return hits


@pytest.mark.parametrize("dim", DIMS)
def test_free_set_cap_and_float32_in_the_kernels_order(dim):
    """(a) and (b), on every case of the GPU test (cases that share rows, queries, tau and operand form share the masks)."""
    done = {}
    worst = (0, 0, 1)
    for case in R.gpu_cases(dim):
        if case.kernel == R.NONE:
            continue
        key = (case.family, case.n, case.nq, case.int8, case.two_planes, case.dead, case.mu_random, case.cap < case.span)
        if key in done:
            continue
        Rs = _restated(case.family, dim, case.n, case.nq, case.mu_random)
        tau = case.tau()
        safety, tight = R.case_masks(case, Rs)
        ok, (free, must, pairs) = R.free_cap_holds(tight, case.lo, case.hi, case.nq)
        assert ok, (case.id, free, must, pairs)
        if free * worst[2] > worst[0] * pairs:
            worst = (free, must, pairs)
        # the two rules never contradict each other: what safety demands, tightness does not forbid
        assert not (safety.must & tight.mustnot).any(), case.id
        hits = _hits(case, Rs, tau)
        assert safety.violations(hits) == 0 and tight.violations(hits) == 0, (case.id, safety.violations(hits), tight.violations(hits))
        done[key] = True
    print(f"dim {dim}: {len(done)} distinct references; largest free share {worst[0]} of {worst[2]} pairs ({worst[1]} must)")


@pytest.mark.parametrize("dim", DIMS)
def test_perturbed_kernels_violate_the_rules(dim):
    """(c): each perturbation on 1,152 rows in range (nine tiles: an odd count), 33 queries, every 7th row dead."""
    found = {}
    for family in ("normal", "adversarial"):
        one = R.Case(dim, R.Q8_RW, 1, family=family, span=1152, nq=33, dead=True)
        two = R.Case(dim, R.Q8_RW2, 1, family=family, span=1152, nq=33, dead=True)
        Rs = _restated(family, dim, one.n, one.nq, False)
        tau, live = one.tau(), one.live()
        lo, hi = one.lo, one.hi
        _, tight1 = R.case_masks(one, Rs)
        safety, tight2 = R.case_masks(two, Rs)

        def both(hits, tight=tight1):
            h = np.zeros((one.n, one.nq), bool)
            h[:hits.shape[0]] = hits
            h[:lo] = False
            h[hi:] = False
            return safety.violations(h) + tight.violations(h)

        def masked(hits):
            hits = hits.copy()
            hits[~live[:hits.shape[0]]] = False
            return hits

        I = Rs.product(False)
        T = R.q8_line32(Rs, tau, False)
        base = masked(R.kernel_hits_q8(I, T))
        assert both(base) == 0
        out = {}
        short = Rs.a[:, :dim - 128] @ Rs.b[:, :dim - 128].T
        out["the last k-chunk never multiplied"] = both(masked(R.kernel_hits_q8(short, T)))
        # the tile whose scale differs most from its neighbour's
        inv = Rs.tmeta[lo // 128:hi // 128, 0]
        with np.errstate(invalid="ignore"):
            ratio = np.abs(np.log(inv[1:] / inv[:-1]))
        t = lo // 128 + int(np.nanargmax(np.where(np.isfinite(ratio), ratio, -1)))
        swapped = Rs.tmeta.copy()
        swapped[t] = Rs.tmeta[t + 1]
        Rsw = _shallow(Rs, tmeta=swapped)
        out["one tile's tmeta taken from its neighbour"] = both(masked(R.kernel_hits_q8(I, R.q8_line32(Rsw, tau, False))))
        I2hi = 128.0 * (Rs.a @ Rs.hi.T)
        out["the lo plane dropped"] = both(masked(R.kernel_hits_q8(I2hi, R.q8_line32(Rs, tau, True))), tight2)
        perm = np.arange(base.shape[0])
        r = perm % 32
        perm = np.where(r % 8 < 4, perm + 4, perm - 4)
        out["rows r and r + 4 of a 32-row fragment exchanged"] = both(base[perm])
        skipped = base.copy()
        skipped[hi - 128:hi] = False
        out["the last 128-row tile of an odd tile count skipped"] = both(skipped)
        wrongq = Rs.q1.copy()
        wrongq[32] = Rs.q1[0]
        tau_w = tau.copy()
        tau_w[32] = tau[0]
        out["query 32 nqt scored with query 0's constants"] = both(masked(R.kernel_hits_q8(I, R.q8_line32(_shallow(Rs, q1=wrongq), tau_w, False))))
        h = np.zeros((one.n, one.nq), bool)
        h[:base.shape[0]] = masked(R.kernel_hits_q8(I, R.q8_line32(Rs, tau, False, l1_only=True)))
        h[:lo] = False
        h[hi:] = False
        assert safety.violations(h) == 0          # a wider band drops nothing ...
        out["the band's L1 side only (tightness)"] = tight1.violations(h)   # ... and passes what the line forbids
        unmasked = R.kernel_hits_q8(I, T)
        out["a dead bit ignored"] = both(unmasked)
        found[family] = out
    for what in found["normal"]:
        line = {fam: found[fam][what] for fam in found}
        print(f"dim {dim}, {what}: " + ", ".join(f"{fam} {v} pairs violated" for fam, v in line.items()))
        assert min(line.values()) > 0, (what, line)


def _shallow(Rs, **changed):
    import copy

    c = copy.copy(Rs)
    for k, v in changed.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("dim", DIMS)
def test_perturbed_f16_kernels_violate_the_rules(dim):
    """The same for the f16 operands: a k-chunk never multiplied, exchanged fragment rows, a skipped last tile, a dead bit."""
    case = R.Case(dim, R.F16_RW, 1, span=1152, nq=33, dead=True)
    Rs = _restated("normal", dim, case.n, case.nq, False)
    tau, live = case.tau(), case.live()
    safety, tight = R.case_masks(case, Rs)
    thr = (tau - R.filter_margin(dim)).astype(np.float32)[None, :]

    def viol(hits, dead_masked=True):
        h = hits.copy()
        h[:case.lo] = False
        h[case.hi:] = False
        if dead_masked:
            h[~live] = False
        return safety.violations(h) + tight.violations(h)

    with np.errstate(invalid="ignore"):
        base = ~(R.f16_scores32(Rs) <= thr)
        short = ~((Rs.rows_h[:, :dim - 64].astype(np.float64) @ Rs.q_h[:, :dim - 64].astype(np.float64).T).astype(np.float32) <= thr)
    assert viol(base) == 0
    perm = np.arange(case.n)
    perm = np.where((perm % 32) % 8 < 4, perm + 4, perm - 4)
    skipped = base.copy()
    skipped[case.hi - 128:case.hi] = False
    out = {"the last k-chunk never multiplied": viol(short), "rows r and r + 4 of a 32-row fragment exchanged": viol(base[perm]),
           "the last 128-row tile skipped": viol(skipped), "a dead bit ignored": viol(base, dead_masked=False)}
    for what, v in out.items():
        print(f"dim {dim}, f16, {what}: {v} pairs violated")
        assert v > 0, what


def test_the_families_reach_what_they_claim():
    rows = R.make_rows("adversarial", 384, R.ROW_LO + 1152 + R.BEHIND)
    Rs = R.Restated(rows, R.make_queries("adversarial", 384, rows.shape[0], 33))
    t = R.NAN_ROWS[0] // 128
    assert Rs.flagged[t] and not Rs.flagged[t - 1] and not Rs.flagged[t + 1] and Rs.flagged.sum() == 1
    assert np.isnan(Rs.tmeta[t, 0])
    assert (rows[R.ROW_LO + 20] == 0).all() and (Rs.a[R.ROW_LO + 20] == np.rint(-Rs.mu * Rs.tmeta[(R.ROW_LO + 20) // 128, 0])).all()
    # the outlier coordinate collapses its tile's scale: rows of that tile use a fraction of the int8 range
    assert Rs.q1[3, 0] == 1 and not Rs.b[3].any()          # the zero query: inv = 1, all-zero bytes
    assert np.abs(Rs.b[1]).sum() == 127                      # the one-hot query
    cos = R.cosines64(rows, R.make_queries("adversarial", 384, rows.shape[0], 33))
    dup = cos[R.DUP_TILE:R.DUP_TILE + 128, 0]
    assert dup.min() > 0.999                                 # a tile of near-duplicates of query 0
    # tau = +inf takes no row and tau = -inf every live row, by both rules
    case = R.Case(384, R.Q8_RW, 2, span=384, nq=33)
    Rn = R.Restated(case.rows(), case.queries())
    safety, tight = R.case_masks(case, Rn)
    tau = case.tau()
    assert tau[5] == -np.inf and tau[6] == np.inf
    assert tight.must[case.lo:case.hi, 5].all() and tight.mustnot[case.lo:case.hi, 6].all() and not safety.must[:, 6].any()
