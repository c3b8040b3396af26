"""The kernels of csrc/scan_filter.hip alone — the nine filter kernels in all thirty instantiations of filter_insts<J>(), the
quantiser of the int8 copy (corpus_q8_kernel), the f16 copy's builder (unit_f16_rows_kernel), the mean-row kernels,
prep_queries_kernel and tail_candidates_kernel — each through ONE cs_debug_filter call on at most 5,120 + 1,152 rows, against
numpy (tests/filter_ref.py: float64 cosines, the restated quantiser, the decision rules; tests/test_filter_bar.py shows that the
rules bite and that a correct float32 evaluation meets them).

The searches of tests/test_gpu_filter_int8.py and its scoped / similar variants compare the final top k, which the exact
refine keeps right whatever a filter lets through and which shows a dropped row only when it belongs in some top k.  Here the
SET a kernel returns is checked: it holds every *must* pair (float64 cosine >= tau; above the kernel's own line), no *must not*
pair (below the line, dead, outside the rows, beyond nq), no duplicate; the counters equal the sets' sizes, the padded
queries' stay zero, and no guard word changes."""
import ctypes as C

import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd._lib import f32p, u32p
from tests import filter_ref as R

pytestmark = pytest.mark.gpu

DIMS = (384, 768, 1024)
i8p, u16p = C.POINTER(C.c_int8), C.POINTER(C.c_uint16)


def run_filter(lib, dim, rows, queries, tau, kernel, nqt, lo, hi, cap, grid=0, dead=None, mu_in=None, tail=(0, 0), copies=False):
    n, nq = rows.shape[0], queries.shape[0]
    n8 = n // 128 * 128
    out = {"norms": np.empty(n, np.float32), "mu": np.empty(dim, np.float32), "qmag": np.empty(nq, np.float32),
           "cnt": np.empty(nq + R.CNT_PAD, np.uint32), "cand": np.empty((nq, cap), np.uint32)}
    if copies:
        out.update(f16=np.empty((n, dim), np.uint16), q8=np.empty((n8, dim), np.int8), tmeta=np.empty((n8 // 128, 4), np.float32),
                   qunit=np.empty((nq, dim), np.uint16), q8q=np.empty((nq, dim), np.int8), hi=np.empty((nq, dim), np.int8),
                   lo=np.empty((nq, dim), np.int8), qmeta=np.empty((4 * nq, 4), np.float32))
    guard = C.c_uint32(0xffffffff)
    p = lambda a, t=f32p: None if a is None else a.ctypes.data_as(t)
    g = lambda name, t=f32p: p(out.get(name), t)
    rows, queries, tau = np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(queries, np.float32), np.ascontiguousarray(tau, np.float32)
    _lib.check_diag(lib.cs_debug_filter(0, dim, p(rows), n, p(queries), nq, p(tau), p(dead, u32p), p(mu_in), kernel, nqt, lo, hi, cap, grid,
                                        tail[0], tail[1], g("norms"), g("mu"), g("f16", u16p), g("q8", i8p), g("tmeta"),
                                        g("qunit", u16p), g("q8q", i8p), g("hi", i8p), g("lo", i8p), g("qmeta"), g("qmag"),
                                        g("cnt", u32p), g("cand", u32p), C.byref(guard)))
    out["guard_changed"] = guard.value
    return out


def check_inputs(rows, queries, out, mu_given):
    """What the restatement takes from the launch — norms, magnitudes, mu — against float64 first.  Norms: an f32 sum of dim
    squares in any order is within dim 2^-24 of the sum, relatively; its root within half of that, plus the root's own rounding."""
    dim = rows.shape[1]
    _, nr, ok = R.unit64(rows)
    bound = (dim / 2 + 1) * 2.0 ** -24
    assert (np.abs(out["norms"][ok] - nr[ok]) <= bound * nr[ok]).all()
    assert (out["norms"][nr == 0] == 0).all()
    _, qn, qok = R.unit64(queries)
    assert (np.abs(out["qmag"][qok] - qn[qok]) <= 2.0 ** -22 * qn[qok]).all() and (out["qmag"][qn == 0] == 0).all()
    if not mu_given:   # zero and non-finite rows count as zero rows
        assert np.abs(out["mu"] - R.mean_unit_row64(rows)).max() <= 1e-6


def sets_of(out, nq, cap, n):
    """hits [n, nq] from the returned slots; no duplicate, no row that is not stored; the padded queries' counters zero."""
    hits = np.zeros((n, nq), bool)
    cnt = out["cnt"]
    assert (cnt[nq:] == 0).all(), np.flatnonzero(cnt[nq:])[:4]
    for q in range(nq):
        used = min(int(cnt[q]), cap)
        got = out["cand"][q, :used]
        assert (got < n).all(), (q, got[got >= n][:4])
        assert len(np.unique(got)) == used, ("duplicates", q)
        hits[got, q] = True
        assert (out["cand"][q, used:] == R.GUARD_WORD).all()
    return hits, cnt[:nq].astype(np.int64)


def run_case(lib, case, copies=False):
    rows, queries, tau = case.rows(), case.queries(), case.tau()
    dead = R.dead_words(case.dead_rows(), case.n) if case.dead else None
    tail = (case.hi, case.hi + case.tail) if case.tail else (0, 0)
    mu_in = case.mu_in()
    out = run_filter(lib, case.dim, rows, queries, tau, case.kernel, case.nqt, case.lo, case.hi, case.cap, case.grid(), dead, mu_in,
                     tail, copies)
    check_inputs(rows, queries, out, mu_in is not None)
    if mu_in is not None:
        assert np.array_equal(out["mu"], mu_in)
    return out


def check_case(lib, case):
    """One launch: safety and tightness of every query's set, counters, guards -> (must pairs, free pairs)."""
    out = run_case(lib, case)
    rows, queries, tau, live = case.rows(), case.queries(), case.tau(), case.live()
    Rs = R.Restated(rows, queries, mu=out["mu"], norms=out["norms"], qmag=out["qmag"])
    safety, tight = R.case_masks(case, Rs)
    if case.tail:   # the rows behind row_hi handed to tail_candidates_kernel: every live one, for every query, once
        for m in (safety, tight):
            m.must[case.hi:case.hi + case.tail] = live[case.hi:case.hi + case.tail, None]
            m.mustnot[case.hi:case.hi + case.tail] = ~live[case.hi:case.hi + case.tail, None]
    hits, cnt = sets_of(out, case.nq, case.cap, case.n)
    assert out["guard_changed"] == 0, (case.id, out["guard_changed"])
    over = cnt > case.cap
    n_live = live[case.lo:case.hi].sum() * (case.kernel != R.NONE) + live[case.hi:case.hi + case.tail].sum()
    if case.kernel != R.NONE:   # tau = -inf: the counter is the number of live rows in range, whatever the buffer holds
        assert (cnt[tau == -np.inf] == n_live).all(), (case.id, cnt[tau == -np.inf], n_live)
    if case.cap < case.span:
        q = min(1, case.nq - 1)   # ... of which an overflowed buffer keeps the first `cap`, distinct, live and in range
        assert tau[q] == -np.inf and over[q] and not over.all(), (case.id, cnt[q])
        assert (hits.sum(axis=0)[over] == case.cap).all()
    else:
        assert not over.any(), (case.id, cnt.max())
    assert (hits.sum(axis=0)[~over] == cnt[~over]).all()
    for name, m in (("safety", safety), ("tightness", tight)):
        miss = m.must & ~hits
        miss[:, over] = False          # an overflowed query keeps `cap` of its rows
        extra = m.mustnot & hits
        assert not miss.any() and not extra.any(), (case.id, name, "missing", np.argwhere(miss)[:4].tolist(), "extra", np.argwhere(extra)[:4].tolist())
    return int(tight.must.sum()), int(tight.free.sum())


def _insts():
    return [pytest.param(dim, k, nqt, id=f"{dim}-{R.KERNEL_NAMES[k]}{nqt or ''}") for dim in DIMS for k, nqt in R.INSTS[dim]]


@pytest.mark.parametrize("dim,kernel,nqt", _insts())
def test_candidate_sets(diag_lib, dim, kernel, nqt):
    """Every case of tests/filter_ref.py gpu_cases for this instantiation: row spans of 128 / 384 / 1,152 / 5,120 rows (f16:
    also 1,000) from row 1,024 with rows below and behind; the plan's grid, the smallest legal one (five tiles per block at 5,120
    rows) and one with idle blocks; the query counts around a query tile; tombstones; a 64-slot buffer that overflows for one
    query; a tail; the other two families on one instantiation of each kernel; a test-chosen mu."""
    cases = [c for c in R.gpu_cases(dim) if (c.kernel, c.nqt) == (kernel, nqt)]
    assert len(cases) >= 16
    must = free = 0
    for case in cases:
        m, f = check_case(diag_lib, case)
        must, free = must + m, free + f
    print(f"{dim} {R.KERNEL_NAMES[kernel]} nqt {nqt}: {len(cases)} launches, {must} must pairs, {free} free pairs")


@pytest.mark.parametrize("dim", DIMS)
def test_tail_alone(diag_lib, dim):
    """tail_candidates_kernel with no filter launch in front: 1, 77 and 127 rows, every query gets exactly the live ones."""
    cases = [c for c in R.gpu_cases(dim) if c.kernel == R.NONE]
    assert [c.tail for c in cases] == [1, 77, 127]
    for case in cases:
        check_case(diag_lib, case)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("dim", DIMS)
def test_quantiser_copies_and_queries(diag_lib, dim, family):
    """corpus_q8_kernel, unit_f16_rows_kernel, unit_mean_kernel + mean_finish_kernel and prep_queries_kernel against the
    restatement tests/test_filter_int8_bound.py proves the band for, on the read-back norms, mu and magnitudes."""
    case = R.Case(dim, R.Q8_RW, 1, family=family, span=1152, nq=33)
    rows, queries = case.rows(), case.queries()
    out = run_case(diag_lib, case, copies=True)
    Rs = R.Restated(rows, queries, mu=out["mu"], norms=out["norms"], qmag=out["qmag"])
    tiles = case.n // 128
    good = np.repeat(~Rs.flagged, 128)
    # the int8 bytes: the restatement's, but where the restated product lies within 4 ulps of a rounding tie (at most 1e-4 of them)
    t = Rs.t_f32[good].astype(np.float64)
    near_tie = np.abs(np.abs(t - np.floor(t)) - 0.5) <= 4 * np.spacing(np.abs(Rs.t_f32[good]).astype(np.float32))
    assert near_tie.mean() <= 1e-4
    differ = out["q8"][good].astype(np.float64) != Rs.a[good]
    assert not (differ & ~near_tie).any(), np.argwhere(differ & ~near_tie)[:4]
    tm = out["tmeta"]
    assert np.array_equal(np.isnan(tm[:, 0]), Rs.flagged)           # a tile with a non-finite element, and not its neighbours
    assert Rs.flagged.sum() == (1 if family == "adversarial" else 0)
    ok = ~Rs.flagged
    assert np.array_equal(tm[ok, 0], Rs.tmeta[ok, 0]) and np.array_equal(tm[ok, 1], Rs.tmeta[ok, 1])   # inv_t, 0.5001 B_t: exact
    for ti in np.flatnonzero(ok):
        r = slice(128 * ti, 128 * ti + 128)
        e64 = np.sqrt(((Rs.t_f32[r].astype(np.float64) - Rs.a[r]) ** 2).sum(axis=1).max())
        n64 = np.sqrt((Rs.a[r] ** 2).sum(axis=1).max())
        assert e64 <= tm[ti, 2] <= e64 * (1 + 2e-3) + 2e-3, (ti, e64, tm[ti, 2])
        assert n64 <= tm[ti, 3] <= n64 * (1 + 2e-3) + 2e-3, (ti, n64, tm[ti, 3])
    # the f16 copy: f16(v / norm) bit for bit, subnormals kept, zero-norm rows zero
    fin = np.isfinite(rows).all(axis=1)
    assert np.array_equal(out["f16"][fin], Rs.rows_h[fin].view(np.uint16))
    zero = np.flatnonzero(out["norms"] == 0)
    assert (out["f16"][zero] == 0).all() and (len(zero) > 0) == (family == "adversarial")
    if family == "adversarial":
        sub = Rs.rows_h[fin].view(np.uint16) & 0x7fff
        assert ((sub > 0) & (sub < 0x0400)).any()                     # f16 subnormals are among the values compared
    assert np.array_equal(out["qunit"], Rs.q_h.view(np.uint16))
    # the query side
    nq = case.nq
    qm = out["qmeta"]
    assert np.array_equal(out["q8q"].astype(np.float64), Rs.b)
    assert np.array_equal(qm[:nq, 0], Rs.q1[:, 0]) and np.array_equal(qm[:nq, 1], Rs.q1[:, 1])
    B = 128.0 * out["hi"].astype(np.float64) + out["lo"]
    assert np.array_equal(B, 128.0 * Rs.hi + Rs.lo) and np.abs(out["hi"].astype(int)).max() <= 127 and np.abs(out["lo"].astype(int)).max() <= 64
    assert np.array_equal(qm[2 * nq:3 * nq, 0], Rs.q2[:, 0])
    assert np.abs(qm[2 * nq:3 * nq, 1] - Rs.q2[:, 1]).max() <= 1e-6 * Rs.q2[:, 1].max()
    uq = np.where(Rs.qmag[:, None] == 0, 0, queries / np.where(Rs.qmag == 0, 1, Rs.qmag)[:, None]).astype(np.float32).astype(np.float64)
    for base, b, inv in ((0, Rs.b, Rs.q1[:, 0]), (2 * nq, 128.0 * Rs.hi + Rs.lo, Rs.q2[:, 0])):
        tq = (uq.astype(np.float32) * inv[:, None]).astype(np.float32).astype(np.float64)
        nb64, dq64 = np.sqrt((b * b).sum(axis=1)), np.sqrt(((tq - b) ** 2).sum(axis=1))
        nb, dq = qm[base:base + nq, 3], qm[base + nq:base + 2 * nq, 0]
        assert (nb64 <= nb).all() and (nb <= nb64 * (1 + 2e-3) + 2e-3).all()
        assert (dq64 <= dq).all() and (dq <= dq64 * (1 + 2e-3) + 2e-3).all()
        assert np.abs(qm[base:base + nq, 2] - uq @ out["mu"].astype(np.float64)).max() <= dim * 2.0 ** -23
    assert qm[3, 0] == 1 and not out["q8q"][3].any() and not out["hi"][3].any() and not out["lo"][3].any()   # the zero query


def test_any_mu_keeps_the_filter_exact(diag_lib):
    """A second run with a test-chosen mu (a random vector of norm 0.5): every safety assertion holds (gpu_cases runs it on one
    instantiation of each int8 kernel per dim; here on the adversarial rows too)."""
    for dim in DIMS:
        k, nqt = next((k, n) for k, n in R.INSTS[dim] if k == R.Q8_RW)
        check_case(diag_lib, R.Case(dim, k, nqt, family="adversarial", span=1152, nq=33, mu_random=True, dead=True))


@pytest.mark.parametrize("dim", DIMS)
def test_same_bytes_same_set(diag_lib, dim):
    """The one-plane int8 kernels share q8_threshold and exact integers: on the same operands (mu handed in) and tau they return
    the same sets, free pairs included.  The f16 kernels accumulate in different orders: the same sets outside *free*."""
    span, nq = 1152, 257
    base = R.Case(dim, R.Q8_RW, 1, span=span, nq=nq)
    rows, queries, tau = base.rows(), base.queries(), base.tau()
    mu = R.mean_unit_row64(rows).astype(np.float32)
    got = {}
    for k, nqt in R.INSTS[dim]:
        if k == R.Q8_RW2:
            continue
        out = run_filter(diag_lib, dim, rows, queries, tau, k, nqt, base.lo, base.hi, base.cap, mu_in=mu)
        hits, _ = sets_of(out, nq, base.cap, base.n)
        got[(k, nqt)] = (hits, out)
    i8 = [v for (k, _), v in got.items() if k in R.INT8]
    assert len(i8) >= 2
    for hits, _ in i8[1:]:
        assert np.array_equal(hits, i8[0][0])
    f16 = [v for (k, _), v in got.items() if k not in R.INT8]
    assert len(f16) >= 3
    out = f16[0][1]
    free = R.f16_masks(R.Restated(rows, queries, mu=mu, norms=out["norms"], qmag=out["qmag"]), tau, base.lo, base.hi, base.live()).free
    for hits, _ in f16[1:]:
        assert np.array_equal(hits & ~free, f16[0][0] & ~free)


def test_bad_arguments_are_the_launchers(diag_lib):
    rows, queries = R.make_rows("normal", 768, 1280), R.make_queries("normal", 768, 1280, 65)
    tau = np.zeros(65, np.float32)

    def refused(kernel, nqt, lo, hi, grid=0):
        with pytest.raises(_lib.CsError) as e:
            run_filter(diag_lib, 768, rows, queries, tau, kernel, nqt, lo, hi, 64, grid)
        assert e.value.code == _lib.CS_ERR_BAD_ARG, str(e.value)

    refused(R.Q8_RQ, 8, 1024, 1152)          # not in filter_insts<6>()
    refused(R.Q8_RW, 8, 1024, 1152)
    refused(R.F16_RW, 4, 1024, 1152)
    refused(R.Q8_RW, 2, 1000, 1152)          # row_lo off a tile
    refused(R.F16_RW, 2, 1000, 1152)
    refused(R.Q8_RW, 2, 1024, 1100)          # an int8 row_hi off a tile
    refused(R.Q8_RW, 1, 1024, 1152, grid=20)  # a resident-query grid: a multiple of 8 ...
    refused(R.Q8_RW, 1, 1024, 1152, grid=16)  # ... and 8 per query tile (65 queries: three tiles of 32)
    refused(R.F16_RW, 1, 1024, 1152, grid=16)
    out = run_filter(diag_lib, 768, rows, queries, tau, R.F16_RW, 2, 1024, 1100, 256)   # the f16 kernels mask a partial tile
    assert out["guard_changed"] == 0
