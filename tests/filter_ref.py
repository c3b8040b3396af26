"""References and decision rules for the filter kernels of codesearch_amd/csrc/scan_filter.hip run alone
(tests/test_gpu_filter_kernels.py through cs_debug_filter; that the rules bite: tests/test_filter_bar.py).

A filter kernel returns, per query, a SET of rows.  What the set must be is decided here from the f32 inputs alone:
  safety     a row whose float64 cosine is >= tau is in the set — else a search could return a wrong top k;
  tightness  the set is the one the kernel's own arithmetic defines: the exact integer product against the line of
             q8_threshold evaluated in float64 (int8 kernels), or the float64 product of the f16 operands against tau - margin
             (f16 kernels) — else the filter does needless work, or the proof in tests/test_filter_int8_bound.py is about a
             different quantiser.
Every rule returns three masks over (row, query): must, must not, free (the few pairs within the rounding of the kernel's own
f32 evaluation of the line).  Nothing a kernel returns enters a mask: the quantiser is restated in numpy (the functions
below, which tests/test_filter_int8_bound.py proves the band for) from the f32 rows, the norms, mu and the query magnitudes
— numpy's own on the CPU; on the GPU the read-back ones, each checked against float64 first."""
import functools

import numpy as np

F = np.float32

# cs::FilterKernel (csrc/filter_plan.hpp)
NONE, Q8_TILE256, Q8_RQ, Q8_RQ1, Q8_RW, Q8_RW2, F16_RW, F16_TILE256, F16_TILE128 = range(9)
KERNEL_NAMES = {NONE: "None", Q8_TILE256: "Q8Tile256", Q8_RQ: "Q8Rq", Q8_RQ1: "Q8Rq1", Q8_RW: "Q8Rw", Q8_RW2: "Q8Rw2",
                F16_RW: "F16Rw", F16_TILE256: "F16Tile256", F16_TILE128: "F16Tile128"}
INT8 = (Q8_TILE256, Q8_RQ, Q8_RQ1, Q8_RW, Q8_RW2)
RESIDENT = (Q8_RQ, Q8_RQ1, Q8_RW, Q8_RW2, F16_RW)
# filter_insts<dim / 128>() (scan_filter.hip): every (kernel, 32-query groups per query tile) that is built
INSTS = {
    384: [(F16_TILE128, 0), (F16_TILE256, 0), (Q8_TILE256, 0), (F16_RW, 1), (F16_RW, 2), (F16_RW, 4), (Q8_RW, 1), (Q8_RW, 2),
          (Q8_RW, 4), (Q8_RW, 8), (Q8_RW2, 1), (Q8_RW2, 2), (Q8_RQ, 8), (Q8_RQ1, 8)],
    768: [(F16_TILE128, 0), (F16_TILE256, 0), (Q8_TILE256, 0), (F16_RW, 1), (F16_RW, 2), (Q8_RW, 1), (Q8_RW, 2), (Q8_RW, 4),
          (Q8_RW2, 1), (Q8_RW2, 2)],
    1024: [(F16_TILE128, 0), (F16_TILE256, 0), (Q8_TILE256, 0), (F16_RW, 1), (Q8_RW, 1), (Q8_RW, 2)],
}
assert sum(len(v) for v in INSTS.values()) == 30
ROW_LO = 1024          # rows below it exist and may never appear
BEHIND = 128           # ... as the rows behind row_hi
CNT_PAD = 256          # CS_DEBUG_FILTER_CNT_PAD
GUARD_WORD = 0xA5A5A5A5


# ---- the quantiser, restated step by step in float32 (corpus_q8_kernel, prep_queries_kernel) -------------------------------
def _quantise_tile(rows, mu, nrm=None):
    """rows: [128, dim] f32 -> (a int8-valued f32, inv_t, hB, E, N) as corpus_q8_kernel.  nrm: the rows' f32 norms as
    launch_row_norms left them (default: numpy's own f32 sum)."""
    if nrm is None:
        nrm = np.sqrt((rows.astype(F) ** 2).sum(axis=1, dtype=F)).astype(F)
    u = np.where(nrm[:, None] == 0, F(0), rows / np.where(nrm == 0, F(1), nrm)[:, None]).astype(F) - mu
    mx = np.abs(u).max()
    inv = F(127.0) / mx if mx > 0 else F(1.0)
    t = (u * inv).astype(F)
    a = np.clip(np.rint(t), -127, 127).astype(F)
    hB = F(0.5001) * np.abs(a).sum(axis=1).max()
    E = F(np.sqrt(((t - a) ** 2).sum(axis=1, dtype=F).max())) * F(1.001) + F(1e-3)
    N = F(np.sqrt((a * a).sum(axis=1, dtype=F).max())) * F(1.0001)
    return a, inv, hB, E, N


def _quantise_query(q, mu, m=None):
    """m: the query's f32 magnitude as prep_queries_kernel left it (default: numpy's own f32 sum)."""
    if m is None:
        m = F(np.sqrt((q.astype(F) ** 2).sum(dtype=F)))
    v = (q / m).astype(F) if m > 0 else np.zeros_like(q, F)
    mx = np.abs(v).max()
    inv = F(127.0) / mx if (mx > 0 and np.isfinite(mx)) else F(1.0)
    t = (v * inv).astype(F)
    b = np.clip(np.rint(t), -127, 127).astype(F)
    return (b, inv, F(0.5001) * np.abs(b).sum(), F(np.sqrt((b * b).sum(dtype=F))) * F(1.0001),
            F(np.sqrt(((t - b) ** 2).sum(dtype=F))) * F(1.001) + F(1e-3), F((v * mu).sum(dtype=F)))


def _quantise_query_two_planes(q, mu, m=None):
    """prep_queries_kernel's second quantisation: B = rint(v * 128 inv) = 128 hi + lo; the MFMAs compute a . hi and a . lo."""
    if m is None:
        m = F(np.sqrt((q.astype(F) ** 2).sum(dtype=F)))
    v = (q / m).astype(F) if m > 0 else np.zeros_like(q, F)
    mx = np.abs(v).max()
    inv = (F(127.0) / mx if (mx > 0 and np.isfinite(mx)) else F(1.0)) * F(128.0)
    t = (v * inv).astype(F)
    B = np.clip(np.rint(t), -16256, 16256).astype(F)
    hi = np.rint(B * F(0.0078125)).astype(F)
    lo = (B - F(128.0) * hi).astype(F)
    assert np.abs(hi).max() <= 127 and np.abs(lo).max() <= 64
    return (hi, lo, inv, F(0.5001) * np.abs(B).sum(dtype=F) * F(1.0001), F(np.sqrt((B * B).sum(dtype=F))) * F(1.0001),
            F(np.sqrt(((t - B) ** 2).sum(dtype=F))) * F(1.001) + F(1e-3), F((v * mu).sum(dtype=F)))


def q8_slack(dim):
    return F(dim) * F(1.1920929e-07) + F(4.0e-5)


def filter_margin(dim, subnormals_exact=True):
    """scan_filter.hip filter_margin, in its float32 arithmetic."""
    sq = F(np.sqrt(F(dim)))
    small = F(5.9604645e-08) * sq if subnormals_exact else F(2.0) * F(6.1035156e-05) * sq
    return F(F(F(F(9.8e-4) + F(dim) * F(5.9604645e-08)) + small) + F(2.0e-5))


# ---- input families -----------------------------------------------------------------------------------------------------
def shared_rows(rng, n, dim, c=1.2):
    """Rows with a large common component (mean pairwise cosine ~0.59): the shape of real sentence embeddings."""
    mu = rng.normal(size=(1, dim)).astype(F)
    mu /= np.linalg.norm(mu)
    x = rng.normal(size=(n, dim)).astype(F) / np.sqrt(dim) + F(c) * mu
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F)


FAMILIES = ("normal", "shared", "adversarial")
NAN_ROWS = (ROW_LO + 128 + 45, ROW_LO + 128 + 46, ROW_LO + 128 + 47)   # one tile: NaN, +Inf, -Inf
DUP_TILE = ROW_LO + 256                                                 # a tile of near-duplicates of query 0


@functools.lru_cache(maxsize=None)
def make_rows(family, dim, n):
    rng = np.random.default_rng(1000 * dim + n + 7 * FAMILIES.index(family))
    if family == "shared":
        return shared_rows(rng, n, dim)
    rows = rng.normal(size=(n, dim)).astype(F)
    if family == "adversarial":   # the rows of test_gpu_filter_int8.py::test_rows_that_stress_the_quantiser
        rows[5::97, 17] = 40.0                 # outlier coordinate: the tile's scale collapses for everyone else
        rows[7::101] = 0.0
        rows[7::101, ::64] = 1.0               # sparse rows
        rows[11::53] *= F(1e6)
        rows[13::59] *= F(1e-12)
        rows[ROW_LO + 20] = 0.0
        if n > NAN_ROWS[2]:
            rows[NAN_ROWS[0], 9] = np.nan
            rows[NAN_ROWS[1], 10] = np.inf
            rows[NAN_ROWS[2], 11] = -np.inf
        if n >= DUP_TILE + 128:
            base = rng.normal(size=dim).astype(F)
            rows[DUP_TILE:DUP_TILE + 128] = base[None, :] + rng.normal(0, 2e-3, (128, dim)).astype(F)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def make_queries(family, dim, n, nq):
    """Gaussian queries, plus: 0 a near-duplicate of a stored row, 1 one-hot, 2 scaled by 1e-7, 3 zero, 4 scaled by 1e5."""
    rows = make_rows(family, dim, n)
    rng = np.random.default_rng(77 + dim + nq)
    q = (shared_rows(rng, nq, dim) if family == "shared" else rng.normal(size=(nq, dim)).astype(F)).copy()
    src = DUP_TILE if (family == "adversarial" and n >= DUP_TILE + 128) else ROW_LO + 5
    q[0] = rows[src] * F(2.0) + rng.normal(0, 1e-3, dim).astype(F)
    if nq > 1:
        q[1] = 0.0
        q[1, 17] = -2.0
    if nq > 2:
        q[2] *= F(1e-7)
    if nq > 3:
        q[3] = 0.0
    if nq > 4:
        q[4] *= F(1e5)
    q.setflags(write=False)
    return q


# ---- float64 ground truth -------------------------------------------------------------------------------------------------
def unit64(x):
    """float64 unit rows; a zero or non-finite row counts as a zero row (and is reported)."""
    x = x.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        nr = np.sqrt((x * x).sum(axis=1))
        ok = np.isfinite(nr) & (nr > 0) & np.isfinite(x).all(axis=1)
        u = np.where(ok[:, None], x / np.where(ok, nr, 1.0)[:, None], 0.0)
    return u, nr, ok


def cosines64(rows, queries):
    """[rows, queries] float64 cosines of the f32 vectors themselves; 0 where a norm is zero (what the refine returns), NaN
    for a row that holds a non-finite value."""
    ur, _, okr = unit64(rows)
    uq, _, _ = unit64(queries)
    cos = ur @ uq.T
    cos[~np.isfinite(rows).all(axis=1)] = np.nan
    return cos


def mean_unit_row64(rows):
    u, _, _ = unit64(rows)
    return u.sum(axis=0) / rows.shape[0]


def dead_words(dead_rows, n):
    w = np.zeros((n + 31) // 32, np.uint32)
    for r in dead_rows:
        w[r >> 5] |= np.uint32(1 << (r & 31))
    return w


def choose_tau(cos, lo, hi, live, modes=True, plus_inf=True):
    """Per query: the 10th best float64 cosine among the live rows of [lo, hi); query 2 the 200th best; with `modes`, every
    query q % 7 == 5 gets -inf (every live row must be a candidate) and, with plus_inf, q % 7 == 6 gets +inf (none may be)."""
    nq = cos.shape[1]
    tau = np.empty(nq, F)
    c = np.where(live[lo:hi, None], cos[lo:hi], np.nan)
    for q in range(nq):
        col = np.sort(c[:, q][np.isfinite(c[:, q])])[::-1]
        rank = 200 if q == 2 else 10
        tau[q] = F(col[min(rank, len(col)) - 1]) if len(col) else F(0)
        if modes and q % 7 == 5:
            tau[q] = -np.inf
        if modes and plus_inf and q % 7 == 6:
            tau[q] = np.inf
    return tau


# ---- the restated operands ---------------------------------------------------------------------------------------------------
class Restated:
    """The int8 copy (a [tiles * 128, dim], tmeta [tiles, 4] = inv_t, hB, E, N, flagged [tiles]), the query planes and
    constants, and the f16 operands, from f32 inputs, norms, mu and magnitudes alone."""

    def __init__(self, rows, queries, mu=None, norms=None, qmag=None):
        n, dim = rows.shape
        self.dim, self.n, self.nq = dim, n, queries.shape[0]
        with np.errstate(all="ignore"):
            if norms is None:
                norms = np.sqrt((rows.astype(F) ** 2).sum(axis=1, dtype=F)).astype(F)
            if qmag is None:
                qmag = np.sqrt((queries.astype(F) ** 2).sum(axis=1, dtype=F)).astype(F)
            if mu is None:
                mu = mean_unit_row64(rows).astype(F)
            self.norms, self.qmag, self.mu = norms.astype(F), qmag.astype(F), mu.astype(F)
            tiles = n // 128
            self.a = np.zeros((tiles * 128, dim), np.float64)
            self.tmeta = np.zeros((tiles, 4), F)
            self.flagged = np.zeros(tiles, bool)
            self.t_f32 = np.zeros((tiles * 128, dim), F)   # the products before rint (for the tie count)
            for t in range(tiles):
                r = slice(128 * t, 128 * t + 128)
                u = np.where(norms[r, None] == 0, F(0), rows[r] / np.where(norms[r] == 0, F(1), norms[r])[:, None]).astype(F) - self.mu
                self.flagged[t] = not np.isfinite(u).all()
                if self.flagged[t]:
                    self.tmeta[t] = (np.nan, 0, 0, 0)
                    continue
                a, inv, hB, E, N = _quantise_tile(rows[r], self.mu, norms[r])
                self.a[r] = a
                self.tmeta[t] = (inv, hB, E, N)
                self.t_f32[r] = (u * inv).astype(F)
            one = [_quantise_query(queries[q], self.mu, self.qmag[q]) for q in range(self.nq)]
            two = [_quantise_query_two_planes(queries[q], self.mu, self.qmag[q]) for q in range(self.nq)]
            self.b = np.stack([o[0] for o in one]).astype(np.float64)
            self.q1 = np.array([[o[1], o[2], o[3], o[4], o[5]] for o in one], F)        # inv, hA, nb, Dq, q.mu
            self.hi = np.stack([o[0] for o in two]).astype(np.float64)
            self.lo = np.stack([o[1] for o in two]).astype(np.float64)
            self.q2 = np.array([[o[2], o[3], o[4], o[5], o[6]] for o in two], F)
            # f16 operands: f16(f32(v) / f32(norm)), zero norm -> zero row
            self.rows_h = np.where(norms[:, None] == 0, F(0), rows / np.where(norms == 0, F(1), norms)[:, None]).astype(F).astype(np.float16)
            self.q_h = np.where(self.qmag[:, None] == 0, F(0), queries / np.where(self.qmag == 0, F(1), self.qmag)[:, None]).astype(F).astype(np.float16)

    def product(self, two_planes):
        """I [tiles * 128, nq]: exact in float64 (|I| < 2^31)."""
        if two_planes:
            return 128.0 * (self.a @ self.hi.T) + self.a @ self.lo.T
        return self.a @ self.b.T


def q8_line64(R, tau, two_planes, l1_only=False):
    """(lead, T) [tiles, nq]: the line of q8_threshold in float64 over the restated constants."""
    qm = (R.q2 if two_planes else R.q1).astype(np.float64)
    tm = R.tmeta.astype(np.float64)
    inv_q, hA, nb, Dq, qmu = (qm[:, i][None, :] for i in range(5))
    inv_t, hB, E, N = (tm[:, i][:, None] for i in range(4))
    with np.errstate(all="ignore"):
        lead = (tau.astype(np.float64)[None, :] - float(q8_slack(R.dim)) - qmu) * inv_q * inv_t
        if l1_only:
            band = hA + hB + 0.2501 * R.dim + 0 * E
        else:
            band = np.minimum(hA, nb * E) + np.minimum(hB, N * Dq) + np.minimum(float(F(0.2501) * F(R.dim)), E * Dq)
        T = np.floor(lead - band - 4.0 - np.abs(lead) * 4.0e-7)
        T = np.where(lead == np.inf, np.inf, T)      # tau = +inf: nothing can beat it
    return lead, T


def q8_line32(R, tau, two_planes, l1_only=False):
    """T [tiles, nq] as the kernels evaluate it: q8_threshold in float32, operation by operation."""
    qm = R.q2 if two_planes else R.q1
    inv_q, hA, nb, Dq, qmu = (qm[:, i][None, :] for i in range(5))
    inv_t, hB, E, N = (R.tmeta[:, i][:, None] for i in range(4))
    with np.errstate(all="ignore"):
        tqs = ((tau.astype(F)[None, :] - q8_slack(R.dim)).astype(F) - qmu).astype(F) * inv_q
        if l1_only:
            tA, tB, tC = hA + 0 * E, hB + 0 * Dq, F(0.2501) * F(R.dim) + 0 * E * Dq
        else:
            tA = np.minimum(hA, (nb * E).astype(F))
            tB = np.minimum(hB, (N * Dq).astype(F))
            tC = np.minimum(F(0.2501) * F(R.dim), (E * Dq).astype(F))
        lead = (tqs * inv_t).astype(F)
        rel = np.minimum((np.abs(lead) * F(4.0e-7)).astype(F), F(3.0e38))
        T = np.floor((lead - ((((tA + tB).astype(F) + tC).astype(F) + F(4.0)).astype(F) + rel).astype(F)).astype(F))
    return T


def kernel_hits_q8(I, T32):
    """What an int8 kernel appends given the products and its own thresholds: I > T, every row where T is NaN or below -2e9."""
    Tr = np.repeat(T32.astype(np.float64), 128, axis=0)
    with np.errstate(invalid="ignore"):
        return np.isnan(Tr) | (Tr < -2.0e9) | ((I > Tr) & ~(Tr > 2.0e9))


def f16_scores64(R):
    return R.rows_h.astype(np.float64) @ R.q_h.astype(np.float64).T


def f16_scores32(R):
    """f32 accumulation in 16-wide k steps (one MFMA step: an exact sum of 16 products, rounded into the accumulator)."""
    a, b = R.rows_h.astype(np.float64), R.q_h.astype(np.float64)
    acc = np.zeros((a.shape[0], b.shape[0]), F)
    with np.errstate(invalid="ignore"):
        for k in range(0, R.dim, 16):
            acc = (acc.astype(np.float64) + a[:, k:k + 16] @ b[:, k:k + 16].T).astype(F)
    return acc


# ---- decision rules -----------------------------------------------------------------------------------------------------------
class Masks:
    def __init__(self, must, mustnot):
        self.must, self.mustnot = must, mustnot
        self.free = ~(must | mustnot)

    def violations(self, hits):
        """(row, query) pairs a returned set `hits` gets wrong."""
        return int(((self.must & ~hits) | (self.mustnot & hits)).sum())


def _outside(n, nq, lo, hi, live):
    out = np.ones((n, nq), bool)
    out[lo:hi] = False
    out[~live] = True
    return out


def safety_masks(rows, queries, tau, lo, hi, live, int8, flagged=None):
    """float64 cosine >= tau => must (every kernel).  int8: every row of a tile holding a non-finite value is a must for every
    query with tau < +inf; f16: the rows that hold one are.  Dead rows and rows outside [lo, hi): must not."""
    n, nq = rows.shape[0], queries.shape[0]
    cos = cosines64(rows, queries)
    with np.errstate(invalid="ignore"):
        must = cos >= tau.astype(np.float64)[None, :]
    bad = ~np.isfinite(rows).all(axis=1)
    if int8:
        tiles = n // 128
        bt = bad[:tiles * 128].reshape(tiles, 128).any(axis=1) if flagged is None else flagged
        bad = np.concatenate([np.repeat(bt, 128), np.zeros(n - tiles * 128, bool)])
    must |= bad[:, None] & (tau < np.inf)[None, :]
    outside = _outside(n, nq, lo, hi, live)
    must &= ~outside
    return Masks(must, outside)


def q8_masks(R, tau, two_planes, lo, hi, live):
    """Tightness of an int8 kernel: I > T + delta => must, I < T - delta => must not, delta = 2 + |lead| 2^-21 (two f32 products
    and a difference in lead, the floor, the integer conversion: the size of the allowance |lead| 4e-7 the kernel takes for
    that evaluation).  Rows of a flagged tile: must while tau < +inf, free at +inf."""
    n, nq = R.n, R.nq
    n8 = R.a.shape[0]
    I = R.product(two_planes)
    lead, T = q8_line64(R, tau, two_planes)
    with np.errstate(invalid="ignore"):
        delta = 2.0 + np.where(np.isfinite(lead), np.abs(lead), 0.0) * 2.0 ** -21
        Tr, dr = np.repeat(T, 128, axis=0), np.repeat(delta, 128, axis=0)
        must8 = I > Tr + dr
        mustnot8 = I < Tr - dr
    fl = np.repeat(R.flagged, 128)
    must8[fl] = (tau < np.inf)[None, :]
    mustnot8[fl] = False
    must = np.zeros((n, nq), bool)
    mustnot = np.zeros((n, nq), bool)
    must[:n8], mustnot[:n8] = must8, mustnot8
    outside = _outside(n, nq, lo, hi, live)
    outside[n8:] = True
    return Masks(must & ~outside, mustnot | outside)


def f16_masks(R, tau, lo, hi, live):
    """Tightness of an f16 kernel: s = the float64 product of the f16 operands; s > tau - margin + e => must, s < tau - margin - e
    => must not, e = dim 2^-24 sum |a_i||b_i| + 2^-24 (f32 accumulation in any order, the rounding of tau - margin).  A NaN product
    (a row or a query holding a non-finite value) is a candidate: must."""
    s = f16_scores64(R)
    with np.errstate(invalid="ignore"):
        e = R.dim * 2.0 ** -24 * (np.abs(R.rows_h.astype(np.float64)) @ np.abs(R.q_h.astype(np.float64)).T) + 2.0 ** -24
        line = (tau.astype(np.float64) - float(filter_margin(R.dim)))[None, :]
        must = (s > line + e) | (np.isnan(s) & (tau < np.inf)[None, :])
        mustnot = s < line - e
    outside = _outside(R.n, R.nq, lo, hi, live)
    return Masks(must & ~outside, (mustnot & ~np.isnan(s)) | outside)


def free_cap_holds(m, lo, hi, nq):
    """At most 0.1 % of the (row, query) pairs are free, and fewer than a tenth of the must pairs."""
    free, must, pairs = int(m.free.sum()), int(m.must.sum()), (hi - lo) * nq
    return free <= 1e-3 * pairs and (free == 0 or free < must / 10.0), (free, must, pairs)


# ---- the cases of the GPU test --------------------------------------------------------------------------------------------------
class Case:
    """One cs_debug_filter call."""

    def __init__(self, dim, kernel, nqt, family="normal", span=128, nq=1, grid="plan", dead=False, cap=None, tail=0,
                 mu_random=False, modes=True):
        self.dim, self.kernel, self.nqt, self.family, self.span, self.nq = dim, kernel, nqt, family, span, nq
        self.grid_mode, self.dead, self.tail, self.mu_random, self.modes = grid, dead, tail, mu_random, modes
        self.lo, self.hi = ROW_LO, ROW_LO + span
        self.n = self.hi + BEHIND
        self.cap = cap if cap is not None else span + 256
        self.int8 = kernel in INT8
        self.two_planes = kernel == Q8_RW2

    @property
    def id(self):
        return (f"{self.dim}-{KERNEL_NAMES[self.kernel]}{self.nqt or ''}-{self.family}-rows{self.span}-nq{self.nq}-{self.grid_mode}"
                + ("-dead" if self.dead else "") + (f"-cap{self.cap}" if self.cap < self.span else "") + (f"-tail{self.tail}" if self.tail else "")
                + ("-mu" if self.mu_random else ""))

    def qtiles(self):
        per = 32 * self.nqt if self.kernel in RESIDENT else (128 if self.kernel == F16_TILE128 else 256)
        return (self.nq + per - 1) // per

    def grid(self):
        """0 = the plan's rule; "min" the smallest legal grid (8 per query tile: five tiles per block at 5,120 rows); "idle" more
        blocks than tiles."""
        if self.grid_mode == "plan":
            return 0
        tiles = (self.span + 127) // 128
        if self.kernel == F16_TILE128:
            return 0 if self.grid_mode == "min" else ((tiles + 7) // 8 * 8 + 16) * self.qtiles()
        if self.grid_mode == "min":
            return 8 * self.qtiles()
        return ((tiles + 7) // 8 * 8 + 16) * self.qtiles()

    def rows(self):
        return make_rows(self.family, self.dim, self.n)

    def queries(self):
        return make_queries(self.family, self.dim, self.n, self.nq)

    def mu_in(self):
        if not self.mu_random:
            return None
        v = np.random.default_rng(5).normal(size=self.dim)
        return (0.5 * v / np.linalg.norm(v)).astype(F)

    def dead_rows(self):
        """Every 7th row, plus what would otherwise be query 0's best three in range."""
        if not self.dead:
            return np.zeros(0, np.int64)
        cos = _cos_cached(self.family, self.dim, self.n, self.nq)[self.lo:self.hi, 0]
        best = self.lo + np.argsort(np.where(np.isfinite(cos), cos, -np.inf))[::-1][:3]
        return np.unique(np.concatenate([np.arange(0, self.n, 7), best]))

    def live(self):
        live = np.ones(self.n, bool)
        live[self.dead_rows()] = False
        return live

    def tau(self):
        cos = _cos_cached(self.family, self.dim, self.n, self.nq)
        # adversarial family: no tau = +inf.  Its flagged tile has inv_t = NaN, which no tau can be compared with: at +inf its
        # 128 rows would be free for every such query (more than the cap on the free set allows), so +inf is left to the
        # other two families
        tau = choose_tau(cos, self.lo, self.hi, self.live(), self.modes, plus_inf=self.family != "adversarial")
        if self.cap < self.span:   # overflow: one query takes every live row in range
            tau[min(1, self.nq - 1)] = -np.inf
        return tau


@functools.lru_cache(maxsize=64)
def _cos_cached(family, dim, n, nq):
    return cosines64(make_rows(family, dim, n), make_queries(family, dim, n, nq))


def resident_nqs(nqt):
    r = 32 * nqt
    return [1, r - 1, r, r + 1]


def gpu_cases(dim):
    """Every instantiation on the normal family over the row spans, grids and query counts that reach its edges; `shared` and
    `adversarial` on one instantiation of each kernel."""
    cases = []
    seen = set()
    for kernel, nqt in INSTS[dim]:
        f16 = kernel not in INT8
        nqs = resident_nqs(nqt) if kernel in RESIDENT else [1, 127, 129, 257, 300]
        spans = [128, 384, 1152] + ([1000] if f16 else [])
        for i, span in enumerate(spans):
            for j, grid in enumerate(("plan", "min", "idle")):
                cases.append(Case(dim, kernel, nqt, span=span, nq=nqs[(i + j) % len(nqs)], grid=grid))
        for nq in nqs:   # five tiles per block: rings wrap across tile boundaries, the tile kernels walk several slots
            cases.append(Case(dim, kernel, nqt, span=5120, nq=nq, grid="min"))
        mid = nqs[len(nqs) // 2]
        cases.append(Case(dim, kernel, nqt, span=1152, nq=mid, dead=True))
        cases.append(Case(dim, kernel, nqt, span=1152, nq=nqs[-1], cap=64, grid="min"))
        cases.append(Case(dim, kernel, nqt, span=384, nq=mid, tail=77))
        if kernel not in seen:   # one instantiation of each kernel per dim
            seen.add(kernel)
            for fam in ("shared", "adversarial"):
                cases.append(Case(dim, kernel, nqt, family=fam, span=1152, nq=nqs[-1], dead=fam == "adversarial"))
                cases.append(Case(dim, kernel, nqt, family=fam, span=5120, nq=mid, grid="min"))
            if not f16:
                cases.append(Case(dim, kernel, nqt, span=1152, nq=mid, mu_random=True))
    for tail in (1, 77, 127):
        cases.append(Case(dim, NONE, 0, span=384, nq=33, tail=tail, dead=tail == 77))
    return cases


def case_masks(case, R):
    """(safety, tightness) of a case over the restated operands R."""
    rows, queries, tau, live = case.rows(), case.queries(), case.tau(), case.live()
    lo, hi = case.lo, case.hi
    if case.kernel == NONE:
        none = Masks(np.zeros((case.n, case.nq), bool), np.ones((case.n, case.nq), bool))
        return none, none
    safety = safety_masks(rows, queries, tau, lo, hi, live, case.int8, R.flagged if case.int8 else None)
    tight = q8_masks(R, tau, case.two_planes, lo, hi, live) if case.int8 else f16_masks(R, tau, lo, hi, live)
    return safety, tight
