"""Similar-chunk search (cs_index_search_similar) against what a caller can do without it — read the source's row back
(cs_index_read_rows), search with it on the streaming route at k + 1 (cs_index_search) and drop the source on the host —
over the same 10M x 384 store, in one process, alternated (new, baseline, new again, --reps calls each).  The baseline is
exact for "self" only: for "file" it is the rank-then-filter method the feature replaces, and its answer is recorded beside
the exact one.  Per source kind, k (10, 200), sources per call (1, 9), mode (none, self, file) and bound (none, 0.9): the
median wall time of the host-buffer call over both new series, each series' own median, the baseline's median and the
ratio.  One JSON object per line on stdout (and in --out).

The baseline of several sources (baseline_ms) is one read and one one-query streaming search PER SOURCE: cs_index_search
has no streaming route for nine queries in one call.  What one call of nine rows costs is recorded beside it, measured
once per shape and not alternated with the new call: on the library's default route (the int8 filter + exact refine: baseline_one_call_default_ms) and
with the filter switched off (five or more queries then take the exact-f32 MFMA path: baseline_one_call_nofilter_ms).

    python benchmarks/similar_search.py [--rows 10000000] [--dim 384] [--reps 20] [--out FILE] [--tree DIR] [--scoped] [--routes]

The store: synthetic rows in files of 8 ids, with rows [2/10, 3/10) of it replaced by one file of near-duplicates of its
first row (0.95 s + 0.05 noise).  The "hog" source is that first row; the "ordinary" source is a row far from the file.
With 9 sources per call the other 8 are ordinary rows.

--tree DIR: load the package and the library of another checkout (the parent commit's, built): the entry point it lacks is
not timed, so the same script gives the baseline's times under the parent's library.

--routes: the call's two routes against each other instead (cs_index_set_similar_route), in one process, alternated: FILTER,
SCAN, FILTER again, --reps calls each.  The yardstick is the SCAN route — the f32 streaming scan under the exclusions, what
the call did before it had a route — and the spread of a case is the difference between the two FILTER series' medians.
Ordinary source, 1 and 9 sources per call, k 10 and 200, modes none / self / file, with and without the bound 0.9; then the
fallback case, the source inside the near-duplicate file with the file excluded: the filter's candidate buffer overflows
and the scan answers, so the call costs both (filter_fallbacks counts them).  auto_route: what CS_SIMILAR_ROUTE_AUTO picks
for the case, read from the counters.  The single-query route stays on its default here (AUTO follows it).  Under --tree
with a library that has no route the call itself is timed: the scan, under the parent's library.

--scoped: the scoped cases instead (cs_index_search_similar_scoped) over the same store: scopes of every id, a random 10 %, a
random 1 % and the near-duplicate file plus a random 1 %; the source is the file's first row for the last scope and the
ordinary row for the others, which does not lie in the random scopes' ids unless drawn.  The baseline is what a caller can
do without the call: one read per source (cs_index_read_rows), then ONE cs_index_search_scoped of those rows with the
scope on CS_SCOPE_ROUTE_GATHER at k + 1, the excluded rows dropped on the host — exact for "self" only.  The same
alternation, and baseline_exact_found as above.

--scoped --routes: the scoped call's two routes against each other (cs_scope_set_route), as --routes does for the unscoped
call: FILTER, GATHER, FILTER again in one process, --reps calls each, the bytes of the two routes compared before anything
is timed.  The scopes of --scoped and a contiguous 10 % in the store's far half.  planned_span: the rows the filter phases
stream for the case (scoped_filter_plan.hpp: from the end of the granule that holds list entry 3,071 to the end of the
granule that holds the last one) and span_over_live its ratio to the scope's rows; auto_route: what CS_SCOPE_ROUTE_AUTO
picks, read from the scope's counters; filter_calls / overflow_reruns: whether the FILTER series were answered by the filter
and how many of them fell back to the gathered similar scan after an overflowed candidate buffer (the call then costs
both).  Under --tree with a library whose scoped call has no filter route, filter_calls is 0 and both series time the
gathered scan."""
import argparse
import json
import os
import sys
import time

import numpy as np


def timed(fn, reps):
    """-> the wall times of `reps` calls after one untimed call, ms."""
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def scoped_cases(a, st, lib, h, _lib, emit, sources, others, groups, hog_lo, hog_n, modes, med):
    from codesearch_amd._lib import f32p, u32p

    n, dim = a.rows, a.dim
    has_new = "cs_index_search_similar_scoped" in _lib.SIGNATURES
    rng = np.random.default_rng(3)
    tenth, hundredth = np.sort(rng.choice(n, n // 10, replace=False)), np.sort(rng.choice(n, n // 100, replace=False))
    hog = np.union1d(np.arange(hog_lo, hog_lo + hog_n), np.sort(rng.choice(n, n // 100, replace=False)))
    for sname, ids, kind in (("all", np.arange(n), "ordinary"), ("10%", tenth, "ordinary"), ("1%", hundredth, "ordinary"),
                             ("hog+1%", hog, "hog")):
        sc = st.scope(ids)
        sc.set_route("gather")
        in_scope = np.zeros(n, bool)
        in_scope[ids] = True
        src = sources[kind]
        for nq in (1, 9):
            srcs = np.ascontiguousarray(np.concatenate([[src], others[:nq - 1]]), np.uint32)
            rows = np.zeros((nq, dim), np.float32)
            for k in (10, 200):
                cos, idb, cnt = np.zeros((nq, k), np.float32), np.zeros((nq, k), np.uint32), np.zeros(nq, np.uint32)
                bcos, bid, bcnt = np.zeros((nq, k + 1), np.float32), np.zeros((nq, k + 1), np.uint32), np.zeros(nq, np.uint32)

                def baseline():
                    for q in range(nq):
                        _lib.check(lib.cs_index_read_rows(h, int(srcs[q]), 1, rows[q:q + 1].ctypes.data_as(f32p)))
                    _lib.check(lib.cs_index_search_scoped(h, sc.handle, rows.ctypes.data_as(f32p), nq, dim, k + 1,
                                                          bcos.ctypes.data_as(f32p), bid.ctypes.data_as(u32p),
                                                          bcnt.ctypes.data_as(u32p)))

                for mname, mode in modes.items():
                    for bound in (None, 0.9):
                        rec = {"scope": sname, "scope_ids": int(ids.size), "source": kind, "source_in_scope": bool(in_scope[src]),
                               "rows": n, "dim": dim, "nq": nq, "k": k, "mode": mname, "min_cos": bound, "reps": a.reps,
                               "library": "new" if has_new else "parent"}
                        if has_new:
                            def similar():
                                _lib.check(lib.cs_index_search_similar_scoped(h, sc.handle, srcs.ctypes.data_as(u32p), nq, k, mode,
                                                                              float("-inf") if bound is None else bound,
                                                                              cos.ctypes.data_as(f32p), idb.ctypes.data_as(u32p),
                                                                              cnt.ctypes.data_as(u32p)))

                            t1 = timed(similar, a.reps)
                            tb = timed(baseline, a.reps)
                            t2 = timed(similar, a.reps)
                            rec.update({"similar_ms": med(t1 + t2), "similar_before_ms": med(t1), "similar_after_ms": med(t2),
                                        "baseline_ms": med(tb), "count": int(cnt[0])})
                            rec["ratio_vs_baseline"] = round(rec["similar_ms"] / rec["baseline_ms"], 4)
                            kept = [int(i) for i, c in zip(bid[0][:bcnt[0]], bcos[0][:bcnt[0]])
                                    if (mode == 0 or i != src) and (mode != 2 or groups[i] != groups[src])
                                    and (bound is None or c > bound)][:k]
                            rec["baseline_hits"] = len(kept)
                            rec["baseline_exact_found"] = len(set(kept) & set(idb[0][:cnt[0]].tolist()))
                        else:
                            rec["baseline_ms"] = med(timed(baseline, a.reps))
                        emit(rec)
        sc.close()


def scoped_route_cases(a, st, lib, h, _lib, emit, sources, others, hog_lo, hog_n, modes, med):
    from codesearch_amd._lib import f32p, u32p

    n, dim = a.rows, a.dim
    rng = np.random.default_rng(3)
    tenth, hundredth = np.sort(rng.choice(n, n // 10, replace=False)), np.sort(rng.choice(n, n // 100, replace=False))
    hog = np.union1d(np.arange(hog_lo, hog_lo + hog_n), np.sort(rng.choice(n, n // 100, replace=False)))
    far = np.arange(n - n // 10 - n // 20, n - n // 20)  # contiguous 10 % in the far half
    up = lambda v: (int(v) + 1023) // 1024 * 1024  # noqa: E731
    for sname, ids, kind in (("all", np.arange(n), "ordinary"), ("10%", tenth, "ordinary"), ("1%", hundredth, "ordinary"),
                             ("hog+1%", hog, "hog"), ("far 10%", far, "ordinary")):
        sc = st.scope(ids)
        span = (min(up(ids[-1] + 1), n) - up(ids[3071] + 1)) if ids.size > 3072 else 0
        for nq, k, mname, bound in ((nq, k, m, b) for nq in (1, 9) for k in (10, 200) for m in modes for b in (None, 0.9)):
            srcs = np.ascontiguousarray(np.concatenate([[sources[kind]], others[:nq - 1]]), np.uint32)
            cos, idb, cnt = np.zeros((nq, k), np.float32), np.zeros((nq, k), np.uint32), np.zeros(nq, np.uint32)

            def similar():
                _lib.check(lib.cs_index_search_similar_scoped(h, sc.handle, srcs.ctypes.data_as(u32p), nq, k, modes[mname],
                                                              float("-inf") if bound is None else bound,
                                                              cos.ctypes.data_as(f32p), idb.ctypes.data_as(u32p),
                                                              cnt.ctypes.data_as(u32p)))

            rec = {"scope": sname, "scope_ids": int(ids.size), "source": kind, "rows": n, "dim": dim, "nq": nq, "k": k,
                   "mode": mname, "min_cos": bound, "reps": a.reps, "planned_span": int(span),
                   "span_over_live": round(span / ids.size, 3)}
            sc.set_route("auto")
            i0 = sc.route_info()
            similar()
            i1 = sc.route_info()
            rec["auto_route"] = "filter" if i1[0] > i0[0] else "gather"
            sc.set_route("filter")
            similar()
            got = (cos.copy(), idb.copy(), cnt.copy())
            sc.set_route("gather")
            similar()
            rec["same_bytes"] = all(x.tobytes() == y.tobytes() for x, y in zip(got, (cos, idb, cnt)))
            i1 = sc.route_info()
            sc.set_route("filter")
            t1 = timed(similar, a.reps)
            sc.set_route("gather")
            tg = timed(similar, a.reps)
            sc.set_route("filter")
            t2 = timed(similar, a.reps)
            i2 = sc.route_info()
            calls = 2 * (a.reps + 1)
            rec.update({"filter_ms": med(t1 + t2), "filter_before_ms": med(t1), "filter_after_ms": med(t2), "gather_ms": med(tg),
                        "spread_ms": round(abs(med(t1) - med(t2)), 4), "count": int(cnt[0]), "filter_series_calls": calls,
                        "filter_calls": i2[0] - i1[0], "overflow_reruns": i2[2] - i1[2]})
            rec["fell_back"] = rec["filter_calls"] < calls or rec["overflow_reruns"] > 0
            rec["ratio_vs_gather"] = round(rec["filter_ms"] / rec["gather_ms"], 4)
            emit(rec)
        sc.close()


def route_cases(a, st, lib, h, _lib, emit, sources, others, modes, med):
    from codesearch_amd._lib import f32p, u32p

    n, dim = a.rows, a.dim
    has_route = "cs_index_set_similar_route" in _lib.SIGNATURES
    cases = [("ordinary", nq, k, mname, bound) for nq in (1, 9) for k in (10, 200) for mname in modes for bound in (None, 0.9)]
    cases += [("hog", nq, k, "file", None) for nq in (1, 9) for k in (10, 200)]  # the fallback case
    for kind, nq, k, mname, bound in cases:
        srcs = np.ascontiguousarray(np.concatenate([[sources[kind]], others[:nq - 1]]), np.uint32)
        cos, idb, cnt = np.zeros((nq, k), np.float32), np.zeros((nq, k), np.uint32), np.zeros(nq, np.uint32)

        def similar():
            _lib.check(lib.cs_index_search_similar(h, srcs.ctypes.data_as(u32p), nq, k, modes[mname],
                                                   float("-inf") if bound is None else bound, cos.ctypes.data_as(f32p),
                                                   idb.ctypes.data_as(u32p), cnt.ctypes.data_as(u32p)))

        rec = {"source": kind, "rows": n, "dim": dim, "nq": nq, "k": k, "mode": mname, "min_cos": bound, "reps": a.reps,
               "library": "new" if has_route else "parent"}
        if not has_route:
            rec["scan_ms"] = med(timed(similar, a.reps))
            emit(rec)
            continue
        st.set_similar_route("auto")
        i0 = st.similar_route_info()
        similar()
        i1 = st.similar_route_info()
        rec["auto_route"] = "filter" if i1[0] > i0[0] else "scan"
        st.set_similar_route("filter")
        t1 = timed(similar, a.reps)
        got = (cos.copy(), idb.copy(), cnt.copy())
        st.set_similar_route("scan")
        ts = timed(similar, a.reps)
        rec["same_bytes"] = all(x.tobytes() == y.tobytes() for x, y in zip(got, (cos, idb, cnt)))
        st.set_similar_route("filter")
        t2 = timed(similar, a.reps)
        i2 = st.similar_route_info()
        rec.update({"filter_ms": med(t1 + t2), "filter_before_ms": med(t1), "filter_after_ms": med(t2), "scan_ms": med(ts),
                    "spread_ms": round(abs(med(t1) - med(t2)), 4), "count": int(cnt[0]),
                    "filter_calls": i2[0] - i1[0], "filter_fallbacks": i2[2] - i1[2]})
        rec["ratio_vs_scan"] = round(rec["filter_ms"] / rec["scan_ms"], 4)
        emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--scoped", action="store_true")
    ap.add_argument("--routes", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from codesearch_amd import VectorStore, _lib
    from codesearch_amd._lib import f32p, u32p
    from codesearch_amd.synth import synth_rows

    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    n, dim, seed = a.rows, a.dim, 0x5EA4C5
    hog_lo, hog_n = n // 5, n // 10
    st = VectorStore(None, dim, capacity=n)
    st.insert_synthetic(hog_lo, seed, 0)
    s_row = synth_rows(seed, hog_lo, 1, dim)
    st.insert_embeddings(s_row)
    rng = np.random.default_rng(2)
    scale = float(np.linalg.norm(s_row)) / np.sqrt(dim)
    step = 100_000
    for lo in range(1, hog_n, step):
        cnt = min(step, hog_n - lo)
        noise = rng.standard_normal((cnt, dim), dtype=np.float32) * np.float32(scale)
        st.insert_embeddings(np.float32(0.95) * s_row + np.float32(0.05) * noise)
    st.insert_synthetic(n - hog_lo - hog_n, seed, hog_lo + hog_n)
    st.build_index()
    if not a.routes:
        st.set_single_query_route(st.ROUTE_STREAM)
    assert st.next_id() == n
    lib, h = st._lib, st.handle
    has_new = "cs_index_search_similar" in _lib.SIGNATURES
    ids = np.arange(n, dtype=np.uint32)
    groups = ids // 8
    groups[hog_lo:hog_lo + hog_n] = 0xFFFFFFF0
    st.set_groups(ids, groups)
    others = (np.arange(8, dtype=np.uint32) * 1000 + n // 2 + 17).astype(np.uint32)
    kinds = [("ordinary", np.uint32(n - n // 7)), ("hog", np.uint32(hog_lo))]
    modes = {"none": 0, "self": 1, "file": 2}
    med = lambda t: round(float(np.median(t)), 4)  # noqa: E731
    if a.routes and a.scoped:
        scoped_route_cases(a, st, lib, h, _lib, emit, dict(kinds), others, hog_lo, hog_n, modes, med)
        kinds = []
    elif a.routes:
        route_cases(a, st, lib, h, _lib, emit, dict(kinds), others, modes, med)
        kinds = []
    elif a.scoped:
        scoped_cases(a, st, lib, h, _lib, emit, dict(kinds), others, groups, hog_lo, hog_n, modes, med)
        kinds = []
    for kind, src in kinds:
        for nq in (1, 9):
            srcs = np.ascontiguousarray(np.concatenate([[src], others[:nq - 1]]), np.uint32)
            rows = np.zeros((nq, dim), np.float32)
            for k in (10, 200):
                cos, idb, cnt = np.zeros((nq, k), np.float32), np.zeros((nq, k), np.uint32), np.zeros(nq, np.uint32)
                bcos, bid, bcnt = np.zeros((nq, k + 1), np.float32), np.zeros((nq, k + 1), np.uint32), np.zeros(nq, np.uint32)

                def baseline():  # the streaming route: one query per call (set_single_query_route above)
                    for q in range(nq):
                        _lib.check(lib.cs_index_read_rows(h, int(srcs[q]), 1, rows[q:q + 1].ctypes.data_as(f32p)))
                        _lib.check(lib.cs_index_search(h, rows[q:q + 1].ctypes.data_as(f32p), 1, dim, k + 1,
                                                       bcos[q:q + 1].ctypes.data_as(f32p), bid[q:q + 1].ctypes.data_as(u32p),
                                                       bcnt[q:q + 1].ctypes.data_as(u32p)))

                def one_call():  # the sources are not neighbours: one read per source, then all rows in one search
                    for q in range(nq):
                        _lib.check(lib.cs_index_read_rows(h, int(srcs[q]), 1, rows[q:q + 1].ctypes.data_as(f32p)))
                    _lib.check(lib.cs_index_search(h, rows.ctypes.data_as(f32p), nq, dim, k + 1, bcos.ctypes.data_as(f32p),
                                                   bid.ctypes.data_as(u32p), bcnt.ctypes.data_as(u32p)))

                base_first = timed(baseline, a.reps)
                one_default = one_nofilter = None
                if nq > 1:
                    one_default = med(timed(one_call, a.reps))
                    st.set_filter_min_queries(1 << 20)
                    one_nofilter = med(timed(one_call, a.reps))
                    st.set_filter_min_queries(2)
                for mname, mode in modes.items():
                    for bound in (None, 0.9):
                        rec = {"source": kind, "rows": n, "dim": dim, "nq": nq, "k": k, "mode": mname, "min_cos": bound,
                               "reps": a.reps, "library": "new" if has_new else "parent"}
                        if has_new:
                            def similar():
                                _lib.check(lib.cs_index_search_similar(h, srcs.ctypes.data_as(u32p), nq, k, mode,
                                                                       float("-inf") if bound is None else bound,
                                                                       cos.ctypes.data_as(f32p), idb.ctypes.data_as(u32p),
                                                                       cnt.ctypes.data_as(u32p)))

                            t1 = timed(similar, a.reps)
                            tb = timed(baseline, a.reps)
                            t2 = timed(similar, a.reps)
                            rec.update({"similar_ms": med(t1 + t2), "similar_before_ms": med(t1), "similar_after_ms": med(t2),
                                        "baseline_ms": med(tb), "count": int(cnt[0])})
                            rec["ratio_vs_baseline"] = round(rec["similar_ms"] / rec["baseline_ms"], 4)
                            # what the baseline's ranked list holds of the exact answer once the mode's rows are dropped
                            baseline()
                            kept = [int(i) for i, c in zip(bid[0][:bcnt[0]], bcos[0][:bcnt[0]])
                                    if (mode == 0 or i != src) and (mode != 2 or groups[i] != groups[src])
                                    and (bound is None or c > bound)][:k]
                            rec["baseline_hits"] = len(kept)
                            rec["baseline_exact_found"] = len(set(kept) & set(idb[0][:cnt[0]].tolist()))
                        else:
                            rec["baseline_ms"] = med(timed(baseline, a.reps))
                        rec["baseline_first_series_ms"] = med(base_first)
                        if nq > 1:
                            rec["baseline_one_call_default_ms"] = one_default
                            rec["baseline_one_call_nofilter_ms"] = one_nofilter
                        emit(rec)
    if out:
        out.close()


if __name__ == "__main__":
    main()
