"""Grouped search inside a scope and across query variants (cs_index_search_grouped_scoped,
cs_index_search_variants_grouped_scoped) against the searches they extend, over one store, in one process, alternated
(new, the baselines, new again, --reps calls each).  Per scope (all ids, 10 % random, 1 % random), k (10, 200) and
per_group (1, 3), files of 8 contiguous ids:

    one query      grouped scoped   vs  cs_index_search_scoped of the same scope (gathered route, and the scope's default
                                        route) and vs cs_index_search_grouped over the whole store
    nine variants  variants grouped scoped  vs  cs_index_search_variants_scoped (gathered route)

Medians of the wall times of the host-buffer calls, ms, and the ratios.  One JSON object per line on stdout (and in --out).

    python benchmarks/grouped_scoped_search.py [--rows 10000000] [--dim 384] [--reps 20] [--out FILE] [--tree DIR]

--tree DIR: load the package and the library of another checkout (the parent commit's, built): entry points it lacks are
not timed, so the same script gives the baselines' times under the parent's library."""
import argparse
import ctypes as C
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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

    n, dim = a.rows, a.dim
    st = VectorStore(None, dim, capacity=n)
    st.insert_synthetic(n, 0x5EA4C5, 0)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    lib, h = st._lib, st.handle
    has_new = "cs_index_search_grouped_scoped" in _lib.SIGNATURES
    ids = np.arange(n, dtype=np.uint32)
    st.set_groups(ids, ids // 8)
    q1 = np.ascontiguousarray(synth_rows(0x9E5, 1, 1, dim))
    noise = synth_rows(0x9E7, 0, 9, dim)
    q9 = np.ascontiguousarray(q1 + np.float32(0.15) * noise)
    q9[0] = q1[0]
    rng = np.random.default_rng(3)
    scopes = [("all", ids), ("random10pct", np.flatnonzero(rng.random(n) < 0.10).astype(np.uint32)),
              ("random1pct", np.flatnonzero(rng.random(n) < 0.01).astype(np.uint32))]
    med = lambda t: round(float(np.median(t)), 4)  # noqa: E731
    for sname, sids in scopes:
        sc = st.scope(sids)
        for k in (10, 200):
            cos, idb, cnt = np.zeros((1, k), np.float32), np.zeros((1, k), np.uint32), np.zeros(1, np.uint32)
            count, flag = C.c_uint32(), C.c_int32()
            lists = (cos.ctypes.data_as(f32p), idb.ctypes.data_as(u32p), cnt.ctypes.data_as(u32p))
            merged = (cos.ctypes.data_as(f32p), idb.ctypes.data_as(u32p), C.byref(count), C.byref(flag))
            p1, p9 = q1.ctypes.data_as(f32p), q9.ctypes.data_as(f32p)

            def scoped():
                _lib.check(lib.cs_index_search_scoped(h, sc.handle, p1, 1, dim, k, *lists))

            def variants_scoped():
                _lib.check(lib.cs_index_search_variants_scoped(h, sc.handle, p9, 9, dim, k, *merged))

            for m in (1, 3):
                def grouped():
                    _lib.check(lib.cs_index_search_grouped(h, p1, 1, dim, k, m, *lists))

                def grouped_scoped():
                    _lib.check(lib.cs_index_search_grouped_scoped(h, sc.handle, p1, 1, dim, k, m, *lists))

                def variants_grouped_scoped():
                    _lib.check(lib.cs_index_search_variants_grouped_scoped(h, sc.handle, p9, 9, dim, k, m, *merged))

                rec = {"scope": sname, "scope_ids": int(sids.size), "rows": n, "dim": dim, "k": k, "m": m, "reps": a.reps,
                       "library": "new" if has_new else "parent"}
                sc.set_route("gather")
                new1 = timed(grouped_scoped, a.reps) if has_new else []
                rec["scoped_gather_ms"] = med(timed(scoped, a.reps))
                sc.set_route("auto")
                rec["scoped_auto_ms"] = med(timed(scoped, a.reps))
                rec["grouped_ms"] = med(timed(grouped, a.reps))
                if has_new:
                    new1 += timed(grouped_scoped, a.reps)
                    rec["grouped_scoped_ms"] = med(new1)
                    rec["grouped_scoped_count"] = int(cnt[0])
                    rec["ratio_vs_scoped_gather"] = round(rec["grouped_scoped_ms"] / rec["scoped_gather_ms"], 4)
                    rec["ratio_vs_grouped"] = round(rec["grouped_scoped_ms"] / rec["grouped_ms"], 4)
                sc.set_route("gather")
                new9 = timed(variants_grouped_scoped, a.reps) if has_new else []
                rec["variants_scoped_gather_ms"] = med(timed(variants_scoped, a.reps))
                if has_new:
                    new9 += timed(variants_grouped_scoped, a.reps)
                    rec["variants_grouped_scoped_ms"] = med(new9)
                    rec["variants_grouped_scoped_count"] = int(count.value)
                    rec["variants_ratio_vs_variants_scoped_gather"] = round(rec["variants_grouped_scoped_ms"] /
                                                                            rec["variants_scoped_gather_ms"], 4)
                sc.set_route("auto")
                emit(rec)
        sc.close()
    st.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
