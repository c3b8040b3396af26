"""Scoped search through the int8 filter (cs_scope_set_route CS_SCOPE_ROUTE_FILTER) against the gathered f32 scan of the
same scope (CS_SCOPE_ROUTE_GATHER: the route every scoped search took before) and against the same search unscoped
(default route: int8 filter + exact refine), over one 10M x 384 store, in one process, ALTERNATED: per mask and search
shape, `rounds` rounds of (reps gathered calls, reps filter calls, reps unscoped calls); reported are the median over the
rounds of each round's median wall time of the host-buffer call, and the spread (largest minus smallest round median) of
each.  Before anything is timed the two scoped answers are compared, bytes for bytes.  Per record also: what AUTO picks
(auto_route) and span_over_live = (last row - first row + 1) / allowed, the mask's own measure of what the route's span
rule weighs (CS_SCOPE_FILTER_MAX_SPAN: rows the filter phases stream per live row).  Per mask: scope creation and
refresh with the bitmap (this store) and without it (a second store of the same rows whose index keeps no int8 copy, CS_FILTER_INT8=0: its scopes hold no bitmap).
One JSON object per line on stdout (and in --out).

    python benchmarks/scoped_filter_search.py [--rows 10000000] [--reps 20] [--rounds 5] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from codesearch_amd import VectorStore, _lib  # noqa: E402
from codesearch_amd._lib import f32p, u32p  # noqa: E402
from codesearch_amd.synth import synth_rows  # noqa: E402

from scoped_search import Caller, median_ms  # noqa: E402


def masks(n, rng):
    far = n // 2 + n // 8
    return {
        "all": np.arange(n),
        "random_50": np.sort(rng.choice(n, n // 2, replace=False)),
        "random_25": np.sort(rng.choice(n, n // 4, replace=False)),
        "random_10": np.sort(rng.choice(n, n // 10, replace=False)),
        "contiguous_10_far": np.arange(far, far + n // 10),
        "two_blocks_5": np.concatenate([np.arange(n // 20, n // 10), np.arange(n - n // 10, n - n // 20)]),
    }


def unscoped(call, q):
    """The same search with no scope, on its default route (the variants form for the variants shape)."""
    if not call.variants:
        return call.stream(q)
    _lib.check(call.st._fn("search_variants")(call.st.handle, q.ctypes.data_as(f32p), call.nq, call.dim, call.k, *call._tail()))


def create_and_refresh_ms(st, ids32, rounds):
    """Median time of cs_index_scope_create and of one refresh (a build that changes nothing, then cs_scope_info does not
    refresh: the first scoped search does — timed as that search minus the same search again)."""
    create = []
    for _ in range(rounds + 1):
        t0 = time.perf_counter()
        h = C.c_void_p()
        _lib.check(st._fn("scope_create")(st.handle, ids32.ctypes.data_as(u32p), ids32.size, C.byref(h)))
        create.append((time.perf_counter() - t0) * 1e3)
        st._lib.cs_scope_destroy(h)
    sc = st.scope(ids32)
    sc.set_route("gather")
    q = synth_rows(0x9E5, 0, 1, st.dimensions)
    call = Caller(st, 1, st.dimensions, 10, False)
    call.scoped(q, sc)
    refresh = []
    for _ in range(rounds):
        st.build_index()
        t0 = time.perf_counter()
        call.scoped(q, sc)
        t1 = time.perf_counter()
        call.scoped(q, sc)
        refresh.append(((t1 - t0) - (time.perf_counter() - t1)) * 1e3)
    extra = sc.route_info()[3]
    sc.close()
    return float(np.median(create[1:])), float(np.median(refresh)), extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-plain-store", action="store_true", help="skip the second store (creation / refresh without the bitmap)")
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    n, dim = a.rows, a.dim
    st = VectorStore(None, dim)
    st.insert_synthetic(n, 0x5EA4C4, 0)
    st.build_index()
    plain = None
    if not a.no_plain_store:
        os.environ["CS_FILTER_INT8"] = "0"  # read at cs_index_create: this index keeps no int8 copy, its scopes no bitmap
        plain = VectorStore(None, dim)
        del os.environ["CS_FILTER_INT8"]
        plain.insert_synthetic(n, 0x5EA4C4, 0)
        plain.build_index()
    rng = np.random.default_rng(1)
    qs = synth_rows(0x9E4, 0, 9, dim)
    shapes = [("q1_k10", 1, 10, False), ("q1_k200", 1, 200, False), ("v9_k200", 9, 200, True)]
    for mname, ids in masks(n, rng).items():
        ids32 = np.ascontiguousarray(ids, np.uint32)
        c_with, r_with, extra = create_and_refresh_ms(st, ids32, a.rounds)
        rec = {"mask": mname, "allowed": int(ids.size), "extra_bytes": int(extra), "scope_create_ms": round(c_with, 4),
               "refresh_ms": round(r_with, 4)}
        if plain is not None:
            c_wo, r_wo, extra_wo = create_and_refresh_ms(plain, ids32, a.rounds)
            rec.update({"scope_create_no_bitmap_ms": round(c_wo, 4), "refresh_no_bitmap_ms": round(r_wo, 4),
                        "extra_bytes_no_bitmap": int(extra_wo)})
        emit(rec)
        scope = st.scope(ids)
        for sname, nq, k, variants in shapes:
            q = np.ascontiguousarray(qs[:nq])
            call = Caller(st, nq, dim, k, variants)
            scope.set_route("gather")
            call.scoped(q, scope)  # warm-up of both routes, and the outputs compared
            want = call.answer()
            scope.set_route("filter")
            f0 = scope.route_info()[0]
            call.scoped(q, scope)
            same = call.answer() == want
            took_filter = scope.route_info()[0] == f0 + 1
            scope.set_route("auto")
            f0 = scope.route_info()[0]
            call.scoped(q, scope)
            auto = "filter" if scope.route_info()[0] == f0 + 1 else "gather"
            unscoped(call, q)
            tg, tf, tu = [], [], []
            for _ in range(a.rounds):
                scope.set_route("gather")
                tg.append(median_ms(lambda: call.scoped(q, scope), a.reps))
                scope.set_route("filter")
                tf.append(median_ms(lambda: call.scoped(q, scope), a.reps))
                tu.append(median_ms(lambda: unscoped(call, q), a.reps))
            rec = {"shape": sname, "mask": mname, "allowed": int(ids.size), "same_bytes": bool(same),
                   "forced_filter_took_filter": bool(took_filter), "auto_route": auto,
                   "span_over_live": round(float(int(ids[-1]) - int(ids[0]) + 1) / ids.size, 3),
                   "gather_ms": round(float(np.median(tg)), 4), "gather_spread_ms": round(max(tg) - min(tg), 4),
                   "filter_ms": round(float(np.median(tf)), 4), "filter_spread_ms": round(max(tf) - min(tf), 4),
                   "unscoped_ms": round(float(np.median(tu)), 4), "unscoped_spread_ms": round(max(tu) - min(tu), 4),
                   "overflow_reruns": scope.route_info()[2]}
            rec["filter_over_gather"] = round(rec["filter_ms"] / rec["gather_ms"], 4)
            emit(rec)
        scope.close()
    if out:
        out.close()
    if plain is not None:
        plain.close()
    st.close()


if __name__ == "__main__":
    main()
