"""Scope algebra on the device (cs_scope_combine, cs_index_scope_create_range) against what a caller does without it — numpy's
set operation on the two id arrays followed by VectorStore.scope(ids), i.e. a host pass and an upload — in one process,
alternated (device, host, device, host, ...), medians over --reps calls of each, every time host to host: from the call to a
scope whose row list is made and ready to search.

    python benchmarks/scope_algebra.py [--rows 10000000] [--dim 384] [--reps 5] [--out FILE]

The store: --rows synthetic rows, built.  Prepared scopes: a random 10 % (r10), a random 50 % (r50) and a contiguous 10 % (c10,
starting at 30 % of the ids).  Pairs: r50 x r10, r50 x c10, r10 x c10, r50 x r50 (two handles of the same ids), and the
exclusion all - r10, whose device time includes making the range scope of every id and whose host time includes np.arange.
Per pair and operation one JSON object per line on stdout (and appended to --out): device_ms, host_ms (= numpy_ms +
scope_create_ms, also given apart), the sizes, and whether the device-made scope's ids equal the host-made ones byte for
byte.  Then, for the union r50 | r10, one scoped search of 1 query and one of 9 variants through each route (auto, gather,
filter) on the device-made scope and on its host-made twin: the times and whether the answers' bytes agree."""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from codesearch_amd import VectorStore
    from codesearch_amd.synth import synth_rows

    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    n, dim = a.rows, a.dim
    st = VectorStore(None, dim, capacity=n)
    st.insert_synthetic(n, 0x5C09EA, 0)
    st.build_index()
    rng = np.random.default_rng(8)
    ids = {"r10": np.sort(rng.choice(n, n // 10, replace=False)).astype(np.uint32),
           "r50": np.sort(rng.choice(n, n // 2, replace=False)).astype(np.uint32),
           "c10": np.arange(3 * n // 10, 4 * n // 10, dtype=np.uint32)}
    ids["r50'"] = ids["r50"]
    scopes = {k: st.scope(v) for k, v in ids.items()}
    np_ops = {"union": np.union1d, "intersection": np.intersect1d, "difference": np.setdiff1d}
    ms = lambda t0: (time.perf_counter() - t0) * 1e3
    med = lambda v: float(np.median(v))

    def bench(label, device_fn, host_fn):
        """device_fn() -> Scope; host_fn() -> (Scope, numpy_ms).  Alternated; the last of each is compared and closed."""
        dev, host, host_np = [], [], []
        same = None
        for r in range(a.reps + 1):  # (one unrecorded warm-up round: first launches, first allocations)
            t0 = time.perf_counter()
            d = device_fn()
            t_d = ms(t0)
            t0 = time.perf_counter()
            h, t_np = host_fn()
            t_h = ms(t0)
            if r:
                dev.append(t_d)
                host.append(t_h)
                host_np.append(t_np)
            if r == a.reps:
                same = d.ids.tobytes() == h.ids.tobytes() and d.info()[:2] == h.info()[:2]
                label.update(n_out=len(d), live_rows=d.info()[1])
            d.close()
            h.close()
        emit(dict(label, rows=n, dim=dim, reps=a.reps, device_ms=round(med(dev), 3), host_ms=round(med(host), 3),
                  numpy_ms=round(med(host_np), 3), scope_create_ms=round(med(host) - med(host_np), 3),
                  speedup=round(med(host) / med(dev), 2), same_ids=bool(same)))

    for x, y in (("r50", "r10"), ("r50", "c10"), ("r10", "c10"), ("r50", "r50'")):
        for op, f in np_ops.items():
            def host_fn(f=f, x=x, y=y):
                t0 = time.perf_counter()
                v = f(ids[x], ids[y])
                t_np = ms(t0)
                return st.scope(v), t_np
            bench({"what": "combine", "op": op, "a": x, "b": y, "n_a": int(ids[x].size), "n_b": int(ids[y].size)},
                  lambda op=op, x=x, y=y: getattr(scopes[x], op)(scopes[y]), host_fn)

    def device_rest():
        with st.scope_all() as every:
            return every - scopes["r10"]

    def host_rest():
        t0 = time.perf_counter()
        v = np.setdiff1d(np.arange(n, dtype=np.uint32), ids["r10"])
        t_np = ms(t0)
        return st.scope(v), t_np

    bench({"what": "exclusion", "op": "difference", "a": "all", "b": "r10", "n_a": n, "n_b": int(ids["r10"].size)},
          device_rest, host_rest)

    def device_range():
        return st.scope_all()

    def host_range():
        t0 = time.perf_counter()
        v = np.arange(n, dtype=np.uint32)
        t_np = ms(t0)
        return st.scope(v), t_np

    bench({"what": "range", "op": "range", "a": "all", "b": "", "n_a": n, "n_b": 0}, device_range, host_range)

    # the result is a first-class scope: one search through each route, against the host-made twin
    queries = synth_rows(0x5C09EB, 0, 9, dim)
    got = scopes["r50"] | scopes["r10"]
    twin = st.scope(np.union1d(ids["r50"], ids["r10"]))
    for route in ("auto", "gather", "filter"):
        rec = {"what": "search", "route": route, "rows": n, "dim": dim, "n_ids": len(got)}
        for name, sc in (("device_made", got), ("host_made", twin)):
            sc.set_route(route)
            st.search_raw(queries[0], 10, scope=sc)  # warm
            t1, tv = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                one = st.search_raw(queries[0], 10, scope=sc)
                t1.append(ms(t0))
                t0 = time.perf_counter()
                var = st.search_variants_raw(queries, 10, scope=sc)
                tv.append(ms(t0))
            rec[name + "_search_ms"] = round(med(t1), 3)
            rec[name + "_variants_ms"] = round(med(tv), 3)
            rec[name] = [x.tobytes() if isinstance(x, np.ndarray) else x for x in one + var]
        rec["same_answers"] = rec.pop("device_made") == rec.pop("host_made")
        rec["route_info_device_made"] = list(got.route_info())
        rec["route_info_host_made"] = list(twin.route_info())
        emit(rec)
    st.close()


if __name__ == "__main__":
    main()
