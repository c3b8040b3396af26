"""Boosted search (cs_index_search_boosted / _scoped) against the unmasked streaming search — and, for the scoped call, the
scoped search on the gathered route — over the same 10M x 384 store, in one process, alternated (boosted, plain, boosted
again, --reps calls each): per case and k the median wall time of the host-buffer call over both boosted series, each
series' own median, and the ratio to the plain search's median of the same run.  The kind15 case also records how many of
the exact boosted top-k the reference's method finds — rank k hits, then boost them (src/search/mod.rs:238-252): the set it
can return is the streaming top-k.  One JSON object per line on stdout (and in --out).

    python benchmarks/boosted_search.py [--rows 10000000] [--dim 384] [--reps 20] [--out FILE]

Cases (one query per call):
  ones      every id has a class (id % 18), every weight is 1: the pure cost of the form
  kind15    15 % of the rows in one class at 1.15, the rest in another at 1: the reference's kind boost
  lang414   414 classes (23 languages x 18 kinds), 1.2 for one language, 1.15 for one kind, f32(1.2 * 1.15) for both
  hot4      id % 18, one class at 4.0: the pre-gate admits every row within a factor 4 of the k-th best
  scoped    kind15's classes and table through scopes of all ids, 10 % and 1 % of them"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from codesearch_amd import VectorStore, _lib  # noqa: E402
from codesearch_amd._lib import f32p, u32p  # noqa: E402
from codesearch_amd.synth import synth_rows  # noqa: E402


class Caller:
    def __init__(self, st, dim, k):
        self.st, self.dim, self.k = st, dim, k
        self.score = np.zeros((1, k), np.float32)
        self.cos = np.zeros((1, k), np.float32)
        self.ids = np.zeros((1, k), np.uint32)
        self.cnt = np.zeros(1, np.uint32)

    def run(self, q, weights=None, scope=None):
        lib, h = self.st._lib, self.st.handle
        qp, sp, cp = q.ctypes.data_as(f32p), self.score.ctypes.data_as(f32p), self.cos.ctypes.data_as(f32p)
        ip, np_ = self.ids.ctypes.data_as(u32p), self.cnt.ctypes.data_as(u32p)
        if weights is None:
            if scope is None:
                s = lib.cs_index_search(h, qp, 1, self.dim, self.k, cp, ip, np_)
            else:
                s = lib.cs_index_search_scoped(h, scope.handle, qp, 1, self.dim, self.k, cp, ip, np_)
        else:
            wp = weights.ctypes.data_as(f32p)
            if scope is None:
                s = lib.cs_index_search_boosted(h, qp, 1, self.dim, self.k, wp, weights.size, sp, cp, ip, np_)
            else:
                s = lib.cs_index_search_boosted_scoped(h, scope.handle, qp, 1, self.dim, self.k, wp, weights.size, sp, cp, ip, np_)
        _lib.check(s)
        return self.ids[0][:int(self.cnt[0])].copy()


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
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    n, dim = a.rows, a.dim
    q = np.ascontiguousarray(synth_rows(0xB005, 0, 1, dim))
    st = VectorStore(None, dim, capacity=n)
    st.insert_synthetic(n, 0x5EA4C5, 0)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    ids = np.arange(n, dtype=np.uint32)
    kinds = np.ones(18, np.float32)
    kinds[3] = np.float32(1.15)
    lang = np.ones((23, 18), np.float32)
    lang[5, :] = np.float32(1.2)
    lang[:, 3] = np.float32(1.15)
    lang[5, 3] = np.float32(1.2) * np.float32(1.15)
    hot = np.ones(18, np.float32)
    hot[3] = 4.0
    kind15 = np.where(ids % 20 < 3, 3, 0).astype(np.uint16)
    cases = [
        ("ones", (ids % 18).astype(np.uint16), np.ones(18, np.float32)),
        ("kind15", kind15, kinds),
        ("lang414", (ids % 414).astype(np.uint16), np.ascontiguousarray(lang.ravel())),
        ("hot4", (ids % 18).astype(np.uint16), hot),
    ]
    med = lambda t: round(float(np.median(t)), 4)  # noqa: E731

    def measure(rec, call, weights, scope):
        t0 = time.perf_counter()
        call.run(q, weights, scope)  # the first search after an assignment uploads the table
        rec["first_search_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        t1 = timed(lambda: call.run(q, weights, scope), a.reps)
        tp = timed(lambda: call.run(q, None, scope), a.reps)
        t2 = timed(lambda: call.run(q, weights, scope), a.reps)
        rec.update({"boosted_ms": med(t1 + t2), "boosted_before_ms": med(t1), "boosted_after_ms": med(t2), "plain_ms": med(tp),
                    "reps": a.reps})
        rec["ratio_vs_plain"] = round(rec["boosted_ms"] / rec["plain_ms"], 4)

    for cname, classes, weights in cases:
        t0 = time.perf_counter()
        st.set_classes(ids, classes)
        set_ms = (time.perf_counter() - t0) * 1e3
        for k in (10, 200):
            call = Caller(st, dim, k)
            rec = {"case": cname, "rows": n, "dim": dim, "k": k, "n_classes": int(weights.size), "plain": "cs_index_search (streaming)",
                   "set_classes_ms": round(set_ms, 1)}
            measure(rec, call, weights, None)
            exact = call.run(q, weights)
            rec["count"] = int(exact.size)
            if cname == "kind15":  # the reference's method: rank k, then boost — it can only return the streaming top-k
                ranked = call.run(q)
                rec["rank_then_boost_exact_found"] = len(set(exact.tolist()) & set(ranked.tolist()))
                rec["boosted_class_hits"] = int((classes[exact] == 3).sum())
            emit(rec)
    st.set_classes(ids, kind15)
    rng = np.random.default_rng(4)
    for sname, chosen in (("all", ids), ("10pct", np.sort(rng.choice(ids, n // 10, replace=False))),
                          ("1pct", np.sort(rng.choice(ids, n // 100, replace=False)))):
        sc = st.scope(chosen)
        sc.set_route("gather")
        for k in (10, 200):
            call = Caller(st, dim, k)
            rec = {"case": "scoped_" + sname, "rows": n, "scope_rows": int(chosen.size), "dim": dim, "k": k, "n_classes": 18,
                   "plain": "cs_index_search_scoped (gathered)"}
            measure(rec, call, kinds, sc)
            rec["count"] = int(call.run(q, kinds, sc).size)
            emit(rec)
        sc.close()
    st.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
