"""Boosted search across query variants, in a scope, under the per-file cap (cs_index_search_variants_boosted and its
_scoped / _grouped / _grouped_scoped forms) against what a caller had before it, over the same 10M x 384 store, in one
process, alternated (new, baseline, new; --reps calls each): per case, scope, k and cap the median wall time of the
host-buffer call over both series of the new call, each series' own median, and two baselines of the same run:

  variants_ms      cs_index_search_variants[_scoped] (uncapped cases) or cs_index_search_variants_grouped[_scoped] (capped
                   cases) of the same variants, scope, k and cap: the same search without the boost
  nine_boosted_ms  one cs_index_search_boosted[_scoped] call per variant (top k each) and the merge on the host: the best
                   a caller could do for the uncapped answer, and what under a cap cannot give the answer at all

One JSON object per line on stdout (and in --out).

    python benchmarks/boosted_variants_search.py [--rows 10000000] [--dim 384] [--nv 9] [--reps 10] [--out FILE]

The store: synthetic rows, with rows [2/10, 3/10) of it replaced by a hog — 0.9 q0 + 0.1 noise (benchmarks/grouped_search.py).
Cases (nine variants per call: the query and eight perturbations of it):
  kind15   15 % of the rows in one class at 1.15, files of 8 ids; a query unrelated to the hog; the whole store, a 10 % and
           a 1 % scope; uncapped, m = 1 and m = 3
  hog      the hog is one file and carries the boosted kind; the hog's query; the whole store; m = 1 and m = 3"""
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
from codesearch_amd.sharded import key_pack  # noqa: E402
from codesearch_amd.synth import synth_rows  # noqa: E402


class Caller:
    def __init__(self, st, dim, nv, k):
        self.st, self.dim, self.nv, self.k = st, dim, nv, k
        self.score = np.zeros((nv, k), np.float32)
        self.cos = np.zeros((nv, k), np.float32)
        self.ids = np.zeros((nv, k), np.uint32)
        self.cnt = np.zeros(nv, np.uint32)
        self.count, self.flag = C.c_uint32(), C.c_int32()

    def _out(self):
        return (self.score.ctypes.data_as(f32p), self.cos.ctypes.data_as(f32p), self.ids.ctypes.data_as(u32p))

    def new(self, q, w, scope, m):
        """The new call -> the ids returned."""
        lib, h = self.st._lib, self.st.handle
        name = "cs_index_search_variants_boosted" + ("_grouped" if m else "") + ("_scoped" if scope else "")
        head = (h,) + ((scope.handle,) if scope else ()) + (q.ctypes.data_as(f32p), self.nv, self.dim, self.k) + ((m,) if m else ())
        _lib.check(getattr(lib, name)(*head, w.ctypes.data_as(f32p), w.size, *self._out(), C.byref(self.count), C.byref(self.flag)))
        return self.ids[0][:self.count.value].copy()

    def variants(self, q, scope, m):
        """The same search without the boost."""
        lib, h = self.st._lib, self.st.handle
        name = "cs_index_search_variants" + ("_grouped" if m else "") + ("_scoped" if scope else "")
        head = (h,) + ((scope.handle,) if scope else ()) + (q.ctypes.data_as(f32p), self.nv, self.dim, self.k) + ((m,) if m else ())
        _lib.check(getattr(lib, name)(*head, *self._out()[1:], C.byref(self.count), C.byref(self.flag)))

    def nine_boosted(self, q, w, scope):
        """One boosted search per variant, merged on the host: best b per id, the first k by key -> the ids."""
        lib, h = self.st._lib, self.st.handle
        wp, cp = w.ctypes.data_as(f32p), self.cnt.ctypes.data_as(u32p)
        for v in range(self.nv):
            out = tuple(C.cast(C.c_void_p(p.ctypes.data + v * self.k * 4), t) for p, t in
                        ((self.score, f32p), (self.cos, f32p), (self.ids, u32p)))
            qv = C.cast(C.c_void_p(q.ctypes.data + v * self.dim * 4), f32p)
            if scope:
                _lib.check(lib.cs_index_search_boosted_scoped(h, scope.handle, qv, 1, self.dim, self.k, wp, w.size, *out, cp))
            else:
                _lib.check(lib.cs_index_search_boosted(h, qv, 1, self.dim, self.k, wp, w.size, *out, cp))
        keys = np.sort(key_pack(self.score.ravel(), self.ids.ravel()))[::-1]
        ids = ~(keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        _, first = np.unique(ids, return_index=True)  # a chunk's best key comes first
        return ids[np.sort(first)][:self.k]


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
    ap.add_argument("--nv", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    n, dim, nv = a.rows, a.dim, a.nv
    hog_lo, hog_n = n // 5, n // 10
    qs = synth_rows(0x9E5, 0, 2, dim)
    noise = synth_rows(0x9E6, 0, 2 * nv, dim)

    def variants_of(q, salt):  # the query and nv - 1 perturbations of it
        return np.ascontiguousarray(np.concatenate([q[None], np.float32(0.9) * q + np.float32(0.1) * noise[salt * nv:salt * nv + nv - 1]]))

    q_hog, q_other = variants_of(qs[0], 0), variants_of(qs[1], 1)
    st = VectorStore(None, dim, capacity=n)
    st.insert_synthetic(hog_lo, 0x5EA4C5, 0)
    rng = np.random.default_rng(2)
    scale = float(np.linalg.norm(qs[0])) / np.sqrt(dim)
    step = 100_000
    for lo in range(0, hog_n, step):
        cnt = min(step, hog_n - lo)
        st.insert_embeddings(np.float32(0.9) * qs[0] + np.float32(0.1) * rng.standard_normal((cnt, dim), dtype=np.float32) * np.float32(scale))
    st.insert_synthetic(n - hog_lo - hog_n, 0x5EA4C5, hog_lo + hog_n)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    assert st.next_id() == n
    ids = np.arange(n, dtype=np.uint32)
    kinds = np.ones(18, np.float32)
    kinds[3] = np.float32(1.15)
    kind15 = np.where(ids % 20 < 3, 3, 0).astype(np.uint16)
    files8 = ids // 8
    hog_files = files8.copy()
    hog_files[hog_lo:hog_lo + hog_n] = 0xFFFFFFF0
    hog_kind = np.zeros(n, np.uint16)
    hog_kind[hog_lo:hog_lo + hog_n] = 3
    med = lambda t: round(float(np.median(t)), 4)  # noqa: E731

    def measure(case, q, scope, scope_rows, k, m):
        call = Caller(st, dim, nv, k)
        rec = {"case": case, "rows": n, "scope_rows": scope_rows, "dim": dim, "nv": nv, "k": k, "m": m, "reps": a.reps}
        t1 = timed(lambda: call.new(q, kinds, scope, m), a.reps)
        tv = timed(lambda: call.variants(q, scope, m), a.reps)
        tb = timed(lambda: call.nine_boosted(q, kinds, scope), a.reps)
        t2 = timed(lambda: call.new(q, kinds, scope, m), a.reps)
        got = call.new(q, kinds, scope, m)
        rec.update({"new_ms": med(t1 + t2), "new_before_ms": med(t1), "new_after_ms": med(t2), "variants_ms": med(tv),
                    "nine_boosted_ms": med(tb), "count": int(got.size)})
        rec["ratio_vs_variants"] = round(rec["new_ms"] / rec["variants_ms"], 4)
        rec["ratio_vs_nine_boosted"] = round(rec["new_ms"] / rec["nine_boosted_ms"], 4)
        merged = call.nine_boosted(q, kinds, scope)
        if m is None:
            rec["same_ids_as_nine_boosted"] = bool(np.array_equal(got, merged))
        else:  # what the host-merged boosted list gives under the cap: the files among its k rows
            groups = hog_files if case == "hog" else files8
            rec["files_returned"] = int(np.unique(groups[got]).size)
            rec["files_in_host_merged_top_k"] = int(np.unique(groups[merged]).size)
        emit(rec)

    st.set_classes(ids, kind15)
    st.set_groups(ids, files8)
    pick = np.random.default_rng(4)
    for sname, chosen in (("all", None), ("10pct", np.sort(pick.choice(ids, n // 10, replace=False))),
                          ("1pct", np.sort(pick.choice(ids, n // 100, replace=False)))):
        sc = st.scope(chosen) if chosen is not None else None
        if sc:
            sc.set_route("gather")
        for k in (10, 200):
            for m in (None, 1, 3):
                measure("kind15", q_other, sc, n if chosen is None else int(chosen.size), k, m)
        if sc:
            sc.close()
    st.set_classes(ids, hog_kind)
    st.set_groups(ids, hog_files)
    for k in (10, 200):
        for m in (1, 3):
            measure("hog", q_hog, None, n, k, m)
    st.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
