"""Scoped search (cs_index_search_scoped) against the masked search (cs_index_search_masked) over the same 10M x 384
store, in one process, ALTERNATED: per mask shape and search shape, `rounds` rounds of (reps masked calls, reps scoped
calls); reported are the median over the rounds of each round's median wall time of the host-buffer call, and the spread
(largest minus smallest round median) of each.  Per mask also: the median time of cs_index_scope_create (host check, id
upload, first making of the row list) and of one refresh (the first scoped search after a build minus the scoped median of
that shape; a refresh waits for the device's work first, idle here).  For one query also the unmasked streaming search in
the same rounds (stream_ms).  Before anything is timed the scoped answer is compared with the masked one, bytes for bytes.
One JSON object per line on stdout (and in --out).

    python benchmarks/scoped_search.py [--rows 10000000] [--reps 20] [--rounds 5] [--out FILE]"""
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
from codesearch_amd.vector_store import allow_mask  # noqa: E402

from masked_search import masks  # noqa: E402  (the masks of DESIGN §8b's table)


class Caller:
    def __init__(self, st, nq, dim, k, variants):
        self.st, self.nq, self.dim, self.k, self.variants = st, nq, dim, k, variants
        self.cos = np.zeros((nq, k), np.float32)
        self.ids = np.zeros((nq, k), np.uint32)
        self.cnt = np.zeros(nq, np.uint32)
        self.vc, self.vf = C.c_uint32(), C.c_int32()

    def _tail(self):
        cp, ip = self.cos.ctypes.data_as(f32p), self.ids.ctypes.data_as(u32p)
        if self.variants:
            return cp, ip, C.byref(self.vc), C.byref(self.vf)
        return cp, ip, self.cnt.ctypes.data_as(u32p)

    def masked(self, q, words, bits):
        fn = self.st._fn("search_variants_masked" if self.variants else "search_masked")
        wp = words.ctypes.data_as(u32p) if words.size else None
        _lib.check(fn(self.st.handle, q.ctypes.data_as(f32p), self.nq, self.dim, self.k, wp, bits if words.size else 0,
                      *self._tail()))

    def scoped(self, q, scope):
        fn = self.st._fn("search_variants_scoped" if self.variants else "search_scoped")
        _lib.check(fn(self.st.handle, scope.handle, q.ctypes.data_as(f32p), self.nq, self.dim, self.k, *self._tail()))

    def stream(self, q):
        """The unmasked search on the streaming route (single query): the denominator of DESIGN §8b's targets."""
        _lib.check(self.st._fn("search")(self.st.handle, q.ctypes.data_as(f32p), self.nq, self.dim, self.k, *self._tail()))

    def answer(self):
        meta = (self.vc.value, self.vf.value) if self.variants else tuple(self.cnt.tolist())
        rows = 1 if self.variants else self.nq
        return self.cos[:rows].tobytes(), self.ids[:rows].tobytes(), meta


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
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
    st = VectorStore(None, dim)
    st.insert_synthetic(n, 0x5EA4C4, 0)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    rng = np.random.default_rng(1)
    qs = synth_rows(0x9E4, 0, 9, dim)
    shapes = [("q1_k10", 1, 10, False), ("q1_k200", 1, 200, False), ("v9_k200", 9, 200, True)]
    for mname, ids in masks(n, rng).items():
        words = allow_mask(ids, n)
        # scope creation: the caller's list is already sorted u32 (VectorStore.chunk_ids_under returns one)
        ids32 = np.ascontiguousarray(ids, np.uint32)
        create = []
        for _ in range(a.rounds + 1):
            t0 = time.perf_counter()
            h = C.c_void_p()
            _lib.check(st._fn("scope_create")(st.handle, ids32.ctypes.data_as(u32p) if ids32.size else None, ids32.size,
                                              C.byref(h)))
            create.append((time.perf_counter() - t0) * 1e3)
            st._lib.cs_scope_destroy(h)
        scope = st.scope(ids)
        for sname, nq, k, variants in shapes:
            q = np.ascontiguousarray(qs[:nq])
            call = Caller(st, nq, dim, k, variants)
            call.masked(q, words, n)   # warm-up of both paths, and the outputs compared
            want = call.answer()
            call.scoped(q, scope)
            same = call.answer() == want
            tm, tsc, tst = [], [], []
            for _ in range(a.rounds):
                tm.append(median_ms(lambda: call.masked(q, words, n), a.reps))
                tsc.append(median_ms(lambda: call.scoped(q, scope), a.reps))
                if not variants:  # (nine unmasked variants take the int8 filter route: no stream to compare with)
                    tst.append(median_ms(lambda: call.stream(q), a.reps))
            # one refresh: a build (nothing changed, the generation advances), then the first scoped search
            first = []
            for _ in range(a.rounds):
                st.build_index()
                t0 = time.perf_counter()
                call.scoped(q, scope)
                first.append((time.perf_counter() - t0) * 1e3)
            rec = {"shape": sname, "mask": mname, "allowed": int(ids.size), "same_bytes": bool(same),
                   "masked_ms": round(float(np.median(tm)), 4), "masked_spread_ms": round(max(tm) - min(tm), 4),
                   "scoped_ms": round(float(np.median(tsc)), 4), "scoped_spread_ms": round(max(tsc) - min(tsc), 4),
                   "scope_create_ms": round(float(np.median(create[1:])), 4),
                   "first_after_build_ms": round(float(np.median(first)), 4)}
            rec["refresh_ms"] = round(rec["first_after_build_ms"] - rec["scoped_ms"], 4)
            rec["scoped_over_masked"] = round(rec["scoped_ms"] / rec["masked_ms"], 4)
            if tst:
                rec["stream_ms"] = round(float(np.median(tst)), 4)
                rec["scoped_vs_stream"] = round(rec["scoped_ms"] / rec["stream_ms"], 4)
            rec["live_rows"], rec["refreshes"] = scope.info()[1:]
            emit(rec)
        scope.close()
    if out:
        out.close()
    st.close()


if __name__ == "__main__":
    main()
