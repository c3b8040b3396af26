"""Masked search (cs_index_search_masked) against the unmasked search over the same 10M x 384 store, in one process,
alternated: per mask shape and search shape, the median wall time of the host-buffer call, and the recall@limit of the
reference's own method (unmasked top limit * 3, then drop what the mask excludes: src/mcp/mod.rs:251-252,400-425) against
the exact masked answer.  One JSON object per line on stdout (and in --out).

    python benchmarks/masked_search.py [--rows 10000000] [--reps 30] [--out FILE] [--no-prime-store]

--no-prime-store: also build a second store with the prime pass off (CS_SCAN_PRIME_MIN_K=0) and time the masked searches
there (the prime A/B of the masked path)."""
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


def masks(n, rng):
    c10, c1 = n // 10, n // 100
    return {
        "all": np.arange(n),
        "random50": np.sort(rng.choice(n, n // 2, replace=False)),
        "contig10": np.arange(n // 3, n // 3 + c10),
        "random10": np.sort(rng.choice(n, c10, replace=False)),
        "contig1": np.arange(n // 2, n // 2 + c1),
        "random1": np.sort(rng.choice(n, c1, replace=False)),
        "contig1000": np.arange(7 * n // 10, 7 * n // 10 + 1000),
        "empty": np.zeros(0, np.int64),
    }


class Caller:
    def __init__(self, st, nq, dim, k):
        self.st, self.nq, self.dim, self.k = st, nq, dim, k
        self.cos = np.zeros((nq, k), np.float32)
        self.ids = np.zeros((nq, k), np.uint32)
        self.cnt = np.zeros(nq, np.uint32)
        self.vc, self.vf = C.c_uint32(), C.c_int32()

    def run(self, q, words=None, bits=0, variants=False):
        st, h = self.st, self.st.handle
        qp, cp, ip = q.ctypes.data_as(f32p), self.cos.ctypes.data_as(f32p), self.ids.ctypes.data_as(u32p)
        wp = words.ctypes.data_as(u32p) if words is not None and words.size else None
        if variants and words is None:
            s = st._fn("search_variants")(h, qp, self.nq, self.dim, self.k, cp, ip, C.byref(self.vc), C.byref(self.vf))
        elif variants:
            s = st._fn("search_variants_masked")(h, qp, self.nq, self.dim, self.k, wp, bits, cp, ip, C.byref(self.vc),
                                                 C.byref(self.vf))
        elif words is None:
            s = st._fn("search")(h, qp, self.nq, self.dim, self.k, cp, ip, self.cnt.ctypes.data_as(u32p))
        else:
            s = st._fn("search_masked")(h, qp, self.nq, self.dim, self.k, wp, bits, cp, ip, self.cnt.ctypes.data_as(u32p))
        _lib.check(s)


def timed(fn, reps):
    fn()
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-prime-store", action="store_true")
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
    st2 = None
    if a.no_prime_store:
        os.environ["CS_SCAN_PRIME_MIN_K"] = "0"
        st2 = VectorStore(None, dim)
        del os.environ["CS_SCAN_PRIME_MIN_K"]
        st2.insert_synthetic(n, 0x5EA4C4, 0)
        st2.build_index()
    rng = np.random.default_rng(1)
    ms = {name: (ids, allow_mask(ids, n)) for name, ids in masks(n, rng).items()}
    qs = synth_rows(0x9E4, 0, 9, dim)
    shapes = [("q1_k10", 1, 10, False), ("q1_k200", 1, 200, False), ("v9_k200", 9, 200, True)]
    for sname, nq, k, variants in shapes:
        q = np.ascontiguousarray(qs[:nq])
        call = Caller(st, nq, dim, k)
        base = {}
        for route in ("stream", "cost"):
            st.set_single_query_route(st.ROUTE_STREAM if route == "stream" else st.ROUTE_COST)
            base[route] = timed(lambda: call.run(q, variants=variants), a.reps)
        st.set_single_query_route(st.ROUTE_STREAM)
        for mname, (ids, words) in ms.items():
            # alternate: masked, unmasked stream, masked again (the median of both masked runs is reported)
            t1 = timed(lambda: call.run(q, words, n, variants), a.reps)
            ts = timed(lambda: call.run(q, variants=variants), a.reps)
            t2 = timed(lambda: call.run(q, words, n, variants), a.reps)
            rec = {"shape": sname, "mask": mname, "allowed": int(ids.size), "masked_ms": round(min(t1, t2), 4),
                   "stream_ms": round(min(ts, base["stream"]), 4), "cost_ms": round(base["cost"], 4)}
            rec["ratio_vs_stream"] = round(rec["masked_ms"] / rec["stream_ms"], 4)
            if st2 is not None:
                c2 = Caller(st2, nq, dim, k)
                rec["masked_noprime_ms"] = round(timed(lambda: c2.run(q, words, n, variants), a.reps), 4)
            if not variants and k == 10:
                # recall@10 of the reference's post-filter (top 30 unmasked, keep the allowed) against the exact answer
                call.run(q, words, n)
                exact = set(call.ids[0][: int(call.cnt[0])].tolist())
                c30 = Caller(st, 1, dim, 30)
                c30.run(q)
                allowed = np.zeros(n, bool)
                allowed[ids] = True
                post = [i for i in c30.ids[0][: int(c30.cnt[0])].tolist() if allowed[i]][:10]
                rec["postfilter_hits"] = len(post)
                rec["postfilter_recall_at_10"] = round(len(exact & set(post)) / len(exact), 4) if exact else None
            emit(rec)
    if out:
        out.close()


if __name__ == "__main__":
    main()
