"""Grouped search (cs_index_search_grouped) against the unmasked streaming search over the same 10M x 384 store, in one
process, alternated (grouped, streaming, grouped again, --reps calls each): per grouping and search shape, the median
wall time of the host-buffer call over both grouped series, each series' own median, and the ratio to the streaming
search's median of the same run.  The hog case also records what the reference's method finds — rank k hits,
then cap each file's (src/search/mod.rs:1007-1038) — against the exact grouped answer, for a post-cap over k hits and over
1,024 (CS_MAX_K: the most a caller could fetch).  One JSON object per line on stdout (and in --out).

    python benchmarks/grouped_search.py [--rows 10000000] [--dim 384] [--nq 1] [--reps 20] [--out FILE]

--nq N: N queries per call (the case's query, then N - 1 unrelated ones), so that the kernels of two and four queries
per pass are timed; the recorded answers are query 0's.

The store: synthetic rows, with rows [2/10, 3/10) of it replaced by a hog — 0.9 q0 + 0.1 noise, one group.  The hog case
searches q0; every other case searches a query unrelated to the hog."""
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
from codesearch_amd.search import cap_per_group  # noqa: E402
from codesearch_amd.synth import synth_rows  # noqa: E402


class Caller:
    def __init__(self, st, dim, k, nq=1):
        self.st, self.dim, self.k, self.nq = st, dim, k, nq
        self.cos = np.zeros((nq, k), np.float32)
        self.ids = np.zeros((nq, k), np.uint32)
        self.cnt = np.zeros(nq, np.uint32)

    def run(self, q, per_group=None):
        h = self.st.handle
        qp, cp, ip, np_ = q.ctypes.data_as(f32p), self.cos.ctypes.data_as(f32p), self.ids.ctypes.data_as(u32p), self.cnt.ctypes.data_as(u32p)
        if per_group is None:
            s = self.st._lib.cs_index_search(h, qp, self.nq, self.dim, self.k, cp, ip, np_)
        else:
            s = self.st._lib.cs_index_search_grouped(h, qp, self.nq, self.dim, self.k, per_group, cp, ip, np_)
        _lib.check(s)
        n = int(self.cnt[0])
        return self.cos[0][:n].copy(), self.ids[0][:n].copy()


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
    ap.add_argument("--nq", type=int, default=1)
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
    more = synth_rows(0x9E6, 0, max(a.nq - 1, 1), dim)[:a.nq - 1]
    hog_lo, hog_n = n // 5, n // 10
    qs = np.ascontiguousarray(synth_rows(0x9E5, 0, 2, dim))
    q_hog, q_other = qs[0:1], qs[1:2]
    st = VectorStore(None, dim, capacity=n)
    st.insert_synthetic(hog_lo, 0x5EA4C5, 0)
    rng = np.random.default_rng(2)
    scale = float(np.linalg.norm(q_hog)) / np.sqrt(dim)
    step = 100_000
    for lo in range(0, hog_n, step):
        cnt = min(step, hog_n - lo)
        noise = rng.standard_normal((cnt, dim), dtype=np.float32) * np.float32(scale)
        st.insert_embeddings(np.float32(0.9) * q_hog + np.float32(0.1) * noise)
    st.insert_synthetic(n - hog_lo - hog_n, 0x5EA4C5, hog_lo + hog_n)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    assert st.next_id() == n
    ids = np.arange(n, dtype=np.uint32)
    files8 = ids // 8
    hog = files8.copy()
    hog[hog_lo:hog_lo + hog_n] = 0xFFFFFFF0
    cases = [
        ("files8", files8, q_other),            # groups of 8 contiguous ids: the shape of files
        ("groups1000", ids // max(1, n // 1000), q_other),  # 1,000 groups of n / 1,000 ids
        ("groups5", ids % 5, q_other),          # fewer groups than k / m: no list ever fills
        ("hog", hog, q_hog),                    # one group holds a tenth of the store and every near-duplicate of the query
    ]
    for cname, groups, q in cases:
        q = np.ascontiguousarray(np.concatenate([q, more]))
        t0 = time.perf_counter()
        st.set_groups(ids, groups)
        set_ms = (time.perf_counter() - t0) * 1e3
        for k in (10, 200):
            call = Caller(st, dim, k, a.nq)
            for m in (1, 3):
                t0 = time.perf_counter()
                call.run(q, m)  # the first search after an assignment uploads the table
                first_ms = (time.perf_counter() - t0) * 1e3
                # alternate: grouped, streaming, grouped again
                t1 = timed(lambda: call.run(q, m), a.reps)
                ts = timed(lambda: call.run(q), a.reps)
                t2 = timed(lambda: call.run(q, m), a.reps)
                gc, gi = call.run(q, m)
                med = lambda t: round(float(np.median(t)), 4)  # noqa: E731
                rec = {"case": cname, "rows": n, "dim": dim, "nq": a.nq, "k": k, "m": m, "grouped_ms": med(t1 + t2), "grouped_before_ms": med(t1),
                       "grouped_after_ms": med(t2), "stream_ms": med(ts), "reps": a.reps,
                       "count": int(gi.size), "set_groups_ms": round(set_ms, 1), "first_search_ms": round(first_ms, 2)}
                rec["ratio_vs_stream"] = round(rec["grouped_ms"] / rec["stream_ms"], 4)
                # the reference's method: rank, then cap
                exact = set(gi.tolist())
                for depth, name in ((k, "postcap_k"), (1024, "postcap_1024")):
                    c2 = Caller(st, dim, depth)
                    pc, pi = c2.run(q[0:1])
                    post = cap_per_group(pc, pi, groups[pi], k, m)[1]
                    rec[name + "_hits"] = len(post)
                    rec[name + "_exact_found"] = len(exact & set(post))
                emit(rec)
    if out:
        out.close()


if __name__ == "__main__":
    main()
