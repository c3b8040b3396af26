"""Scoped similar-pairs search (cs_index_similar_pairs_scoped) against what a caller can do without it, over the store of
benchmarks/similar_pairs.py, in one process:

  * the unscoped call (cs_index_similar_pairs) followed by search.pairs_between on the host — alternated with the scoped
    call (scoped x reps, unscoped x reps, scoped x reps, unscoped x reps), medians over all 2 x reps calls of each;
  * cs_index_search_similar_scoped once per source of the scope, in calls of CS_MAX_QUERIES sources at k = 1,024 with the same
    bound.  --baseline-calls N times only the first N of those calls and scales to all of them: such a figure is marked
    EXTRAPOLATED (similar_scoped_extrapolated: true).

    python benchmarks/similar_pairs_scoped.py [--rows 100000] [--dim 384] [--reps 5] [--baseline-calls 2] [--out FILE]

The store: synthetic rows in files of 8 ids; one file of --hog (10,000) near-duplicates of one row; 1 % of the rows in
planted clone pairs at cosines 0.92 .. 0.99 (sources rows [0, rows / 200), each clone in another file at the end of the
store).  Bound 0.9, CS_PAIRS_OTHER_GROUP, max_pairs 1 << 20.

Scopes: every id; a random 10 %; a contiguous 10 % (the first tenth of the ids); a random 1 %; the random 10 % against its
complement.  Per scope one JSON object per line on stdout (and in --out): the wall times — the unscoped side's with its host
filter (pairs_between: numpy set operations over the scopes' ids) also timed apart: unscoped_call_ms, host_reduce_ms —
whether the scoped answer's bytes equal the reduced unscoped answer's, and from cs_index_similar_pairs_info / _scoped_info the pack's, the filter bands' and the
refine's device time, the ordering's host time, candidates, bands and tile pairs of the scoped call's last run."""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--hog", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-pairs", type=int, default=1 << 20)
    ap.add_argument("--min-cos", type=float, default=0.9)
    ap.add_argument("--baseline-calls", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from codesearch_amd import VectorStore, _lib
    from codesearch_amd.search import pairs_between
    from codesearch_amd.synth import synth_rows

    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    n, dim, seed = a.rows, a.dim, 0x9A125
    n_src = n // 200
    n_syn = n - a.hog - n_src
    assert n_syn > n_src > 0
    rng = np.random.default_rng(4)
    st = VectorStore(None, dim, capacity=n)
    st.insert_synthetic(n_syn, seed, 0)
    s_row = synth_rows(seed, n_syn, 1, dim)
    scale = float(np.linalg.norm(s_row)) / np.sqrt(dim)
    hog = np.float32(0.95) * s_row + np.float32(0.05) * rng.standard_normal((a.hog, dim), dtype=np.float32) * np.float32(scale)
    hog[0] = s_row[0]
    st.insert_embeddings(hog)
    src = synth_rows(seed, 0, n_src, dim).astype(np.float64)
    u = src / np.linalg.norm(src, axis=1, keepdims=True)
    w = rng.standard_normal((n_src, dim))
    w -= (w * u).sum(1, keepdims=True) * u
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    c = rng.uniform(0.92, 0.99, (n_src, 1))
    st.insert_embeddings((np.linalg.norm(src, axis=1, keepdims=True) * (c * u + np.sqrt(1 - c * c) * w)).astype(np.float32))
    st.build_index()
    assert st.next_id() == n
    ids = np.arange(n, dtype=np.uint32)
    groups = ids // 8
    groups[n_syn:n_syn + a.hog] = 0xFFFFFFF0
    st.set_groups(ids, groups)
    bound = np.float32(a.min_cos)

    pick = np.random.default_rng(11)
    tenth = np.sort(pick.choice(n, n // 10, replace=False)).astype(np.uint32)
    rest = np.setdiff1d(ids, tenth).astype(np.uint32)
    cases = [("all ids", ids, None), ("random 10 %", tenth, None), ("contiguous 10 %", ids[:n // 10], None),
             ("random 1 %", np.sort(pick.choice(n, n // 100, replace=False)).astype(np.uint32), None),
             ("random 10 % x complement", tenth, rest)]

    def timed(call):
        t0 = time.perf_counter()
        r = call()
        return (time.perf_counter() - t0) * 1e3, r

    for name, ids_a, ids_b in cases:
        sa = st.scope(ids_a)
        sb = None if ids_b is None else st.scope(ids_b)
        scoped = lambda: st.similar_pairs_raw(bound, other_files=True, max_pairs=a.max_pairs, scope=sa, other=sb)

        reduce_ms = []  # the host filter's share of every unscoped() call, timed apart

        def unscoped():
            full = st.similar_pairs_raw(bound, other_files=True, max_pairs=a.max_pairs)
            assert full[3] <= a.max_pairs  # neither refused nor cut
            t0 = time.perf_counter()
            r = pairs_between(full[0], full[1], full[2], ids_a, ids_a if ids_b is None else ids_b)
            reduce_ms.append((time.perf_counter() - t0) * 1e3)
            return r

        scoped()  # untimed: code objects, the pooled buffers, the scopes' lists
        unscoped()
        reduce_ms.clear()
        ts, tu = [], []
        for _ in range(2):
            ts += [timed(scoped) for _ in range(a.reps)]
            info = st.similar_pairs_info()  # the scoped call's last run
            tu += [timed(unscoped) for _ in range(a.reps)]
        got, want = ts[-1][1], tu[-1][1]
        same = got[3] == want[3] and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(got[:3], want[:3]))
        # the similar-chunk search through the scope, once per source of A
        calls = [ids_a[lo:lo + _lib.CS_MAX_QUERIES] for lo in range(0, len(ids_a), _lib.CS_MAX_QUERIES)]
        timed_calls = calls if a.baseline_calls <= 0 else calls[:a.baseline_calls]
        through = sa if sb is None else sb
        t0 = time.perf_counter()
        cut = 0
        for part in timed_calls:
            cos, hit, cnt = st.similar_raw(part, 1024, exclude="file", min_cos=bound, scope=through)
            cut += int((cnt == 1024).sum())
        tb = (time.perf_counter() - t0) * 1e3
        ws, wu = [t for t, _ in ts], [t for t, _ in tu]
        emit({"rows": n, "dim": dim, "scope": name, "rows_a": int(len(ids_a)), "rows_b": int(len(ids_a if ids_b is None else ids_b)),
              "mode": "other_group", "min_cos": float(bound), "max_pairs": a.max_pairs, "reps": 2 * a.reps,
              "scoped_ms": round(float(np.median(ws)), 3), "scoped_min_ms": round(min(ws), 3), "scoped_max_ms": round(max(ws), 3),
              "unscoped_plus_reduce_ms": round(float(np.median(wu)), 3), "unscoped_min_ms": round(min(wu), 3),
              "unscoped_max_ms": round(max(wu), 3), "host_reduce_ms": round(float(np.median(reduce_ms)), 3),
              "unscoped_call_ms": round(float(np.median(np.array(wu) - np.array(reduce_ms))), 3),
              "ratio_vs_unscoped_call": round(float(np.median(ws)) / float(np.median(np.array(wu) - np.array(reduce_ms))), 4),
              "ratio_vs_unscoped": round(float(np.median(ws)) / float(np.median(wu)), 4),
              "bytes_equal": bool(same), "total": int(got[3]),
              "pack_ms": round(info["pack_ms"], 3), "filter_ms": round(info["filter_ms"], 3), "refine_ms": round(info["refine_ms"], 3),
              "order_ms": round(info["order_ms"], 3), "candidates": info["candidates"], "bands": info["bands"],
              "tile_pairs": info["tile_pairs"],
              "filter_tflops": round(info["tile_pairs"] * 2.0 * 128 * 128 * dim / (info["filter_ms"] * 1e-3) / 1e12, 1)
              if info["filter_ms"] > 0 else None,
              "similar_scoped_ms": round(tb * len(calls) / len(timed_calls), 3), "similar_scoped_timed_ms": round(tb, 3),
              "similar_scoped_calls": len(calls), "similar_scoped_calls_timed": len(timed_calls),
              "similar_scoped_extrapolated": len(timed_calls) < len(calls), "similar_scoped_sources_cut_at_1024": cut})
        sa.close()
        if sb is not None:
            sb.close()
    st.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
