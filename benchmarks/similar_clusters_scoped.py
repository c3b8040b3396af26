"""Scoped similar-clusters search (cs_index_similar_clusters_scoped) against the two calls a caller had before it, over the
stores of benchmarks/similar_clusters.py, in one process, alternated per scope (scoped x reps, (a) x reps, scoped x reps,
(b) x reps; the scoped figure is the median over its 2 x reps calls):

  (a) the unscoped clusters call (cs_index_similar_clusters) — which pays the whole store's triangle and answers another
      question (its labels restricted to the scope join chunks through chunks outside it), so only its time is compared;
  (b) the scoped pairs call (cs_index_similar_pairs_scoped, max_pairs 1 << 20) followed by search.clusters_of_pairs on the
      host, timed apart.  Where it answers uncut, its labels are compared with the scoped call's; where it refuses (a scope
      that holds the file of near-duplicates), the time to the refusal is recorded.

    python benchmarks/similar_clusters_scoped.py [--rows 100000] [--dim 384] [--reps 3] [--layouts pairs,first,last] [--out FILE]

The stores: synthetic rows in files of 8 ids; one file of --hog (10,000) near-duplicates of one row; 1 % of the rows in
planted clone pairs at cosines 0.92 .. 0.99, each clone in another file.  --layouts says where the hog file sits among the
ids ("pairs": behind the synthetic rows, "first", "last").  Bound 0.9, both modes.
Scopes: every id; a random 10 %; a contiguous 10 % (the first tenth of the ids); a random 1 %; the random 10 % against its
complement; the hog file plus a random 1 %.  One JSON object per line on stdout (and in --out), with what
cs_index_similar_clusters_info / _scoped_info report of the scoped call's last run."""
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-pairs", type=int, default=1 << 20)
    ap.add_argument("--min-cos", type=float, default=0.9)
    ap.add_argument("--layouts", default="pairs,first,last")
    ap.add_argument("--modes", default="other_group,all")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from codesearch_amd import VectorStore, _lib
    from codesearch_amd.search import clusters_of_pairs
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
    bound = np.float32(a.min_cos)
    tiles = (n + 127) // 128

    def build(layout):
        """benchmarks/similar_clusters.py's store -> (the store, the hog file's first id)."""
        rng = np.random.default_rng(4)
        s_row = synth_rows(seed, n_syn, 1, dim)
        scale = float(np.linalg.norm(s_row)) / np.sqrt(dim)
        hog = np.float32(0.95) * s_row + np.float32(0.05) * rng.standard_normal((a.hog, dim), dtype=np.float32) * np.float32(scale)
        hog[0] = s_row[0]
        src = synth_rows(seed, 0, n_src, dim).astype(np.float64)
        u = src / np.linalg.norm(src, axis=1, keepdims=True)
        w = rng.standard_normal((n_src, dim))
        w -= (w * u).sum(1, keepdims=True) * u
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        c = rng.uniform(0.92, 0.99, (n_src, 1))
        clones = (np.linalg.norm(src, axis=1, keepdims=True) * (c * u + np.sqrt(1 - c * c) * w)).astype(np.float32)
        order = {"pairs": ("syn", "hog", "clones"), "first": ("hog", "syn", "clones"), "last": ("syn", "clones", "hog")}[layout]
        st = VectorStore(None, dim, capacity=n)
        hog_at = 0
        for seg in order:
            if seg == "syn":
                st.insert_synthetic(n_syn, seed, 0)
            elif seg == "hog":
                hog_at = st.next_id()
                st.insert_embeddings(hog)
            else:
                st.insert_embeddings(clones)
        st.build_index()
        assert st.next_id() == n
        ids = np.arange(n, dtype=np.uint32)
        groups = ids // 8 + np.uint32(1)
        groups[hog_at:hog_at + a.hog] = 0xFFFFFFF0
        st.set_groups(ids, groups)
        return st, hog_at

    def timed(call):
        t0 = time.perf_counter()
        r = call()
        return (time.perf_counter() - t0) * 1e3, r

    for layout in a.layouts.split(","):
        st, hog_at = build(layout)
        ids = np.arange(n, dtype=np.uint32)
        pick = np.random.default_rng(11)
        tenth = np.sort(pick.choice(n, n // 10, replace=False)).astype(np.uint32)
        rest = np.setdiff1d(ids, tenth).astype(np.uint32)
        hundredth = np.sort(pick.choice(n, n // 100, replace=False)).astype(np.uint32)
        hog_ids = ids[hog_at:hog_at + a.hog]
        cases = [("all ids", ids, None), ("random 10 %", tenth, None), ("contiguous 10 %", ids[:n // 10], None),
                 ("random 1 %", hundredth, None), ("random 10 % x complement", tenth, rest),
                 ("hog file + random 1 %", np.union1d(hog_ids, hundredth).astype(np.uint32), None)]
        for name, ids_a, ids_b in cases:
            sa = st.scope(ids_a)
            sb = None if ids_b is None else st.scope(ids_b)
            vertices = ids_a if ids_b is None else np.union1d(ids_a, ids_b)
            for mode in a.modes.split(","):
                other = mode == "other_group"
                scoped = lambda: st.similar_clusters_scoped_raw(bound, other, sa, sb)
                unscoped = lambda: st.similar_clusters_raw(bound, other_files=other)

                def pairs():
                    try:
                        return st.similar_pairs_raw(bound, other_files=other, max_pairs=a.max_pairs, scope=sa, other=sb), None
                    except _lib.CsError as e:
                        if e.code != _lib.CS_ERR_UNSUPPORTED:
                            raise
                        return None, str(e)

                scoped()  # untimed: code objects, the pooled buffers, the scopes' lists
                unscoped()
                pairs()
                ts = [timed(scoped) for _ in range(a.reps)]
                ta = [timed(unscoped) for _ in range(a.reps)]
                ts += [timed(scoped) for _ in range(a.reps)]
                info = st.similar_clusters_info(scoped=True)  # the scoped call's last run
                tb = [timed(pairs) for _ in range(a.reps)]
                ws, wa, wb = [t for t, _ in ts], [t for t, _ in ta], [t for t, _ in tb]
                got_ids, got_labels, n_clusters, n_members = ts[-1][1]
                plan_pairs = info["tile_pairs_scored"] + info["tile_pairs_skipped"]
                rec = {"rows": n, "dim": dim, "layout": layout, "hog_first_id": int(hog_at), "scope": name, "mode": mode,
                       "min_cos": float(bound), "rows_a": info["rows_a"], "rows_b": info["rows_b"], "vertices": info["vertices"],
                       "reps": a.reps, "scoped_ms": round(float(np.median(ws)), 3), "scoped_min_ms": round(min(ws), 3),
                       "scoped_max_ms": round(max(ws), 3), "unscoped_clusters_ms": round(float(np.median(wa)), 3),
                       "ratio_vs_unscoped_clusters": round(float(np.median(ws)) / float(np.median(wa)), 4),
                       "clusters": n_clusters, "members": n_members,
                       "largest_class": int(np.unique(got_labels, return_counts=True)[1].max()) if len(got_labels) else 0,
                       "tile_pairs": plan_pairs, "tile_pairs_share_of_store": round(plan_pairs / (tiles * (tiles + 1) // 2), 4),
                       "tile_pairs_scored": info["tile_pairs_scored"], "tile_pairs_skipped": info["tile_pairs_skipped"],
                       "rescored_pairs": info["rescored_pairs"], "launches": info["launches"], "pack_ms": round(info["pack_ms"], 3),
                       "join_ms": round(info["join_ms"], 3), "label_ms": round(info["label_ms"], 3),
                       "scoped_pairs_ms": round(float(np.median(wb)), 3)}
                r, refusal = tb[-1][1]
                rec["scoped_pairs_refused"] = refusal is not None
                if refusal is None:
                    rec.update({"pairs_total": r[3], "pairs_cut": r[3] > a.max_pairs})
                    if r[3] <= a.max_pairs:
                        t0 = time.perf_counter()
                        want, wc, wm = clusters_of_pairs(vertices.tolist(), r[1], r[2])
                        rec["host_reduce_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                        rec["scoped_pairs_plus_reduce_ms"] = round(rec["scoped_pairs_ms"] + rec["host_reduce_ms"], 3)
                        rec["labels_match"] = bool((wc, wm) == (n_clusters, n_members) and got_ids.tolist() == vertices.tolist()
                                                   and all(want[i] == lab for i, lab in zip(got_ids.tolist(), got_labels.tolist())))
                else:
                    rec["scoped_pairs_refusal"] = refusal
                emit(rec)
            sa.close()
            if sb is not None:
                sb.close()
        st.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
