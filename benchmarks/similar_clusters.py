"""Similar-clusters search (cs_index_similar_clusters) beside what a caller can do without it — cs_index_similar_pairs and a
union-find on the host (search.clusters_of_pairs) — over the same store, in one process, alternated (clusters, pairs,
clusters again).  One JSON object per line on stdout (and in --out).

    python benchmarks/similar_clusters.py [--rows 100000] [--dim 384] [--reps 5] [--layouts pairs,first,last] [--out FILE]

The stores are those of benchmarks/similar_pairs.py: synthetic rows in files of 8 ids; one file of --hog (10,000)
near-duplicates of one row (0.95 s + 0.05 noise); 1 % of the rows in planted clone pairs at cosines 0.92 .. 0.99, each clone
in another file.  Bound 0.9, both modes.  --layouts says where the hog file sits among the ids: "pairs" is that benchmark's
order (synthetic rows, the hog, the clones), "first" puts the hog at the front of the store, "last" at its end.

Per layout and mode: the wall time of the clusters call (median of 2 x --reps, after one untimed call) with what
cs_index_similar_clusters_info reports of the last one (tile pairs scored and skipped, pairs re-scored, launches, device
time of the launches and of the labelling), and the wall time of the pairs call with max_pairs 1 << 20 — answered
(other_group: its pairs are then reduced on the host, timed apart, and the two label arrays compared) or refused (all: the
hog file alone holds 5e7 pairs), with the time the refusal took."""
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
    ap.add_argument("--layouts", default="pairs,first,last")
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
        """-> the store; the segments in id order and the hog's group assigned."""
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

    def clusters(st, other):
        t0 = time.perf_counter()
        r = st.similar_clusters_raw(bound, other_files=other)
        return time.perf_counter() - t0, r

    def pairs(st, other):
        t0 = time.perf_counter()
        try:
            r = st.similar_pairs_raw(bound, other_files=other, max_pairs=a.max_pairs)
        except _lib.CsError as e:
            if e.code != _lib.CS_ERR_UNSUPPORTED:
                raise
            return time.perf_counter() - t0, None, str(e)
        return time.perf_counter() - t0, r, None

    for layout in a.layouts.split(","):
        st, hog_at = build(layout)
        for other in (True, False):
            rec = {"rows": n, "dim": dim, "layout": layout, "hog_first_id": int(hog_at), "mode": "other_group" if other else "all",
                   "min_cos": float(bound), "hog_rows": a.hog, "planted_pairs": n_src, "reps": a.reps,
                   "tile_pairs": tiles * (tiles + 1) // 2}
            clusters(st, other)  # untimed: code objects, the pooled buffers
            pairs(st, other)
            c1 = [clusters(st, other) for _ in range(a.reps)]
            p = [pairs(st, other) for _ in range(a.reps)]
            c2 = [clusters(st, other) for _ in range(a.reps)]
            info = st.similar_clusters_info()
            wall = [t[0] * 1e3 for t in c1 + c2]
            labels, n_clusters, n_members = c2[-1][1]
            rec.update({"clusters_ms": round(float(np.median(wall)), 3), "clusters_before_ms": round(float(np.median(wall[:a.reps])), 3),
                        "clusters_after_ms": round(float(np.median(wall[a.reps:])), 3), "clusters_min_ms": round(min(wall), 3),
                        "clusters_max_ms": round(max(wall), 3), "clusters": n_clusters, "members": n_members,
                        "largest_class": int(np.bincount(labels[labels != _lib.CS_NO_ID]).max()),
                        "tile_pairs_scored": info["tile_pairs_scored"], "tile_pairs_skipped": info["tile_pairs_skipped"],
                        "rescored_pairs": info["rescored_pairs"], "launches": info["launches"],
                        "join_ms": round(info["join_ms"], 3), "label_ms": round(info["label_ms"], 3)})
            pw = [t[0] * 1e3 for t in p]
            _, r, refusal = p[-1]
            rec.update({"pairs_ms": round(float(np.median(pw)), 3), "pairs_min_ms": round(min(pw), 3),
                        "pairs_max_ms": round(max(pw), 3), "pairs_refused": refusal is not None})
            if refusal is None:
                pinfo = st.similar_pairs_info()
                t0 = time.perf_counter()
                want, wc, wm = clusters_of_pairs(range(n), r[1], r[2])
                rec.update({"pairs_total": r[3], "pairs_cut": r[3] > a.max_pairs, "pairs_filter_ms": round(pinfo["filter_ms"], 3),
                            "pairs_bands": pinfo["bands"], "host_reduce_ms": round((time.perf_counter() - t0) * 1e3, 3),
                            "labels_match": bool(r[3] <= a.max_pairs and (wc, wm) == (n_clusters, n_members)
                                                 and all(int(labels[i]) == lab for i, lab in want.items()))})
            else:
                rec["pairs_refusal"] = refusal
            emit(rec)
        st.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
