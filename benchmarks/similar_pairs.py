"""Similar-pairs search (cs_index_similar_pairs) against what a caller can do without it — cs_index_search_similar once per
chunk, in calls of CS_MAX_QUERIES sources at k = 1,024 with the same bound, the hits b > a kept and ordered on the host —
over the same store, in one process, alternated (new, baseline, new again).  One JSON object per line on stdout (and in
--out).

    python benchmarks/similar_pairs.py [--rows 100000] [--dim 384] [--reps 5] [--baseline-calls N] [--out FILE]
                                       [--tree DIR] [--probe PATH]

The store: synthetic rows in files of 8 ids; one file of --hog (10,000) near-duplicates of one row (0.95 s + 0.05 noise);
1 % of the rows in planted clone pairs at cosines 0.92 .. 0.99 — the sources are rows [0, rows / 200), each clone sits in
another file at the end of the store.  Bound 0.9, both modes, max_pairs 1 << 20.

Per mode: the wall time of the call (median of --reps, after one untimed call), the filter bands' and the refine's device
time (HIP events inside the call) and the ordering's host time (cs_index_similar_pairs_info), candidates against qualifying
pairs, and the filter's achieved f16 FLOP/s — 2 * 128 * 128 * dim per tile pair, T (T + 1) / 2 tile pairs, over the bands'
device time.  --probe PATH: the built benchmarks/mfma_rate_probe is run first and its best "f32_32x32x16_f16 random data"
figure is recorded beside it.  A call the library refuses (more candidates than 2 * max_pairs + 4096: CS_PAIRS_ALL over a
file of 10,000 near-duplicates holds 5e7 pairs) is recorded as refused, with the time the refusal took.

--baseline-calls N: time only the first N similar-chunk calls and scale to all of them (baseline_extrapolated: true); 0 =
all of them.  The baseline is exact only where no source has more than 1,024 hits above the bound.

--tree DIR: load the package and the library of another checkout (the parent commit's, built): the entry point it lacks is
not timed, so the same script gives the baseline's times under the parent's library."""
import argparse
import json
import os
import re
import subprocess
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
    ap.add_argument("--baseline-calls", type=int, default=0)
    ap.add_argument("--out", default="")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--probe", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from codesearch_amd import VectorStore, _lib
    from codesearch_amd.synth import synth_rows

    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    probe_tops = None
    if a.probe:
        txt = subprocess.run([a.probe], capture_output=True, text=True, timeout=120, check=True).stdout
        rates = [float(m.group(1)) for m in re.finditer(r"f32_32x32x16_f16 random data\s+[\d.]+ ms\s+([\d.]+) TOP/s", txt)]
        probe_tops = max(rates) if rates else None

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
    has_new = "cs_index_similar_pairs" in _lib.SIGNATURES
    tiles = (n + 127) // 128
    flop = tiles * (tiles + 1) // 2 * 2.0 * 128 * 128 * dim
    bound = np.float32(a.min_cos)
    calls = [ids[lo:lo + _lib.CS_MAX_QUERIES] for lo in range(0, n, _lib.CS_MAX_QUERIES)]
    timed_calls = calls if a.baseline_calls <= 0 else calls[:a.baseline_calls]

    def baseline(other):
        """-> (seconds over the timed calls, pairs found, sources whose list was cut at 1,024)."""
        t0 = time.perf_counter()
        found = cut = 0
        for part in timed_calls:
            cos, hit, cnt = st.similar_raw(part, 1024, exclude="file" if other else "self", min_cos=bound)
            keep = (np.arange(1024)[None, :] < cnt[:, None]) & (hit > part[:, None])
            pa, pc = np.broadcast_to(part[:, None], hit.shape)[keep], cos[keep]
            order = np.lexsort((hit[keep], pa, -pc))  # (cosine desc, a asc, b asc)
            found += int(order.size)
            cut += int((cnt == 1024).sum())
        return time.perf_counter() - t0, found, cut

    def pairs(other):
        t0 = time.perf_counter()
        try:
            r = st.similar_pairs_raw(bound, other_files=other, max_pairs=a.max_pairs)
        except _lib.CsError as e:
            if e.code != _lib.CS_ERR_UNSUPPORTED:
                raise
            return time.perf_counter() - t0, None, str(e)
        return time.perf_counter() - t0, r, None

    for other in (True, False):
        rec = {"rows": n, "dim": dim, "mode": "other_group" if other else "all", "min_cos": float(bound), "max_pairs": a.max_pairs,
               "hog_rows": a.hog, "planted_pairs": n_src, "reps": a.reps, "library": "new" if has_new else "parent",
               "tile_pairs": tiles * (tiles + 1) // 2, "filter_flop": flop, "mfma_probe_f16_32x32x16_tops": probe_tops,
               "baseline_calls": len(calls), "baseline_calls_timed": len(timed_calls),
               "baseline_extrapolated": len(timed_calls) < len(calls)}
        if has_new:
            pairs(other)  # untimed: code objects, the pooled buffers
            t1 = [pairs(other) for _ in range(a.reps)]
        tb, found, cut = baseline(other)
        rec.update({"baseline_ms": round(tb * 1e3 * len(calls) / len(timed_calls), 3), "baseline_timed_ms": round(tb * 1e3, 3),
                    "baseline_pairs_in_timed_calls": found, "baseline_sources_cut_at_1024": cut})
        if has_new:
            t2 = [pairs(other) for _ in range(a.reps)]
            wall = [t[0] * 1e3 for t in t1 + t2]
            _, r, refusal = t2[-1]
            rec.update({"call_ms": round(float(np.median(wall)), 3), "call_before_ms": round(float(np.median(wall[:a.reps])), 3),
                        "call_after_ms": round(float(np.median(wall[a.reps:])), 3), "call_min_ms": round(min(wall), 3),
                        "call_max_ms": round(max(wall), 3), "refused": refusal is not None})
            if refusal is None:
                info = st.similar_pairs_info()
                rec.update({"total": r[3], "returned": int(len(r[0])), "candidates": info["candidates"], "bands": info["bands"],
                            "filter_ms": round(info["filter_ms"], 3), "refine_ms": round(info["refine_ms"], 3),
                            "order_ms": round(info["order_ms"], 3),
                            "filter_tflops": round(flop / (info["filter_ms"] * 1e-3) / 1e12, 1) if info["filter_ms"] > 0 else None,
                            "ratio_vs_baseline": round(float(np.median(wall)) / rec["baseline_ms"], 6)})
            else:
                rec["refusal"] = refusal
        emit(rec)
    st.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
