"""Grouped search over a sharded store (cs_shards_search_grouped, cs_shards_search_variants_grouped) against the searches
it extends, in one process, alternated (new, the baselines, new again, --reps calls each).  Files of 8 contiguous ids, one
query and nine variants, k in (10, 200), per_group in (1, 3):

    one query      sharded grouped            vs  cs_shards_search of the same shape, and cs_index_search_grouped on one index
    nine variants  sharded variants grouped   vs  cs_shards_search_variants, and cs_index_search_variants_grouped

Medians of the wall times of the host-buffer calls, ms, and the ratios.  One JSON object per line on stdout (and in --out);
every line says how many shards there were and on which devices.  Shards that share one device share its bandwidth: such a
run shows the merge and launch overhead of the sharded form, not scaling.

    python benchmarks/shards_grouped_search.py [--rows 10000000] [--dim 384] [--shards 8] [--devices 0,0,...] [--reps 20]
                                               [--out FILE]

The root's merge alone (the capped shard merge against the plain shard merge) is read from a kernel trace, which this
script does not take itself:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python benchmarks/shards_grouped_search.py --rows 200000 --trace-shape 9,200,1
    python benchmarks/shards_grouped_search.py --kernel-stats DIR/.../*_kernel_stats.csv --trace-shape 9,200,1 [--out FILE]

--trace-shape NQ,K,M runs that one shape only (the sharded grouped call and cs_shards_search, --reps times each, no single
index), so the trace's per-kernel averages belong to it; --kernel-stats reads them back and emits one line."""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    """-> the wall times of `reps` calls after one untimed call, ms."""
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def kernel_stats(path, shape):
    """The two merge kernels' rows of a rocprofv3 kernel-stats file -> one record.  merge_shards_grouped_kernel runs on the
    root only; merge_topk_kernel also finishes every shard's own plain search, so its average is over those launches and the
    root's plain shard merge together (the root's alone needs the per-launch trace)."""
    rec = {"trace_shape": shape, "note": "merge_topk_kernel_all: every launch of the run, the shards' own merges and the root's "
                                         "plain shard merge together; no ratio is formed from it"}
    for row in csv.DictReader(open(path)):
        name = row.get("Name", "")
        for key, kernel in (("capped_shard_merge", "merge_shards_grouped_kernel"), ("merge_topk_kernel_all", "merge_topk_kernel")):
            if kernel in name:
                rec[key + "_calls"] = int(row["Calls"])
                rec[key + "_avg_us"] = round(float(row["AverageNs"]) / 1e3, 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--devices", default="", help="comma-separated device per shard (default: every shard on device 0)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-shape", default="", help="NQ,K,M: run this shape only, for a kernel trace")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 *_kernel_stats.csv of a --trace-shape run")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    if a.kernel_stats is not None:
        if not os.path.isfile(a.kernel_stats):
            sys.exit("no kernel-stats file at %r" % a.kernel_stats)
        emit(kernel_stats(a.kernel_stats, a.trace_shape))
        return

    from codesearch_amd import VectorStore, _lib
    from codesearch_amd._lib import f32p, u32p
    from codesearch_amd.synth import synth_rows

    n, dim = a.rows, a.dim
    devices = [int(d) for d in a.devices.split(",")] if a.devices else [0] * a.shards
    where = {"shards": len(devices), "devices": devices,
             "placement": "all shards on one device" if len(set(devices)) == 1 else "%d devices" % len(set(devices))}
    stripe = (n + len(devices) - 1) // len(devices)
    sh = VectorStore(None, dim, devices=devices, rows_per_stripe=stripe, capacity=n)
    sh.insert_synthetic(n, 0x5EA4C5, 0)
    sh.build_index()
    sh.set_single_query_route(sh.ROUTE_STREAM)
    ids = np.arange(n, dtype=np.uint32)
    lib, hs = sh._lib, sh.handle
    files = np.ascontiguousarray(ids // 8)  # (the C call: the Python class does not bind the sharded grouped forms)
    _lib.check(lib.cs_shards_set_groups(hs, ids.ctypes.data_as(u32p), files.ctypes.data_as(u32p), n))
    q1 = np.ascontiguousarray(synth_rows(0x9E5, 1, 1, dim))
    q9 = np.ascontiguousarray(q1 + np.float32(0.15) * synth_rows(0x9E7, 0, 9, dim))
    q9[0] = q1[0]
    med = lambda t: round(float(np.median(t)), 4)  # noqa: E731

    if a.trace_shape:
        nq, k, m = (int(x) for x in a.trace_shape.split(","))
        q = q1 if nq == 1 else q9[:nq]
        cos, idb, cnt = np.zeros((nq, k), np.float32), np.zeros((nq, k), np.uint32), np.zeros(nq, np.uint32)
        lists = (cos.ctypes.data_as(f32p), idb.ctypes.data_as(u32p), cnt.ctypes.data_as(u32p))
        p = q.ctypes.data_as(f32p)
        g = timed(lambda: _lib.check(lib.cs_shards_search_grouped(hs, p, nq, dim, k, m, *lists)), a.reps)
        s = timed(lambda: _lib.check(lib.cs_shards_search(hs, p, nq, dim, k, *lists)), a.reps)
        emit(dict(where, rows=n, dim=dim, nq=nq, k=k, m=m, reps=a.reps, traced=True, shards_grouped_ms=med(g), shards_search_ms=med(s)))
        sh.close()
        return

    single = VectorStore(None, dim, capacity=n)
    single.insert_synthetic(n, 0x5EA4C5, 0)
    single.build_index()
    single.set_single_query_route(single.ROUTE_STREAM)
    single.set_groups(ids, ids // 8)
    h1 = single.handle
    for k in (10, 200):
        cos, idb, cnt = np.zeros((1, k), np.float32), np.zeros((1, k), np.uint32), np.zeros(1, np.uint32)
        count, flag = C.c_uint32(), C.c_int32()
        lists = (cos.ctypes.data_as(f32p), idb.ctypes.data_as(u32p), cnt.ctypes.data_as(u32p))
        merged = (cos.ctypes.data_as(f32p), idb.ctypes.data_as(u32p), C.byref(count), C.byref(flag))
        p1, p9 = q1.ctypes.data_as(f32p), q9.ctypes.data_as(f32p)
        for m in (1, 3):
            def shards_grouped():
                _lib.check(lib.cs_shards_search_grouped(hs, p1, 1, dim, k, m, *lists))

            def shards_plain():
                _lib.check(lib.cs_shards_search(hs, p1, 1, dim, k, *lists))

            def index_grouped():
                _lib.check(lib.cs_index_search_grouped(h1, p1, 1, dim, k, m, *lists))

            def shards_variants_grouped():
                _lib.check(lib.cs_shards_search_variants_grouped(hs, p9, 9, dim, k, m, *merged))

            def shards_variants():
                _lib.check(lib.cs_shards_search_variants(hs, p9, 9, dim, k, *merged))

            def index_variants_grouped():
                _lib.check(lib.cs_index_search_variants_grouped(h1, p9, 9, dim, k, m, *merged))

            rec = dict(where, rows=n, dim=dim, k=k, m=m, reps=a.reps)
            new1 = timed(shards_grouped, a.reps)
            rec["shards_grouped_count"] = int(cnt[0])
            rec["shards_search_ms"] = med(timed(shards_plain, a.reps))
            rec["index_grouped_ms"] = med(timed(index_grouped, a.reps))
            new1 += timed(shards_grouped, a.reps)
            rec["shards_grouped_ms"] = med(new1)
            rec["ratio_vs_shards_search"] = round(rec["shards_grouped_ms"] / rec["shards_search_ms"], 4)
            rec["ratio_vs_index_grouped"] = round(rec["shards_grouped_ms"] / rec["index_grouped_ms"], 4)
            new9 = timed(shards_variants_grouped, a.reps)
            rec["shards_variants_grouped_count"] = int(count.value)
            rec["shards_variants_ms"] = med(timed(shards_variants, a.reps))
            rec["index_variants_grouped_ms"] = med(timed(index_variants_grouped, a.reps))
            new9 += timed(shards_variants_grouped, a.reps)
            rec["shards_variants_grouped_ms"] = med(new9)
            rec["variants_ratio_vs_shards_variants"] = round(rec["shards_variants_grouped_ms"] / rec["shards_variants_ms"], 4)
            rec["variants_ratio_vs_index_variants_grouped"] = round(rec["shards_variants_grouped_ms"] /
                                                                    rec["index_variants_grouped_ms"], 4)
            emit(rec)
    sh.close()
    single.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
