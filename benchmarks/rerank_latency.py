#!/usr/bin/env python3
"""Latency of the neural second pass of `codesearch search --rerank` (src/search/mod.rs:829-866 of the reference:
NeuralReranker::rerank_and_blend over the top results) on the shape of its default model, jina-reranker-v1-turbo-en: a
JinaBert encoder of 6 layers x 384, 12 heads, intermediate 1536, vocabulary 61,056, with synthetic weights (the arithmetic
does not depend on their values) and the score head.

For 25 and 100 pairs of 128, 256 and 512 tokens (every pair at full length: the worst case of that truncation length) it
reports: host-to-host time of one cs_reranker_score_ids call, the device time of that call (the encoder's own profile,
cs_embedder_profile_read), and the score head's share of the device time from the stage table (a second pass:
cs_embedder_profile_stages runs the forward on one stream with an event after every kernel).  One JSON line per case, also
appended to the file given with --out.

Every case runs in a child process of its own under a time limit; the first one that fails ends the run.

    python benchmarks/rerank_latency.py --out profiles/rerank_latency.jsonl"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(n, L) for L in (128, 256, 512) for n in (25, 100)]
CASE_TIMEOUT_S = 120


def run_case(n, L, reps):
    import ctypes as C

    import numpy as np

    from codesearch_amd import _lib, rerank
    from codesearch_amd.bert_params import ARCH_JINA, POOL_CLS, BertConfig

    cfg = BertConfig(vocab_size=61056, hidden=384, layers=6, heads=12, intermediate=1536, max_position=512, pooling=POOL_CLS,
                     arch=ARCH_JINA)
    rng = np.random.default_rng(7)
    head = rerank.pack_head(rng.normal(0, 0.05, (384, 384)), rng.normal(0, 0.1, 384), rng.normal(0, 0.05, 384), rng.normal(0, 0.1, 1))
    rr = rerank.NeuralReranker(cfg, head, seed=11)
    lib, emb = _lib.load(), rr.embedder_handle
    ids = rng.integers(5, cfg.vocab_size, (n, L)).astype(np.int32)
    mask = np.ones((n, L), np.int32)
    types = np.zeros((n, L), np.int32)
    types[:, L // 8:] = 1          # a short query in front of a long document
    for _ in range(5):
        rr.score_ids(ids, mask, types)
    fwd, cnt = C.c_double(), C.c_uint64()
    lib.cs_embedder_profile_read(emb, C.byref(fwd), C.byref(cnt), 1)
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        rr.score_ids(ids, mask, types)
        wall.append(time.perf_counter() - t0)
    lib.cs_embedder_profile_read(emb, C.byref(fwd), C.byref(cnt), 1)
    device_ms = fwd.value / max(cnt.value, 1)
    # the stage table: one stream, an event after every kernel
    lib.cs_embedder_profile_stages(emb, 1)
    us = (C.c_double * 9)()
    lib.cs_embedder_profile_stages_read(emb, us, C.byref(cnt), 1)
    for _ in range(max(3, reps // 4)):
        rr.score_ids(ids, mask, types)
    lib.cs_embedder_profile_stages_read(emb, us, C.byref(cnt), 1)
    lib.cs_embedder_profile_stages(emb, 0)
    stages = [u / max(cnt.value, 1) for u in us]
    wall.sort()
    rr.close()
    return {"pairs": n, "tokens": L, "reps": reps, "host_to_host_ms_median": round(wall[len(wall) // 2] * 1e3, 4),
            "host_to_host_ms_min": round(wall[0] * 1e3, 4), "device_ms_per_rerank": round(device_ms, 4),
            "head_us_one_stream": round(stages[8], 2), "all_stages_us_one_stream": round(sum(stages), 2),
            "head_share_of_device_time": round(stages[8] / max(sum(stages), 1e-9), 5),
            "model": "6 x 384, 12 heads, intermediate 1536, vocabulary 61056 (jina-reranker-v1-turbo-en's shape), synthetic weights"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--case", nargs=2, type=int, default=None, metavar=("PAIRS", "TOKENS"), help="run one case in this process")
    a = ap.parse_args()
    if a.case:
        print(json.dumps(run_case(a.case[0], a.case[1], a.reps)), flush=True)
        return 0
    for n, L in CASES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(n), str(L), "--reps", str(a.reps)],
                               capture_output=True, text=True, timeout=CASE_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print(f"case {n} x {L} ran into its {CASE_TIMEOUT_S} s limit: stopping", file=sys.stderr)
            return 1
        if p.returncode != 0:
            print(f"case {n} x {L} failed with status {p.returncode}: stopping\n{p.stderr[-2000:]}", file=sys.stderr)
            return 1
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
