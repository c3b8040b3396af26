"""Host side of the masked search, no GPU: the mask's bit layout (vector_store.allow_mask), the reference's filter_path
rule (search.path_matches), and the C++ plan (codesearch_amd/csrc/masked_plan.hpp) through tests/cpp/masked_plan_test.cpp,
including the per-shard restatement of a mask against numpy."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from codesearch_amd.search import normalize_path_str, path_matches
from codesearch_amd.vector_store import allow_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "masked_plan_test.cpp")


def test_allow_mask_bit_layout():
    m = allow_mask([0, 5, 31, 32, 63, 64, 99], 100)
    assert m.dtype == np.uint32 and m.shape == (4,)
    assert int(m[0]) == (1 << 0) | (1 << 5) | (1 << 31)
    assert int(m[1]) == (1 << 0) | (1 << 31)
    assert int(m[2]) == 1
    assert int(m[3]) == 1 << (99 - 96)
    # ids outside [0, next_id) are dropped; duplicates are harmless
    m = allow_mask([-1, 3, 3, 100, 5000], 100)
    assert m.tolist() == [1 << 3, 0, 0, 0]
    assert allow_mask([], 0).size == 0
    # every id round-trips through the layout the C ABI documents: bit i = bit i & 31 of word i >> 5
    ids = np.random.default_rng(1).choice(1000, 137, replace=False)
    m = allow_mask(ids, 1000)
    back = [i for i in range(1000) if (int(m[i >> 5]) >> (i & 31)) & 1]
    assert back == sorted(ids.tolist())


def test_normalize_path_str():
    assert normalize_path_str("\\\\?\\C:\\repo\\src\\x.rs") == "C:/repo/src/x.rs"
    assert normalize_path_str("src/a.rs") == "src/a.rs"


@pytest.mark.parametrize("path, filt, root, mcp, want", [
    # MCP trims the filter's trailing '/', the CLI does not
    ("src/search/mod.rs", "src/search/", "", True, True),
    ("src/search.rs", "src/search/", "", True, True),     # ... so 'src/search/' also passes a sibling file, as there
    ("src/search.rs", "src/search/", "", False, False),
    ("src/search/mod.rs", "src/search/", "", False, True),
    ("src/search.rs", "src/search", "", True, True),   # a plain prefix test, as in the reference
    ("src/a.rs", "src/a.rs/", "", True, True),
    ("src/a.rs", "src/a.rs/", "", False, False),
    # a Windows path with the UNC prefix under a Windows root, with and without the root's trailing separator
    ("\\\\?\\C:\\repo\\src\\x.rs", "src", "C:\\repo", True, True),
    ("\\\\?\\C:\\repo\\src\\x.rs", "src/", "C:\\repo\\", False, True),
    ("\\\\?\\C:\\repo\\lib\\x.rs", "src", "C:\\repo", True, False),
    # './src' filters and './' paths
    ("./src/a.rs", "./src", "", True, True),
    ("/home/u/repo/src/a.rs", "./src", "/home/u/repo/", True, True),
    ("/home/u/repo/src/a.rs", "./src", "/home/u/repo", False, True),
    ("/home/u/repo/tests/a.rs", "./src", "/home/u/repo", True, False),
    # a path outside the root keeps its own form (leading '/' trimmed)
    ("/elsewhere/src/a.rs", "elsewhere/src", "/home/u/repo", True, True),
    # an empty filter passes everything
    ("src/a.rs", "", "", True, True),
])
def test_path_matches(path, filt, root, mcp, want):
    assert path_matches(path, filt, root, mcp) is want


def _build(d):
    exe = os.path.join(d, "masked_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
    return exe


def test_masked_plan_cpp():
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([_build(d)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "masked plan ok" in r.stdout


def _numpy_restate(mask_bits, next_id, stripe, n):
    """Brute force: global id g -> shard (g // stripe) % n, local id ((g // stripe) // n) * stripe + g % stripe."""
    g = np.arange(min(len(mask_bits), next_id), dtype=np.int64)
    on = g[mask_bits[: g.size]]
    out = []
    for s in range(n):
        mine = g[(g // stripe) % n == s]
        local_bits = int(((mine[-1] // stripe) // n) * stripe + mine[-1] % stripe + 1) if mine.size else 0
        sel = on[(on // stripe) % n == s]
        out.append((local_bits, ((sel // stripe) // n) * stripe + sel % stripe))
    return out


@pytest.mark.parametrize("stripe, n", [(1, 1), (1, 3), (7, 2), (32, 4), (100, 8), (4096, 8), (65536, 3)])
def test_shard_mask_restatement_matches_numpy(stripe, n):
    rng = np.random.default_rng(stripe * 31 + n)
    with tempfile.TemporaryDirectory() as d:
        exe = _build(d)
        for next_id, allow_bits in ((1, 1), (5000, 5000), (20000, 12345), (9000, 9100)):
            bits = rng.random(allow_bits) < 0.3
            words = np.zeros((allow_bits + 31) // 32, np.uint32)
            idx = np.nonzero(bits)[0]
            np.bitwise_or.at(words, idx >> 5, np.left_shift(np.uint32(1), (idx & 31).astype(np.uint32)))
            r = subprocess.run([exe, "restate", str(stripe), str(n), str(allow_bits), str(next_id)],
                               input=words.tobytes(), capture_output=True, timeout=60)
            assert r.returncode == 0, r.stderr
            buf, off = r.stdout, 0
            for s, (want_bits, want_ids) in enumerate(_numpy_restate(bits, next_id, stripe, n)):
                (got_bits,) = np.frombuffer(buf, np.uint64, 1, off)
                off += 8
                nw = (int(got_bits) + 31) // 32
                got = np.frombuffer(buf, np.uint32, nw, off)
                off += 4 * nw
                got_ids = [i for i in range(int(got_bits)) if (int(got[i >> 5]) >> (i & 31)) & 1]
                # the local bit count may stop at the last local id the mask could allow (never beyond the issued ids)
                assert int(got_bits) <= want_bits, (s, got_bits, want_bits)
                assert got_ids == want_ids.tolist(), (stripe, n, s)
            assert off == len(buf)
