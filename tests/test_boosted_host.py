"""Host side of the boosted search, no GPU: the contract as host Python (search.boost_order: the GPU tests' ground truth)
on hand-worked cases, the ABI additions (declared, exported, bound; cs_abi_version stays 6), the argument refusals of
vector_store._filters_ok, and the class table (index_ledger.hpp IdTable as ClassTable) through
tests/cpp/boosted_table_test.cpp."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from codesearch_amd.search import boost_order
from codesearch_amd.sharded import key_pack
from codesearch_amd.vector_store import CHUNK_KINDS, NO_CLASS, _filters_ok, cos_to_score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cs_index_set_classes", "cs_index_classes_info", "cs_index_search_boosted", "cs_index_search_boosted_scoped"]
f32 = np.float32


def _order(rows, weights, k):
    """rows: (cos, id, class) already in (cosine desc, id asc) order -> (score, cos, ids) as lists."""
    cos, ids, cls = zip(*rows)
    s, c, i = boost_order(np.array(cos, f32), np.array(ids, np.uint32), np.array(cls, np.uint16), weights, k)
    assert s.dtype == f32 and c.dtype == f32 and i.dtype == np.uint32
    return s.tolist(), c.tolist(), i.tolist()


def test_boost_order_contract():
    # cosines exact in f32, so the scores are (1 + c) / 2 exactly: 0.75 -> 0.875, 0.5 -> 0.75, 0.25 -> 0.625, 0 -> 0.5
    rows = [(0.75, 4, 0), (0.5, 1, 1), (0.5, 2, 0), (0.25, 9, 2), (0.0, 0, NO_CLASS), (-0.5, 5, 1)]
    ones = np.ones(3, f32)
    s, c, i = _order(rows, ones, 10)
    assert i == [4, 1, 2, 9, 0, 5] and s == [0.875, 0.75, 0.75, 0.625, 0.5, 0.25] and c == [r[0] for r in rows]
    assert _order(rows, None, 3)[2] == [4, 1, 2]      # no table: every row weighs 1
    assert _order(rows, ones, 2)[2] == [4, 1]          # a tie at the k-th slot: the lower id
    # class 1 at 1.25: 0.75 * 1.25 = 0.9375 passes the unboosted best; 0.25 * 1.25 = 0.3125 stays last
    s, c, i = _order(rows, np.array([1, 1.25, 1], f32), 10)
    assert i == [1, 4, 2, 9, 0, 5] and s == [0.9375, 0.875, 0.75, 0.625, 0.5, 0.3125]
    assert c == [0.5, 0.75, 0.5, 0.25, 0.0, -0.5]      # the cosine travels with its row
    # weight 0: the class sinks to score 0, ordered among itself by id; nothing is excluded
    s, c, i = _order(rows, np.array([0, 1, 1], f32), 10)
    assert i == [1, 9, 0, 5, 2, 4] and s[-2:] == [0.0, 0.0]
    # a class the table does not cover weighs 1, and so does NO_CLASS — also when every covered class is boosted
    s, c, i = _order(rows, np.array([2, 2], f32), 10)  # class 2 and NO_CLASS uncovered
    assert i == [4, 1, 2, 9, 0, 5] and s == [1.75, 1.5, 1.5, 0.625, 0.5, 0.5]
    assert _order(rows, np.zeros(0, f32), 10)[0] == _order(rows, ones, 10)[0]


def test_boost_order_ties_in_score_go_by_id_whatever_the_cosine():
    """s = 1 - (1 - c) / 2 is not injective in f32: two neighbouring cosines at 0.75 share the score 0.875.  The boosted order
    breaks that tie by id, where the cosine order has the larger cosine first."""
    c_hi = f32(0.75)                       # s = 0.875 exactly
    c_lo = np.nextafter(c_hi, f32(0.0))    # 1 - (0.125 + 2^-25) lies halfway between two floats and rounds to 0.875
    assert c_hi != c_lo and cos_to_score(c_hi) == cos_to_score(c_lo)
    rows = [(c_hi, 7, 0), (c_lo, 3, 0), (0.5, 1, 0)]  # (cosine desc, id asc): id 7 first
    s, c, i = _order(rows, np.ones(1, f32), 3)
    assert i == [3, 7, 1] and s[0] == s[1] and c[:2] == [float(c_lo), float(c_hi)]
    # one rounding of s * w, in f32: against the product formed in float64
    w = f32(1.15)
    cos = np.linspace(-1, 1, 4001).astype(f32)
    s, _, _ = boost_order(cos[::-1], np.arange(cos.size), np.zeros(cos.size, np.uint16), [w], cos.size)
    want = (cos_to_score(cos[::-1]).astype(np.float64) * np.float64(w)).astype(f32)
    assert np.array_equal(np.sort(s), np.sort(want))
    assert (np.diff(key_pack(s, np.zeros(s.size, np.uint32)).astype(np.float64)) <= 0).all()  # best first


def test_chunk_kinds_are_the_reference_enum():
    assert len(CHUNK_KINDS) == 18 and len(set(CHUNK_KINDS)) == 18
    assert CHUNK_KINDS[0] == "Function" and CHUNK_KINDS[3] == "Struct" and CHUNK_KINDS[-1] == "Other"
    assert NO_CLASS == 0xFFFF


def _declared():
    text = open(os.path.join(ROOT, "include", "codesearch_gpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_abi_additions(gpu_lib):
    from codesearch_amd import _lib

    hdr = _declared()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name + " is not declared"
        assert hasattr(raw, name) and re.search(r"\b" + name + r"$", exported, re.M), name + " is not exported"
        assert name in _lib.SIGNATURES
        args = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len([a for a in args.split(",") if a.strip()]), name
    assert open(os.path.join(ROOT, "codesearch_amd", "csrc", "exports.map")).read().count("global: cs_*;") == 1
    assert gpu_lib.cs_abi_version() == 6
    full = open(os.path.join(ROOT, "include", "codesearch_gpu.h")).read()
    assert re.search(r"#define CS_NO_CLASS 0xFFFFu\b", full) and re.search(r"#define CS_MAX_CLASSES 4096u\b", full)
    assert (_lib.CS_NO_CLASS, _lib.CS_MAX_CLASSES) == (0xFFFF, 4096)


def test_class_weights_refusals():
    w = np.ones(3, f32)
    _filters_ok(None, None, None, w)
    _filters_ok(None, object(), None, w)      # class_weights= may come with scope=
    _filters_ok(None, object(), 2, None)      # (and per_file= with scope=, as before)
    with pytest.raises(ValueError, match="class_weights= is exclusive with chunk_ids="):
        _filters_ok([1], None, None, w)
    with pytest.raises(ValueError, match="class_weights= is exclusive with per_file="):
        _filters_ok(None, None, 2, w)
    with pytest.raises(ValueError, match="class_weights= is exclusive with per_file="):
        _filters_ok(None, object(), 2, w)
    with pytest.raises(ValueError, match="exclusive"):
        _filters_ok([1], object(), None, None)  # what it refused before


def test_class_table_cpp():
    src = os.path.join(ROOT, "tests", "cpp", "boosted_table_test.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "boosted_table_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", src, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "class table ok" in r.stdout
