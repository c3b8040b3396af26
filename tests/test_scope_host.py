"""Host side of search scopes, no GPU: the C++ plan (codesearch_amd/csrc/masked_plan.hpp, "scopes") through
tests/cpp/scope_plan_test.cpp — the ascending-ids check, the grid of the id-list pass, the refresh rule and the per-shard
split of an id list against numpy — and the argument handling of VectorStore.scope / `scope=` that needs no device."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from codesearch_amd.vector_store import Scope, VectorStore, scope_ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "scope_plan_test.cpp")


@pytest.fixture(scope="module")
def exe():
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "scope_plan_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", path], check=True)
        yield path


def test_scope_plan_cpp(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scope plan ok" in r.stdout


def _split(exe, ids, stripe, n):
    r = subprocess.run([exe, "split", str(stripe), str(n)], input=np.ascontiguousarray(ids, "<u4").tobytes(),
                       capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr
    buf, off, out = r.stdout, 0, []
    for _ in range(n):
        (cnt,) = np.frombuffer(buf, np.uint64, 1, off)
        off += 8
        out.append(np.frombuffer(buf, np.uint32, int(cnt), off))
        off += 4 * int(cnt)
    assert off == len(buf)
    return out


def _numpy_split(ids, stripe, n):
    """Global id g -> shard (g // stripe) % n, local id ((g // stripe) // n) * stripe + g % stripe, order kept."""
    g = np.asarray(ids, np.int64)
    t = g // stripe
    return [(((t // n) * stripe + g % stripe)[t % n == s]) for s in range(n)]


@pytest.mark.parametrize("stripe, n", [(1, 1), (1, 3), (7, 2), (32, 4), (100, 8), (4096, 8), (65536, 3)])
def test_shard_split_matches_numpy(exe, stripe, n):
    rng = np.random.default_rng(stripe * 31 + n)
    next_id = 20_000
    lists = [
        np.zeros(0, np.int64),
        np.array([0]),
        np.arange(next_id),                                                 # every issued id
        np.sort(rng.choice(next_id, 3000, replace=False)),
        np.arange(next_id - 700, next_id + 700),                            # straddles the issued ids
        np.sort(rng.choice(np.arange(next_id // 2, 3 * next_id), 2500, replace=False)),  # mostly not issued yet
        np.array([5, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]),      # the top of the id space
    ]
    for ids in lists:
        got = _split(exe, ids, stripe, n)
        want = _numpy_split(ids, stripe, n)
        for s in range(n):
            assert got[s].tolist() == want[s].tolist(), (stripe, n, s, ids.size)
            assert (np.diff(got[s].astype(np.int64)) > 0).all()  # ascending global ids stay ascending per shard
        # which of a straddling list's ids are issued is kept by the restatement: an id below next_id lands below the
        # shard's own next local id, the others at or above it
        issued = [w.size for w in _numpy_split(np.arange(next_id), stripe, n)]
        for s in range(n):
            mine = np.asarray(ids, np.int64)[(np.asarray(ids, np.int64) // stripe) % n == s]
            assert ((mine < next_id) == (got[s].astype(np.int64) < issued[s])).all()


@pytest.mark.parametrize("ids, want", [
    ([], -1), ([9], -1), ([1, 2, 3], -1), ([0, 2 ** 32 - 1], -1),
    ([1, 1], 1), ([5, 6, 6, 7], 2), ([5, 4], 1), ([1, 2, 9, 3, 2], 3), ([2 ** 32 - 1, 0], 1),
])
def test_validation_names_the_first_offending_position(exe, ids, want):
    r = subprocess.run([exe, "check"], input=np.asarray(ids, "<u4").tobytes(), capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) == want


def test_scope_ids_sorts_dedups_and_drops_negatives():
    got = scope_ids([9, 3, 3, -1, 0, 9, -70, 2 ** 32 - 1, 2 ** 32, 5])
    assert got.dtype == np.uint32 and got.tolist() == [0, 3, 5, 9, 2 ** 32 - 1]
    assert scope_ids([]).size == 0 and scope_ids(np.zeros((0,), np.int64)).dtype == np.uint32
    assert scope_ids(np.array([[4, 1], [1, 2]])).tolist() == [1, 2, 4]  # any shape
    rng = np.random.default_rng(3)
    raw = rng.integers(-50, 5000, 4000)
    got = scope_ids(raw)
    assert got.tolist() == sorted(set(int(x) for x in raw if x >= 0))
    assert (np.diff(got.astype(np.int64)) > 0).all()


class _NoDevice(VectorStore):
    """The argument checks run before anything reaches the library."""

    def __init__(self):  # no handle, no library
        self._h = None
        self.dimensions = 8


def test_scope_and_chunk_ids_are_exclusive():
    st = _NoDevice()
    sc = Scope.__new__(Scope)
    q = np.zeros((1, 8), np.float32)
    for call in (st.search_raw, st.search, st.search_batch, st.search_variants):
        with pytest.raises(ValueError, match="exclusive"):
            call(q, 5, chunk_ids=[1, 2], scope=sc)


def test_an_empty_scope_is_truthy():
    # an empty scope searches nothing; were it falsy, `if scope:` would make its search an unscoped one over the whole store
    sc = Scope.__new__(Scope)
    sc.ids = scope_ids([])
    assert len(sc) == 0 and bool(sc)
