"""Host side of the similar-chunk search inside a scope, no GPU: the header, the export map, the library and the Python
binding agreeing on cs_index_search_similar_scoped; what the Python layer refuses by itself (a closed scope, a sharded
store); and the contract's worked example — search.drop_excluded applied to a scoped order — as DESIGN.md §8d quotes it."""
import ctypes
import fnmatch
import os
import re

import pytest

from codesearch_amd import _lib
from codesearch_amd.search import NO_GROUP, drop_excluded
from codesearch_amd.vector_store import Scope, VectorStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cs_index_search_similar_scoped"


def test_header_export_map_library_and_binding_agree(gpu_lib):
    hdr = open(os.path.join(ROOT, "include", "codesearch_gpu.h")).read()
    nc = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"CS_API int32_t %s\s*\(([^;]*?)\)\s*;" % NAME, nc, re.S)
    assert m, "include/codesearch_gpu.h does not declare " + NAME
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["h", "scope", "ids", "nq", "k", "exclude", "min_cos", "out_cos",
                                                        "out_ids", "out_counts"]
    plain = re.search(r"CS_API int32_t cs_index_search_similar\s*\(([^;]*?)\)\s*;", nc, re.S)
    assert [a.strip() for a in plain.group(1).split(",")] == args[:1] + args[2:]  # the unscoped call plus the scope
    # the header's "no ... form yet" lists: the unscoped call no longer names a scoped form as missing
    assert "No cs_shards_, scoped or device-pointer form yet" not in hdr
    exports = open(os.path.join(ROOT, "codesearch_amd", "csrc", "exports.map")).read()
    globs = re.search(r"global:\s*([^;]*);", re.sub(r"/\*.*?\*/", "", exports, flags=re.S)).group(1).split()
    assert any(fnmatch.fnmatchcase(NAME, g) for g in globs)
    res, argtypes = _lib.SIGNATURES[NAME]
    plain_res, plain_types = _lib.SIGNATURES["cs_index_search_similar"]
    assert res is plain_res is ctypes.c_int32 and len(argtypes) == len(args)
    assert argtypes[0] is ctypes.c_void_p and argtypes[1] is ctypes.c_void_p and list(argtypes[2:]) == list(plain_types[1:])
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert hasattr(ctypes.CDLL(_lib.DIAG_LIB_PATH, mode=ctypes.RTLD_LOCAL), NAME)
    assert gpu_lib.cs_abi_version() == 6  # only a declaration was added


class _NoLibrary:
    """Stands where the loaded library goes: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


def _stand_in(pfx):
    st = VectorStore.__new__(VectorStore)  # no device: the checks under test come before any library call
    st._lib, st._pfx, st._h = _NoLibrary(), pfx, None
    return st


def _closed_scope(st):
    sc = Scope.__new__(Scope)
    sc._h, sc.store = None, st
    return sc


def test_a_closed_scope_is_refused():
    st = _stand_in("cs_index_")
    sc = _closed_scope(st)
    for call in (lambda: st.similar_raw([0], 5, scope=sc), lambda: st.similar(0, 5, scope=sc),
                 lambda: st.similar(0, 5, other_files=True, min_score=0.5, scope=sc)):
        with pytest.raises(_lib.CsError, match="scope is closed") as e:
            call()
        assert e.value.code == _lib.CS_ERR_BAD_ARG
    with pytest.raises(ValueError, match="exclude must be"):  # the mode is still checked first
        st.similar_raw([0], 5, exclude="group", scope=sc)


def test_a_sharded_store_is_refused():
    st = _stand_in("cs_shards_")
    assert st.sharded
    for sc in (None, _closed_scope(st)):
        for call in (lambda: st.similar_raw([0], 5, scope=sc), lambda: st.similar(0, 5, scope=sc)):
            with pytest.raises(_lib.CsError, match="no similar-chunk search: no cs_shards_ form yet") as e:
                call()
            assert e.value.code == _lib.CS_ERR_UNSUPPORTED


def _drop(rows, src_id, src_group, mode, min_cos, k):
    """rows: (cos, id, group) in (cosine desc, id asc) order -> kept ids."""
    cos, ids, groups = zip(*rows) if rows else ((), (), ())
    kc, ki = drop_excluded(cos, ids, groups, src_id, src_group, mode, min_cos, k)
    assert kc == [cos[ids.index(i)] for i in ki]
    return ki


def test_drop_excluded_over_a_scoped_order():
    """The worked example of DESIGN.md §8d.  The store holds ids 0..19; the scope is the dozen ids below.  File 7 has the ids
    4, 10, 11, 12 and 15 (15 is outside the scope), file 3 has 9 and 8, file 2 has 3 and 13."""
    #        cos  id group          the scoped order for source 4: an identical row with a lower id (3) comes first
    order = [(1.0, 3, 2), (1.0, 4, 7), (0.9, 10, 7), (0.9, 11, 7), (0.8, 12, 7), (0.7, 1, NO_GROUP), (0.7, 2, NO_GROUP),
             (0.6, 9, 3), (0.5, 13, 2), (0.4, 6, NO_GROUP), (0.3, 8, 3), (0.2, 0, NO_GROUP)]
    every = [r[1] for r in order]
    # the source inside the scope
    assert _drop(order, 4, 7, "none", None, 20) == every
    assert _drop(order, 4, 7, "self", None, 20) == [3, 10, 11, 12, 1, 2, 9, 13, 6, 8, 0]
    assert _drop(order, 4, 7, "file", None, 20) == [3, 1, 2, 9, 13, 6, 8, 0]
    assert _drop(order, 4, 7, "self", None, 3) == [3, 10, 11]     # the file fills the list ...
    assert _drop(order, 4, 7, "file", None, 3) == [3, 1, 2]       # ... unless it is excluded inside the selection
    # what a caller can do without the call — the scoped search at k + 1 = 4, then drop the file — keeps one row of three
    assert [i for _, i, g in order[:4] if g != 7] == [3]
    # the bound is strict and applies after the exclusion
    assert _drop(order, 4, 7, "file", 0.7, 20) == [3]
    assert _drop(order, 4, 7, "file", 0.69, 20) == [3, 1, 2]
    assert _drop(order, 4, 7, "self", 0.9, 20) == [3]
    assert _drop(order, 4, 7, "none", 0.99, 20) == [3, 4]
    assert _drop(order, 4, 7, "self", 1.0, 20) == []
    # a source outside the scope (id 15, file 7; it is not a row of the order): "self" is "none", its file still goes
    assert _drop(order, 15, 7, "self", None, 20) == _drop(order, 15, 7, "none", None, 20) == every
    assert _drop(order, 15, 7, "file", None, 20) == [3, 1, 2, 9, 13, 6, 8, 0]
    # an ungrouped source: "file" is "self"
    assert _drop(order, 1, NO_GROUP, "file", None, 20) == _drop(order, 1, NO_GROUP, "self", None, 20) == \
        [3, 4, 10, 11, 12, 2, 9, 13, 6, 8, 0]
    # a scope with no live row
    assert _drop([], 4, 7, "file", None, 10) == []
