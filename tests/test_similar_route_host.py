"""Host side of the similar-chunk search's route, no GPU: the host plan (codesearch_amd/csrc/similar_route.hpp) through
tests/cpp/similar_route_test.cpp — once as an ordinary build, once under AddressSanitizer + UBSan, a stand-alone program both
times — and the header, both libraries, the Python binding, the C++ wrapper and INTEGRATION.md agreeing on
cs_index_set_similar_route / cs_index_similar_route_info."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "similar_route_test.cpp")


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "similar route ok", r.stdout + r.stderr


def test_similar_route_cpp():
    assert os.path.exists(os.path.join(ROOT, "codesearch_amd", "csrc", "similar_route.hpp"))
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "similar_route_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
        _run(exe)


def test_similar_route_under_sanitizers():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "similar_route_asan")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", SRC, "-o", exe], check=True)
        _run(exe, dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                       UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))


def test_header_libraries_and_binding_agree_on_the_similar_route(gpu_lib):
    from codesearch_amd import VectorStore, _lib

    hdr = open(os.path.join(ROOT, "include", "codesearch_gpu.h")).read()
    nc = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, value in (("CS_SIMILAR_ROUTE_AUTO", 0), ("CS_SIMILAR_ROUTE_SCAN", 1), ("CS_SIMILAR_ROUTE_FILTER", 2)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), nc), name
        assert getattr(_lib, name) == value
    assert VectorStore.SIMILAR_ROUTES == {"auto": 0, "scan": 1, "filter": 2}
    m = re.search(r"CS_API int32_t cs_index_similar_route_info\s*\(([^;]*?)\)\s*;", nc, re.S)
    assert m, "include/codesearch_gpu.h does not declare cs_index_similar_route_info"
    args = [x.strip().split()[-1].lstrip("*") for x in m.group(1).split(",")]
    assert args == ["h", "filter_searches", "scan_searches", "filter_fallbacks"]
    res, argtypes = _lib.SIGNATURES["cs_index_similar_route_info"]
    assert res is ctypes.c_int32 and argtypes[1:] == [_lib.u64p] * 3
    assert _lib.SIGNATURES["cs_index_set_similar_route"][1][1] is ctypes.c_int32
    wrapper = open(os.path.join(ROOT, "codesearch_amd", "host", "codesearch_gpu.hpp")).read()
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("cs_index_set_similar_route", "cs_index_similar_route_info"):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        assert hasattr(ctypes.CDLL(_lib.DIAG_LIB_PATH, mode=ctypes.RTLD_LOCAL), name)
        assert name + "(" in wrapper and name + "(" in md
    # the similar search's comment keeps its last sentence and gains the route paragraph
    comment = re.search(r"/\* Similar-chunk search —((?:(?!\*/).)*?)\*/", hdr, re.S).group(1)
    assert "No cs_shards_ or device-pointer form yet" in comment and "CS_SIMILAR_ROUTE_AUTO" in comment
    assert gpu_lib.cs_abi_version() == 6  # only declarations were added
    # a null handle is refused before anything else is looked at
    assert gpu_lib.cs_index_set_similar_route(None, 0) == _lib.CS_ERR_BAD_ARG
    assert gpu_lib.cs_index_similar_route_info(None, None, None, None) == _lib.CS_ERR_BAD_ARG
