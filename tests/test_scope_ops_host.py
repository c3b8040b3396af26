"""Host side of scope algebra, no GPU: the diagonal split, the tie rule and the per-thread walk of
codesearch_amd/csrc/scope_ops_plan.hpp — the functions the kernels of scope_ops.hip call — walked tile by tile against
std::set_union / set_intersection / set_difference by tests/cpp/scope_ops_plan_test.cpp, once as an ordinary build and once
under AddressSanitizer + UBSan, a stand-alone program both times; and the header, both libraries, the Python binding, the
C++ wrapper and INTEGRATION.md agreeing on the five new entry points."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "scope_ops_plan_test.cpp")
NAMES = ("cs_scope_combine", "cs_index_scope_create_range", "cs_shards_scope_create_range", "cs_scope_read_ids",
         "cs_scope_ops_tile")


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "scope ops plan ok", r.stdout + r.stderr


def test_scope_ops_plan_cpp():
    assert os.path.exists(os.path.join(ROOT, "codesearch_amd", "csrc", "scope_ops_plan.hpp"))
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "scope_ops_plan_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
        _run(exe)


def test_scope_ops_plan_under_sanitizers():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "scope_ops_plan_asan")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", SRC, "-o", exe], check=True)
        _run(exe, dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                       UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))


def test_header_libraries_and_binding_agree_on_scope_algebra(gpu_lib):
    from codesearch_amd import VectorStore, _lib
    from codesearch_amd.vector_store import Scope

    hdr = open(os.path.join(ROOT, "include", "codesearch_gpu.h")).read()
    nc = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"enum \{ CS_SCOPE_OP_UNION = 0, CS_SCOPE_OP_INTERSECT = 1, CS_SCOPE_OP_DIFFERENCE = 2\s*\};", nc)
    assert m, "include/codesearch_gpu.h does not declare CS_SCOPE_OP_*"
    assert Scope.OPS == {"union": 0, "intersection": 1, "difference": 2}
    m = re.search(r"CS_API int32_t cs_scope_combine\s*\(([^;]*?)\)\s*;", nc, re.S)
    assert [x.strip().split()[-1].lstrip("*") for x in m.group(1).split(",")] == ["a", "b", "op", "out"]
    res, argtypes = _lib.SIGNATURES["cs_scope_combine"]
    assert res is ctypes.c_int32 and argtypes[2] is ctypes.c_int32
    assert _lib.SIGNATURES["cs_scope_read_ids"][1][1:] == [ctypes.c_uint64, ctypes.c_uint64, _lib.u32p]
    assert _lib.SIGNATURES["cs_index_scope_create_range"][1][1:3] == [ctypes.c_uint32, ctypes.c_uint64]
    assert _lib.SIGNATURES["cs_index_scope_create_range"] == _lib.SIGNATURES["cs_shards_scope_create_range"]
    assert _lib.SIGNATURES["cs_scope_ops_tile"] == (ctypes.c_uint32, [])
    wrapper = open(os.path.join(ROOT, "codesearch_amd", "host", "codesearch_gpu.hpp")).read()
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        assert hasattr(ctypes.CDLL(_lib.DIAG_LIB_PATH, mode=ctypes.RTLD_LOCAL), name)
        assert name + "(" in md, name
        assert name == "cs_scope_ops_tile" or name + "(" in wrapper, name
    for method in ("union", "intersection", "difference", "__or__", "__and__", "__sub__"):
        assert callable(getattr(Scope, method))
    assert callable(VectorStore.scope_range) and callable(VectorStore.scope_all)
    assert gpu_lib.cs_abi_version() == 6  # only declarations were added
    # the tile is the plan header's, and the handle-level refusals need no device
    plan = open(os.path.join(ROOT, "codesearch_amd", "csrc", "scope_ops_plan.hpp")).read()
    block = int(re.search(r"kScopeOpsBlock = (\d+);", plan).group(1))
    per = int(re.search(r"kScopeOpsPerThread = (\d+);", plan).group(1))
    assert gpu_lib.cs_scope_ops_tile() == block * per
    out = ctypes.c_void_p(1)
    assert gpu_lib.cs_scope_combine(None, None, 0, None) == _lib.CS_ERR_BAD_ARG and "out is null" in _lib.last_error()
    assert gpu_lib.cs_scope_combine(None, None, 0, ctypes.byref(out)) == _lib.CS_ERR_BAD_ARG and not out.value
    assert "null scope handle (a)" in _lib.last_error()
    out = ctypes.c_void_p(1)
    assert gpu_lib.cs_index_scope_create_range(None, 0, 1, ctypes.byref(out)) == _lib.CS_ERR_BAD_ARG and not out.value
    assert gpu_lib.cs_shards_scope_create_range(None, 0, 1, ctypes.byref(out)) == _lib.CS_ERR_BAD_ARG
    assert gpu_lib.cs_scope_read_ids(None, 0, 0, None) == _lib.CS_ERR_BAD_ARG
