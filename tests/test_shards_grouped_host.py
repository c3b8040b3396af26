"""Host side of the grouped search over a sharded store, no GPU: the plan of codesearch_amd/csrc/shards_grouped_plan.hpp —
levels, scratch, the (shard, local id) <-> global id maps and the host statement of the root's capped shard merge —
through tests/cpp/shards_grouped_plan_test.cpp, once as an ordinary build and once as the same stand-alone program under
AddressSanitizer + UBSan; and the ABI additions: declared, exported, bound, cs_abi_version unchanged."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "shards_grouped_plan_test.cpp")
FLAGS = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"]

NEW_CALLS = ("cs_shards_set_groups", "cs_shards_groups_info", "cs_shards_search_grouped", "cs_shards_search_grouped_scoped",
             "cs_shards_search_variants_grouped", "cs_shards_search_variants_grouped_scoped")


def _build_and_run(extra, env=None):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "shards_grouped_plan_test")
        subprocess.run(["g++"] + FLAGS + extra + [SRC, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "shards grouped plan ok", r.stdout + r.stderr


def test_shards_grouped_plan_cpp():
    _build_and_run([])


def test_shards_grouped_plan_cpp_under_sanitizers():
    _build_and_run(["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
                   dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                        UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))


def test_the_sharded_grouped_calls_are_declared_exported_and_bound(gpu_lib):
    from codesearch_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "codesearch_gpu.h")).read()
    for name in NEW_CALLS:
        assert "CS_API int32_t %s(" % name in hdr, name
        assert name in _lib.SIGNATURES and hasattr(gpu_lib, name), name
        # the argument list of the cs_index_ call of the same name (the handle is a pointer either way)
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("cs_shards_", "cs_index_")], name
    assert gpu_lib.cs_abi_version() == 6  # only declarations were added


def test_null_handles_are_refused_without_a_device(gpu_lib):
    """The handle check comes first in every new call, before anything touches a device."""
    import ctypes as C

    from codesearch_amd import _lib

    q = (C.c_float * 4)()
    cos, ids, cnt, flag = (C.c_float * 4)(), (C.c_uint32 * 4)(), (C.c_uint32 * 1)(), (C.c_int32 * 1)()
    assert gpu_lib.cs_shards_set_groups(None, ids, ids, 1) == _lib.CS_ERR_BAD_ARG
    assert gpu_lib.cs_shards_groups_info(None, None, None) == _lib.CS_ERR_BAD_ARG
    assert gpu_lib.cs_shards_search_grouped(None, q, 1, 4, 1, 1, cos, ids, cnt) == _lib.CS_ERR_BAD_ARG
    assert gpu_lib.cs_shards_search_grouped_scoped(None, None, q, 1, 4, 1, 1, cos, ids, cnt) == _lib.CS_ERR_BAD_ARG
    assert gpu_lib.cs_shards_search_variants_grouped(None, q, 1, 4, 1, 1, cos, ids, cnt, flag) == _lib.CS_ERR_BAD_ARG
    assert gpu_lib.cs_shards_search_variants_grouped_scoped(None, None, q, 1, 4, 1, 1, cos, ids, cnt, flag) == _lib.CS_ERR_BAD_ARG
    assert b"null shards handle" in gpu_lib.cs_last_error()
