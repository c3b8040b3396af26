"""The index life cycle under the grouped scoped searches (tests/store_model.py): the walks of tests/test_gpu_store_walk.py —
appends, tombstones, reclaiming builds, an emptied index, clear, reopening, groups assigned before and after — applied to a
VectorStore and to the model side by side, with ONE scope of every other id held across the builds, so that it is remade
after each.  At every searchable state one grouped scoped search and one grouped variants scoped search are judged by the
model's `check` (float64 cosines, the derived band, allowed= the scope's ids, per_file= the cap).  Sharded walks are
skipped: a sharded store has no grouped search."""
import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd.synth import synth_rows
from tests.store_model import WALKS, apply, make_walk, new_model, resolve

pytestmark = pytest.mark.gpu

SPAN = 12_000  # the scope names every other id of [id_base, id_base + SPAN): more than any walk issues


@pytest.fixture(scope="module")
def VS(gpu_lib):
    from codesearch_amd import VectorStore

    assert gpu_lib.cs_device_count() >= 1, "no HIP device visible"
    return VectorStore


def _queries(m, step):
    """Three queries: two random, one planted on a live row inside the scope when there is one."""
    qs = [q for q in synth_rows(9400 + step, 0, 2, m.dim)]
    inside = [int(i) for i in m.live_ids() if (int(i) - m.id_base) % 2 == 0 and m.rows[int(i)].any()]
    qs.append(m.rows[inside[step % len(inside)]].copy() if inside else synth_rows(9450 + step, 0, 1, m.dim)[0])
    return np.stack(qs)


@pytest.mark.parametrize("seed,dim", [(s, d) for s, d, sharded in WALKS if not sharded])
def test_walk(VS, tmp_path, seed, dim):
    walk = make_walk(seed, dim, False)
    head = walk[0]
    m = new_model(walk)
    path = str(tmp_path / "db")
    st = VS(path, dim, id_base=head["id_base"])
    scope_ids = np.arange(head["id_base"], head["id_base"] + SPAN, 2)
    sc = st.scope(scope_ids)
    judged = refreshed = 0
    try:
        for step, op in enumerate(walk[1:], 1):
            try:
                kind = op["op"]
                args = resolve(op, m)
                if kind == "insert":
                    assert st.insert_embeddings(args).tolist() == apply(op, args, m)
                elif kind == "delete":
                    assert st.delete_chunks(list(args)) == apply(op, args, m)
                elif kind == "build":
                    st.build_index()
                    apply(op, args, m)
                elif kind == "clear":
                    st.clear()
                    apply(op, args, m)
                elif kind == "reopen":
                    st.close()  # (closes the scope)
                    st = VS(path, dim, id_base=head["id_base"])
                    sc = st.scope(scope_ids)
                    apply(op, args, m)
                elif kind == "groups":
                    st.set_groups(*args)
                    apply(op, args, m)
                assert m.next_id <= head["id_base"] + SPAN
                if not (kind in ("build", "reopen") and m.built):
                    continue
                qs = _queries(m, step)
                made = sc.info()[2]
                for k, per_file in ((10, 1), (200, 3)) if step % 2 else ((1, 1), (200, 2)):
                    got = st.search_raw(qs, k, scope=sc, per_file=per_file)
                    for n in range(len(qs)):
                        m.check(qs[n], k, (got[0][n], got[1][n], got[2][n]), allowed=scope_ids, per_file=per_file)
                    cos, ids, count, _flag = st.search_variants_raw(qs, k, scope=sc, per_file=per_file)
                    m.check(qs, k, (cos, ids, count), allowed=scope_ids, per_file=per_file)
                    judged += len(qs) + 1
                refreshed += sc.info()[2] > made
                live_inside = int(np.isin(m.live_ids(), scope_ids).sum())
                assert sc.info()[1] == live_inside
            except (AssertionError, _lib.CsError) as e:
                raise AssertionError(f"walk {head} failed at step {step}, {op}: {e}\nreplay: {walk[:step + 1]}") from e
    finally:
        st.close()
    assert judged >= 100 and refreshed >= 10, (judged, refreshed)
