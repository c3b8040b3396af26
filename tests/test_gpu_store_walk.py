"""The index life cycle, model-checked on every search kind (tests/store_model.py).

A walk is a deterministic list of about 40 operations — appends, tombstones, reclaiming builds, an index whose rows are
all deleted, clear, reopening from disk, scopes and groups made before and used after — applied to a VectorStore and to
the model side by side.  What the store reports (ids of an insert, count of a delete, len, next_id, stored_rows,
is_indexed, a scope's and the groups' books) must be the model's, and after every build every search kind — plain on the
streaming and the default route, one query and batched; masked; scoped on each route; grouped; variants — is judged by
the model's `check` (float64 cosines, the derived band 2 * (dim + 8) * 2**-24), next to the project's own bit-for-bit
identities between the kinds.  tests/test_store_model.py asserts on the CPU that each walk run here reaches every state
it is meant to.  A failure's message carries the walk, the step and the operations up to it: a directed test to replay.

Below the walks: directed regressions of what they found — the index that a reclaiming build leaves without a row, whose
ids are spent all the same (cs_index: `compacted`)."""
import ctypes as C
import time

import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd._lib import f32p, u32p
from codesearch_amd.synth import synth_rows
from tests.store_model import NO_ID, NOT_BUILT, WALKS, StoreModel, apply, make_walk, new_model, resolve

pytestmark = pytest.mark.gpu

KS = (1, 10, 200)


@pytest.fixture(scope="module")
def VS(gpu_lib):
    from codesearch_amd import VectorStore

    assert gpu_lib.cs_device_count() >= 1, "no HIP device visible"
    return VectorStore


@pytest.fixture(scope="module")
def seen():
    """What the module's searches added up to: printed once, at the end (run with -s)."""
    s = {"max_err": 0.0, "tol_of_max": 0.0, "judged": 0, "searches": 0, "t0": time.perf_counter()}
    yield s
    print(f"\nstore walks: {s['searches']} searches, {s['judged']} lists judged, largest |cos_gpu - cos_f64| = "
          f"{s['max_err']:.3e} (tol {s['tol_of_max']:.3e}), {time.perf_counter() - s['t0']:.1f} s")


def _open(VS, head, path):
    if head["shards"] > 1:
        return VS(path, head["dim"], devices=[0] * head["shards"], rows_per_stripe=head["stripe"])
    return VS(path, head["dim"], id_base=head["id_base"])


def _variants_raw(st, qs, k, chunk_ids=None, scope=None):
    """search_variants without the metadata join (the walks' rows carry none) -> (cos [k], ids [k], count)."""
    q = np.ascontiguousarray(qs, np.float32)
    cos, ids, count, flag = np.zeros(k, np.float32), np.zeros(k, np.uint32), C.c_uint32(), C.c_int32()
    out = (cos.ctypes.data_as(f32p), ids.ctypes.data_as(u32p), C.byref(count), C.byref(flag))
    if scope is not None:
        _lib.check(st._fn("search_variants_scoped")(st._h, scope.handle, q.ctypes.data_as(f32p), len(q), q.shape[1], k, *out))
    elif chunk_ids is not None:
        allow, bits, _keep = st._mask_args(chunk_ids)
        _lib.check(st._fn("search_variants_masked")(st._h, q.ctypes.data_as(f32p), len(q), q.shape[1], k, allow, bits, *out))
    else:
        _lib.check(st._fn("search_variants")(st._h, q.ctypes.data_as(f32p), len(q), q.shape[1], k, *out))
    return cos, ids, int(count.value)


def _same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


class Pair:
    """A VectorStore and its model, driven together."""

    def __init__(self, VS, head, path, seen):
        self.VS, self.head, self.path, self.seen = VS, head, path, seen
        self.m = StoreModel(head["dim"], head["id_base"], head["shards"], head["stripe"])
        self.st = _open(VS, head, path)
        self.single = head["shards"] == 1
        self.scopes = {}   # name -> (Scope, ids): the walk's long-lived scopes
        self.memo = set()
        self.zero_done = self.big_k_done = False
        self.int8_states = 0

    def close(self):
        self.st.close()

    # ---- the operations ----
    def insert(self, rows):
        got, exp = self.st.insert_embeddings(rows).tolist(), self.m.insert(rows)
        assert got == exp, f"insert returned ids {got[:3]}..{got[-1:]}, the model issues {exp[:3]}..{exp[-1:]}"
        return exp

    def delete(self, ids):
        got, exp = self.st.delete_chunks(list(ids)), self.m.delete(ids)
        assert got == exp, f"delete counted {got}, the model {exp}"
        return exp

    def build(self):
        self.st.build_index()
        return self.m.build()

    def clear(self):
        self.st.clear()
        self.m.clear()

    def reopen(self):
        self.scopes = {}
        self.st.close()   # (closes its scopes first)
        self.st = _open(self.VS, self.head, self.path)
        self.m.reopen()

    def set_groups(self, ids, groups):
        self.st.set_groups(ids, groups)
        self.m.set_groups(ids, groups)

    def books(self):
        st, m = self.st, self.m
        got = (len(st), st.next_id(), st.stored_rows(), st.is_indexed())
        assert got == (len(m), m.next_id, m.stored_rows(), m.built), f"(len, next_id, stored_rows, indexed) = {got}, the model: " \
            f"{(len(m), m.next_id, m.stored_rows(), m.built)}"
        if self.single:
            assert st.groups_info()[0] == m.groups_assigned()

    # ---- judging ----
    def judge(self, qs, k, got, allowed=None, per_file=None, tag=""):
        """Every list of a batched answer (cos [nq, k], ids [nq, k], counts [nq]) through the model's check; a list
        whose bytes were judged before under the same terms is not judged twice."""
        cos, ids, counts = got
        self.seen["searches"] += 1
        akey = None if allowed is None else np.asarray(allowed, np.int64).tobytes()
        for n in range(len(counts)):
            key = (self.m.version, qs[n].tobytes(), k, akey, per_file, cos[n].tobytes(), ids[n].tobytes(), int(counts[n]))
            if key in self.memo:
                continue
            try:
                err = self.m.check(qs[n], k, (cos[n], ids[n], counts[n]), allowed=allowed, per_file=per_file)
            except AssertionError as e:
                raise AssertionError(f"{tag}, query {n}: {e}") from None
            self.memo.add(key)
            self.seen["judged"] += 1
            if err > self.seen["max_err"]:
                self.seen["max_err"], self.seen["tol_of_max"] = err, self.m.tol

    def queries(self, step):
        """Six queries: two random, the rest planted on live rows at structural positions (-> their expected top-1:
        the lowest id that holds the same bytes); once per walk a zero query takes a planted one's place."""
        m, dim = self.m, self.m.dim
        qs = [q for q in synth_rows(9100 + step, 0, 2, dim)]
        expect = [None, None]
        order = m.stored_live()
        want = 4
        if order and not self.zero_done:
            qs.append(np.zeros(dim, np.float32))
            expect.append(None)
            self.zero_done, want = True, 3
        cand = []
        if order:
            cand += [order[0], order[-1]]
            for stored in m.stored:                      # both sides of each edge the stored rows span
                for e in (128, 1024):
                    if len(stored) > e:
                        cand += [i for i in (stored[e - 1], stored[e]) if m.is_live(i)]
            cand += [i for i in (m.last_appended, m.moved) if i is not None and m.is_live(i)]
        cand = [i for i in dict.fromkeys(cand) if m.rows[i].any()]
        live, cls = m.live_ids(), m._dup_class()
        for j in range(min(want, len(cand))):
            i = cand[(step + j) % len(cand)] if len(cand) > want else cand[j]
            qs.append(m.rows[i].copy())
            expect.append(int(cls[np.searchsorted(live, i)]))
        while len(qs) < 6:
            qs.append(synth_rows(9200 + step, len(qs), 1, dim)[0])
            expect.append(None)
        return np.stack(qs), expect

    def check_state(self, step):
        """Every search kind at the state the store is in (built)."""
        st, m = self.st, self.m
        qs, expect = self.queries(step)
        live = m.live_ids()
        rng = np.random.default_rng(step)
        issued = np.arange(m.id_base, m.next_id)
        sets = {"half": np.sort(rng.choice(issued, len(issued) // 2, replace=False)) if len(issued) else issued,
                "tenth": live[len(live) // 3: len(live) // 3 + max(1, len(live) // 10)],
                "empty": np.zeros(0, np.int64), "all": live}
        ks = list(KS)
        if not self.big_k_done and 0 < len(live) and len(live) + 5 <= _lib.CS_MAX_K and (m.removed or any(m.compacted)):
            ks.append(len(live) + 5)
            self.big_k_done = True
        routes = ("auto", "gather", "filter") if self.single else (None,)
        adhoc = {name: st.scope(ids) for name, ids in sets.items()}
        serving = self.single and m.dim == 384 and st.filter_state()[0] == 2
        try:
            for k in ks:
                # plain: one query on the streaming route and on the default route, then batched
                for route in (st.ROUTE_STREAM, st.ROUTE_COST):
                    st.set_single_query_route(route)
                    for n, q in enumerate(qs):
                        got = st.search_raw(q, k)
                        self.judge(qs[n:n + 1], k, got, tag=f"plain, one query, route {route}, k={k}")
                        if expect[n] is not None:
                            assert got[1][0][0] == expect[n], f"planted query {n}: top-1 is {got[1][0][0]}, not {expect[n]}"
                before = st.debug_counters()[0] if serving else 0
                plain = st.search_raw(qs, k)
                if serving and st.debug_counters()[0] > before and st.filter_state()[0] == 2:
                    self.int8_states += 1
                    serving = False
                self.judge(qs, k, plain, tag=f"plain, batched, k={k}")
                for n, e in enumerate(expect):
                    assert e is None or plain[1][n][0] == e, f"planted query {n} (batched): top-1 is {plain[1][n][0]}, not {e}"
                self.judge(qs[None], k, tuple(np.asarray(x)[None] for x in _variants_raw(st, qs, k)), tag=f"variants, k={k}")
                # masked and scoped over the same sets; the long-lived scopes of the walk
                for name, ids in list(sets.items()) + [(f"walk scope {n}", i) for n, (_, i) in self.scopes.items()]:
                    masked = st.search_raw(qs, k, chunk_ids=ids)
                    self.judge(qs, k, masked, allowed=ids, tag=f"masked({name}), k={k}")
                    sc = adhoc[name] if name in adhoc else self.scopes[name[len("walk scope "):]][0]
                    for route in routes:
                        if route:
                            sc.set_route(route)
                        scoped = st.search_raw(qs, k, scope=sc)
                        self.judge(qs, k, scoped, allowed=ids, tag=f"scoped({name}), route {route}, k={k}")
                        assert _same(masked, scoped), f"masked({name}) != scoped({name}) on route {route}, k={k}"
                    if route:
                        sc.set_route("auto")
                    n_live = int(np.isin(ids, live).sum())
                    assert sc.info()[:2] == (len(ids), n_live), f"scope {name}: info {sc.info()}, expected {(len(ids), n_live)}"
                    if name == "all":
                        assert _same(plain, masked), f"plain != masked(all live), k={k}"
                    if name == "half":  # one query and the variants form, masked against scoped
                        one_m, one_s = st.search_raw(qs[3], k, chunk_ids=ids), st.search_raw(qs[3], k, scope=sc)
                        self.judge(qs[3:4], k, one_m, allowed=ids, tag=f"masked({name}), one query, k={k}")
                        assert _same(one_m, one_s), f"masked({name}) != scoped({name}), one query, k={k}"
                        var_m, var_s = _variants_raw(st, qs, k, chunk_ids=ids), _variants_raw(st, qs, k, scope=sc)
                        self.judge(qs[None], k, tuple(np.asarray(x)[None] for x in var_m), allowed=ids, tag=f"variants masked({name}), k={k}")
                        assert _same(var_m, var_s), f"variants: masked({name}) != scoped({name}), k={k}"
                if self.single:
                    for per_file in (1, 3):
                        grouped = st.search_raw(qs, k, per_file=per_file)
                        self.judge(qs, k, grouped, per_file=per_file, tag=f"grouped, per_file={per_file}, k={k}")
                    assert _same(plain, st.search_raw(qs, k, per_file=k)), f"grouped with per_file = k != plain, k={k}"
        finally:
            for sc in adhoc.values():
                sc.close()


def _run_walk(VS, walk, path, seen):
    p = Pair(VS, walk[0], path, seen)
    try:
        for step, op in enumerate(walk[1:], 1):
            try:
                kind = op["op"]
                args = resolve(op, p.m)
                if kind == "insert":
                    p.insert(args)
                elif kind == "delete":
                    p.delete(args)
                elif kind == "build":
                    p.build()
                elif kind == "clear":
                    p.clear()
                elif kind == "reopen":
                    p.reopen()
                elif kind == "groups":
                    p.set_groups(*args)
                elif kind == "scope":
                    p.scopes[op["name"]] = (p.st.scope(args), np.asarray(args, np.int64))
                p.books()
                if kind in ("build", "reopen") and p.m.built:
                    p.check_state(step)
                elif not p.m.built:
                    with pytest.raises(_lib.CsError, match=NOT_BUILT):
                        p.st.search_raw(np.ones(p.m.dim, np.float32), 1)
            except (AssertionError, _lib.CsError) as e:
                raise AssertionError(f"walk {walk[0]} failed at step {step}, {op}: {e}\nreplay: {walk[:step + 1]}") from e
        return p
    finally:
        p.close()


@pytest.mark.parametrize("seed,dim,sharded", WALKS)
def test_walk(VS, tmp_path, seen, seed, dim, sharded):
    p = _run_walk(VS, make_walk(seed, dim, sharded), str(tmp_path / "db"), seen)
    assert p.zero_done and p.big_k_done
    if not sharded and dim == 384:
        # (only dim 384 keeps filter copies here, and a shard of these walks stays below phase 0 of the filter)
        assert p.int8_states >= 1, "the int8 filter served no checked state: the walk never left the exact kernels"


# ---- directed regressions: the index a reclaiming build leaves without a row -------------------------

def _planted(p, rows, base, rs, gone=()):
    """rows[r] as a query finds id base + r first — one query, batched, masked, scoped, grouped, on either route."""
    st = p.st
    qs = np.stack([rows[r] for r in rs])
    want = [base + r for r in rs]
    for route in (st.ROUTE_STREAM, st.ROUTE_COST):
        st.set_single_query_route(route)
        for q, w in zip(qs, want):
            got = st.search_raw(q, 5)
            p.judge(q[None], 5, got, tag=f"planted, route {route}")
            assert got[1][0][0] == w, f"the row of id {w} is reported as id {got[1][0][0]}"
            assert not set(got[1][0].tolist()) & set(gone)
    got = st.search_raw(qs, 5)
    p.judge(qs, 5, got, tag="planted, batched")
    assert got[1][:, 0].tolist() == want
    live = p.m.live_ids()
    with st.scope(live) as sc:
        assert _same(got, st.search_raw(qs, 5, chunk_ids=live)) and _same(got, st.search_raw(qs, 5, scope=sc))
    if p.single:
        assert _same(got, st.search_raw(qs, 5, per_file=5))


def _emptied_holds(p, rows, base, old, new):
    """The emptied state's consequences, for reclaimed ids `old` and live ids `new` (rows[i - base] is the row of i)."""
    st = p.st
    assert st.delete_chunks([old[0]]) == 0 and st.is_indexed()            # a spent id names no row
    a, b = new[0], new[1]
    assert p.delete([a]) == 1
    p.build()
    p.books()
    _planted(p, rows, base, [b - base], gone=[a])                          # a is gone, its neighbour is found
    got = st.search_raw(rows[a - base], 5)
    assert a not in got[1][0].tolist()
    assert np.array_equal(st.read_rows(b - base, 1)[0], rows[b - base])    # rows by id
    with pytest.raises(_lib.CsError, match="reclaimed"):
        st.read_rows(old[5] - base, 1)
    with st.scope(old) as sc:                                              # a scope over the spent ids matches nothing
        c, i, n = st.search_raw(rows[b - base], 5, scope=sc)
        assert sc.info()[:2] == (len(old), 0) and n[0] == 0 and (i == NO_ID).all()
    c, i, n = st.search_raw(rows[b - base], 5, chunk_ids=old)
    assert n[0] == 0 and (i == NO_ID).all()


@pytest.mark.parametrize("base", [0, 1000])
def test_an_emptied_index_goes_on_counting(VS, tmp_path, seen, base):
    """Insert 300, build, delete all 300, build: the index stores nothing, and its first 300 ids are spent.  The parent of
    this test's commit fell back to id = id_base + row there: the 200 rows inserted next were issued ids 300..499 and
    reported by every search as ids 0..199."""
    dim = 384
    rows = synth_rows(51, 0, 700, dim)
    p = Pair(VS, {"dim": dim, "id_base": base, "shards": 1, "stripe": 1 << 32}, str(tmp_path / "db"), seen)
    st = p.st
    try:
        assert p.insert(rows[:300]) == list(range(base, base + 300))
        p.build()
        assert p.delete(range(base, base + 300)) == 300
        p.build()
        p.books()
        assert st.stored_rows() == 0 and len(st) == 0 and st.next_id() == base + 300
        c, i, n = st.search_raw(rows[:2], 10)
        assert n.tolist() == [0, 0] and (i == NO_ID).all() and (c == 0).all()
        assert p.insert(rows[300:500]) == list(range(base + 300, base + 500))
        p.build()
        p.books()
        _planted(p, rows, base, [300, 301, 427, 499])
        old, new = list(range(base, base + 300)), list(range(base + 300, base + 500))
        _emptied_holds(p, rows, base, old, new)
        p.reopen()                                                          # the loader re-adds, removes and builds
        p.books()
        assert st is not p.st and p.st.stored_rows() == 199
        st = p.st
        _planted(p, rows, base, [301, 302, 499])
        _emptied_holds(p, rows, base, old, new[1:])
        assert p.insert(rows[500:700]) == list(range(base + 500, base + 700))
        assert p.delete(p.m.live_ids()[::2]) == 199
        assert p.build()                                                    # a reclaim over the compacted index
        p.books()
        live = (p.m.live_ids() - base).tolist()
        _planted(p, rows, base, [live[0], live[57], live[-1]])
        assert np.array_equal(st.read_rows(live[57], 1)[0], rows[live[57]])
        p.clear()                                                           # back to the identity numbering
        assert p.insert(rows[:50]) == list(range(base, base + 50))
        p.build()
        p.books()
        _planted(p, rows, base, [0, 49])
        assert np.array_equal(st.read_rows(0, 50), rows[:50])
    finally:
        p.close()


def test_an_emptied_shard_goes_on_counting(VS, tmp_path, seen):
    """The same through a sharded store: deleting exactly the ids one shard holds empties that shard alone."""
    dim, stripe = 384, 64
    rows = synth_rows(52, 0, 1100, dim)
    p = Pair(VS, {"dim": dim, "id_base": 0, "shards": 3, "stripe": stripe}, str(tmp_path / "db"), seen)
    try:
        assert p.insert(rows[:600]) == list(range(600))
        p.build()
        old = [i for i in range(600) if (i // stripe) % 3 == 1]
        assert p.delete(old) == len(old)
        assert p.build() and p.st.shard_lens()[1] == 0
        p.books()
        assert p.insert(rows[600:900]) == list(range(600, 900))
        p.build()
        p.books()
        new = [i for i in range(600, 900) if (i // stripe) % 3 == 1]
        assert len(new) > 64 and p.st.shard_lens()[1] == len(new)
        _planted(p, rows, 0, [new[0], new[1], new[-1], 0, 899])
        _emptied_holds(p, rows, 0, old, new)
        p.reopen()
        p.books()
        _planted(p, rows, 0, [new[1], new[2], new[-1], 0])
        _emptied_holds(p, rows, 0, old, new[1:])
        assert p.insert(rows[900:1100]) == list(range(900, 1100))
        half = p.m.live_ids()[::2]
        assert p.delete(half) == len(half)
        assert p.build()
        p.books()
        live = p.m.live_ids().tolist()
        _planted(p, rows, 0, [live[0], live[101], live[-1]])
        assert np.array_equal(p.st.read_rows(live[101], 1)[0], rows[live[101]])
    finally:
        p.close()
