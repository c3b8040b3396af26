"""The index life cycle under the kinds that start from stored rows — similar chunks, similar pairs, similar clusters — and
under the boosted search (tests/store_model.py): the extended walks — the walks of tests/test_gpu_store_walk.py with a class
table assigned beside every group table and near-copies planted around the pairs' bound in every larger insert — applied
to a VectorStore and to the model side by side.  After every operation the books must agree, the class table's included;
at every searchable state every one of these kinds is judged against float64 cosines by the model's check_similar,
check_pairs, check_clusters and check_boosted (the derived band 2 * (dim + 8) * 2**-24 and nothing measured), next to the
project's own identities: equal bytes across the routes, the labels of clusters_of_pairs over the pairs just returned, the
all-ones table against the plain search (in the boosted search's own order: Pair.all_ones_is_plain).  Two scopes — every
other id (E) and the rest (O) of a span larger than a walk issues — are held across the whole walk.
tests/test_store_model.py vouches on the CPU for the judges and for what each walk run here reaches.  A failure's message
carries the walk, the step and the operations up to it: a directed test to replay.

Deliberately left out: the boosted search with per_file (the capped walk over scores), the grouped scoped kinds (they
have tests/test_gpu_store_walk_grouped_scoped.py) and sharded stores, which have none of these kinds (one test below keeps
asserting that each call refuses there)."""
import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd.search import clusters_of_pairs
from codesearch_amd.synth import synth_rows
from tests.store_model import BOUND, EDGES, NO_ID, NOT_BUILT, Planted, StoreModel, apply, make_walk, new_model, resolve

pytestmark = pytest.mark.gpu

SPAN = 12_000  # the scopes name the ids of [id_base, id_base + SPAN): more than any walk issues
MODES = ("none", "self", "file")
TABLES = (np.array([1, 1.15, 0.5, 0, 1.01], np.float32), np.array([1, 1.15, 0.5], np.float32), np.zeros(0, np.float32))
WALKS = [(s, 384) for s in range(4)] + [(s, 100) for s in range(2)]
UNSUPPORTED_DIM = "dim 384, 768 or 1024"


@pytest.fixture(scope="module")
def VS(gpu_lib):
    from codesearch_amd import VectorStore

    assert gpu_lib.cs_device_count() >= 1, "no HIP device visible"
    return VectorStore


def _same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


class Pair:
    """A VectorStore and its model, driven together, with the two scopes and what the inserts planted."""

    def __init__(self, VS, head, path):
        self.VS, self.head, self.path = VS, head, path
        self.m = new_model([head])
        self.planted = Planted()
        base = head["id_base"]
        self.e_ids, self.o_ids = np.arange(base, base + SPAN, 2), np.arange(base + 1, base + SPAN, 2)
        self.judged = {"similar": 0, "pairs": 0, "clusters": 0, "boosted": 0}
        self.once = {"zero_source": False, "tombstoned_source": False, "reclaimed_source": False, "never_issued_source": False,
                     "below_base_source": not base, "emptied": False, "under_two_live": False, "full_join": False,
                     "min_cos": False}
        self.refreshed = self.filter_states = self.max_err = 0
        self._open()

    def _open(self):
        self.st = self.VS(self.path, self.head["dim"], id_base=self.head["id_base"])
        self.E, self.O = self.st.scope(self.e_ids), self.st.scope(self.o_ids)

    def close(self):
        self.st.close()

    def step(self, op):
        st, m = self.st, self.m
        kind = op["op"]
        args = resolve(op, m)
        ids = None
        if kind == "insert":
            ids = apply(op, args, m)
            assert st.insert_embeddings(args).tolist() == ids
        elif kind == "delete":
            assert st.delete_chunks(list(args)) == apply(op, args, m)
        elif kind == "build":
            st.build_index()
            apply(op, args, m)
        elif kind == "clear":
            st.clear()
            apply(op, args, m)
        elif kind == "reopen":
            st.close()  # (closes the scopes)
            self._open()
            apply(op, args, m)
        elif kind == "groups":
            st.set_groups(*args)
            apply(op, args, m)
        elif kind == "classes":
            st.set_classes(*args)
            apply(op, args, m)
        self.planted.after(op, ids, m)
        return kind

    def books(self):
        st, m = self.st, self.m
        got = (len(st), st.next_id(), st.stored_rows(), st.is_indexed(), st.groups_info()[0], st.classes_info()[0])
        exp = (len(m), m.next_id, m.stored_rows(), m.built, m.groups_assigned(), m.classes_assigned())
        assert got == exp, f"(len, next_id, stored_rows, indexed, groups, classes) = {got}, the model: {exp}"
        assert m.next_id <= self.head["id_base"] + SPAN

    def refuses_unbuilt(self):
        st, q = self.st, np.ones((1, self.m.dim), np.float32)
        for call in (lambda: st.similar_raw([self.m.id_base], 1), lambda: st.similar_raw([self.m.id_base], 1, scope=self.E),
                     lambda: st.similar_pairs_raw(BOUND), lambda: st.similar_pairs_raw(BOUND, scope=self.E, other=self.O),
                     lambda: st.similar_clusters_raw(BOUND), lambda: st.search_raw(q, 1, class_weights=TABLES[0]),
                     lambda: st.search_raw(q, 1, class_weights=TABLES[0], scope=self.E),
                     lambda: st.search_variants_raw(q, 1, class_weights=TABLES[0])):
            with pytest.raises(_lib.CsError, match=NOT_BUILT):
                call()

    # ---- similar ----
    def sources(self, step):
        """Up to 8 live source ids with magnitude: the first and last stored, last_appended, moved, a planted clone, its
        source, a chain's middle, a member of an exact-duplicate class, both sides of each edge the stored rows span."""
        m = self.m
        order = m.stored_live()
        cand = [order[0], order[-1]] + [i for i in (m.last_appended, m.moved) if i is not None and m.is_live(i)]
        clones = self.planted.live_clones(m)
        if clones:
            cand += list(clones[step % len(clones)][:2])
        cand += [c[1] for c in self.planted.chains if m.is_live(c[1])][:1]
        live, cls = m.live_ids(), m._dup_class()
        cand += live[cls != live][-1:].tolist()
        edges = [i for e in EDGES if len(m.stored[0]) > e for i in (m.stored[0][e - 1], m.stored[0][e]) if m.is_live(i)]
        cand += edges[step % 2:] + edges[:step % 2]  # (as many as fit: which side of which edge comes first turns with the step)
        cand = [int(i) for i in dict.fromkeys(cand) if m.rows[i].any()][:8]
        if not self.once["zero_source"]:
            zero = [int(i) for i in live if not m.rows[int(i)].any()]
            if zero and cand:
                cand[-1] = zero[0]
                self.once["zero_source"] = True
        return cand, (clones[step % len(clones)][0] if clones else cand[0] if cand else None)

    def judge_similar(self, srcs, k, got, mode, min_cos=None, allowed=None, tag=""):
        m = self.m
        live, cls = m.live_ids(), m._dup_class()
        for n, s in enumerate(srcs):
            err = m.check_similar(s, k, (got[0][n], got[1][n], got[2][n]), mode, min_cos=min_cos, allowed=allowed)
            self.max_err = max(self.max_err, err)
            if mode == "none" and allowed is None and min_cos is None and m.rows[s].any():
                first = int(cls[np.searchsorted(live, s)])
                assert got[1][n][0] == first, f"{tag}: similar from id {s} under 'none' starts with {got[1][n][0]}, not {first}"
            self.judged["similar"] += 1

    def check_similar(self, step):
        st, m = self.st, self.m
        if not len(m):
            return
        srcs, bounded = self.sources(step)
        calls = [(srcs, k, mode, None) for mode in MODES for k in (1, 10)] + [(srcs[:1], 200, mode, None) for mode in MODES]
        if len(m) >= 2:
            calls.append(([bounded], 10, "self", m.pick_min_cos(bounded)))
            self.once["min_cos"] = True
        answers = {}
        for route in ("scan", "filter"):
            st.set_similar_route(route)
            before = st.similar_route_info()[0]
            answers[route] = [st.similar_raw(s, k, exclude=mode, min_cos=b) for s, k, mode, b in calls]
            if route == "filter" and st.similar_route_info()[0] > before:
                self.filter_states += 1
        st.set_similar_route("auto")
        for (s, k, mode, b), scan, filt in zip(calls, answers["scan"], answers["filter"]):
            tag = f"similar, k={k}, exclude={mode}, min_cos={b}"
            self.judge_similar(s, k, scan, mode, min_cos=b, tag=tag)
            assert _same(scan, filt), f"{tag}: the scan route and the filter route differ"
        made = self.E.info()[2]
        for mode in MODES:
            got = {}
            for route in ("auto", "gather", "filter"):
                self.E.set_route(route)
                got[route] = st.similar_raw(srcs, 10, exclude=mode, scope=self.E)
            self.E.set_route("auto")
            self.judge_similar(srcs, 10, got["gather"], mode, allowed=self.e_ids, tag=f"similar, scope=E, exclude={mode}")
            assert _same(got["gather"], got["auto"]) and _same(got["gather"], got["filter"]), \
                f"similar, scope=E, exclude={mode}: the scope's routes differ"
        self.refreshed += self.E.info()[2] > made
        assert self.E.info()[1] == int(np.isin(m.live_ids(), self.e_ids).sum())

    def refused_sources(self):
        """A source that names no live row is refused with the documented text — each kind of it once per walk."""
        st, m = self.st, self.m
        stored_dead = sorted(i for i in m.removed if i in m.rows)
        for flag, ids, text in (("tombstoned_source", stored_dead, "the chunk was deleted"),
                                ("reclaimed_source", sorted(m.reclaimed), "the chunk was deleted"),
                                ("never_issued_source", [m.next_id + 3], "was never issued"),
                                ("below_base_source", [m.id_base - 1] if m.id_base else [], "was never issued")):
            if self.once[flag] or not ids or not len(m):
                continue
            live = int(m.live_ids()[0])
            for scope in (None, self.E):
                with pytest.raises(_lib.CsError, match=r"ids\[1\] = %d.*%s" % (ids[-1], text)) as e:
                    st.similar_raw([live, ids[-1]], 5, scope=scope)
                assert e.value.code == _lib.CS_ERR_BAD_ARG
            self.once[flag] = True

    # ---- pairs and clusters ----
    def check_pairs_and_clusters(self, step):
        st, m = self.st, self.m
        if m.dim != 384:
            for call in (lambda: st.similar_pairs_raw(BOUND), lambda: st.similar_pairs_raw(BOUND, scope=self.E),
                         lambda: st.similar_clusters_raw(BOUND)):
                with pytest.raises(_lib.CsError, match=UNSUPPORTED_DIM) as e:
                    call()
                assert e.value.code == _lib.CS_ERR_UNSUPPORTED
            return
        odd = bool(step % 2)
        for other_files in (False, True):
            full = st.similar_pairs_raw(BOUND, other_files=other_files)
            self.max_err = max(self.max_err, m.check_pairs(BOUND, other_files, full))
            cut = st.similar_pairs_raw(BOUND, other_files=other_files, max_pairs=5)
            m.check_pairs(BOUND, other_files, cut, max_pairs=5)
            assert _same(cut[:3], [x[:5] for x in full[:3]]), "the cut list is not the head of the full list"
            labels, clusters, members = st.similar_clusters_raw(BOUND, other_files=other_files)
            m.check_clusters(BOUND, other_files, labels, clusters, members)
            assert full[3] == len(full[1])
            want, n_clusters, n_members = clusters_of_pairs(m.live_ids(), full[1], full[2])
            mine = np.full(len(labels), NO_ID, np.uint32)
            for i, root in want.items():
                mine[i - m.id_base] = root
            assert (labels.tobytes(), clusters, members) == (mine.tobytes(), n_clusters, n_members), \
                "the clusters are not clusters_of_pairs over the pairs just returned"
            self.judged["pairs"] += 2
            self.judged["clusters"] += 1
        inside = st.similar_pairs_raw(BOUND, other_files=odd, scope=self.E)
        m.check_pairs(BOUND, odd, inside, inside=self.e_ids)
        between = st.similar_pairs_raw(BOUND, other_files=not odd, scope=self.E, other=self.O)
        m.check_pairs(BOUND, not odd, between, inside=self.e_ids, other=self.o_ids)
        self.judged["pairs"] += 2
        if 2 <= len(m) <= 128:
            for other_files in (False, True):
                m.check_pairs(None, other_files, st.similar_pairs_raw(None, other_files=other_files))
                self.judged["pairs"] += 1
            self.once["full_join"] = True
        if len(m) < 2:
            assert st.similar_pairs_raw(BOUND)[3] == 0 and st.similar_pairs_raw(None, scope=self.E, other=self.O)[3] == 0
            labels, clusters, members = st.similar_clusters_raw(None)
            assert (clusters, members) == (0, 0) and labels[labels != NO_ID].tolist() == m.live_ids().tolist()
            self.once["under_two_live"] = True

    # ---- boosted ----
    def check_boosted(self, step):
        st, m = self.st, self.m
        qs = [q for q in synth_rows(9300 + step, 0, 2, m.dim)]
        live = [int(i) for i in m.live_ids() if m.rows[int(i)].any()]
        qs.append(m.rows[live[step % len(live)]].copy() if live else synth_rows(9350 + step, 0, 1, m.dim)[0])
        qs = np.stack(qs)
        for k in (10, 200):
            plain = st.search_raw(qs, k)
            ones = st.search_raw(qs, k, class_weights=np.ones(5, np.float32))
            for n in range(len(qs)):
                self.all_ones_is_plain(k, tuple(x[n] for x in plain), tuple(x[n] for x in ones))
                m.check_boosted(qs[n], k, tuple(x[n] for x in ones), np.ones(5, np.float32))
            for table in TABLES if k == 10 else TABLES[step % 3:step % 3 + 1]:  # (k = 200: one table per state, in turn)
                for allowed, scope in ((None, None), (self.e_ids, self.E)):
                    got = st.search_raw(qs, k, class_weights=table, scope=scope)
                    for n in range(len(qs)):
                        err = m.check_boosted(qs[n], k, tuple(x[n] for x in got), table, allowed=allowed)
                        self.max_err = max(self.max_err, err)
                    self.judged["boosted"] += len(qs)
                got = st.search_variants_raw(qs, k, class_weights=table)
                m.check_boosted(qs, k, got[:4], table)
                self.judged["boosted"] += 1
        if not m.stored_rows():
            score, cos, ids, counts = st.search_raw(qs, 10, class_weights=TABLES[0])
            assert (counts == 0).all() and (ids == NO_ID).all() and (cos == 0).all() and (score == 0).all()

    @staticmethod
    def all_ones_is_plain(k, plain, ones):
        """With every weight 1 the boosted search returns the plain search's ids and cosines, equal bytes — in its own
        order: the score s = 1 - (1 - c) / 2 is not injective in the cosine, rows whose scores tie go by id whatever their
        cosines (codesearch_gpu.h, the boosted search's rule), and check_boosted holds the call to that order.  So the plain
        list is put in (score desc, id asc) order first, and a tie that the cut at k runs through is left to the judge."""
        cos, ids, cnt = plain[0][:plain[2]], plain[1][:plain[2]], int(plain[2])
        assert int(ones[3]) == cnt, f"all-ones boosted search: count {ones[3]}, the plain search's is {cnt}, k={k}"
        b = StoreModel.score_of(cos, np.float32(1))
        order = np.lexsort((ids, -b))
        keep = cnt if cnt < k else int((b > b[order[-1]]).sum())
        want = (b[order][:keep], cos[order][:keep], ids[order][:keep])
        assert _same(want, [x[:keep] for x in ones[:3]]), \
            f"boosted with an all-ones table is not the plain search in (score, id) order, k={k}: ids {ones[2][:keep].tolist()} " \
            f"against {want[2].tolist()}, cos {ones[1][:keep].tolist()} against {want[1].tolist()}"

    def check_state(self, step):
        m = self.m
        if not m.stored_rows() and m.next_id > m.id_base:  # the emptied index goes on counting: a spent id names no row
            for scope in (None, self.E):
                with pytest.raises(_lib.CsError, match="the chunk was deleted"):
                    self.st.similar_raw([m.next_id - 1], 5, scope=scope)
            self.once["emptied"] = True
        self.check_similar(step)
        self.refused_sources()
        self.check_pairs_and_clusters(step)
        self.check_boosted(step)


def _run_walk(VS, walk, path):
    p = Pair(VS, walk[0], path)
    try:
        for step, op in enumerate(walk[1:], 1):
            try:
                kind = p.step(op)
                p.books()
                if kind in ("build", "reopen") and p.m.built:
                    p.check_state(step)
                elif not p.m.built:
                    p.refuses_unbuilt()
            except (AssertionError, _lib.CsError) as e:
                raise AssertionError(f"walk {walk[0]} (extended) failed at step {step}, {op}: {e}\nreplay: {walk[:step + 1]}") from e
        return p
    finally:
        p.close()


@pytest.mark.parametrize("seed,dim", WALKS)
def test_walk(VS, tmp_path, seed, dim):
    p = _run_walk(VS, make_walk(seed, dim, False, extended=True), str(tmp_path / "db"))
    print(f"\nextended walk {seed}/{dim}: judged {p.judged}, scope remade {p.refreshed} times, {p.filter_states} states through "
          f"the similar filter, largest |cos_gpu - cos_f64| = {p.max_err:.3e} (tol {p.m.tol:.3e})")
    assert all(p.once.values()) or dim != 384, p.once
    assert all(v for f, v in p.once.items() if f not in ("full_join", "under_two_live")), p.once
    assert p.judged["similar"] >= 100 and p.judged["boosted"] >= 100 and p.refreshed >= 10, (p.judged, p.refreshed)
    if dim == 384:
        assert p.judged["pairs"] >= 100 and p.judged["clusters"] >= 30, p.judged
        assert p.filter_states >= 1, "the filter served no similar search at any checked state"


def test_a_sharded_store_refuses_each_of_these_kinds(VS):
    st = VS(None, 384, devices=[0, 0])
    try:
        st.insert_embeddings(synth_rows(9399, 0, 64, 384))
        st.build_index()
        q = np.ones((1, 384), np.float32)
        for call in (lambda: st.similar_raw([0], 5), lambda: st.set_similar_route("scan"), lambda: st.similar_route_info(),
                     lambda: st.similar_pairs_raw(BOUND), lambda: st.similar_clusters_raw(BOUND),
                     lambda: st.set_classes([0], [1]), lambda: st.classes_info(),
                     lambda: st.search_raw(q, 5, class_weights=TABLES[0]),
                     lambda: st.search_variants_raw(q, 5, class_weights=TABLES[0])):
            with pytest.raises(_lib.CsError, match="a sharded store has no .*no cs_shards_ form yet") as e:
                call()
            assert e.value.code == _lib.CS_ERR_UNSUPPORTED
    finally:
        st.close()
