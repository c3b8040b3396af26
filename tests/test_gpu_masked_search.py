"""Masked search (cs_index_search_masked & co., codesearch_amd/csrc/scan_masked.hip): the exact top-k over the live rows
whose chunk id a bitmap allows — the exact form of the reference's filter_path, which post-filters the top `limit * 3`
(/root/reference/src/mcp/mod.rs:251-252,400-425).

Bars: a masked search answers exactly like a FRESH store of the allowed rows on the streaming route — the same cosines bit
for bit, the same ids through the allowed rows' numbering — for every dim path, mask shape, k and query count; ids match
the CPU oracle over 1M rows; deleted rows never come back; ids are absolute (id_base, masks shorter or longer than
next_id); the variant merge and the sharded store agree; concurrent masks do not mix; errors are cs_index_search's."""
import threading

import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd.search import merge_variant_results, should_use_vector_only
from codesearch_amd.synth import synth_planted, synth_rows
from codesearch_amd.vector_store import allow_mask

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def VS(gpu_lib):
    from codesearch_amd import VectorStore

    assert gpu_lib.cs_device_count() >= 1, "no HIP device visible"
    return VectorStore


def _fresh(VS, rows):
    st = VS(None, rows.shape[1])
    st.insert_embeddings(rows)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    return st


def _masks(n, rng):
    """name -> sorted allowed row numbers of an n-row store."""
    lo = n // 3
    return {
        "all": np.arange(n),
        "none": np.zeros(0, np.int64),
        "single": np.array([n // 2 + 7]),
        "contig10": np.arange(lo, lo + n // 10),
        "random1": np.sort(rng.choice(n, max(1, n // 100), replace=False)),
        "random50": np.sort(rng.choice(n, n // 2, replace=False)),
    }


def _check_against_fresh(st, fresh, allowed_ids, qs, k):
    """st searched with mask = allowed_ids (absolute ids) vs fresh (ids 0.. over the same rows): one query per fresh call,
    so every reference answer comes from the streaming scan."""
    c0, i0, n0 = st.search_raw(qs, k, chunk_ids=allowed_ids)
    for q in range(qs.shape[0]):
        if fresh is None:
            assert n0[q] == 0
            continue
        c1, i1, n1 = fresh.search_raw(qs[q], k)
        assert n0[q] == n1[0] == min(k, allowed_ids.size)
        assert c0[q].tobytes() == c1[0].tobytes()
        assert i0[q][:n0[q]].tolist() == allowed_ids[i1[0][:n1[0]]].tolist()


SHAPES = [(1, 1), (10, 1), (10, 3), (200, 9), (1024, 16), (10, 40), (200, 1), (1024, 1)]  # (k, nq)


@pytest.mark.parametrize("dim", [384, 768, 1024, 100])
def test_masked_equals_fresh_store_of_allowed_rows(VS, dim):
    rng = np.random.default_rng(dim)
    n, seed = 12_000, 7100 + dim
    rows = synth_rows(seed, 0, n, dim)
    st = VS(None, dim)
    st.insert_embeddings(rows)
    st.build_index()
    qs = np.concatenate([synth_rows(seed + 1, 0, 38, dim), rows[[5, n - 3]]])
    for name, allowed in _masks(n, rng).items():
        fresh = _fresh(VS, rows[allowed]) if allowed.size else None
        for k, nq in SHAPES:
            _check_against_fresh(st, fresh, allowed.astype(np.uint32), qs[:nq], k)
        if fresh is not None:
            fresh.close()


@pytest.mark.parametrize("k", [10, 200])
def test_masked_ids_match_oracle_over_1m_rows(VS, oracle, k):
    n, dim, seed = 1_000_000, 384, 0x5EED
    st = VS(None, dim)
    st.insert_synthetic(n, seed, 0)
    st.build_index()
    corpus = oracle.synth_rows(seed, 0, n, dim)
    rng = np.random.default_rng(k)
    qs = synth_rows(seed + 9, 0, 2, dim)
    for allowed in (np.sort(rng.choice(n, n // 2, replace=False)),      # prime pass + gathered scan
                    np.arange(200_000, 300_000),                          # a contiguous tenth
                    np.sort(rng.choice(n, n // 100, replace=False))):
        dead = ~allow_mask(allowed, n)  # the oracle's tombstones: everything not allowed
        cos, ids, cnt = st.search_raw(qs, k, chunk_ids=allowed)
        for q in range(qs.shape[0]):
            ec, ei = oracle.scan_topk(corpus, qs[q], k, dead=dead, mode="omp")
            assert cnt[q] == k and ids[q].tolist() == ei.tolist()
            assert np.abs(cos[q] - ec).max() < 1e-4


def test_mask_finds_what_the_post_filter_misses(VS):
    """The reference's filter_path: top limit * 3, then drop what is outside the directory.  A query whose exact match
    lies outside the mask and whose best in-mask rows are weaker than hundreds of outside rows gets nothing from the
    post-filter; the masked search returns the in-mask rows."""
    n, dim, seed, limit = 50_000, 384, 0xF117, 10
    rows = synth_rows(seed, 0, n, dim)
    inside = np.arange(40_000, 40_000 + 300)  # "a directory": 0.6 % of the chunks
    q = rows[123].copy()                      # its exact match is outside
    rows[inside[37]] = 0.8 * q + 0.2 * rows[inside[37]]  # a weaker match inside
    st = VS(None, dim)
    st.insert_embeddings(rows)
    st.build_index()
    c, i, cnt = st.search_raw(q, limit)
    assert i[0][0] == 123
    c3, i3, n3 = st.search_raw(q, limit * 3)
    post = [x for x in i3[0][:n3[0]].tolist() if 40_000 <= x < 40_300]
    cm, im, nm = st.search_raw(q, limit, chunk_ids=inside)
    assert nm[0] == limit and im[0][0] == inside[37]
    assert set(im[0].tolist()) <= set(inside.tolist())
    assert len(post) < limit  # the post-filter comes back short
    # the masked answer is the exact in-mask top-k
    fresh = _fresh(VS, rows[inside])
    cf, if_, nf = fresh.search_raw(q, limit)
    assert cm[0].tobytes() == cf[0].tobytes() and im[0].tolist() == inside[if_[0]].tolist()


def test_deleted_rows_never_return_and_ids_are_absolute(VS):
    n, dim, seed, k = 20_000, 384, 0xDE1, 50
    rows = synth_rows(seed, 0, n, dim)
    base = 1_000_000
    st = VS(None, dim, id_base=base)
    ids = st.insert_embeddings(rows)
    assert ids[0] == base
    st.build_index()
    rng = np.random.default_rng(3)
    allowed = np.sort(rng.choice(n, 4000, replace=False))
    dead = np.sort(rng.choice(allowed, 300, replace=False))  # 1.5 % of the rows: tombstones, no reclaim
    st.delete_chunks((dead + base).tolist())
    st.build_index()
    assert st.stored_rows() == n
    live = np.setdiff1d(allowed, dead)
    qs = np.concatenate([synth_rows(seed + 1, 0, 3, dim), rows[dead[:2]]])
    fresh = _fresh(VS, rows[live])
    _check_against_fresh(st, fresh, (live + base).astype(np.uint32), qs, k)
    # the mask may name the dead ids too: they stay out
    c0, i0, n0 = st.search_raw(qs, k, chunk_ids=allowed + base)
    c1, i1, n1 = st.search_raw(qs, k, chunk_ids=live + base)
    assert c0.tobytes() == c1.tobytes() and i0.tobytes() == i1.tobytes() and n0.tolist() == n1.tolist()
    # k above the allowed live rows: counts = those rows
    few = live[:7] + base
    _, i2, n2 = st.search_raw(qs, 100, chunk_ids=few)
    assert n2.tolist() == [7] * qs.shape[0] and sorted(i2[0][:7].tolist()) == few.tolist()
    # reclaiming build (>= 10 % dead): the same answers
    more = np.setdiff1d(np.arange(n), allowed)[:3000]
    st.delete_chunks((more + base).tolist())
    st.build_index()
    assert st.stored_rows() == n - 3300
    c3, i3, n3 = st.search_raw(qs, k, chunk_ids=allowed + base)
    assert c3.tobytes() == c1.tobytes() and i3.tobytes() == i1.tobytes() and n3.tolist() == n1.tolist()


def test_mask_length_and_ids_never_issued(VS, gpu_lib):
    from codesearch_amd._lib import f32p, u32p

    n, dim, k = 5_000, 768, 20
    rows = synth_rows(0xAB, 0, n, dim)
    st = VS(None, dim)
    st.insert_embeddings(rows)
    st.build_index()
    q = synth_rows(0xAC, 0, 1, dim)
    fresh = _fresh(VS, rows[:1000])

    def masked(words, bits):
        cos = np.zeros((1, k), np.float32)
        ids = np.zeros((1, k), np.uint32)
        cnt = np.zeros(1, np.uint32)
        _lib.check(gpu_lib.cs_index_search_masked(st.handle, q.ctypes.data_as(f32p), 1, dim, k,
                                                   words.ctypes.data_as(u32p) if words is not None else None, bits,
                                                   cos.ctypes.data_as(f32p), ids.ctypes.data_as(u32p),
                                                   cnt.ctypes.data_as(u32p)))
        return cos, ids, cnt

    c1, i1, _ = fresh.search_raw(q, k)
    # a mask shorter than next_id: ids [0, 1000) only
    c, i, cnt = masked(np.full(32, ~np.uint32(0), np.uint32), 1000)
    assert cnt[0] == k and c.tobytes() == c1.tobytes() and i.tobytes() == i1.tobytes()
    # bits beyond next_id (never issued) are ignored
    w = np.zeros(1000, np.uint32)
    w[:32] = allow_mask(np.arange(1000), 1024)
    w[200:] = ~np.uint32(0)  # ids 6,400 .. 31,999: never issued
    c, i, cnt = masked(w, 32000)
    assert c.tobytes() == c1.tobytes() and i.tobytes() == i1.tobytes()
    # allow_bits == 0: nothing allowed, success, count 0 (the pointer may be null)
    c, i, cnt = masked(None, 0)
    assert cnt[0] == 0 and (i == 0xFFFFFFFF).all()
    # a null mask with allow_bits > 0 is an argument error
    with pytest.raises(_lib.CsError) as e:
        masked(None, 64)
    assert e.value.code == _lib.CS_ERR_BAD_ARG


def test_masked_variants_equal_merge_of_masked_searches(VS):
    n, dim, k, seed = 30_000, 384, 200, 0x7A7
    rows = synth_rows(seed, 0, n, dim)
    st = VS(None, dim)
    st.insert_embeddings(rows)
    st.build_index()
    rng = np.random.default_rng(5)
    allowed = np.sort(rng.choice(n, 3000, replace=False))
    # nine variants of one query, two of them near an allowed row (a confident answer)
    base = rows[allowed[11]]
    qs = np.stack([base + 0.01 * synth_rows(seed + 2 + v, 0, 1, dim)[0] for v in range(9)]).astype(np.float32)
    from codesearch_amd import Chunk, EmbeddedChunk

    st2 = VS(None, dim)  # the same rows with metadata, so merge_variant_results sees SearchResults
    st2.insert_chunks([EmbeddedChunk(Chunk(f"c{i}", 1, 2, "Function", f"f{i // 100}.rs"), rows[i]) for i in range(n)])
    st2.build_index()
    per = st2.search_batch(qs, k, chunk_ids=allowed)
    want = merge_variant_results(per, k)
    got, flag = st2.search_variants(qs, k, chunk_ids=allowed)
    assert len(got) == len(want) == k
    assert [r.score for r in got] == [r.score for r in want]
    assert sorted(r.id for r in got) == sorted(r.id for r in want)
    assert set(r.id for r in got) <= set(allowed.tolist())
    assert flag == should_use_vector_only(want, False)
    # and the raw variant outputs against cs_index_search_variants over a fresh store of the allowed rows
    import ctypes as C

    from codesearch_amd._lib import f32p, u32p

    def raw(store, mask):
        cos = np.zeros(k, np.float32)
        ids = np.zeros(k, np.uint32)
        cnt, fl = C.c_uint32(), C.c_int32()
        if mask is None:
            _lib.check(store._fn("search_variants")(store._h, qs.ctypes.data_as(f32p), 9, dim, k, cos.ctypes.data_as(f32p),
                                                    ids.ctypes.data_as(u32p), C.byref(cnt), C.byref(fl)))
        else:
            _lib.check(store._fn("search_variants_masked")(store._h, qs.ctypes.data_as(f32p), 9, dim, k,
                                                           mask.ctypes.data_as(u32p), n, cos.ctypes.data_as(f32p),
                                                           ids.ctypes.data_as(u32p), C.byref(cnt), C.byref(fl)))
        return cos, ids, cnt.value, fl.value

    cm, im, nm, fm = raw(st, allow_mask(allowed, n))
    fresh = _fresh(VS, rows[allowed])
    cf, if_, nf, ff = raw(fresh, None)
    assert nm == nf and fm == ff and cm.tobytes() == cf.tobytes()
    assert im[:nm].tolist() == allowed[if_[:nf]].tolist()


def _raw_variants(store, qs, k, allowed, next_id):
    import ctypes as C

    from codesearch_amd._lib import f32p, u32p

    mask = allow_mask(allowed, next_id)
    cos = np.zeros(k, np.float32)
    ids = np.zeros(k, np.uint32)
    cnt, fl = C.c_uint32(), C.c_int32()
    _lib.check(store._fn("search_variants_masked")(store._h, qs.ctypes.data_as(f32p), qs.shape[0], qs.shape[1], k,
                                                   mask.ctypes.data_as(u32p) if mask.size else None,
                                                   next_id if mask.size else 0, cos.ctypes.data_as(f32p),
                                                   ids.ctypes.data_as(u32p), C.byref(cnt), C.byref(fl)))
    return cos, ids, cnt.value, fl.value


@pytest.mark.parametrize("stripe", [1, 100, 4096])
def test_shards_masked_equal_single_index(VS, stripe):
    n, dim, seed = 40_000, 384, 0x5A4D
    rows = synth_rows(seed, 0, n, dim)
    one = VS(None, dim)
    one.insert_embeddings(rows)
    one.build_index()
    sh = VS(None, dim, devices=[0] * 8, rows_per_stripe=stripe)
    sh.insert_embeddings(rows)
    rng = np.random.default_rng(stripe)
    gone = rng.choice(n, 500, replace=False)
    one.delete_chunks(gone.tolist())
    sh.delete_chunks(gone.tolist())
    one.build_index()
    sh.build_index()
    qs = synth_rows(seed + 1, 0, 5, dim)
    for allowed in (np.arange(10_000, 14_000), np.sort(rng.choice(n, 2000, replace=False)), np.array([77, 30_001]),
                    np.zeros(0, np.int64)):
        for k in (10, 200):
            a = one.search_raw(qs, k, chunk_ids=allowed)
            b = sh.search_raw(qs, k, chunk_ids=allowed)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), (stripe, allowed.size, k)
        # variants: the raw outputs (these stores carry no metadata)
        va = _raw_variants(one, qs, 50, allowed, n)
        vb = _raw_variants(sh, qs, 50, allowed, n)
        assert va[2] == vb[2] and va[3] == vb[3] and va[0].tobytes() == vb[0].tobytes() and va[1].tobytes() == vb[1].tobytes()
    # unmasked shard searches are untouched by the masked ones in between
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one.search_raw(qs, 10), sh.search_raw(qs, 10)))


def test_concurrent_masks_on_one_store(VS):
    n, dim, k = 60_000, 384, 25
    st = VS(None, dim)
    st.insert_synthetic(n, 0xC0C0, 0)
    st.build_index()
    q = synth_rows(0xC0C1, 0, 2, dim)
    before = st.search_raw(q, k)
    counters = st.debug_counters()
    masks = [np.arange(t * 7000, t * 7000 + 5000) for t in range(8)]
    want = [st.search_raw(q, k, chunk_ids=m) for m in masks]
    got = [None] * 8
    errors = []

    def work(t):
        try:
            for _ in range(6):
                r = st.search_raw(q, k, chunk_ids=masks[t])
                if not all(x.tobytes() == y.tobytes() for x, y in zip(r, want[t])):
                    errors.append(t)
            got[t] = r
        except Exception as e:  # pragma: no cover - reported below
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors
    for t in range(8):
        assert set(got[t][1][0].tolist()) <= set(masks[t].tolist())
    assert st.debug_counters() == counters  # masked searches leave the batched-path counters alone
    after = st.search_raw(q, k)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after))


def test_errors_are_those_of_search(VS, gpu_lib):
    st = VS(None, 384)
    st.insert_synthetic(1000, 1, 0)
    q = synth_rows(2, 0, 1, 384)
    with pytest.raises(_lib.CsError, match="Index not built"):
        st.search_raw(q, 5, chunk_ids=[1, 2])
    st.build_index()
    with pytest.raises(_lib.CsError, match="Query embedding dimension mismatch: expected 384, got 100"):
        st.search_raw(np.zeros((1, 100), np.float32), 5, chunk_ids=[1])
    with pytest.raises(_lib.CsError, match="k must be in 1..1024, got 0"):
        st.search_raw(q, 0, chunk_ids=[1])
    with pytest.raises(_lib.CsError, match="k must be in 1..1024, got 1025"):
        st.search_raw(q, 1025, chunk_ids=[1])
    with pytest.raises(_lib.CsError, match="at most 16 query variants"):
        st.search_variants(np.zeros((17, 384), np.float32), 5, chunk_ids=[1])
    # the same texts as the unmasked search
    for call in (lambda: st.search_raw(q, 1025), lambda: st.search_raw(q, 1025, chunk_ids=[1])):
        with pytest.raises(_lib.CsError) as e:
            call()
        assert "k must be in 1..1024" in str(e.value)
    # an empty id list: success, nothing found
    c, i, cnt = st.search_raw(q, 5, chunk_ids=[])
    assert cnt.tolist() == [0]
    res, flag = st.search_variants(q, 5, chunk_ids=[])
    assert res == [] and flag is False
