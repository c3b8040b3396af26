"""Host-side mirror of the reference's VectorStore over the C ABI.

Same method names, argument meaning and error behaviour as
/root/reference/src/vectordb/store.rs:94-750, so tests read like the reference's own
(`store.rs:833-1028`).  The vectors live in HBM behind `cs_index_*`; chunk metadata
(`ChunkMetadata`, store.rs:19-85) stays in host memory keyed by the u32 id, where the
reference keeps it in a second LMDB database.  A store opened with a path persists itself in a
flat form (vectors.f32 + sidecars); LMDB itself, MDB_MAP_FULL resizing and
page statistics are storage-engine concerns and out of scope.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import hashlib
import json
import os
import weakref
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import CsError, f32p, u32p, u64p


# ---- carrier types ---------------------------------------------------------------------------

@dataclass
class Chunk:
    """src/chunker/mod.rs:22-62 (fields the hot path and its metadata need)."""

    content: str
    start_line: int
    end_line: int
    kind: str  # ChunkKind Debug name, e.g. "Function"
    path: str
    context: List[str] = field(default_factory=list)
    signature: Optional[str] = None
    docstring: Optional[str] = None
    is_complete: bool = True
    split_index: Optional[int] = None
    hash: str = ""
    context_prev: Optional[str] = None
    context_next: Optional[str] = None

    def __post_init__(self):
        if not self.hash:  # Chunk::compute_hash, mod.rs:93-97
            self.hash = hashlib.sha256(self.content.encode("utf-8")).hexdigest()


@dataclass
class EmbeddedChunk:
    """src/embed/batch.rs:47-57."""

    chunk: Chunk
    embedding: Sequence[float]


@dataclass
class ChunkMetadata:
    """store.rs:19-85."""

    content: str
    path: str
    start_line: int
    end_line: int
    kind: str
    signature: Optional[str]
    docstring: Optional[str]
    context: Optional[str]
    hash: str
    context_prev: Optional[str] = None
    context_next: Optional[str] = None
    searchable_text: str = ""

    @staticmethod
    def from_embedded_chunk(ec: EmbeddedChunk) -> "ChunkMetadata":
        ch = ec.chunk
        parts = [p for p in (ch.signature, ch.docstring) if p is not None]
        parts += [ch.kind, ch.content]
        return ChunkMetadata(
            content=ch.content, path=ch.path, start_line=ch.start_line, end_line=ch.end_line,
            kind=ch.kind, signature=ch.signature, docstring=ch.docstring,
            context=" > ".join(ch.context) if ch.context else None, hash=ch.hash,
            context_prev=ch.context_prev, context_next=ch.context_next,
            searchable_text="\n".join(parts),
        )


@dataclass
class SearchResult:
    """store.rs:753-772."""

    id: int
    content: str
    path: str
    start_line: int
    end_line: int
    kind: str
    signature: Optional[str]
    docstring: Optional[str]
    context: Optional[str]
    hash: str
    distance: float
    score: float
    context_prev: Optional[str] = None
    context_next: Optional[str] = None


@dataclass
class StoreStats:
    """store.rs:784-792."""

    total_chunks: int
    total_files: int
    indexed: bool
    dimensions: int
    max_chunk_id: int


def cos_to_distance(cos):
    """arroy 0.5.0 Cosine distance (1 - cos)/2 (third-party)."""
    return (np.float32(1.0) - np.asarray(cos, np.float32)) * np.float32(0.5)


def cos_to_score(cos):
    """store.rs:478: score = 1.0 - distance."""
    return np.float32(1.0) - cos_to_distance(cos)


def score_to_cos(score):
    """The inverse of cos_to_score: score = 1 - (1 - cos) / 2, so cos = 2 score - 1."""
    return np.float32(2.0) * np.asarray(score, np.float32) - np.float32(1.0)


def allow_mask(chunk_ids, next_id: int) -> np.ndarray:
    """The mask of a masked search (cs_index_search_masked): a bitmap over chunk ids [0, next_id), bit i = bit i & 31 of
    word i >> 5, set for every id in `chunk_ids`.  Ids outside [0, next_id) are dropped."""
    next_id = int(next_id)
    words = np.zeros((next_id + 31) // 32, np.uint32)
    ids = np.asarray(chunk_ids, np.int64).ravel()
    ids = ids[(ids >= 0) & (ids < next_id)]
    np.bitwise_or.at(words, ids >> 5, np.left_shift(np.uint32(1), (ids & 31).astype(np.uint32)))
    return words


def scope_ids(chunk_ids) -> np.ndarray:
    """The id list of a scope (cs_index_scope_create): `chunk_ids` sorted, de-duplicated, negatives and ids above u32
    dropped -> strictly ascending u32."""
    ids = np.asarray(chunk_ids, np.int64).ravel()
    ids = ids[(ids >= 0) & (ids <= 0xFFFFFFFF)]
    return np.ascontiguousarray(np.unique(ids), np.uint32)


NO_GROUP = 0xFFFFFFFF  # CS_NO_GROUP: an id that carries no group is never capped
NO_CLASS = 0xFFFF  # CS_NO_CLASS: an id that carries no class weighs 1 in a boosted search
# The reference's ChunkKind (src/chunker/mod.rs:140-159) by its Debug names, in the enum's order: the class a chunk inserted
# with metadata carries is its kind's position here.
CHUNK_KINDS = ["Function", "Class", "Method", "Struct", "Enum", "Trait", "Interface", "Impl", "Mod", "TypeAlias", "Const",
               "Static", "Block", "Anchor", "Comment", "Imports", "ModuleDocs", "Other"]


def _one_of(chunk_ids, scope, per_file=None):
    if per_file is not None and (chunk_ids is not None or scope is not None):
        raise ValueError("per_file= is exclusive with chunk_ids= and scope=: the grouped search runs over the whole store")
    if chunk_ids is not None and scope is not None:
        raise ValueError("chunk_ids= and scope= are exclusive: a scope already is a set of chunk ids")


def _filters_ok(chunk_ids, scope, per_file, class_weights=None, variants=False):
    """The argument check of the searches: per_file= may come with scope= (the grouped scoped search), and so may
    class_weights= (the boosted scoped search); every other pair is refused — class_weights= with chunk_ids= (no masked
    boosted form) or with per_file= (independent queries have no boosted form under the per-file cap; `variants`, the
    variants searches, have: cs_index_search_variants_boosted_grouped), and _one_of's: per_file= with chunk_ids= (no
    masked grouped form), chunk_ids= with scope=."""
    if class_weights is not None and chunk_ids is not None:
        raise ValueError("class_weights= is exclusive with chunk_ids=: the boosted search has no masked form (use scope=)")
    if class_weights is not None and per_file is not None and not variants:
        raise ValueError("class_weights= is exclusive with per_file=: the boosted search has no form under the per-file cap")
    _one_of(chunk_ids, None if (per_file is not None and chunk_ids is None) else scope, per_file)


class Scope:
    """A prepared set of chunk ids of one VectorStore (cs_scope): ids and the row list made from them live on the device,
    and a search with `scope=` returns what the same search with `chunk_ids=` of those ids returns, without building,
    copying or compacting a mask.  The row list follows the store: the first search after a build remakes it.
    Made by VectorStore.scope(); a context manager; keeps its store alive.

    Scopes of one store combine on the device (cs_scope_combine): `a | b`, `a & b`, `a - b` (union, intersection,
    difference) each give a new Scope that answers exactly as VectorStore.scope() of the host-computed id set would;
    VectorStore.scope_range() / scope_all() make a range of ids without a host list, so "everything but X" is
    `store.scope_all() - x`.  The ids of such a scope never pass through the host unless `.ids` is asked for."""

    OPS = {"union": 0, "intersection": 1, "difference": 2}  # CS_SCOPE_OP_*

    def __init__(self, store: "VectorStore", chunk_ids=None, _handle=None):
        self._h = None
        self.store = store  # (a scope must be destroyed before its store)
        if _handle is not None:  # made on the device (combine, scope_range): `ids` is read back when asked for
            self._h = _handle
            return
        self.ids = scope_ids(chunk_ids)
        h = C.c_void_p()
        _lib.check(store._fn("scope_create")(store._h, self.ids.ctypes.data_as(u32p) if self.ids.size else None,
                                             self.ids.size, C.byref(h)))
        self._h = h

    _ids = None  # the id set on the host: a host-made scope's from the start, a device-made one's once asked for
    _n = None    # a device-made scope's length (cs_scope_info), asked once

    @property
    def ids(self) -> np.ndarray:
        """The scope's id set, ascending u32.  A device-made scope reads it back at the first use (cs_scope_read_ids) and
        keeps it — the set never changes.  Ids read before close() stay readable after it; ids never read then raise
        "scope is closed".  Two threads that both ask first both read back, the same bytes; one array is kept."""
        if self._ids is None:
            if not self._h:
                raise CsError(_lib.CS_ERR_BAD_ARG, "scope is closed")
            ids = np.empty(len(self), np.uint32)
            _lib.check(self.store._lib.cs_scope_read_ids(self._h, 0, ids.size, ids.ctypes.data_as(u32p) if ids.size else None))
            self._ids = ids
        return self._ids

    @ids.setter
    def ids(self, value) -> None:
        self._ids = value

    def __len__(self) -> int:
        if self._ids is not None:
            return int(self._ids.size)
        if self._n is None:
            self._n = self.info()[0]
        return self._n

    def _combine(self, other: "Scope", op: str) -> "Scope":
        if not isinstance(other, Scope):
            raise TypeError(f"a Scope combines with a Scope, not {type(other).__name__}")
        if not self._h or not other._h:
            raise CsError(_lib.CS_ERR_BAD_ARG, "scope is closed")
        h = C.c_void_p()  # (a scope of another store is the library's to refuse)
        _lib.check(self.store._lib.cs_scope_combine(self._h, other._h, self.OPS[op], C.byref(h)))
        sc = Scope(self.store, _handle=h)
        self.store._scopes.add(sc)
        return sc

    def union(self, other: "Scope") -> "Scope":
        """A new Scope of this store holding the ids of either (cs_scope_combine, on the device)."""
        return self._combine(other, "union")

    def intersection(self, other: "Scope") -> "Scope":
        """A new Scope holding the ids of both."""
        return self._combine(other, "intersection")

    def difference(self, other: "Scope") -> "Scope":
        """A new Scope holding the ids of this scope that `other` does not hold."""
        return self._combine(other, "difference")

    def __or__(self, other):
        return self.union(other) if isinstance(other, Scope) else NotImplemented

    def __and__(self, other):
        return self.intersection(other) if isinstance(other, Scope) else NotImplemented

    def __sub__(self, other):
        return self.difference(other) if isinstance(other, Scope) else NotImplemented

    def __bool__(self) -> bool:
        return True  # an empty scope is still a scope: `if scope:` must not turn its search into an unscoped one

    def info(self):
        """-> (n_ids, live_rows, refreshes): ids held, rows of the list as last made, makings of the list."""
        if not self._h:
            raise CsError(_lib.CS_ERR_BAD_ARG, "scope is closed")
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _lib.check(self.store._lib.cs_scope_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    ROUTES = {"auto": 0, "gather": 1, "filter": 2}  # CS_SCOPE_ROUTE_*

    def set_route(self, route):
        """The route of this scope's host-buffer searches — search_raw(scope=), the variants form and similar_raw(scope=)
        (cs_scope_set_route): "auto" (default), "gather" (always the gathered f32 scan) or "filter" (the int8 filter + exact
        refine wherever it can serve), or the CS_SCOPE_ROUTE_* value.  The answers' bytes do not depend on it.  Grouped scoped
        searches always gather."""
        if not self._h:
            raise CsError(_lib.CS_ERR_BAD_ARG, "scope is closed")
        _lib.check(self.store._lib.cs_scope_set_route(self._h, self.ROUTES.get(route, route)))

    def route_info(self):
        """-> (filter_searches, gathered_searches, overflow_reruns, extra_bytes): host-buffer searches, similar-chunk
        searches included, answered through the filter / by the gathered scan, exact reruns after an overflowed candidate
        buffer (counted in filter_searches too), and the bytes of HBM held beyond 8 per id (cs_scope_route_info)."""
        if not self._h:
            raise CsError(_lib.CS_ERR_BAD_ARG, "scope is closed")
        v = [C.c_uint64() for _ in range(4)]
        _lib.check(self.store._lib.cs_scope_route_info(self._h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            # VectorStore.close() closes its open scopes first, so the store is still there; a scope that the collector
            # had already dropped from that set gets here after it, and cs_scope_destroy frees only what the scope owns
            # (its buffers and its stream) without touching the index, so nothing is leaked either way
            self.store._lib.cs_scope_destroy(self._h)
            self._h = None
            self.store._scopes.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- the store ---------------------------------------------------------------------------------

class VectorStore:
    """`VectorStore::new(db_path, dimensions)` — store.rs:110-176.

    `db_path = None`: a purely HBM-resident store.  With a path the store is persistent the way the
    reference's is across process restarts (it reopens its LMDB environment, `next_id = last_key + 1`,
    `indexed` = a built index exists, store.rs:139-170), in a flat form the GPU can ingest at full
    PCIe rate, written at `build_index()` next to where the reference keeps its
    `data.mdb`:
        <db_path>/vectors.f32         rows [next_id - id_base, dim] f32 little-endian, row = id - id_base
        <db_path>/vectors.meta.json   {"format", "dimensions", "id_base", "next_id", "removed": [ids], "built"}
        <db_path>/chunks.jsonl        one ChunkMetadata per line (the `chunks` database, store.rs:98)
    Rows appended after the last `build_index()` are in HBM only (the reference commits each insert
    to LMDB but cannot search it before the next build either).
    `device`, `capacity` and `id_base` are the GPU-side additions (shard placement).
    """

    FORMAT = 1

    def __init__(self, db_path, dimensions: int, device: int = 0, capacity: int = 0, id_base: int = 0,
                 devices: Optional[Sequence[int]] = None, rows_per_stripe: int = 65536, grouped: bool = False):
        """devices=[d0, d1, ...]: the store is row-sharded over those GPUs inside this one process
        (cs_shards_*: ids stay contiguous, rows dealt in stripes of `rows_per_stripe`; a search broadcasts
        the queries, scans every shard and merges on d0).  Otherwise one cs_index on `device`.
        grouped=True (a sharded store only; one index always is): the store keeps groups — set_groups, groups_info, a
        chunk's file as its group, and per_file= on the searches, alone and with scope= (cs_shards_set_groups,
        cs_shards_search_grouped & co.: 8 B per id, a table on the first device and one on every shard).  A sharded store
        opened without it refuses those calls, as it always has."""
        self._lib = _lib.load()
        self._grouped = bool(grouped) or devices is None
        self.db_path = None if db_path is None else str(db_path)
        self.dimensions = int(dimensions)
        self.id_base = int(id_base)
        self.readonly = False
        if self.db_path is not None:  # reopening: reserve the persisted row count at once instead of growing by doubling
            try:
                with open(os.path.join(self.db_path, "vectors.meta.json")) as f:
                    capacity = max(int(capacity), int(json.load(f)["next_id"]) - self.id_base)
            except (OSError, ValueError, KeyError):
                pass
        handle = C.c_void_p()
        if devices is not None:
            if id_base:
                raise CsError(_lib.CS_ERR_BAD_ARG, "a sharded store hands out ids from 0")
            devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            _lib.check(self._lib.cs_shards_create(self.dimensions, len(devices), devs, int(rows_per_stripe), capacity,
                                                  C.byref(handle)))
            self._pfx = "cs_shards_"
        else:
            _lib.check(self._lib.cs_index_create(self.dimensions, capacity, device, id_base, C.byref(handle)))
            self._pfx = "cs_index_"
        self._h = handle
        self._scopes = weakref.WeakSet()  # open scopes: closed with the store, before it
        self._meta: Dict[int, ChunkMetadata] = {}
        self._file_groups: Dict[str, int] = {}  # path -> group of the grouped search (per_file=), in order of first sight
        self._removed: set = set()
        self._persisted_rows = 0
        self._persisted_meta_ids: set = set()   # ids whose line is already in chunks.jsonl
        self._chunks_rewrite = False            # a persisted line was deleted: rewrite the file instead of appending
        if self.db_path is not None:
            os.makedirs(self.db_path, exist_ok=True)  # store.rs:113
            self._load()

    @classmethod
    def open_readonly(cls, db_path, dimensions: int, **kw) -> "VectorStore":
        """store.rs:183-250: same data, mutators refuse."""
        st = cls(db_path, dimensions, **kw)
        st.readonly = True
        return st

    # -- persistence
    def _paths(self):
        j = os.path.join
        return j(self.db_path, "vectors.f32"), j(self.db_path, "vectors.meta.json"), j(self.db_path, "chunks.jsonl")

    def _load(self) -> None:
        vec, meta, chunks = self._paths()
        if not (os.path.exists(vec) and os.path.exists(meta)):
            return
        m = json.load(open(meta))
        if m.get("format") != self.FORMAT:
            raise CsError(_lib.CS_ERR_BAD_ARG, f"unknown vector file format {m.get('format')!r} in {meta}")
        if int(m["dimensions"]) != self.dimensions:  # the reference would fail at the first insert/search
            raise CsError(_lib.CS_ERR_DIM_MISMATCH,
                          f"Embedding dimension mismatch: expected {self.dimensions}, got {m['dimensions']}")
        if int(m["id_base"]) != self.id_base:
            raise CsError(_lib.CS_ERR_BAD_ARG, f"store was written with id_base {m['id_base']}, opened with {self.id_base}")
        n = int(m["next_id"]) - self.id_base
        rows = np.memmap(vec, dtype="<f4", mode="r", shape=(n, self.dimensions)) if n else np.zeros((0, self.dimensions), np.float32)
        step = max(1, (256 << 20) // (4 * self.dimensions))  # 256 MB host pieces
        for lo in range(0, n, step):
            piece = np.ascontiguousarray(rows[lo:lo + step], np.float32)
            _lib.check(self._fn("add")(self._h, piece.ctypes.data_as(f32p), piece.shape[0], self.dimensions, None))
        self._persisted_rows = n
        removed = [int(i) for i in m.get("removed", [])]
        if removed:
            ids = np.ascontiguousarray(removed, np.uint32)
            _lib.check(self._fn("remove")(self._h, ids.ctypes.data_as(u32p), ids.size, None))
            self._removed = set(removed)
        if os.path.exists(chunks):
            for line in open(chunks):
                try:
                    d = json.loads(line)
                except ValueError:
                    self._chunks_rewrite = True  # a torn last line of an interrupted append
                    continue
                cid = int(d.pop("id"))
                if cid >= int(m["next_id"]):  # appended after the last commit point
                    self._chunks_rewrite = True
                    continue
                self._meta[cid] = ChunkMetadata(**d)
            self._persisted_meta_ids = set(self._meta)
            if self._grouped:  # the groups are not stored: they follow from the sidecar's paths
                self._assign_file_groups([i for i in sorted(self._meta) if i >= self.id_base])  # (< next_id: above)
            if not self.sharded:
                self._assign_kind_classes([i for i in sorted(self._meta) if i >= self.id_base])  # (nor are the classes)
        for cid in self._removed:  # deletes committed after the last build (delete_chunks) win over older lines
            if self._meta.pop(cid, None) is not None:
                self._chunks_rewrite = True
        if m.get("built"):
            _lib.check(self._fn("build")(self._h))

    def _persist(self) -> None:
        vec, meta, chunks = self._paths()
        n = self.next_id() - self.id_base
        with open(vec, "r+b" if os.path.exists(vec) else "w+b") as f:
            f.truncate(self._persisted_rows * self.dimensions * 4)  # drop anything past the last consistent state
            f.seek(0, 2)
            step = max(1, (256 << 20) // (4 * self.dimensions))
            for lo in range(self._persisted_rows, n, step):
                f.write(self._read_rows_for_file(lo, min(step, n - lo)).astype("<f4").tobytes())
        self._write_chunks(chunks)
        self._write_meta(meta, built=True)  # the meta file is the commit point
        self._persisted_rows = n

    def _read_rows_for_file(self, lo: int, cnt: int) -> np.ndarray:
        """Rows of ids [id_base + lo, + cnt) for the flat vector file, which stays indexed by id: a deleted id's row may
        have been reclaimed by the build (cs_index_build) — its slot in the file is zeros, and the meta file's removed
        list keeps it dead on reopening."""
        gone = sorted(i - self.id_base - lo for i in self._removed if lo <= i - self.id_base < lo + cnt)
        if not gone:
            return self.read_rows(lo, cnt)
        out = np.zeros((cnt, self.dimensions), np.float32)
        start = 0
        for g in gone + [cnt]:
            if g > start:
                out[start:g] = self.read_rows(lo + start, g - start)
            start = g + 1
        return out

    def _write_chunks(self, chunks: str) -> None:
        """chunks.jsonl: appended to when only new chunks arrived (the reference builds per file: rewriting N lines per
        build would be O(N) per file), rewritten atomically when a persisted line was deleted."""
        def line(cid):
            d = dataclasses.asdict(self._meta[cid])
            d["id"] = cid
            return json.dumps(d) + "\n"

        if self._chunks_rewrite or not os.path.exists(chunks):
            with open(chunks + ".tmp", "w") as f:
                for cid in sorted(self._meta):
                    f.write(line(cid))
            os.replace(chunks + ".tmp", chunks)
        else:
            new = sorted(set(self._meta) - self._persisted_meta_ids)
            if new:
                with open(chunks, "a") as f:
                    for cid in new:
                        f.write(line(cid))
        self._persisted_meta_ids = set(self._meta)
        self._chunks_rewrite = False

    def _write_meta(self, meta: str, built: bool) -> None:
        with open(meta + ".tmp", "w") as f:
            json.dump({"format": self.FORMAT, "dimensions": self.dimensions, "id_base": self.id_base,
                       "next_id": self.id_base + self._persisted_rows if not built else self.next_id(),
                       "removed": sorted(self._removed), "built": built}, f)
        os.replace(meta + ".tmp", meta)

    def db_size(self) -> int:
        """store.rs:741-749: bytes on disk."""
        if self.db_path is None:
            return 0
        return sum(os.path.getsize(p) for p in self._paths() if os.path.exists(p))

    def _fn(self, name: str):
        """cs_index_<name> or, for a store sharded over several GPUs, cs_shards_<name> (same signature)."""
        return getattr(self._lib, self._pfx + name)

    @property
    def sharded(self) -> bool:
        return self._pfx == "cs_shards_"

    def shard_lens(self) -> List[int]:
        """Live rows per shard (sharded stores only)."""
        if not self.sharded:
            return [len(self)]
        return [int(self._lib.cs_shards_shard_len(self._h, i)) for i in range(int(self._lib.cs_shards_count(self._h)))]

    def root_device(self) -> int:
        """The device whose HBM holds queries and results of the device-pointer search API."""
        return int(self._lib.cs_shards_root_device(self._h)) if self.sharded else int(self._lib.cs_index_device(self._h))

    def shard_handle(self, shard: int):
        """Borrowed cs_index of one shard (diagnostics: profile, counters)."""
        return C.c_void_p(self._lib.cs_shards_shard_index(self._h, shard)) if self.sharded else self._h

    def search_device(self, d_queries: int, nq: int, limit: int, d_keys: int = 0, d_cos: int = 0, d_ids: int = 0,
                      d_counts: int = 0, stream: int = 0) -> None:
        """cs_index_search_device / cs_shards_search_device: raw HBM pointers on root_device(), asynchronous on
        `stream`; never waits for the device."""
        p = lambda a: C.c_void_p(a) if a else None
        _lib.check(self._fn("search_device")(self._h, p(d_queries), nq, self.dimensions, limit, p(d_keys), p(d_cos),
                                             p(d_ids), p(d_counts), p(stream)))

    def search_status(self, stream: int = 0) -> bool:
        """True when a device search of more than 16 queries issued on `stream` overflowed a candidate buffer since
        the last call (rerun it in slices of <= 16 queries or through search_raw)."""
        ov = C.c_uint32(0)
        _lib.check(self._fn("search_status")(self._h, C.c_void_p(stream) if stream else None, C.byref(ov)))
        return bool(ov.value)

    def insert_device(self, d_rows: int, n: int, src_device: Optional[int] = None, stream: int = 0) -> np.ndarray:
        """Append n rows already in HBM (cs_index_add_device / cs_shards_add_device) -> ids."""
        self._writable()
        ids = np.zeros(n, np.uint32)
        st = C.c_void_p(stream) if stream else None
        if self.sharded:
            src = self.root_device() if src_device is None else int(src_device)
            _lib.check(self._lib.cs_shards_add_device(self._h, C.c_void_p(d_rows), src, n, self.dimensions,
                                                      ids.ctypes.data_as(u32p), st))
        else:
            _lib.check(self._lib.cs_index_add_device(self._h, C.c_void_p(d_rows), n, self.dimensions,
                                                     ids.ctypes.data_as(u32p), st))
        return ids

    def _writable(self):
        if self.readonly:
            raise CsError(_lib.CS_ERR_BAD_ARG, "store opened read-only (open_readonly)")

    # -- lifecycle
    def close(self):
        if getattr(self, "_h", None):
            for sc in list(getattr(self, "_scopes", ())):  # a scope is destroyed before its store
                sc.close()
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- writes (`&mut self` in the reference)
    def insert_chunks_with_ids(self, chunks: Sequence[EmbeddedChunk]) -> List[int]:
        """store.rs:618-686 -> assigned ids (contiguous from next_id)."""
        self._writable()
        if not chunks:
            return []
        for ch in chunks:  # store.rs:666-672: first bad row aborts the transaction
            if len(ch.embedding) != self.dimensions:
                raise CsError(_lib.CS_ERR_DIM_MISMATCH,
                              f"Embedding dimension mismatch: expected {self.dimensions}, got {len(ch.embedding)}")
        rows = np.ascontiguousarray([ch.embedding for ch in chunks], dtype=np.float32)
        ids = np.zeros(len(chunks), np.uint32)
        _lib.check(self._fn("add")(self._h, rows.ctypes.data_as(f32p), len(chunks), self.dimensions,
                                          ids.ctypes.data_as(u32p)))
        for i, ch in zip(ids.tolist(), chunks):
            self._meta[i] = ChunkMetadata.from_embedded_chunk(ch)
        if self._grouped:
            self._assign_file_groups(ids.tolist())
        if not self.sharded:
            self._assign_kind_classes(ids.tolist())
        return ids.tolist()

    def insert_chunks(self, chunks: Sequence[EmbeddedChunk]) -> int:
        """store.rs:334-379 -> number inserted."""
        return len(self.insert_chunks_with_ids(chunks))

    def insert_embeddings(self, rows: np.ndarray) -> np.ndarray:
        """Vector-only append (no metadata) for bulk/bench use -> ids."""
        self._writable()
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2:
            raise ValueError("rows must be [n, dim]")
        ids = np.zeros(rows.shape[0], np.uint32)
        _lib.check(self._fn("add")(self._h, rows.ctypes.data_as(f32p), rows.shape[0], rows.shape[1],
                                          ids.ctypes.data_as(u32p)))
        return ids

    def reserve_rows(self, n: int) -> int:
        """Room for n more rows -> the device address they are to be written at (cs_index_reserve_rows: E8 in place — an
        embedder's *_to_device call with this address stores its pooled rows straight into the corpus).  commit_rows(n)
        then makes them rows with the next n ids.  One cs_index only (a sharded store plans placement: cs_shards_plan_append)."""
        self._writable()
        if self.sharded:
            raise CsError(_lib.CS_ERR_UNSUPPORTED, "reserve_rows: a sharded store appends through cs_shards_add_device")
        p = C.c_void_p()
        _lib.check(self._lib.cs_index_reserve_rows(self._h, int(n), self.dimensions, C.byref(p)))
        return int(p.value or 0)

    def commit_rows(self, n: int) -> np.ndarray:
        ids = np.zeros(int(n), np.uint32)
        _lib.check(self._lib.cs_index_commit_rows(self._h, int(n), ids.ctypes.data_as(u32p)))
        return ids

    def insert_synthetic(self, n: int, seed: int, first_row: int = 0) -> int:
        """Generate n rows in HBM with include/cs_synth.h -> first id."""
        first = C.c_uint32()
        _lib.check(self._fn("add_synthetic")(self._h, n, seed, first_row, C.byref(first)))
        return int(first.value)

    def delete_chunks(self, chunk_ids: Sequence[int]) -> int:
        """store.rs:548-610 -> number deleted."""
        self._writable()
        ids = np.ascontiguousarray(chunk_ids, np.uint32)
        removed = C.c_uint64()
        _lib.check(self._fn("remove")(self._h, ids.ctypes.data_as(u32p), ids.size, C.byref(removed)))
        nxt = self.next_id()
        for i in ids.tolist():
            if self._meta.pop(i, None) is not None and i in self._persisted_meta_ids:  # store.rs:598
                self._chunks_rewrite = True
            if self.id_base <= i < nxt:
                self._removed.add(i)
        # The reference commits a delete to LMDB at once (store.rs:584-610).  Here the removed list of the persisted
        # state is committed at once too (atomic rewrite of the small meta file): a process that dies before the next
        # build_index() reopens without the deleted chunks.  Rows appended since the last build stay HBM-only until
        # that build, as arroy's tree does.
        if self.db_path is not None and os.path.exists(self._paths()[1]):
            m = json.load(open(self._paths()[1]))
            keep = int(m["next_id"])
            with open(self._paths()[1] + ".tmp", "w") as f:
                m["removed"] = sorted(i for i in self._removed if i < keep)
                json.dump(m, f)
            os.replace(self._paths()[1] + ".tmp", self._paths()[1])
        return int(removed.value)

    def build_index(self) -> None:
        """store.rs:386-430 (+ the flat vector file when the store has a path)."""
        self._writable()
        _lib.check(self._fn("build")(self._h))
        if self.db_path is not None:
            self._persist()

    def clear(self) -> None:
        """store.rs:690-707."""
        self._writable()
        _lib.check(self._fn("clear")(self._h))
        self._meta.clear()
        self._file_groups.clear()  # (cs_index_clear drops the groups of the ids)
        self._removed.clear()
        self._persisted_rows = 0
        if self.db_path is not None:
            for p in self._paths():
                if os.path.exists(p):
                    os.remove(p)

    # -- reads (`&self`)
    def is_indexed(self) -> bool:
        return bool(self._fn("is_built")(self._h))

    def next_id(self) -> int:
        return int(self._fn("next_id")(self._h))

    def __len__(self) -> int:
        return int(self._fn("len")(self._h))

    def stored_rows(self) -> int:
        """Rows the corpus matrix physically holds, tombstoned ones included: len(self) right after a build that reclaimed
        the deleted rows (cs_index_build, from 10 % dead rows on), more in between."""
        return int(self._fn("stored_rows")(self._h))

    def set_groups(self, ids, groups) -> None:
        """cs_index_set_groups: groups[i] becomes the group of chunk id ids[i] (NO_GROUP un-assigns it); takes effect at
        the next search(per_file=...), no rebuild.  An id never issued is an error; a deleted one is accepted.
        Group numbers are one space: chunks inserted with metadata are given their file's number, counted up from 0 in
        order of first sight (insert_chunks_with_ids), so a caller who groups other rows by hand and does not mean to
        join them to a file numbers them from the top down (below NO_GROUP)."""
        self._writable()
        self._needs_groups()
        ids = np.ascontiguousarray(ids, np.uint32).ravel()
        groups = np.ascontiguousarray(groups, np.uint32).ravel()
        if ids.size != groups.size:
            raise ValueError("ids and groups must have one entry per id")
        _lib.check(self._fn("set_groups")(self._h, ids.ctypes.data_as(u32p), groups.ctypes.data_as(u32p), ids.size))

    def _needs_groups(self) -> None:
        """The grouped calls of a sharded store are its opt-in: VectorStore(..., devices=[...], grouped=True)."""
        if not self._grouped:
            raise CsError(_lib.CS_ERR_UNSUPPORTED, "a sharded store has no grouped search (per_file) unless it is opened with "
                          "grouped=True (cs_shards_set_groups, cs_shards_search_grouped & co.)")

    def groups_info(self):
        """-> (ids that carry a group, bytes of HBM the group tables hold) (cs_index_groups_info; a sharded store opened with
        grouped=True: cs_shards_groups_info, the root's table by global id and every shard's by local id)."""
        self._needs_groups()
        a, b = C.c_uint64(), C.c_uint64()
        _lib.check(self._fn("groups_info")(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def _assign_file_groups(self, ids) -> None:
        """The chunks' files as groups: one group per distinct path, numbered in order of first sight."""
        if not len(ids):
            return
        groups = [self._file_groups.setdefault(self._meta[i].path, len(self._file_groups)) for i in ids]
        ids = np.ascontiguousarray(ids, np.uint32)
        groups = np.ascontiguousarray(groups, np.uint32)
        _lib.check(self._fn("set_groups")(self._h, ids.ctypes.data_as(u32p), groups.ctypes.data_as(u32p), ids.size))

    def set_classes(self, ids, classes) -> None:
        """cs_index_set_classes: classes[i] (16 bits) becomes the class of chunk id ids[i] (NO_CLASS un-assigns it); takes
        effect at the next search(class_weights=...), no rebuild.  An id never issued is an error and nothing is assigned;
        a deleted one is accepted.  Chunks inserted with metadata carry CHUNK_KINDS.index(kind) (insert_chunks_with_ids);
        a caller who boosts by something else re-assigns them, e.g. class = language * len(CHUNK_KINDS) + kind."""
        self._writable()
        if self.sharded:
            raise CsError(_lib.CS_ERR_UNSUPPORTED, "a sharded store has no boosted search (class_weights): no cs_shards_ form yet")
        ids = np.ascontiguousarray(ids, np.uint32).ravel()
        classes = np.ascontiguousarray(classes, np.uint16).ravel()
        if ids.size != classes.size:
            raise ValueError("ids and classes must have one entry per id")
        _lib.check(self._lib.cs_index_set_classes(self._h, ids.ctypes.data_as(u32p), classes.ctypes.data_as(_lib.u16p), ids.size))

    def classes_info(self):
        """-> (ids that carry a class, bytes of HBM the class table holds) (cs_index_classes_info)."""
        if self.sharded:
            raise CsError(_lib.CS_ERR_UNSUPPORTED, "a sharded store has no boosted search (class_weights): no cs_shards_ form yet")
        a, b = C.c_uint64(), C.c_uint64()
        _lib.check(self._lib.cs_index_classes_info(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def _assign_kind_classes(self, ids) -> None:
        """The chunks' kinds as classes: the kind's position in CHUNK_KINDS, NO_CLASS for a kind that is not there."""
        if not len(ids):
            return
        classes = [CHUNK_KINDS.index(self._meta[i].kind) if self._meta[i].kind in CHUNK_KINDS else NO_CLASS for i in ids]
        ids = np.ascontiguousarray(ids, np.uint32)
        classes = np.ascontiguousarray(classes, np.uint16)
        _lib.check(self._lib.cs_index_set_classes(self._h, ids.ctypes.data_as(u32p), classes.ctypes.data_as(_lib.u16p), ids.size))

    def _mask_args(self, chunk_ids):
        """(allow pointer, allow_bits, keep-alive) of a masked search over `chunk_ids`."""
        nxt = self.next_id()
        mask = allow_mask(chunk_ids, nxt)
        return (mask.ctypes.data_as(u32p) if mask.size else None), (nxt if mask.size else 0), mask

    def scope(self, chunk_ids) -> Scope:
        """A Scope over `chunk_ids` (sorted and de-duplicated here, negatives dropped): prepare once, then pass it as
        `scope=` to the searches below instead of `chunk_ids=`.  Works over a sharded store too."""
        sc = Scope(self, chunk_ids)
        self._scopes.add(sc)
        return sc

    def scope_range(self, first_id: int, n: int) -> Scope:
        """A Scope of the ids [first_id, first_id + n), written on the device (cs_index_scope_create_range /
        cs_shards_scope_create_range): no host list, no upload.  A snapshot of the ids named, like any scope."""
        if first_id < 0 or first_id > 0xFFFFFFFF or n < 0:
            raise ValueError(f"scope_range: first_id must be a u32 and n >= 0, got {first_id}, {n}")
        h = C.c_void_p()
        _lib.check(self._fn("scope_create_range")(self._h, int(first_id), int(n), C.byref(h)))
        sc = Scope(self, _handle=h)
        self._scopes.add(sc)
        return sc

    def scope_all(self) -> Scope:
        """scope_range over every id issued so far, [id_base, next_id): `store.scope_all() - x` is "everything but x"."""
        return self.scope_range(self.id_base, self.next_id() - self.id_base)

    def _scope_handle(self, scope: Scope):
        if not scope._h:  # (a scope of another store is the library's to refuse)
            raise CsError(_lib.CS_ERR_BAD_ARG, "scope is closed")
        return scope._h

    def search_raw(self, queries, limit: int, chunk_ids=None, scope: Optional[Scope] = None, per_file: Optional[int] = None,
                   class_weights=None):
        """-> (cos [nq, limit] f32, ids [nq, limit] u32, counts [nq] u32); rows best-first.
        class_weights: -> (score, cos, ids, counts) instead — the boosted search (cs_index_search_boosted): one f32 weight
        per class (set_classes; at most 4096, each finite and in [0, 65536]; a row without a class, or with a class past the
        table, weighs 1), the exact top `limit` by b = f32(cos_to_score(cos) * weight), then id; score = b, cos = the row's
        cosine.  May come with scope= (cs_index_search_boosted_scoped); exclusive with chunk_ids= and per_file= (the capped
        boosted search of one query is search_variants_raw(class_weights=, per_file=) with one variant).
        A language boost is the caller's through set_classes, e.g. class = language * len(CHUNK_KINDS) + kind and a table
        of 1.2 for the language's classes, 1.15 for the kind's and f32(1.2 * 1.15) where both hold — which is one rounding
        of the product and so not bit-equal to the reference's two successive multiplies (f32(f32(s * 1.15) * 1.2)).
        chunk_ids: only these chunks are searched (cs_index_search_masked: the exact top `limit` among them).
        scope: the same through a prepared Scope (cs_index_search_scoped); exclusive with chunk_ids.
        per_file: at most this many rows of one group (a chunk's file; set_groups for rows without metadata) among the
        `limit` best, decided on the device (cs_index_search_grouped); with scope=, among the scope's rows
        (cs_index_search_grouped_scoped); exclusive with chunk_ids."""
        _filters_ok(chunk_ids, scope, per_file, class_weights)
        q = np.ascontiguousarray(queries, np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq, dim = q.shape
        cos = np.zeros((nq, max(limit, 1)), np.float32)
        ids = np.zeros((nq, max(limit, 1)), np.uint32)
        counts = np.zeros(nq, np.uint32)
        if class_weights is not None:
            if self.sharded:
                raise CsError(_lib.CS_ERR_UNSUPPORTED, "a sharded store has no boosted search (class_weights): no cs_shards_ form yet")
            w = np.ascontiguousarray(class_weights, np.float32).ravel()
            score = np.zeros_like(cos)
            tail = (w.ctypes.data_as(f32p) if w.size else None, w.size, score.ctypes.data_as(f32p), cos.ctypes.data_as(f32p),
                    ids.ctypes.data_as(u32p), counts.ctypes.data_as(u32p))
            if scope is not None:
                _lib.check(self._lib.cs_index_search_boosted_scoped(self._h, self._scope_handle(scope), q.ctypes.data_as(f32p),
                                                                    nq, dim, limit, *tail))
            else:
                _lib.check(self._lib.cs_index_search_boosted(self._h, q.ctypes.data_as(f32p), nq, dim, limit, *tail))
            return score, cos, ids, counts
        if per_file is not None:
            self._needs_groups()
            if scope is not None:
                _lib.check(self._fn("search_grouped_scoped")(self._h, self._scope_handle(scope), q.ctypes.data_as(f32p),
                                                                    nq, dim, limit, int(per_file), cos.ctypes.data_as(f32p),
                                                                    ids.ctypes.data_as(u32p), counts.ctypes.data_as(u32p)))
            else:
                _lib.check(self._fn("search_grouped")(self._h, q.ctypes.data_as(f32p), nq, dim, limit, int(per_file),
                                                             cos.ctypes.data_as(f32p), ids.ctypes.data_as(u32p),
                                                             counts.ctypes.data_as(u32p)))
        elif scope is not None:
            _lib.check(self._fn("search_scoped")(self._h, self._scope_handle(scope), q.ctypes.data_as(f32p), nq, dim, limit,
                                                 cos.ctypes.data_as(f32p), ids.ctypes.data_as(u32p),
                                                 counts.ctypes.data_as(u32p)))
        elif chunk_ids is None:
            _lib.check(self._fn("search")(self._h, q.ctypes.data_as(f32p), nq, dim, limit,
                                                 cos.ctypes.data_as(f32p), ids.ctypes.data_as(u32p),
                                                 counts.ctypes.data_as(u32p)))
        else:
            allow, bits, _keep = self._mask_args(chunk_ids)
            _lib.check(self._fn("search_masked")(self._h, q.ctypes.data_as(f32p), nq, dim, limit, allow, bits,
                                                 cos.ctypes.data_as(f32p), ids.ctypes.data_as(u32p),
                                                 counts.ctypes.data_as(u32p)))
        return cos, ids, counts

    def search(self, query_embedding, limit: int, chunk_ids=None, scope: Optional[Scope] = None,
               per_file: Optional[int] = None, boost_kind: Optional[str] = None, boost: float = 0.15) -> List[SearchResult]:
        """store.rs:431-486.  Results whose metadata is missing are skipped (store.rs:465).  chunk_ids / scope / per_file:
        search_raw.
        boost_kind (a CHUNK_KINDS name, e.g. "Struct"): the reference's structural-intent boost (src/search/mod.rs:238-252)
        inside the selection — every chunk of that kind weighs 1 + boost, the others 1 (search_raw class_weights=, with its
        exclusions); `score` is then the boosted score and `distance` still the chunk's own."""
        if boost_kind is not None:
            if boost_kind not in CHUNK_KINDS:
                raise ValueError(f"boost_kind must be one of CHUNK_KINDS, got {boost_kind!r}")
            w = np.ones(len(CHUNK_KINDS), np.float32)
            w[CHUNK_KINDS.index(boost_kind)] = np.float32(1.0) + np.float32(boost)
            score, cos, ids, counts = self.search_raw(query_embedding, limit, chunk_ids=chunk_ids, scope=scope, per_file=per_file,
                                                      class_weights=w)
            return self._results(cos[0], ids[0], int(counts[0]), score=score[0])
        cos, ids, counts = self.search_raw(query_embedding, limit, chunk_ids=chunk_ids, scope=scope, per_file=per_file)
        return self._results(cos[0], ids[0], int(counts[0]))

    def search_batch(self, query_embeddings, limit: int, chunk_ids=None, scope: Optional[Scope] = None,
                     per_file: Optional[int] = None) -> List[List[SearchResult]]:
        """One call for all query variants (the par_iter of src/search/mod.rs:508-511).  chunk_ids / scope / per_file:
        search_raw."""
        cos, ids, counts = self.search_raw(query_embeddings, limit, chunk_ids=chunk_ids, scope=scope, per_file=per_file)
        return [self._results(cos[i], ids[i], int(counts[i])) for i in range(len(counts))]

    def search_variants(self, query_embeddings, limit: int, chunk_ids=None, scope: Optional[Scope] = None,
                        per_file: Optional[int] = None, boost_kind: Optional[str] = None, boost: float = 0.15):
        """search::search's vector leg (src/search/mod.rs:508-611) in one call: every variant searched for `limit`
        rows, union with a chunk keeping its best score, best `limit` distinct chunks best-first, merged on
        the device.  -> (results, high_confidence) where high_confidence is the early-termination predicate
        (top five all distance < 0.15).  chunk_ids / scope: only these chunks are searched (search_raw).
        per_file: at most this many chunks of one file among the `limit` returned, the cap applied to the merged order
        on the device (cs_index_search_variants_grouped, with scope= cs_index_search_variants_grouped_scoped); the flag
        is then the predicate on the capped list.  Exclusive with chunk_ids.
        boost_kind / boost: as in search() — the weight is part of the selection and `score` is the boosted score; here it
        combines with scope= and per_file= (search_variants_raw class_weights=)."""
        if boost_kind is not None:
            if boost_kind not in CHUNK_KINDS:
                raise ValueError(f"boost_kind must be one of CHUNK_KINDS, got {boost_kind!r}")
            w = np.ones(len(CHUNK_KINDS), np.float32)
            w[CHUNK_KINDS.index(boost_kind)] = np.float32(1.0) + np.float32(boost)
            score, cos, ids, count, flag = self.search_variants_raw(query_embeddings, limit, chunk_ids=chunk_ids, scope=scope,
                                                                    per_file=per_file, class_weights=w)
            return self._results(cos, ids, count, score=score), flag
        cos, ids, count, flag = self.search_variants_raw(query_embeddings, limit, chunk_ids=chunk_ids, scope=scope,
                                                         per_file=per_file)
        return self._results(cos, ids, count), flag

    def search_variants_raw(self, query_embeddings, limit: int, chunk_ids=None, scope: Optional[Scope] = None,
                            per_file: Optional[int] = None, class_weights=None):
        """search_variants without the metadata join -> (cos [limit] f32, ids [limit] u32, count, high_confidence).
        class_weights (search_raw's table): -> (score, cos, ids, count, high_confidence) instead — the boosted search over
        the variants (cs_index_search_variants_boosted): a chunk's cos is its best cosine over the variants, score = b =
        f32(cos_to_score(cos) * weight), the exact top `limit` by (b, id); the flag is the predicate on the returned
        list's cosines.  Alone, with scope=, with per_file= (the capped walk over b, decided on the device) or with both;
        exclusive with chunk_ids=.  The capped boosted search of ONE query, which search_raw refuses, is this call with
        one variant."""
        _filters_ok(chunk_ids, scope, per_file, class_weights, variants=True)
        q = np.ascontiguousarray(query_embeddings, np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq, dim = q.shape
        cos = np.zeros(max(limit, 1), np.float32)
        ids = np.zeros(max(limit, 1), np.uint32)
        count, flag = C.c_uint32(), C.c_int32()
        if class_weights is not None:
            if self.sharded:
                raise CsError(_lib.CS_ERR_UNSUPPORTED, "a sharded store has no boosted search (class_weights): no cs_shards_ form yet")
            w = np.ascontiguousarray(class_weights, np.float32).ravel()
            score = np.zeros_like(cos)
            head = (self._h,) + ((self._scope_handle(scope),) if scope is not None else ()) + (q.ctypes.data_as(f32p), nq, dim, limit)
            tail = (w.ctypes.data_as(f32p) if w.size else None, w.size, score.ctypes.data_as(f32p), cos.ctypes.data_as(f32p),
                    ids.ctypes.data_as(u32p), C.byref(count), C.byref(flag))
            name = "cs_index_search_variants_boosted" + ("_grouped" if per_file is not None else "") + \
                ("_scoped" if scope is not None else "")
            cap = (int(per_file),) if per_file is not None else ()
            _lib.check(getattr(self._lib, name)(*head, *cap, *tail))
            return score, cos, ids, int(count.value), bool(flag.value)
        if per_file is not None:
            self._needs_groups()
            out = (cos.ctypes.data_as(f32p), ids.ctypes.data_as(u32p), C.byref(count), C.byref(flag))
            if scope is not None:
                _lib.check(self._fn("search_variants_grouped_scoped")(self._h, self._scope_handle(scope),
                                                                             q.ctypes.data_as(f32p), nq, dim, limit,
                                                                             int(per_file), *out))
            else:
                _lib.check(self._fn("search_variants_grouped")(self._h, q.ctypes.data_as(f32p), nq, dim, limit,
                                                                      int(per_file), *out))
        elif scope is not None:
            _lib.check(self._fn("search_variants_scoped")(self._h, self._scope_handle(scope), q.ctypes.data_as(f32p), nq, dim,
                                                          limit, cos.ctypes.data_as(f32p), ids.ctypes.data_as(u32p),
                                                          C.byref(count), C.byref(flag)))
        elif chunk_ids is None:
            _lib.check(self._fn("search_variants")(self._h, q.ctypes.data_as(f32p), nq, dim, limit,
                                                          cos.ctypes.data_as(f32p), ids.ctypes.data_as(u32p),
                                                          C.byref(count), C.byref(flag)))
        else:
            allow, bits, _keep = self._mask_args(chunk_ids)
            _lib.check(self._fn("search_variants_masked")(self._h, q.ctypes.data_as(f32p), nq, dim, limit, allow, bits,
                                                          cos.ctypes.data_as(f32p), ids.ctypes.data_as(u32p),
                                                          C.byref(count), C.byref(flag)))
        return cos, ids, int(count.value), bool(flag.value)

    _SIMILAR_MODES = {"none": _lib.CS_SIMILAR_EXCLUDE_NONE, "self": _lib.CS_SIMILAR_EXCLUDE_SELF,
                      "file": _lib.CS_SIMILAR_EXCLUDE_GROUP}

    def similar_raw(self, chunk_ids, limit: int, exclude: str = "self", min_cos: Optional[float] = None,
                    scope: Optional[Scope] = None):
        """cs_index_search_similar: per source chunk id, the `limit` stored chunks nearest to that chunk's stored row —
        the rows are gathered on the device, no vector crosses the bus — without what `exclude` names: "none" nothing
        (the source comes back first), "self" the source chunk, "file" the source chunk and every chunk of its group
        (its file; set_groups for rows without metadata).  The exclusion is part of the selection, not a filter on a ranked
        list.  min_cos: only chunks whose cosine is strictly greater are returned (None: no bound).
        scope: only the scope's chunks are returned (cs_index_search_similar_scoped: the exact best `limit` among them); the
        sources themselves need not be in it.  The scope's route (Scope.set_route) picks between the gathered scan and the
        int8 filter planned over the scope's rows — same bits — and Scope.route_info() counts the call; set_similar_route
        governs the call without a scope only.
        -> (cos [n, limit] f32, ids [n, limit] u32, counts [n] u32); more than CS_MAX_QUERIES sources go in several calls."""
        if self.sharded:
            raise CsError(_lib.CS_ERR_UNSUPPORTED, "a sharded store has no similar-chunk search: no cs_shards_ form yet")
        if exclude not in self._SIMILAR_MODES:
            raise ValueError(f'exclude must be "self", "file" or "none", got {exclude!r}')
        src = np.ascontiguousarray(chunk_ids, np.uint32).ravel()
        n = src.size
        bound = np.float32(-np.inf) if min_cos is None else np.float32(min_cos)
        cos = np.zeros((n, max(limit, 1)), np.float32)
        ids = np.zeros((n, max(limit, 1)), np.uint32)
        counts = np.zeros(n, np.uint32)
        if scope is None:
            call = lambda *a: self._lib.cs_index_search_similar(self._h, *a)
        else:
            sc = self._scope_handle(scope)
            call = lambda *a: self._lib.cs_index_search_similar_scoped(self._h, sc, *a)
        for lo in range(0, max(n, 1), _lib.CS_MAX_QUERIES):  # (n == 0: one call, refused by the library like nq == 0)
            hi = min(n, lo + _lib.CS_MAX_QUERIES)
            part = src[lo:hi]
            _lib.check(call(part.ctypes.data_as(u32p), hi - lo, limit, self._SIMILAR_MODES[exclude], float(bound),
                            cos[lo:hi].ctypes.data_as(f32p), ids[lo:hi].ctypes.data_as(u32p),
                            counts[lo:hi].ctypes.data_as(u32p)))
        return cos, ids, counts

    SIMILAR_ROUTES = {"auto": _lib.CS_SIMILAR_ROUTE_AUTO, "scan": _lib.CS_SIMILAR_ROUTE_SCAN,
                      "filter": _lib.CS_SIMILAR_ROUTE_FILTER}

    def set_similar_route(self, route) -> None:
        """The route of similar_raw / similar without a scope (cs_index_set_similar_route): "auto" (default: the int8 / f16
        filter with an exact refine where an ordinary search of as many queries would take it, else the scan), "scan" (always
        the f32 streaming scan) or "filter" (the filter whenever a copy can serve).  Same bits on every route."""
        if self.sharded:
            raise CsError(_lib.CS_ERR_UNSUPPORTED, "a sharded store has no similar-chunk search: no cs_shards_ form yet")
        _lib.check(self._lib.cs_index_set_similar_route(self._h, self.SIMILAR_ROUTES.get(route, route)))

    def similar_route_info(self):
        """-> (filter_searches, scan_searches, filter_fallbacks) of the unscoped similar searches so far
        (cs_index_similar_route_info): a call whose candidate buffer overflowed and that the scan then answered counts in
        filter_searches and in filter_fallbacks."""
        if self.sharded:
            raise CsError(_lib.CS_ERR_UNSUPPORTED, "a sharded store has no similar-chunk search: no cs_shards_ form yet")
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _lib.check(self._lib.cs_index_similar_route_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def similar(self, chunk_id: int, limit: int, other_files: bool = False, min_score: Optional[float] = None,
                scope: Optional[Scope] = None) -> List[SearchResult]:
        """The `limit` chunks most similar to chunk `chunk_id`, best first, never the chunk itself; other_files=True: none
        of its file either (the files assigned at insert).  min_score: only chunks whose score — the reference's scale,
        cos_to_score — is above it.  scope: only chunks of the scope (similar_raw; the scope's route picks the gathered scan or
        the int8 filter, same results).  Results whose metadata is missing are skipped, as in search()."""
        min_cos = None if min_score is None else score_to_cos(min_score)
        cos, ids, counts = self.similar_raw([int(chunk_id)], limit, exclude="file" if other_files else "self", min_cos=min_cos,
                                            scope=scope)
        return self._results(cos[0], ids[0], int(counts[0]))

    def similar_pairs_raw(self, min_cos: float, other_files: bool = False, max_pairs: int = 65536,
                          scope: Optional[Scope] = None, other: Optional[Scope] = None):
        """cs_index_similar_pairs: every pair of stored chunks a < b whose cosine — the similar-chunk search's, bit for bit —
        is strictly above min_cos (-inf: no bound), best first by (cosine desc, a asc, b asc); other_files=True: never two
        chunks of one group (file; two ungrouped chunks are never one file).  The corpus is joined with itself on the
        device, exactly.  -> (cos [m] f32, a [m] u32, b [m] u32, total) with m = min(total, max_pairs): total > max_pairs
        says the list was cut.  The call refuses (CS_ERR_UNSUPPORTED) a bound so low that more than 2 * max_pairs + 4096
        pairs come near it: raise min_cos, pass other_files=True or raise max_pairs.
        scope alone: only the pairs inside the scope; scope with other: only the pairs with one chunk in each, every pair
        once however the two overlap (cs_index_similar_pairs_scoped).  The candidate bound then counts those pairs only, so
        near-duplicates elsewhere in the store do not make the call refuse.  other without scope is a ValueError."""
        if other is not None and scope is None:
            raise ValueError("other= needs scope=: the pairs between two scopes")
        if self.sharded:
            raise CsError(_lib.CS_ERR_UNSUPPORTED, "a sharded store has no similar-pairs search: no cs_shards_ form yet")
        room = max(0, min(int(max_pairs), _lib.CS_MAX_PAIRS))
        cos = np.zeros(room, np.float32)
        a = np.zeros(room, np.uint32)
        b = np.zeros(room, np.uint32)
        total = C.c_uint64(0)
        bound = np.float32(-np.inf) if min_cos is None else np.float32(min_cos)
        args = (float(bound), _lib.CS_PAIRS_OTHER_GROUP if other_files else _lib.CS_PAIRS_ALL, int(max_pairs),
                a.ctypes.data_as(u32p), b.ctypes.data_as(u32p), cos.ctypes.data_as(f32p), C.byref(total))
        if scope is None:
            _lib.check(self._lib.cs_index_similar_pairs(self._h, *args))
        else:
            sa = self._scope_handle(scope)
            sb = sa if other is None else self._scope_handle(other)
            _lib.check(self._lib.cs_index_similar_pairs_scoped(self._h, sa, sb, *args))
        m = min(int(total.value), room)
        return cos[:m], a[:m], b[:m], int(total.value)

    def similar_pairs_info(self) -> dict:
        """cs_index_similar_pairs_info: what this thread's last similar_pairs_raw did — candidate pairs, launch bands, the
        filter's and the refine's device time and the ordering's host time (ms); after a scoped call also the packing's
        device time, the two sides' live rows and the tile pairs scored (cs_index_similar_pairs_scoped_info; else zeros)."""
        cand, bands = C.c_uint64(0), C.c_uint32(0)
        f, r, o = C.c_double(0), C.c_double(0), C.c_double(0)
        _lib.check(self._lib.cs_index_similar_pairs_info(C.byref(cand), C.byref(bands), C.byref(f), C.byref(r), C.byref(o)))
        pack, ra, rb, tp = C.c_double(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _lib.check(self._lib.cs_index_similar_pairs_scoped_info(C.byref(pack), C.byref(ra), C.byref(rb), C.byref(tp)))
        return {"candidates": int(cand.value), "bands": int(bands.value), "filter_ms": f.value, "refine_ms": r.value,
                "order_ms": o.value, "pack_ms": pack.value, "rows_a": int(ra.value), "rows_b": int(rb.value),
                "tile_pairs": int(tp.value)}

    def similar_pairs(self, min_score: float, other_files: bool = True, max_pairs: int = 65536,
                      scope: Optional[Scope] = None, other: Optional[Scope] = None):
        """The near-duplicate report: every pair of stored chunks whose score — the reference's scale, cos_to_score — is
        above min_score, best first, as (SearchResult, SearchResult, score) with the lower id first; other_files=True (the
        default): never two chunks of one file (the files assigned at insert).  At most max_pairs pairs.  Pairs with a chunk
        whose metadata is missing are skipped, as in search().  scope / other: only the pairs inside the scope, or between
        the two scopes (similar_pairs_raw) — "src/ against vendor/" is scope(chunk_ids_under("src/")) and the same of
        "vendor/"."""
        cos, a, b, _total = self.similar_pairs_raw(score_to_cos(min_score), other_files=other_files, max_pairs=max_pairs,
                                                   scope=scope, other=other)
        ra, rb = self._results(cos, a, len(a), keep_missing=True), self._results(cos, b, len(b), keep_missing=True)
        return [(x, y, y.score) for x, y in zip(ra, rb) if x is not None and y is not None]

    def similar_clusters_raw(self, min_cos: float, other_files: bool = False, scope: Optional[Scope] = None,
                             other: Optional[Scope] = None):
        """cs_index_similar_clusters: the clone classes of the store — the connected components of the graph whose edges are
        the pairs similar_pairs_raw(min_cos, other_files) would count (-inf / None: no bound).
        -> (labels [next_id - id_base] u32, clusters, members): labels[i] = the smallest id of the class of id id_base + i
        (its own id when it has no clone), CS_NO_ID (0xFFFFFFFF) for an id that is not live; the classes of two or more
        ids; the ids in them.  There is no max_pairs: a store full of duplicates is answered, not refused.
        scope alone: the classes inside the scope; scope with other: the classes of the pairs with one chunk in each
        (similar_clusters_scoped_raw, scattered: ids outside the two scopes are CS_NO_ID too).  That is NOT the unscoped
        answer restricted to the scope: a path through a chunk outside connects nothing.  other without scope is a
        ValueError."""
        if other is not None and scope is None:
            raise ValueError("other= needs scope=: the classes between two scopes")
        if self.sharded:
            raise CsError(_lib.CS_ERR_UNSUPPORTED, "a sharded store has no similar-clusters search: no cs_shards_ form yet")
        n = self.next_id() - self.id_base
        labels = np.full(max(n, 0), _lib.CS_NO_ID, np.uint32)
        if scope is not None:
            ids, lab, clusters, members = self.similar_clusters_scoped_raw(min_cos, other_files, scope, other)
            labels[ids - np.uint32(self.id_base)] = lab
            return labels, clusters, members
        clusters, members = C.c_uint64(0), C.c_uint64(0)
        bound = np.float32(-np.inf) if min_cos is None else np.float32(min_cos)
        _lib.check(self._lib.cs_index_similar_clusters(
            self._h, float(bound), _lib.CS_PAIRS_OTHER_GROUP if other_files else _lib.CS_PAIRS_ALL,
            labels.ctypes.data_as(u32p), n, C.byref(clusters), C.byref(members)))
        return labels, int(clusters.value), int(members.value)

    def similar_clusters_scoped_raw(self, min_cos: float, other_files: bool, scope: Scope, other: Optional[Scope] = None):
        """cs_index_similar_clusters_scoped as it answers: -> (ids [n] u32, labels [n] u32, clusters, members), the live ids
        of the scope (of both scopes, each id once) ascending and, for each, the smallest id of its class."""
        if self.sharded:
            raise CsError(_lib.CS_ERR_UNSUPPORTED, "a sharded store has no similar-clusters search: no cs_shards_ form yet")
        sa = self._scope_handle(scope)
        sb = sa if other is None else self._scope_handle(other)
        cap = len(scope) + (0 if other is None or other is scope else len(other))
        ids = np.zeros(cap, np.uint32)
        lab = np.zeros(cap, np.uint32)
        n, clusters, members = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        bound = np.float32(-np.inf) if min_cos is None else np.float32(min_cos)
        _lib.check(self._lib.cs_index_similar_clusters_scoped(
            self._h, sa, sb, float(bound), _lib.CS_PAIRS_OTHER_GROUP if other_files else _lib.CS_PAIRS_ALL,
            ids.ctypes.data_as(u32p), lab.ctypes.data_as(u32p), cap, C.byref(n), C.byref(clusters), C.byref(members)))
        m = int(n.value)
        return ids[:m], lab[:m], int(clusters.value), int(members.value)

    def similar_clusters_info(self, scoped: bool = False) -> dict:
        """cs_index_similar_clusters_info: what this thread's last similar_clusters_raw of either kind did — the join's tile
        pairs scored and skipped (both tiles already one class), the pairs re-scored exactly, the join's launches, and the
        device time (ms) of the launches and of the labelling.  scoped=True adds cs_index_similar_clusters_scoped_info's
        fields: the packing's device time, the two sides' live rows (the smaller first) and the vertices returned — zeros
        after an unscoped call.  (They are asked for, not always there: callers compare the plain dict as a whole.)"""
        scored, skipped, rescored, launches = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        j, lab = C.c_double(0), C.c_double(0)
        _lib.check(self._lib.cs_index_similar_clusters_info(C.byref(scored), C.byref(skipped), C.byref(rescored),
                                                            C.byref(launches), C.byref(j), C.byref(lab)))
        info = {"tile_pairs_scored": int(scored.value), "tile_pairs_skipped": int(skipped.value),
                "rescored_pairs": int(rescored.value), "launches": int(launches.value), "join_ms": j.value,
                "label_ms": lab.value}
        if scoped:
            pack, ra, rb, nv = C.c_double(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
            _lib.check(self._lib.cs_index_similar_clusters_scoped_info(C.byref(pack), C.byref(ra), C.byref(rb), C.byref(nv)))
            info.update({"pack_ms": pack.value, "rows_a": int(ra.value), "rows_b": int(rb.value), "vertices": int(nv.value)})
        return info

    def similar_clusters(self, min_score: float, other_files: bool = True, min_size: int = 2,
                         scope: Optional[Scope] = None, other: Optional[Scope] = None) -> List[List[SearchResult]]:
        """The duplicate-code report by clone class: the classes of chunks connected by pairs whose score — the reference's
        scale, cos_to_score — is above min_score; other_files=True (the default): a pair of chunks of one file connects
        nothing (the files assigned at insert).  Classes of at least min_size chunks, the largest first, then by label (the
        smallest id); members by id.  A result's distance and score are those of a chunk against itself: a class carries
        no cosine.  Chunks whose metadata is missing are skipped, as in search(); a class is sized by what remains.
        scope / other: the classes inside the scope, or of the pairs between the two scopes (similar_clusters_raw)."""
        labels, _clusters, _members = self.similar_clusters_raw(score_to_cos(min_score), other_files=other_files,
                                                                scope=scope, other=other)
        live = np.flatnonzero(labels != _lib.CS_NO_ID)
        classes = {}
        for i in live.tolist():
            classes.setdefault(int(labels[i]), []).append(int(self.id_base) + i)
        out = []
        for label, ids in classes.items():
            res = self._results(np.ones(len(ids), np.float32), ids, len(ids))
            if len(res) >= max(int(min_size), 1):
                out.append((label, res))
        out.sort(key=lambda t: (-len(t[1]), t[0]))
        return [res for _, res in out]

    def chunk_ids_under(self, filter_path: str, project_root: str = "", mcp: bool = True) -> List[int]:
        """Ids of the chunks whose metadata path passes the reference's filter_path rule (search.path_matches; MCP or
        CLI form), ascending: the chunk_ids of a masked search narrowed to a directory."""
        from .search import path_matches
        return sorted(i for i, m in self._meta.items() if path_matches(m.path, filter_path, project_root, mcp))

    def _results(self, cos, ids, count, keep_missing: bool = False, score=None) -> List[SearchResult]:
        """keep_missing: a None stands where an id has no metadata (the lists of a pair stay aligned).
        score: the results' scores when they are not 1 - distance (a boosted search's)."""
        out = []
        dist = cos_to_distance(cos[:count])
        for i in range(count):
            m = self._meta.get(int(ids[i]))
            if m is None:
                if keep_missing:
                    out.append(None)
                continue
            d = float(dist[i])
            out.append(SearchResult(
                id=int(ids[i]), content=m.content, path=m.path, start_line=m.start_line,
                end_line=m.end_line, kind=m.kind, signature=m.signature, docstring=m.docstring,
                context=m.context, hash=m.hash, distance=d,
                score=float(np.float32(1.0) - np.float32(d)) if score is None else float(score[i]),
                context_prev=m.context_prev, context_next=m.context_next))
        return out

    def get_chunk(self, chunk_id: int) -> Optional[ChunkMetadata]:
        """store.rs:709-713."""
        return self._meta.get(int(chunk_id))

    def get_chunk_as_result(self, chunk_id: int) -> Optional[SearchResult]:
        """store.rs:715-738 (distance/score 0.0, set by caller)."""
        m = self._meta.get(int(chunk_id))
        if m is None:
            return None
        return SearchResult(id=int(chunk_id), content=m.content, path=m.path, start_line=m.start_line,
                            end_line=m.end_line, kind=m.kind, signature=m.signature, docstring=m.docstring,
                            context=m.context, hash=m.hash, distance=0.0, score=0.0,
                            context_prev=m.context_prev, context_next=m.context_next)

    def get_chunks_by_file(self) -> Dict[str, List[int]]:
        """store.rs:529-543: path -> chunk ids."""
        out: Dict[str, List[int]] = {}
        for i, m in self._meta.items():
            out.setdefault(m.path, []).append(i)
        return out

    def stats(self) -> StoreStats:
        """store.rs:488-523."""
        files = {m.path for m in self._meta.values()}
        return StoreStats(total_chunks=len(self._meta), total_files=len(files), indexed=self.is_indexed(),
                          dimensions=self.dimensions, max_chunk_id=max(self._meta.keys(), default=0))

    def read_rows(self, first_row: int, n: int) -> np.ndarray:
        out = np.empty((n, self.dimensions), np.float32)
        _lib.check(self._fn("read_rows")(self._h, first_row, n, out.ctypes.data_as(f32p)))
        return out

    # -- kernel timing (bench.py)
    def profile(self, enable: bool) -> None:
        _lib.check(self._lib.cs_index_profile(self._h, 1 if enable else 0))

    def profile_read(self, reset: bool = True):
        """-> (scan_ms_total, scan_launches, merge_ms_total)."""
        s, m, n = C.c_double(), C.c_double(), C.c_uint64()
        _lib.check(self._lib.cs_index_profile_read(self._h, C.byref(s), C.byref(n), C.byref(m), 1 if reset else 0))
        return s.value, int(n.value), m.value

    def set_filter_min_queries(self, n: int) -> None:
        """Searches of >= n queries use the f16 filter + exact refine path (default 2; 1 = always)."""
        _lib.check(self._lib.cs_index_set_filter_min_queries(self._h, int(n)))

    ROUTE_COST, ROUTE_STREAM, ROUTE_FILTER = 0, 1, 2

    def set_single_query_route(self, route: int) -> None:
        """How one query over a large index is answered (cs_index_set_single_query_route): ROUTE_COST (default: the int8
        filter + exact refine from 32,768 rows on for lists of k < 48 and from 300,000 rows on from k = 48 — the measured
        crossovers, index.hip single_int8_min_rows / single_int8_min_rows_long; CS_FILTER_SINGLE_MIN_ROWS /
        CS_FILTER_SINGLE_MIN_ROWS_LONG override them), ROUTE_STREAM (always the f32 streaming scan), ROUTE_FILTER.  Same bits."""
        if self.sharded:
            for g in range(int(self._lib.cs_shards_count(self._h))):
                _lib.check(self._lib.cs_index_set_single_query_route(self.shard_handle(g), int(route)))
        else:
            _lib.check(self._lib.cs_index_set_single_query_route(self._h, int(route)))

    def debug_counters(self):
        """-> (batched_searches, batched_fallbacks)"""
        a, b = C.c_uint64(), C.c_uint64()
        _lib.check(self._lib.cs_index_debug_counters(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def filter_state(self):
        """-> (copy, spread, int8_reruns): which copy feeds the batched filter (0 none, 1 f16, 2 int8), the spread statistic
        of the last build and the searches the f16 copy answered after the int8 copy overflowed (cs_index_filter_state)."""
        if self.sharded:
            raise ValueError("filter_state is per index: use shard_handle()")
        c, sp, n = C.c_int32(), C.c_float(), C.c_uint64()
        _lib.check(self._lib.cs_index_filter_state(self._h, C.byref(c), C.byref(sp), C.byref(n)))
        return int(c.value), float(sp.value), int(n.value)

    def filter_copies(self):
        """-> (has_int8, has_f16, bytes): which filter copies of the corpus exist in HBM right now and what they occupy
        (cs_index_filter_copies).  An index whose int8 copy serves holds no f16 copy: it is built by the first search
        that needs it (the int8 copy retired) or at a build whose int8 copy does not serve."""
        if self.sharded:
            raise ValueError("filter_copies is per index: use shard_handle()")
        a, b, n = C.c_int32(), C.c_int32(), C.c_uint64()
        _lib.check(self._lib.cs_index_filter_copies(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return bool(a.value), bool(b.value), int(n.value)

    @property
    def handle(self):
        return self._h


# ---- embedding-cache value format --------------------------------------------------

def encode_cached_embedding(vec) -> bytes:
    """The value bytes of the reference's persistent embedding cache
    (`Database<Str, SerdeBincode<Vec<f32>>>`, /root/reference/src/embed/cache.rs:283-285):
    bincode 1.x of a Vec<f32> = u64 little-endian length, then the f32 little-endian elements."""
    v = np.ascontiguousarray(vec, "<f4")
    return int(v.size).to_bytes(8, "little") + v.tobytes()


def decode_cached_embedding(buf: bytes) -> np.ndarray:
    """Inverse of encode_cached_embedding; raises on a length/size mismatch."""
    if len(buf) < 8:
        raise ValueError("bincode Vec<f32>: missing length prefix")
    n = int.from_bytes(buf[:8], "little")
    if len(buf) != 8 + 4 * n:
        raise ValueError(f"bincode Vec<f32>: length {n} does not match {len(buf) - 8} payload bytes")
    return np.frombuffer(buf, "<f4", count=n, offset=8).astype(np.float32)
