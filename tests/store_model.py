"""A plain model of VectorStore's life cycle, and a judge for what its searches return.  numpy only, no GPU.

The model holds what the store is meant to hold — which ids were issued, which are live, their float32 rows as stored,
their groups, whether the index is built and how many rows the corpus matrix physically stores — and mirrors the
mutating calls: insert, delete, build (with the documented reclaim rule: a build drops the tombstoned rows of an index
when removed * 100 >= 10 * stored and removed > 0), clear, set_groups and reopening a persisted store.

It does not predict ONE list for a search.  `check` judges a returned (cos, ids, count) against float64 cosines over the
live rows, within a band that is DERIVED, not measured:

    tol = 2 * (dim + 8) * 2**-24

the forward error bound of the cosine as the kernels compute it in f32 (u = 2**-24): the dot product of dim terms is off by
at most dim * u * sum|x_i y_i| <= dim * u * |x| |y| (Cauchy-Schwarz), i.e. dim * u of the cosine's scale; each of the two
norms is the square root of such a sum of squares, off by at most (dim / 2 + 1) * u relatively; the product of the norms
and the division add 2 * u.  Sum: (2 * dim + 4) * u, rounded up to 2 * (dim + 8) * u = 4.7e-5 at dim 384.  A
zero-magnitude row or query scores 0.0 (the reference's guard, src/embed/batch.rs:320-322).

The second half is the walk generator: `make_walk(seed, dim, sharded)` returns a deterministic list of about 40
operations that drives a store through every state the index keeps books for, `resolve` turns an operation into concrete
arguments for the state the model is in, `apply` performs it on the model, and `walk_coverage` reports — from the model
alone — which states a walk reaches, so a test can refuse a walk that quietly stopped exercising one.

The kinds that start from stored rows (similar chunks, similar pairs, similar clusters) and the boosted search have judges
of their own on the same float64 cosines and the same band: `check_similar` (which hands the eligible rows to `check`),
`check_pairs`, `check_clusters` and `check_boosted`, whose second tolerance — the cosine's band carried through the score
plus the three f32 roundings of the score — is derived too.  A bound that float64 cannot place (a cosine within tol of it) is
refused, not judged: the inputs keep that from happening, never the judge.  `make_walk(..., extended=True)` is the same
walk with a class table beside every group table and near-copies planted around BOUND (`clone_layout`), `Planted` follows
their ids, `extended_coverage` reports what the checked states of such a walk hold.
"""
from __future__ import annotations

import numpy as np

from codesearch_amd.synth import synth_rows

NO_GROUP = 0xFFFFFFFF  # CS_NO_GROUP
NO_ID = 0xFFFFFFFF     # the id of an empty result slot
NO_CLASS = 0xFFFF      # CS_NO_CLASS
BOUND = np.float32(0.9)  # the cosine bound of the walks' pairs and clusters calls: the planted clones straddle it
EDGES = (128, 1024, 1025, 1152, 2048)  # stored-row counts at which the index changes what it does
NOT_BUILT = "Index not built"
# the walks the GPU test runs and the CPU test vouches for: (seed, dim, sharded)
WALKS = [(s, d, False) for s in range(6) for d in (384, 100)] + [(s, 384, True) for s in range(2)]


def tolerance(dim: int) -> float:
    """The band of `check` (module docstring): 2 * (dim + 8) * 2**-24."""
    return 2.0 * (dim + 8) * 2.0 ** -24


class StoreModel:
    def __init__(self, dim: int, id_base: int = 0, shards: int = 1, stripe: int = 1 << 32):
        self.dim, self.id_base, self.shards, self.stripe = int(dim), int(id_base), int(shards), int(stripe)
        self.tol = tolerance(dim)
        self.persisted_next = None  # next_id at the last build (what a reopening finds on disk); None: nothing persisted
        self._reset()

    def _reset(self):
        self.next_id = self.id_base
        self.rows = {}           # id -> float32 row, for every id still in storage (live or tombstoned)
        self.removed = set()     # ids deleted since the last clear()
        self.reclaimed = set()   # ... whose rows a build has dropped
        self.groups = {}         # id -> group, for ids that carry one (every other id: NO_GROUP)
        self.classes = {}        # id -> class, for ids that carry one (every other id: NO_CLASS)
        self.built = False
        self.stored = [[] for _ in range(self.shards)]  # ids in storage order, per shard
        self.compacted = [False] * self.shards
        self.last_appended = None
        self.moved = None        # a live id whose row the last reclaim moved
        self.version = getattr(self, "version", 0) + 1
        self._cache = {}

    def _touch(self):
        self.version += 1
        self._cache = {}

    def shard_of(self, i: int) -> int:
        return ((i - self.id_base) // self.stripe) % self.shards

    # ---- the mutating calls ------------------------------------------------------------------------------
    def insert(self, rows) -> list:
        rows = np.ascontiguousarray(rows, np.float32)
        ids = list(range(self.next_id, self.next_id + len(rows)))
        for i, r in zip(ids, rows):
            self.rows[i] = r.copy()
            self.stored[self.shard_of(i)].append(i)
        self.next_id += len(rows)
        if ids:
            self.built = False
            self.last_appended = ids[-1]
            self._touch()
        return ids

    def is_live(self, i: int) -> bool:
        return i in self.rows and i not in self.removed

    def delete(self, ids) -> int:
        """-> how many of `ids` were live: never issued, already deleted and ids below id_base count as 0."""
        cnt = 0
        for i in ids:
            i = int(i)
            if self.is_live(i):
                self.removed.add(i)
                cnt += 1
        if cnt:
            self.built = False
            self._touch()
        return cnt

    def build(self) -> bool:
        """-> whether any shard reclaimed its tombstones."""
        any_reclaim = False
        for s in range(self.shards):
            st = self.stored[s]
            dead = [i for i in st if i in self.removed]
            if dead and len(dead) * 100 >= 10 * len(st):
                first = st.index(dead[0])
                keep = [i for i in st if i not in self.removed]
                after = [i for i in st[first:] if i not in self.removed]
                self.moved = after[0] if after else self.moved
                for i in dead:
                    del self.rows[i]
                self.reclaimed.update(dead)
                self.stored[s] = keep
                self.compacted[s] = True
                any_reclaim = True
        if self.moved is not None and not self.is_live(self.moved):
            self.moved = None
        self.built = True
        self.persisted_next = self.next_id
        self._touch()
        return any_reclaim

    def clear(self):
        self._reset()
        self.persisted_next = None

    def set_groups(self, ids, groups):
        ids, groups = [int(i) for i in ids], [int(g) for g in groups]
        for i in ids:
            if not self.id_base <= i < self.next_id:
                raise ValueError(f"id {i} was never issued")
        for i, g in zip(ids, groups):
            if g == NO_GROUP:
                self.groups.pop(i, None)
            else:
                self.groups[i] = g
        self._touch()

    def groups_assigned(self) -> int:
        return len(self.groups)

    def set_classes(self, ids, classes):
        ids, classes = [int(i) for i in ids], [int(c) for c in classes]
        for i in ids:
            if not self.id_base <= i < self.next_id:
                raise ValueError(f"id {i} was never issued")
        for i, c in zip(ids, classes):
            if c == NO_CLASS:
                self.classes.pop(i, None)
            else:
                self.classes[i] = c
        self._touch()

    def classes_assigned(self) -> int:
        return len(self.classes)

    def reopen(self):
        """Close and open again from disk: the state of the last build, minus what was deleted since (a delete is
        committed at once); rows appended since are lost; groups and classes are not stored (they follow from chunk
        metadata, which the walks do not use).  The loader re-adds every persisted row, removes the removed ids and builds."""
        keep_next, removed, rows = self.persisted_next, self.removed, self.rows
        self._reset()
        if keep_next is None:
            return
        zero = np.zeros(self.dim, np.float32)
        self.insert([rows.get(i, zero) for i in range(self.id_base, keep_next)])
        self.delete([i for i in removed if i < keep_next])
        self.removed = {i for i in removed if i < keep_next}
        self.build()

    # ---- what the store reports --------------------------------------------------------------------------
    def __len__(self) -> int:
        return sum(1 for i in self.rows if i not in self.removed)

    def stored_rows(self) -> int:
        return sum(len(s) for s in self.stored)

    def live_ids(self) -> np.ndarray:
        if "live" not in self._cache:
            self._cache["live"] = np.array(sorted(i for i in self.rows if i not in self.removed), np.int64)
        return self._cache["live"]

    def stored_live(self) -> list:
        """Live ids in storage order (shard after shard)."""
        return [i for s in self.stored for i in s if i not in self.removed]

    def _matrix(self):
        if "mat" not in self._cache:
            ids = self.live_ids()
            m = np.stack([self.rows[int(i)] for i in ids]).astype(np.float64) if len(ids) else np.zeros((0, self.dim))
            self._cache["mat"] = (m, np.sqrt((m * m).sum(axis=1)))
        return self._cache["mat"]

    def cosines(self, q) -> np.ndarray:
        """float64 cosine of every live row (order of live_ids()) with q; 0.0 where the row or q has no magnitude.
        q [nq, dim]: the best over the queries (what search_variants scores an id with)."""
        q = np.asarray(q, np.float32)
        key = ("cos", q.tobytes())
        if key not in self._cache:
            m, norms = self._matrix()
            best = np.full(len(norms), -np.inf)
            for v in q.reshape(-1, self.dim).astype(np.float64):
                qn = np.sqrt((v * v).sum())
                den = norms * qn
                c = np.where(den > 0, (m @ v) / np.where(den > 0, den, 1.0), 0.0)
                best = np.maximum(best, c)
            self._cache[key] = best
        return self._cache[key]

    def _live_groups(self) -> np.ndarray:
        if "grp" not in self._cache:
            self._cache["grp"] = np.array([self.groups.get(int(i), NO_GROUP) for i in self.live_ids()], np.int64)
        return self._cache["grp"]

    def _dup_class(self) -> np.ndarray:
        """Per live id: the lowest live id with byte-identical stored row (itself when the row is unique)."""
        if "dup" not in self._cache:
            first = {}
            ids = self.live_ids()
            out = np.empty(len(ids), np.int64)
            for n, i in enumerate(ids):
                out[n] = first.setdefault(self.rows[int(i)].tobytes(), int(i))
            self._cache["dup"] = out
        return self._cache["dup"]

    def _dup_members(self) -> dict:
        """class -> positions (in live_ids()) of its members, for the classes of two or more."""
        if "dupm" not in self._cache:
            cls = self._dup_class()
            u, cnt = np.unique(cls, return_counts=True)
            self._cache["dupm"] = {int(c): np.flatnonzero(cls == c) for c in u[cnt > 1]}
        return self._cache["dupm"]

    def has_dups_and_zero(self) -> bool:
        ids, cls = self.live_ids(), self._dup_class()
        return bool((cls != ids).any()) and any(not self.rows[int(i)].any() for i in ids)

    def _eligible(self, allowed) -> np.ndarray:
        ids = self.live_ids()
        if allowed is None:
            return np.ones(len(ids), bool)
        return np.isin(ids, allowed if isinstance(allowed, np.ndarray) else np.asarray(list(allowed), np.int64))

    # ---- the model's own answer --------------------------------------------------------------------------
    def topk(self, q, k, allowed=None, per_file=None):
        """-> (cos [k] f32, ids [k] u32, count): by float64 cosine descending, ties by ascending id, groups capped."""
        if not self.built:
            raise AssertionError(NOT_BUILT)
        ids, c, elig, grp = self.live_ids(), self.cosines(q), self._eligible(allowed), self._live_groups()
        order = [n for n in np.lexsort((ids, -c)) if elig[n]]
        taken, out = {}, []
        for n in order:
            if len(out) == k:
                break
            g = int(grp[n])
            if per_file is not None and g != NO_GROUP:
                if taken.get(g, 0) >= per_file:
                    continue
                taken[g] = taken.get(g, 0) + 1
            out.append(n)
        cos, rid = np.zeros(k, np.float32), np.full(k, NO_ID, np.uint32)
        cos[:len(out)], rid[:len(out)] = c[out], ids[out]
        return cos, rid, len(out)

    # ---- the judge ---------------------------------------------------------------------------------------
    def check(self, q, k, got, allowed=None, per_file=None) -> float:
        """Judges got = (cos [>= k], ids [>= k], count) for query q (or query variants q [nq, dim], merged).  Raises
        AssertionError unless (a) to (f) of the module's contract hold; -> the largest |returned cos - float64 cos|."""
        if not self.built:
            raise AssertionError(NOT_BUILT)
        tol = self.tol
        cos = np.asarray(got[0], np.float32).ravel()
        rid_all = np.asarray(got[1]).ravel().astype(np.int64)
        count = int(got[2])
        ids, c64, elig, grp = self.live_ids(), self.cosines(q), self._eligible(allowed), self._live_groups()
        capped = per_file is not None

        def need(ok, msg):
            if not ok:
                raise AssertionError(f"{msg} (k={k}, allowed={'all' if allowed is None else len(list(allowed))}, "
                                     f"per_file={per_file}, count={count}, ids={rid_all[:min(count, 12)].tolist()})")

        # (a) the count, and the empty tail
        if capped:
            g = grp[elig]
            _, sizes = np.unique(g[g != NO_GROUP], return_counts=True)
            room = int((g == NO_GROUP).sum() + np.minimum(sizes, per_file).sum())
        else:
            room = int(elig.sum())
        need(count == min(k, room), f"count {count}, expected min(k, {room})")
        need(len(cos) >= k and len(rid_all) >= k, "the answer is shorter than k")
        need((rid_all[count:k] == NO_ID).all() and (cos[count:k] == 0.0).all(), "the tail behind count is not empty slots")
        rid, rc = rid_all[:count], cos[:count]
        if count == 0:
            return 0.0
        # (b) distinct, live, allowed, within the cap
        need(len(set(rid.tolist())) == count, "an id is returned twice")
        pos = np.minimum(np.searchsorted(ids, rid), len(ids) - 1) if len(ids) else np.zeros(count, np.int64)
        live = (ids[pos] == rid) if len(ids) else np.zeros(count, bool)
        for i in rid[~live].tolist():
            why = "was deleted and reclaimed" if i in self.reclaimed else "is deleted" if i in self.removed else "was never issued"
            need(False, f"id {i} {why}")
        need(elig[pos].all(), f"ids outside the allowed set: {rid[~elig[pos]].tolist()[:5]}")
        rg = grp[pos]
        ug, inv, cnt_g = np.unique(rg, return_inverse=True, return_counts=True)  # the groups of the returned ids
        if capped:
            over = (cnt_g > per_file) & (ug != NO_GROUP)
            need(not over.any(), f"group {ug[over][:1].tolist()} appears more than {per_file} times")
        # (c) each cosine is that id's
        err = np.abs(rc.astype(np.float64) - c64[pos])
        worst = int(err.argmax())
        need(err[worst] <= tol, f"cos of id {int(rid[worst])} is {rc[worst]!r}, float64 says {c64[pos][worst]!r} (tol {tol:.2e})")
        # (d) order: own cosine descending, equal cosines by ascending id
        bad = ~((rc[:-1] > rc[1:]) | ((rc[:-1] == rc[1:]) & (rid[:-1] < rid[1:])))
        need(not bad.any(), f"not sorted at position {int(bad.argmax()) if bad.any() else -1}")
        # (e) completeness
        returned = np.zeros(len(ids), bool)
        returned[pos] = True
        omitted = elig & ~returned
        if omitted.any():
            ok = np.zeros(len(ids), bool)
            if count == k:
                ok |= c64 <= float(rc[-1]) + tol
            if capped:  # a full group: an omitted member is fine when every returned one is as good, within the band
                worst_of = np.full(len(ug), np.inf)
                np.minimum.at(worst_of, inv, rc.astype(np.float64))
                at = np.minimum(np.searchsorted(ug, grp), len(ug) - 1)
                full = (ug[at] == grp) & (grp != NO_GROUP) & (cnt_g[at] == per_file)
                ok |= full & (c64 - tol <= worst_of[at])
            miss = omitted & ~ok
            if miss.any():
                n = int(np.flatnonzero(miss)[c64[miss].argmax()])
                need(False, f"id {int(ids[n])} (float64 cos {c64[n]!r}) is left out; the last returned cos is {rc[-1]!r}")
        # (f) byte-identical rows: ascending id, and never a higher one in place of an eligible, uncapped lower one
        cls, dup_members = self._dup_class(), self._dup_members()
        rcls = cls[pos]
        for c in (set(rcls.tolist()) & set(dup_members) if dup_members else ()):
            members = dup_members[c]
            seq = rid[rcls == c]
            need((seq[:-1] < seq[1:]).all(), f"duplicates of id {c} are not in ascending id order: {seq.tolist()}")
            for x in seq.tolist():
                gx = int(grp[np.searchsorted(ids, x)])
                for n in members:
                    y, gy = int(ids[n]), int(grp[n])
                    if y >= x or returned[n] or not elig[n]:
                        continue
                    full = capped and gy != NO_GROUP and gy != gx and int((rg == gy).sum()) >= per_file
                    need(full, f"duplicate id {x} is returned while the identical row of lower id {y} is left out")
        return float(err.max())

    # ---- the kinds that start from stored rows: similar, pairs, clusters; and the boosted search ----------
    def _why_not_live(self, i: int) -> str:
        return "was deleted and reclaimed" if i in self.reclaimed else "is deleted" if i in self.removed else "was never issued"

    def _gram(self) -> np.ndarray:
        """float64 cosine of every live row with every live row (order of live_ids()); 0.0 where a row has no magnitude."""
        if "gram" not in self._cache:
            m, norms = self._matrix()
            unit = m / np.where(norms > 0, norms, 1.0)[:, None]
            self._cache["gram"] = unit @ unit.T
        return self._cache["gram"]

    def ambiguous_pairs(self, bound) -> int:
        """How many live pairs a < b have their float64 cosine within tol of `bound`: a judge of pairs or clusters refuses
        to judge a state where there is one (bound None: no pair is near -inf)."""
        if bound is None or len(self.live_ids()) < 2:
            return 0
        key = ("near", float(np.float32(bound)))
        if key not in self._cache:
            self._cache[key] = int(np.triu(np.abs(self._gram() - key[1]) <= self.tol, 1).sum())
        return self._cache[key]

    def _pair_list(self, bound, other_files, inside=None, other=None):
        """The model's pairs -> (a, b, c64): a < b both live, float64 cosine above bound (None: every pair), not in one
        assigned group when other_files; inside: both ends in it; inside and other: one end in each, every pair once."""
        ids = self.live_ids()
        if len(ids) < 2:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
        g = self._gram()
        key = ("above", None if bound is None else float(np.float32(bound)))
        if key not in self._cache:  # positions (in live_ids()) of the pairs above the bound, before the group and scope rules
            above = np.ones(g.shape, bool) if bound is None else g > key[1]
            self._cache[key] = np.nonzero(np.triu(above, 1))
        ia, ib = self._cache[key]
        keep = np.ones(len(ia), bool)
        if other_files:
            grp = self._live_groups()
            keep &= ~((grp[ia] == grp[ib]) & (grp[ia] != NO_GROUP))
        if inside is not None:
            in_a = self._eligible(inside)
            in_b = in_a if other is None else self._eligible(other)
            keep &= (in_a[ia] & in_b[ib]) | (in_b[ia] & in_a[ib])
        elif other is not None:
            raise ValueError("other needs inside")
        ia, ib = ia[keep], ib[keep]
        return ids[ia], ids[ib], g[ia, ib]

    def _need_decidable(self, bound, what):
        n = self.ambiguous_pairs(bound)
        if n:
            raise AssertionError(f"{what}: refused, {n} live pair(s) lie within tol {self.tol:.2e} of the bound {bound!r}: "
                                 f"float64 cannot decide them; change the inputs")

    def pairs(self, bound, other_files, inside=None, other=None, max_pairs=65536):
        """The model's own answer to similar_pairs_raw -> (cos f32, a u32, b u32, total)."""
        if not self.built:
            raise AssertionError(NOT_BUILT)
        a, b, c = self._pair_list(bound, other_files, inside, other)
        c32 = c.astype(np.float32)
        order = np.lexsort((b, a, -c32))[:max_pairs]
        return c32[order], a[order].astype(np.uint32), b[order].astype(np.uint32), len(a)

    def check_pairs(self, bound, other_files, got, inside=None, other=None, max_pairs=65536) -> float:
        """Judges got = (cos, a, b, total) of similar_pairs_raw(bound, other_files, max_pairs, scope=inside, other=other)
        against the model's pairs; -> the largest |returned cos - float64 cos|."""
        if not self.built:
            raise AssertionError(NOT_BUILT)
        tol = self.tol
        cos = np.asarray(got[0], np.float32).ravel()
        ra, rb = np.asarray(got[1]).ravel().astype(np.int64), np.asarray(got[2]).ravel().astype(np.int64)
        total = int(got[3])

        def need(ok, msg):
            if not ok:
                raise AssertionError(f"{msg} (bound={bound!r}, other_files={other_files}, scoped={inside is not None}, "
                                     f"between={other is not None}, max_pairs={max_pairs}, total={total}, returned={len(ra)})")

        self._need_decidable(bound, "check_pairs")
        ma, mb, mc = self._pair_list(bound, other_files, inside, other)
        truth = {(int(x), int(y)): float(c) for x, y, c in zip(ma, mb, mc)}
        need(len(ra) == len(rb) == len(cos), "cos, a and b differ in length")
        ids = self.live_ids()
        pos = {int(i): n for n, i in enumerate(ids)}
        grp = self._live_groups()
        in_a = self._eligible(inside) if inside is not None else None
        in_b = in_a if other is None else self._eligible(other)
        seen = set()
        err = 0.0
        g = self._gram()
        for c, x, y in zip(cos.tolist(), ra.tolist(), rb.tolist()):
            need(x < y, f"pair ({x}, {y}) is not given as a < b")
            need((x, y) not in seen, f"pair ({x}, {y}) is returned twice")
            seen.add((x, y))
            for i in (x, y):
                need(i in pos, f"pair ({x}, {y}): id {i} {self._why_not_live(i)}")
            px, py = pos[x], pos[y]
            if other_files:
                need(not (grp[px] == grp[py] != NO_GROUP), f"pair ({x}, {y}) lies inside group {int(grp[px])}")
            if in_a is not None:
                need((in_a[px] and in_b[py]) or (in_b[px] and in_a[py]), f"pair ({x}, {y}) is outside the scope(s)")
            c64 = float(g[px, py])
            need(np.isfinite(c) and abs(c - c64) <= tol, f"cos of pair ({x}, {y}) is {c!r}, float64 says {c64!r} (tol {tol:.2e})")
            err = max(err, abs(c - c64))
            need((x, y) in truth, f"pair ({x}, {y}) is returned, but its float64 cos {c64!r} is not above the bound")
        need(total == len(truth), f"total {total}, the model counts {len(truth)} pairs")
        need(len(ra) == min(total, max_pairs), f"{len(ra)} pairs returned, expected min(total, max_pairs)")
        if not len(ra):
            return 0.0
        bad = ~((cos[:-1] > cos[1:]) | ((cos[:-1] == cos[1:]) & ((ra[:-1] < ra[1:]) | ((ra[:-1] == ra[1:]) & (rb[:-1] < rb[1:])))))
        need(not bad.any(), f"not sorted by (cos desc, a, b) at position {int(bad.argmax()) if bad.any() else -1}")
        missing = [(c, p) for p, c in truth.items() if p not in seen]
        if total <= max_pairs:
            need(not missing, f"pair {max(missing)[1] if missing else None} (float64 cos {max(missing)[0] if missing else 0!r}) is left out")
        elif missing:
            c, p = max(missing)
            need(c <= float(cos[-1]) + tol, f"the cut list leaves out pair {p} (float64 cos {c!r}); the last returned cos is {cos[-1]!r}")
        return err

    def _components(self, bound, other_files) -> dict:
        """{live id: smallest id of its component} in the graph of the model's pairs: a plain union-find."""
        parent = {int(i): int(i) for i in self.live_ids()}

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        a, b, _ = self._pair_list(bound, other_files)
        for x, y in zip(a.tolist(), b.tolist()):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
        return {i: find(i) for i in parent}

    def clusters(self, bound, other_files):
        """The model's own answer to similar_clusters_raw -> (labels [next_id - id_base] u32, clusters, members)."""
        if not self.built:
            raise AssertionError(NOT_BUILT)
        comp = self._components(bound, other_files)
        labels = np.full(self.next_id - self.id_base, NO_ID, np.uint32)
        sizes = {}
        for i, root in comp.items():
            labels[i - self.id_base] = root
            sizes[root] = sizes.get(root, 0) + 1
        big = [n for n in sizes.values() if n >= 2]
        return labels, len(big), sum(big)

    def check_clusters(self, bound, other_files, labels, clusters, members) -> float:
        """Judges similar_clusters_raw(bound, other_files): with no ambiguous pair the answer is unique, so all three are
        compared for equality.  -> 0.0 (a label carries no cosine)."""
        if not self.built:
            raise AssertionError(NOT_BUILT)
        labels = np.asarray(labels).ravel().astype(np.int64)

        def need(ok, msg):
            if not ok:
                raise AssertionError(f"{msg} (bound={bound!r}, other_files={other_files}, clusters={clusters}, members={members})")

        self._need_decidable(bound, "check_clusters")
        want, n_clusters, n_members = self.clusters(bound, other_files)
        need(len(labels) == len(want), f"{len(labels)} labels, expected next_id - id_base = {len(want)}")
        for n in np.flatnonzero(labels != want.astype(np.int64)).tolist():
            i, got, exp = self.id_base + n, int(labels[n]), int(want[n])
            if exp == NO_ID:
                need(False, f"id {i} {self._why_not_live(i)} and carries label {got}, not NO_ID")
            need(got != NO_ID, f"live id {i} carries NO_ID, the smallest id of its component is {exp}")
            need(False, f"id {i} carries label {got}, the smallest id of its component is {exp}")
        need(int(clusters) == n_clusters, f"clusters {clusters}, the model counts {n_clusters} components of two or more ids")
        need(int(members) == n_members, f"members {members}, the model counts {n_members} ids in those components")
        return 0.0

    def _similar_eligible(self, src, mode, min_cos, allowed):
        """-> (query row, eligible ids) of a similar-chunk search from `src`; refuses a bound float64 cannot place."""
        if mode not in ("none", "self", "file"):
            raise ValueError(mode)
        src = int(src)
        if not self.is_live(src):
            raise AssertionError(f"source id {src} {self._why_not_live(src)}: the store refuses it")
        q = self.rows[src]
        ids, c64, elig, grp = self.live_ids(), self.cosines(q), self._eligible(allowed).copy(), self._live_groups()
        if mode != "none":
            elig &= ids != src
        g = self.groups.get(src, NO_GROUP)
        if mode == "file" and g != NO_GROUP:
            elig &= grp != g
        if min_cos is not None and np.isfinite(min_cos):
            b = float(np.float32(min_cos))
            near = elig & (np.abs(c64 - b) <= self.tol)
            if near.any():
                raise AssertionError(f"check_similar: refused, id {int(ids[near][0])} lies within tol {self.tol:.2e} of min_cos "
                                     f"{b!r}: float64 cannot decide it; pick another bound (pick_min_cos)")
            elig &= c64 > b
        return q, ids[elig]

    def similar_topk(self, src, k, mode, min_cos=None, allowed=None):
        """The model's own answer to similar_raw([src], k, exclude=mode, min_cos, scope) -> (cos, ids, count)."""
        if not self.built:
            raise AssertionError(NOT_BUILT)
        q, elig = self._similar_eligible(src, mode, min_cos, allowed)
        return self.topk(q, k, allowed=elig)

    def check_similar(self, src, k, got, mode, min_cos=None, allowed=None) -> float:
        """Judges got = (cos, ids, count) of similar_raw([src], k, exclude=mode, min_cos=, scope=allowed): the query is the
        stored row of src, the eligible rows are the live ones minus what mode excludes, minus those not above min_cos,
        inside `allowed`; then `check` over that set, rules (a) to (f)."""
        if not self.built:
            raise AssertionError(NOT_BUILT)
        src = int(src)
        q, elig = self._similar_eligible(src, mode, min_cos, allowed)
        count = int(got[2])
        rid = np.asarray(got[1]).ravel().astype(np.int64)[:max(count, 0)]
        ids, c64 = self.live_ids(), self.cosines(q)
        g = self.groups.get(src, NO_GROUP)
        try:
            for i in rid.tolist():
                if mode != "none" and i == src:
                    raise AssertionError(f"the source id {i} is returned under exclude={mode!r}")
                if mode == "file" and g != NO_GROUP and self.is_live(i) and self.groups.get(i, NO_GROUP) == g:
                    raise AssertionError(f"id {i} of the source's group {g} is returned under exclude='file'")
                if min_cos is not None and self.is_live(i) and not c64[np.searchsorted(ids, i)] > float(np.float32(min_cos)):
                    raise AssertionError(f"id {i} (float64 cos {c64[np.searchsorted(ids, i)]!r}) is not above min_cos {min_cos!r}")
            return self.check(q, k, got, allowed=elig)
        except AssertionError as e:
            raise AssertionError(f"similar from id {src}, exclude={mode!r}, min_cos={min_cos!r}: {e}") from None

    def pick_min_cos(self, src) -> float:
        """A bound for a similar-chunk search from `src` that float64 can place: the midpoint (rounded to f32) of the widest
        gap between adjacent float64 cosines among the source's 30 best live rows; the gap must be wider than 4 * tol."""
        c = np.sort(self.cosines(self.rows[int(src)]))[::-1][:30]
        if len(c) < 2:
            raise AssertionError(f"pick_min_cos: id {src} has fewer than two live rows to cut between")
        gaps = c[:-1] - c[1:]
        n = int(gaps.argmax())
        if not gaps[n] > 4 * self.tol:
            raise AssertionError(f"pick_min_cos: the widest gap among the 30 best of id {src} is {gaps[n]!r}, not above 4 * tol")
        return float(np.float32((c[n] + c[n + 1]) / 2))

    def _weights(self, weights) -> np.ndarray:
        """Per live id: weights[class] as f32; 1 for NO_CLASS, a class past the table, an empty table."""
        wt = np.zeros(0, np.float32) if weights is None else np.asarray(weights, np.float32).ravel()
        key = ("w", wt.tobytes())
        if key not in self._cache:
            w = np.ones(len(self.live_ids()), np.float32)
            for n, i in enumerate(self.live_ids().tolist()):
                c = self.classes.get(i, NO_CLASS)
                if c != NO_CLASS and c < len(wt):
                    w[n] = wt[c]
            self._cache[key] = w
        return self._cache[key]

    @staticmethod
    def score_of(cos32, w32):
        """b = f32(cos_to_score(cos) * w) as the boosted search states it: s = 1 - (1 - cos) * 0.5 in f32, one more rounding."""
        cos32 = np.asarray(cos32, np.float32)
        s = np.float32(1.0) - (np.float32(1.0) - cos32) * np.float32(0.5)
        return (s * np.asarray(w32, np.float32)).astype(np.float32)

    def boosted_topk(self, q, k, weights, allowed=None):
        """The model's own answer to search_raw(q, k, class_weights=weights) -> (score, cos, ids, count)."""
        if not self.built:
            raise AssertionError(NOT_BUILT)
        ids, c64, elig, w = self.live_ids(), self.cosines(q), self._eligible(allowed), self._weights(weights)
        c32 = c64.astype(np.float32)
        b = self.score_of(c32, w)
        order = [n for n in np.lexsort((ids, -b)) if elig[n]][:k]
        score, cos, rid = np.zeros(k, np.float32), np.zeros(k, np.float32), np.full(k, NO_ID, np.uint32)
        score[:len(order)], cos[:len(order)], rid[:len(order)] = b[order], c32[order], ids[order]
        return score, cos, rid, len(order)

    def check_boosted(self, q, k, got, weights, allowed=None) -> float:
        """Judges got = (score, cos, ids, count) of a boosted search for q (or variants q [nq, dim], merged) under the
        class-weight table `weights`; -> the largest |returned cos - float64 cos|."""
        if not self.built:
            raise AssertionError(NOT_BUILT)
        tol = self.tol
        score = np.asarray(got[0], np.float32).ravel()
        cos = np.asarray(got[1], np.float32).ravel()
        rid_all = np.asarray(got[2]).ravel().astype(np.int64)
        count = int(got[3])
        ids, c64, elig, w = self.live_ids(), self.cosines(q), self._eligible(allowed), self._weights(weights)

        def need(ok, msg):
            if not ok:
                raise AssertionError(f"{msg} (boosted, k={k}, allowed={'all' if allowed is None else len(list(allowed))}, "
                                     f"weights={np.asarray([] if weights is None else weights).tolist()}, count={count}, "
                                     f"ids={rid_all[:min(count, 12)].tolist()})")

        need(count == min(k, int(elig.sum())), f"count {count}, expected min(k, {int(elig.sum())})")
        need(len(cos) >= k and len(rid_all) >= k and len(score) >= k, "the answer is shorter than k")
        need((rid_all[count:k] == NO_ID).all() and (cos[count:k] == 0.0).all() and (score[count:k] == 0.0).all(),
             "the tail behind count is not empty slots")
        rid, rc, rs = rid_all[:count], cos[:count], score[:count]
        if count == 0:
            return 0.0
        need(len(set(rid.tolist())) == count, "an id is returned twice")
        pos = np.minimum(np.searchsorted(ids, rid), len(ids) - 1) if len(ids) else np.zeros(count, np.int64)
        live = (ids[pos] == rid) if len(ids) else np.zeros(count, bool)
        for i in rid[~live].tolist():
            need(False, f"id {i} {self._why_not_live(i)}")
        need(elig[pos].all(), f"ids outside the allowed set: {rid[~elig[pos]].tolist()[:5]}")
        err = np.abs(rc.astype(np.float64) - c64[pos])
        worst = int(err.argmax())
        need(err[worst] <= tol, f"cos of id {int(rid[worst])} is {rc[worst]!r}, float64 says {c64[pos][worst]!r} (tol {tol:.2e})")
        want = self.score_of(rc, w[pos])
        off = np.flatnonzero(want.view(np.uint32) != rs.view(np.uint32))
        if len(off):
            n = int(off[0])
            need(False, f"score of id {int(rid[n])} is {rs[n]!r}, f32(cos_to_score({rc[n]!r}) * {w[pos][n]!r}) is {want[n]!r}")
        bad = ~((rs[:-1] > rs[1:]) | ((rs[:-1] == rs[1:]) & (rid[:-1] < rid[1:])))
        need(not bad.any(), f"not sorted by (score desc, id) at position {int(bad.argmax()) if bad.any() else -1}")
        returned = np.zeros(len(ids), bool)
        returned[pos] = True
        omitted = elig & ~returned
        if omitted.any():
            w64 = w.astype(np.float64)
            s64 = (1.0 + c64) / 2.0 * w64
            slack = w64 * tol / 2.0 + 3.0 * 2.0 ** -24 * np.maximum(1.0, w64)
            miss = omitted & ~((s64 <= float(rs[-1]) + slack) if count == k else np.zeros(len(ids), bool))
            if miss.any():
                n = int(np.flatnonzero(miss)[s64[miss].argmax()])
                need(False, f"id {int(ids[n])} (float64 score {s64[n]!r}, weight {w[n]!r}) is left out; the last returned score is {rs[-1]!r}")
        # byte-identical rows of one class: ascending id, never a higher one in place of an eligible lower one
        cls, dup_members = self._dup_class(), self._dup_members()
        for c in (set(cls[pos].tolist()) & set(dup_members) if dup_members else ()):
            members = dup_members[c]
            for x, kx in zip(rid.tolist(), [self.classes.get(int(i), NO_CLASS) for i in rid.tolist()]):
                if cls[np.searchsorted(ids, x)] != c:
                    continue
                for n in members:
                    y = int(ids[n])
                    if y < x and elig[n] and not returned[n] and self.classes.get(y, NO_CLASS) == kx:
                        need(False, f"duplicate id {x} is returned while the identical row of lower id {y} (same class) is left out")
        return float(err.max())


# ======================================================================================================
# The walk
# ======================================================================================================

def rows_of(op, dim: int) -> np.ndarray:
    """The rows of an insert operation: n synthetic rows; the last `dups` are exact copies of the first `dups`; with
    `zero`, row 1 has no magnitude; with `clones` (extended walks), some rows are near-copies of others (clone_layout)."""
    rows = synth_rows(op["seed"], op["first"], op["n"], dim)
    d = op.get("dups", 0)
    if d:
        rows[op["n"] - d:] = rows[:d]
    if op.get("zero"):
        rows[1] = 0.0
    for src, dst, t in clone_layout(op)[0]:
        plant(rows, src, dst, t)
    return rows


# the target cosines of the clones of one planted set: four inside the f16 filter's margin (1e-3) around BOUND, where only
# the exact refine can place a pair, and outside the judge's band (4.7e-5 at dim 384), so float64 decides them
LADDER = (0.999, 0.97, float(BOUND) + 5e-4, float(BOUND) + 2e-4, float(BOUND) - 2e-4, float(BOUND) - 5e-4, 0.85)
CHAIN = 0.93  # b from a and c from b at 0.93: the ends come out near 0.865, so a-b and b-c are edges above BOUND, a-c is not


def plant(rows, a: int, b: int, t: float):
    """rows[b] becomes a near-copy of rows[a] at cosine t, in float64: direction t u + sqrt(1 - t^2) w with u the unit
    rows[a] and w the unit part of rows[b] orthogonal to it; rows[b] keeps its norm."""
    u = rows[a].astype(np.float64)
    u /= np.linalg.norm(u)
    x = rows[b].astype(np.float64)
    w = x - (x @ u) * u
    w /= np.linalg.norm(w)
    rows[b] = (np.linalg.norm(x) * (t * u + np.sqrt(1.0 - t * t) * w)).astype(np.float32)


def clone_layout(op):
    """Where an insert operation with the key `clones` (a seed) plants near-copies, as row numbers of the insert ->
    (plants, chains): plants = [(source row, overwritten row, target cosine)] in planting order, chains = [(a, b, c)].
    One set per 256 rows (at least one), each in a segment of its own, clear of the exact duplicates (the first and last
    three rows) and the zero row (row 1).  A set: the two closest clones (0.999, 0.97) right behind their sources — two
    sources five rows apart cannot both end a group of 16 consecutive ids, so at least one pair shares a group; the chain in
    three adjacent rows; the other five clones of LADDER 17 rows or more from their sources, so in another group."""
    seed, n = op.get("clones"), op["n"]
    if not seed:
        return [], []
    assert n >= 64
    sets = max(1, n // 256)
    seg = (n - 8) // sets
    plants, chains = [], []
    for s in range(sets):
        rng = np.random.default_rng([int(seed), int(op["first"]), s])
        lo = 4 + s * seg
        p = lo + int(rng.integers(0, seg - 35 + 1))
        far = p + 28 + np.sort(rng.choice(lo + seg - (p + 28), 5, replace=False))
        plants += [(p, p + 1, LADDER[0]), (p + 5, p + 6, LADDER[1])]
        plants += [(src, int(dst), t) for src, dst, t in zip((p + 2, p + 3, p + 4, p + 7, p + 11), far, LADDER[2:])]
        plants += [(p + 8, p + 9, CHAIN), (p + 9, p + 10, CHAIN)]
        chains.append((p + 8, p + 9, p + 10))
    return plants, chains


class Planted:
    """The ids of what the walk's inserts planted, kept in step with the model: `after(op, ids, model)` follows each
    operation.  clones = [(source id, clone id, target cosine)] (the chains' two links included), chains = [(a, b, c)]."""

    def __init__(self):
        self.clones, self.chains = [], []

    def after(self, op, ids, model):
        kind = op["op"]
        if kind == "clear":  # the ids start over
            self.clones, self.chains = [], []
        elif kind == "reopen":  # ids issued after the last build are issued again, to other rows
            self.clones = [c for c in self.clones if max(c[:2]) < model.next_id]
            self.chains = [c for c in self.chains if max(c) < model.next_id]
        elif kind == "insert" and op.get("clones"):
            plants, chains = clone_layout(op)
            self.clones += [(ids[0] + a, ids[0] + b, t) for a, b, t in plants]
            self.chains += [(ids[0] + a, ids[0] + b, ids[0] + c) for a, b, c in chains]

    def live_clones(self, model):
        return [c for c in self.clones if model.is_live(c[0]) and model.is_live(c[1])]


def resolve(op, model: StoreModel):
    """The concrete arguments of `op` for the state `model` is in (before the operation): insert -> rows; delete ->
    ids; scope -> ids; groups -> (ids, groups); else None."""
    kind = op["op"]
    if kind == "insert":
        return rows_of(op, model.dim)
    if kind == "delete":
        live = model.live_ids()
        rng = np.random.default_rng(op.get("seed", 0))
        pick = op["pick"]
        if pick == "all":
            return live.tolist()
        if pick == "frac":
            return np.sort(rng.choice(live, int(len(live) * op["frac"]), replace=False)).tolist()
        if pick == "keep":  # all but `keep` random survivors
            return np.sort(rng.choice(live, max(0, len(live) - op["keep"]), replace=False)).tolist()
        if pick == "shard":
            return [int(i) for i in live if model.shard_of(int(i)) == op["shard"]]
        if pick == "stale":  # reclaimed, never issued, below id_base: each counts 0
            ids = sorted(model.reclaimed)[:: max(1, len(model.reclaimed) // 5)][:5]
            ids += [model.next_id + 3, model.next_id + 1000]
            if model.id_base:
                ids += [model.id_base - 1, 0]
            return ids
        raise ValueError(pick)
    if kind == "scope":
        rng = np.random.default_rng(op.get("seed", 0))
        issued = np.arange(model.id_base, model.next_id)
        if op["pick"] == "half":
            return np.sort(rng.choice(issued, len(issued) // 2, replace=False))
        if op["pick"] == "issued":
            return issued
        if op["pick"] == "future":  # the last few issued ids and 400 that are not issued yet
            return np.arange(max(model.id_base, model.next_id - 10), model.next_id + 400)
        raise ValueError(op["pick"])
    if kind == "groups":  # about 16 ids per group; "new": the ids no groups operation has seen yet
        lo = model.id_base if op["which"] == "all" else op["from"]
        ids = np.arange(lo, model.next_id)
        return ids, (ids - model.id_base) // 16
    if kind == "classes":  # class (id - id_base) % 5, every seventh id left without one; the ids of the groups op beside it
        lo = model.id_base if op["which"] == "all" else op["from"]
        ids = np.arange(lo, model.next_id)
        off = ids - model.id_base
        return ids, np.where(off % 7 == 6, NO_CLASS, off % 5)
    return None


def apply(op, args, model: StoreModel):
    """Performs `op` (with `args` = resolve(op, model)) on the model -> what the store's call is to return."""
    kind = op["op"]
    if kind == "insert":
        return model.insert(args)
    if kind == "delete":
        return model.delete(args)
    if kind == "build":
        return model.build()
    if kind == "clear":
        return model.clear()
    if kind == "reopen":
        return model.reopen()
    if kind == "groups":
        return model.set_groups(*args)
    if kind == "classes":
        return model.set_classes(*args)
    if kind == "scope":
        return None
    raise ValueError(kind)


def new_model(walk) -> StoreModel:
    h = walk[0]
    assert h["op"] == "open"
    return StoreModel(h["dim"], h["id_base"], h["shards"], h["stripe"])


class _Plan:
    """make_walk's pen: appends operations and keeps a model in step, so sizes can be aimed at."""

    def __init__(self, seed, dim, id_base, shards, stripe, extended=False):
        self.extended = extended
        self.ops = [{"op": "open", "dim": dim, "id_base": id_base, "shards": shards, "stripe": stripe}]
        self.m = StoreModel(dim, id_base, shards, stripe)
        self.seed, self.n_ops, self.first, self.grouped_to = seed, 0, 0, id_base

    def do(self, **op):
        self.n_ops += op["op"] != "classes"  # (the seeds of the deletes and scopes are those of the plain walk)
        if op["op"] in ("delete", "scope"):
            op.setdefault("seed", self.seed * 1000 + self.n_ops)
        apply(op, resolve(op, self.m), self.m)
        self.ops.append(op)

    def insert(self, n, dups=0, zero=False):
        more = {"clones": 8100 + self.seed} if self.extended and n >= 64 else {}
        self.do(op="insert", n=int(n), seed=7000 + self.seed, first=self.first, dups=dups, zero=zero, **more)
        self.first += int(n)

    def to(self, stored, **kw):
        self.insert(stored - self.m.stored_rows(), **kw)

    def groups(self, which):
        span = {"from": self.grouped_to} if which == "new" else {}
        self.do(op="groups", which=which, **span)
        if self.extended:
            self.do(op="classes", which=which, **span)
        self.grouped_to = self.m.next_id

    def build(self):
        self.do(op="build")


def make_walk(seed: int, dim: int, sharded: bool, extended: bool = False):
    """A deterministic list of about 40 operations (module docstring).  The first entry describes the store to open.
    extended: the same operations in the same order with the same sizes, and for the kinds that start from stored rows a
    `classes` operation beside every `groups` operation and planted near-copies (`clones`) in every insert of 64 rows or
    more."""
    rng = np.random.default_rng([seed, dim, int(sharded)])
    r = lambda lo, hi: int(rng.integers(lo, hi + 1))
    if sharded:
        p = _Plan(seed, dim, 0, 3, 64, extended)
        p.insert(r(90, 120))
        p.do(op="scope", name="future", pick="future")
        p.do(op="scope", name="early", pick="half")
        p.build()
        p.to(r(600, 800), dups=3, zero=True)
        p.build()
        p.do(op="delete", pick="frac", frac=0.03)
        p.build()                                   # tombstones stay
        p.to(r(1900, 2200))
        p.build()
        p.do(op="delete", pick="frac", frac=0.4)
        p.build()                                   # every shard reclaims
        p.do(op="delete", pick="stale")
        p.insert(r(40, 60))
        p.build()
        p.insert(r(20, 40))
        p.insert(r(20, 40), dups=2, zero=True)
        p.build()
        p.do(op="delete", pick="shard", shard=r(0, 2))
        p.build()                                   # one shard holds no row, the others do
        p.insert(r(250, 350))
        p.build()
        p.do(op="delete", pick="frac", frac=0.3)
        p.build()                                   # a second reclaim over compacted shards
        p.do(op="reopen")
        p.do(op="scope", name="late", pick="half")
    else:
        p = _Plan(seed, dim, 1000 if seed % 2 else 0, 1, 1 << 32, extended)
        p.insert(r(70, 120))
        p.do(op="scope", name="future", pick="future")
        p.do(op="scope", name="early", pick="half")
        p.build()                                   # below 128
        p.to(r(300, 700), dups=3, zero=True)
        p.groups("all")
        p.build()
        p.do(op="delete", pick="frac", frac=r(3, 8) / 100)
        p.build()                                   # tombstones stay
        p.to(1024)
        p.build()
        p.insert(1)
        p.build()                                   # 1,025
        p.to(1152 + r(0, 100))
        p.build()
        p.to(3200 + r(0, 120))
        p.build()                                   # past phase 0 of the filter: the int8 copy serves
        p.do(op="delete", pick="frac", frac=r(42, 50) / 100)
        p.build()                                   # the first reclaim, down through 2,048
        p.do(op="delete", pick="stale")
        p.insert(r(30, 50))
        p.build()
        p.insert(r(20, 40))
        p.insert(r(20, 40), dups=2, zero=True)
        p.groups("new")
        p.build()
        p.do(op="scope", name="late", pick="half")
        p.do(op="delete", pick="keep", keep=r(1030, 1140))
        p.build()                                   # a second reclaim, over a compacted index, down through 1,152
        p.do(op="delete", pick="keep", keep=r(800, 900))
        p.build()                                   # down through 1,025 and 1,024
        p.do(op="delete", pick="keep", keep=r(60, 110))
        p.build()                                   # down through 128
        p.do(op="reopen")
        p.groups("all")
        p.do(op="scope", name="reopened", pick="half")
    # every row deleted: in memory, then across a reopening
    p.do(op="delete", pick="all")
    p.build()
    p.insert(r(130, 180), dups=2, zero=True)
    p.build()
    p.do(op="delete", pick="all")
    p.build()
    p.do(op="reopen")
    p.do(op="scope", name="spent", pick="issued")
    p.insert(r(150, 250))
    if not sharded:
        p.groups("all")
    p.build()
    p.do(op="clear")
    p.insert(r(150, 300), dups=2, zero=True)
    if not sharded:
        p.groups("all")
    p.build()
    return p.ops


def required_coverage(walk) -> set:
    """The states a walk of this kind must reach (the keys of walk_coverage that must be True)."""
    h = walk[0]
    need = {"tombstone_build", "reclaim_build", "reclaim_over_compacted", "append_after_reclaim_then_build",
            "appends_after_reclaim_without_build", "delete_reclaimed", "delete_never_issued", "emptied_then_refilled",
            "clear_then_insert", "reopen_after_reclaim", "reopen_emptied", "scope_before_reclaim_used_after",
            "scope_future_ids_issued", "dups_and_zero_checked"}
    if h["id_base"]:
        need.add("delete_below_base")
    if h["shards"] == 1:
        need |= {"groups_before_reclaim_used_after", "appended_after_groups_assigned_later", "at_1024", "at_1025"}
        need |= {f"up_{e}_by_append" for e in EDGES} | {f"down_{e}_by_reclaim" for e in EDGES}
    else:
        need.add("shard_emptied_then_refilled")
    return need


def walk_coverage(walk) -> dict:
    """Runs the walk on the model alone -> {state: reached}.  A "checked state" is the state after a build or a
    reopening that left the index built: there a test searches."""
    m = new_model(walk)
    cov = {k: False for k in required_coverage(walk) | {"delete_below_base"}}
    scopes = {}            # name -> (ids, had unissued ids, reclaims seen at creation)
    reclaims = 0
    since_reclaim = None   # operations since the last reclaiming build: "i" insert, "b" build
    emptied = False        # a reclaim left no row while ids are spent; then an insert arrived ("refill")
    refill = False
    shard_emptied, shard_refill = set(), False
    groups_at_reclaims = None
    appended_after_groups = None
    cleared = False
    last_checked = None
    appended_only = True   # between two checked states: only appends (no reclaim) changed the stored count
    for op in walk[1:]:
        kind = op["op"]
        args = resolve(op, m)
        if kind == "delete":
            for i in args:
                if i < m.id_base:
                    cov["delete_below_base"] = True
                elif i >= m.next_id:
                    cov["delete_never_issued"] = True
                elif i in m.reclaimed:
                    cov["delete_reclaimed"] = True
        if kind == "scope":
            scopes[op["name"]] = (args, bool(len(args)) and int(args.max()) >= m.next_id, reclaims)
        if kind == "groups":
            if appended_after_groups is not None and len(args[0]) and int(args[0].max()) >= appended_after_groups:
                cov["appended_after_groups_assigned_later"] = True
            groups_at_reclaims, appended_after_groups = reclaims, None
        if kind == "insert":
            if m.groups and appended_after_groups is None:
                appended_after_groups = m.next_id
            if since_reclaim is not None:
                if since_reclaim.endswith("i"):
                    cov["appends_after_reclaim_without_build"] = True
                since_reclaim += "i"
            if emptied:
                refill = True
            if shard_emptied and any(m.shard_of(m.next_id + j) in shard_emptied for j in range(op["n"])):
                shard_refill = True
            if cleared:
                cov["clear_then_insert"] = True
        if kind == "clear":
            cleared = True
            emptied = refill = False
            shard_emptied, shard_refill = set(), False
            since_reclaim, groups_at_reclaims, appended_after_groups = None, None, None
        if kind == "reopen":
            scopes = {}
            groups_at_reclaims = None
            if any(m.compacted):
                cov["reopen_after_reclaim"] = True
            if emptied and not refill:
                cov["reopen_emptied"] = True
        was_compacted = list(m.compacted)
        before = [len(s) for s in m.stored]
        out = apply(op, args, m)
        if kind in ("build", "reopen"):
            reclaimed_now = kind == "build" and out
            if kind == "reopen":  # the loader's build reclaims what the file still names as removed
                reclaimed_now = any(m.compacted)
                was_compacted = [False] * m.shards
            if reclaimed_now:
                reclaims += 1
                since_reclaim = ""
                appended_only = False
                if kind == "build" and any(w and len(s) < b for w, s, b in zip(was_compacted, m.stored, before)):
                    cov["reclaim_over_compacted"] = True
                cov["reclaim_build"] = True
                if m.stored_rows() == 0 and m.next_id > m.id_base:
                    emptied, refill = True, False
                shard_emptied = {s for s in range(m.shards) if m.compacted[s] and not m.stored[s]} if m.shards > 1 else set()
            elif kind == "build":
                if any(i in m.removed for s in m.stored for i in s):
                    cov["tombstone_build"] = True
                if since_reclaim is not None:
                    if since_reclaim == "i":
                        cov["append_after_reclaim_then_build"] = True
                    since_reclaim += "b"
                if emptied and refill:
                    cov["emptied_then_refilled"] = True
                    emptied = refill = False
                if shard_refill:
                    cov["shard_emptied_then_refilled"] = True
                    shard_emptied, shard_refill = set(), False
        if kind in ("build", "reopen") and m.built:  # a checked state
            for ids, future, at in scopes.values():
                if reclaims > at:
                    cov["scope_before_reclaim_used_after"] = True
                if future and m.next_id > int(ids.min()) + 10:
                    cov["scope_future_ids_issued"] = True
            if groups_at_reclaims is not None and reclaims > groups_at_reclaims and m.groups:
                cov["groups_before_reclaim_used_after"] = True
            if m.has_dups_and_zero():
                cov["dups_and_zero_checked"] = True
            s = m.stored_rows()
            if s in (1024, 1025):
                cov[f"at_{s}"] = True
            if last_checked is not None:
                for e in EDGES:
                    if last_checked < e <= s and appended_only and f"up_{e}_by_append" in cov:
                        cov[f"up_{e}_by_append"] = True
                    if s < e <= last_checked and reclaimed_now and f"down_{e}_by_reclaim" in cov:
                        cov[f"down_{e}_by_reclaim"] = True
            last_checked, appended_only = s, True
        if kind in ("clear",):
            last_checked, appended_only = 0, True
    return cov


def extended_coverage(walk) -> dict:
    """Runs an extended walk on the model alone -> what its checked states hold for the kinds that start from stored rows:
    full_states (dim 384: states with a pair above BOUND inside one group, one across groups, a component of three whose
    ends are not an edge, a pair within 1e-3 below BOUND and one within 1e-3 above), chain_cut (states after a chain's
    middle was deleted while both ends live), classes_before_reclaim, appended_after_classes, checked (all checked states),
    ambiguous (the most live pairs within tol of BOUND at any checked state; dim 384) and min_cos_failed (checked states
    where pick_min_cos finds no gap for the first stored live id)."""
    m = new_model(walk)
    planted = Planted()
    out = {"full_states": 0, "chain_cut": 0, "classes_before_reclaim": 0, "appended_after_classes": 0, "checked": 0,
           "ambiguous": 0, "min_cos_failed": 0}
    reclaims, classes_at, classes_to = 0, None, None
    b = float(BOUND)
    for op in walk[1:]:
        kind = op["op"]
        args = resolve(op, m)
        res = apply(op, args, m)
        planted.after(op, res if kind == "insert" else None, m)
        if kind == "classes":
            classes_at, classes_to = reclaims, m.next_id
        if kind in ("clear", "reopen"):
            classes_at = classes_to = None
        if (kind == "build" and res) or (kind == "reopen" and any(m.compacted)):
            reclaims += 1
        if not (kind in ("build", "reopen") and m.built):
            continue
        out["checked"] += 1
        if m.classes and classes_at is not None and reclaims > classes_at:
            out["classes_before_reclaim"] += 1
        if m.classes and classes_to is not None and len(m.live_ids()) and int(m.live_ids().max()) >= classes_to:
            out["appended_after_classes"] += 1
        if any(m.is_live(a) and m.is_live(c) and not m.is_live(mid) and mid < m.next_id for a, mid, c in planted.chains):
            out["chain_cut"] += 1
        if len(m.live_ids()) >= 2:
            try:
                m.pick_min_cos(m.stored_live()[0])
            except AssertionError:
                out["min_cos_failed"] += 1
        if m.dim != 384:
            continue
        out["ambiguous"] = max(out["ambiguous"], m.ambiguous_pairs(BOUND))
        a, bb, c = m._pair_list(BOUND, False)
        ga = np.array([m.groups.get(int(i), NO_GROUP) for i in a], np.int64)
        gb = np.array([m.groups.get(int(i), NO_GROUP) for i in bb], np.int64)
        inside = bool(((ga == gb) & (ga != NO_GROUP)).any())
        across = bool(((ga != gb) & (ga != NO_GROUP) & (gb != NO_GROUP)).any())
        just_above = bool((c < b + 1e-3).any())
        lo = m._pair_list(np.float32(b - 1e-3), False)[2]
        just_below = bool((lo <= b).any())
        edges = set(zip(a.tolist(), bb.tolist()))
        three = any((x, y) in edges and (y, z) in edges and (x, z) not in edges and m._components(BOUND, False)[x] ==
                    m._components(BOUND, False)[z] for x, y, z in planted.chains if all(m.is_live(i) for i in (x, y, z)))
        out["full_states"] += inside and across and just_above and just_below and three
    return out
