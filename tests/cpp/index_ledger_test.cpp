// The host ledger of an index (codesearch_amd/csrc/index_ledger.hpp) on the CPU, against a model written the slow way:
// the stored rows are a vector of {id, alive} in storage order, the row of an id is a linear search, a reclaim erases the
// dead and the next id is a counter.  The model shares no code with the header.
//   index_ledger_test -> the checks below, "index ledger ok"
// Random walks: 240 seeds x 60 operations; seed s walks id_base {0, 640, 0xFFFFFE00}[s % 3] with dead_pct
// {0, 10, 50}[(s / 3) % 3] (each of the nine pairs 26 or 27 times).  Operations: append of 0..70 rows, remove of a mixed
// list, build (a reclaim when the ledger wants one), set_groups (sometimes followed by the upload a grouped search does),
// clear.  After every operation everything the ledger answers is compared with the model.  Over the seed set the walks must
// reach a reclaim that leaves no row, an append after it, and a remove of a reclaimed id (asserted at the end).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../codesearch_amd/csrc/index_ledger.hpp"

using namespace cs;

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

constexpr uint32_t NO_GROUP = 0xFFFFFFFFu;
constexpr int kSeeds = 240, kOps = 60;

struct ModelRow {
    uint32_t id;
    bool alive;
};

struct Model {
    uint64_t id_base;
    uint64_t next;  // the next id, a counter
    bool reclaimed = false;
    std::vector<ModelRow> rows;
    std::vector<uint32_t> group;  // of every issued id, by id - id_base

    explicit Model(uint32_t base) : id_base(base), next(base) {}

    uint64_t row_of(uint64_t id) const {
        for (size_t r = 0; r < rows.size(); ++r)
            if (rows[r].id == id) return r;
        return kNoRow;
    }
    uint64_t dead() const {
        uint64_t n = 0;
        for (const ModelRow& r : rows) n += !r.alive;
        return n;
    }
    bool fits(uint64_t n) const { return next + n <= 0xFFFFFFFFull; }
    void append(uint64_t n) {
        for (uint64_t i = 0; i < n; ++i) {
            rows.push_back(ModelRow{(uint32_t)next++, true});
            group.push_back(NO_GROUP);
        }
    }
    uint64_t remove(const std::vector<uint32_t>& ids) {
        uint64_t n = 0;
        for (uint32_t id : ids) {
            const uint64_t r = row_of(id);
            if (r == kNoRow || !rows[r].alive) continue;
            rows[r].alive = false;
            ++n;
        }
        return n;
    }
    bool wants_reclaim(uint32_t pct) const { return pct && dead() && dead() * 100 >= (uint64_t)pct * rows.size(); }
    void reclaim() {
        rows.erase(std::remove_if(rows.begin(), rows.end(), [](const ModelRow& r) { return !r.alive; }), rows.end());
        reclaimed = true;
    }
    void clear() { *this = Model((uint32_t)id_base); }
};

// the device copy of the group table as ensure_groups keeps it (index.hip), with a vector for the device memory
struct ShadowDevice {
    std::vector<uint32_t> mem;  // its size is the capacity
    uint64_t valid = 0;         // entries the last upload left equal to the host's

    void upload(GroupTable& g) {
        if (g.assigned() == 0) return;
        const uint64_t n = g.size();
        if (n > mem.size()) {
            mem.assign((size_t)std::max<uint64_t>(n, 2 * mem.size()), 0xDEADBEEFu);
            g.uploaded(0);
        }
        uint64_t lo = 0, hi = 0;
        if (g.pending(&lo, &hi)) {
            CHECK(hi <= n);
            for (uint64_t e = lo; e < hi && e < n; ++e) mem[(size_t)e] = g.data()[e];
        }
        g.uploaded(n);
        valid = n;
        for (uint64_t e = 0; e < n; ++e) CHECK(mem[(size_t)e] == g.data()[e]);
    }
    // pending() names every entry the device copy does not hold as the host does
    void check_pending(const GroupTable& g) const {
        uint64_t lo = 0, hi = 0;
        const bool any = g.pending(&lo, &hi);
        for (uint64_t e = 0; e < g.size(); ++e) {
            const bool differs = e >= valid || e >= mem.size() || mem[(size_t)e] != g.data()[e];
            if (differs) CHECK(any && lo <= e && e < hi);
        }
    }
    void clear() { valid = 0; }  // (cs_index_clear: the device table keeps its room)
};

static bool bit(const std::vector<uint32_t>& w, uint64_t i) { return ((w[(size_t)(i / 32)] >> (i % 32)) & 1u) != 0; }

static void compare(const IndexLedger& l, const GroupTable& g, const Model& m, const ShadowDevice& dev, std::mt19937_64& rng) {
    // every counter
    CHECK(l.id_base() == m.id_base);
    CHECK(l.next_id() == m.next);
    CHECK(l.issued_ids() == m.next - m.id_base);
    CHECK(l.stored() == m.rows.size());
    CHECK(l.removed() == m.dead());
    CHECK(l.live() == m.rows.size() - m.dead());
    CHECK(l.compacted() == m.reclaimed);
    // the row of every id around the issued ones
    const int64_t lo = std::max<int64_t>(0, (int64_t)m.id_base - 2), hi = std::min<int64_t>(0xFFFFFFFFll, (int64_t)m.next + 2);
    for (int64_t id = lo; id <= hi; ++id) {
        CHECK(l.row_of((uint32_t)id) == m.row_of((uint64_t)id));
        CHECK(l.issued((uint32_t)id) == ((uint64_t)id >= m.id_base && (uint64_t)id < m.next));
    }
    CHECK(l.row_of(0xFFFFFFFFu) == kNoRow && !l.issued(0xFFFFFFFFu));
    if (failures) return;  // (the raw reads below trust the counters)
    // the id table
    if (l.compacted())
        for (size_t r = 0; r < m.rows.size(); ++r) CHECK(l.ids_data()[r] == m.rows[r].id);
    // the bitmap: a bit per stored row, nothing set past them
    const std::vector<uint32_t>& words = l.dead_words();
    CHECK(words.size() == (m.rows.size() + 31) / 32);
    if (words.size() == (m.rows.size() + 31) / 32)
        for (uint64_t i = 0; i < (uint64_t)words.size() * 32; ++i) CHECK(bit(words, i) == (i < m.rows.size() && !m.rows[(size_t)i].alive));
    // runs of consecutive ids
    for (int t = 0; t < 8; ++t) {
        const uint64_t rel = rng() % (m.next - m.id_base + 2), n = rng() % 40;
        uint64_t row = rel < m.next - m.id_base ? m.row_of(m.id_base + rel) : kNoRow, len = 0;
        if (row != kNoRow)
            while (len < n && row + len < m.rows.size() && m.rows[(size_t)(row + len)].id == m.id_base + rel + len) ++len;
        const IndexLedger::Run run = l.id_run(rel, n);
        CHECK(run.row == row);
        if (row != kNoRow) CHECK(run.len == len);
    }
    // the survivors, chunk by chunk
    for (uint64_t chunk : {(uint64_t)1, (uint64_t)7, (uint64_t)m.rows.size()}) {
        std::vector<uint64_t> got;
        std::vector<uint32_t> out;
        for (uint64_t c0 = 0; chunk && c0 < m.rows.size(); c0 += chunk) {
            out.clear();
            l.survivors(c0, std::min<uint64_t>(m.rows.size(), c0 + chunk), out);
            for (uint32_t r : out) got.push_back(c0 + r);
        }
        std::vector<uint64_t> want;
        for (size_t r = 0; r < m.rows.size(); ++r)
            if (m.rows[r].alive) want.push_back(r);
        CHECK(got == want);
    }
    // the groups
    uint64_t assigned = 0;
    CHECK(g.size() <= m.group.size());
    for (size_t e = 0; e < m.group.size(); ++e) {
        CHECK((e < g.size() ? g.data()[e] : NO_GROUP) == m.group[e]);
        assigned += m.group[e] != NO_GROUP;
    }
    CHECK(g.assigned() == assigned);
    dev.check_pending(g);
}

// The reclaim as index.hip's compact() drives it: the survivors chunk by chunk (where the device moves them to row dst),
// the commit only once every chunk has moved, and then exactly the live rows have.
static void reclaim_as_compact(IndexLedger& l, uint64_t chunk) {
    const uint64_t live = l.live(), stored = l.stored();
    uint64_t dst = 0;
    std::vector<uint32_t> idx;
    for (uint64_t c0 = 0; c0 < stored; c0 += chunk) {
        idx.clear();
        l.survivors(c0, std::min(stored, c0 + chunk), idx);
        dst += idx.size();
    }
    CHECK(dst == live && l.stored() == stored);
    l.commit_reclaim();
    CHECK(l.stored() == live && l.removed() == 0);
}

struct Coverage {
    int reclaims = 0, emptied = 0, appends_after_emptied = 0, removes_of_reclaimed = 0, full = 0, bad_group_ids = 0;
};

static void walk(int seed, Coverage& cov) {
    static const uint32_t bases[] = {0u, 640u, 0xFFFFFE00u}, pcts[] = {0u, 10u, 50u};
    const uint32_t base = bases[seed % 3], pct = pcts[(seed / 3) % 3];
    std::mt19937_64 rng((uint64_t)seed * 7919 + 1);
    IndexLedger l(base);
    GroupTable g;
    Model m(base);
    ShadowDevice dev;
    bool emptied = false;  // the last reclaim left no row and nothing was appended or cleared since
    for (int op = 0; op < kOps; ++op) {
        const uint64_t issued = m.next - m.id_base;
        switch (rng() % 8) {
        case 0: case 1: case 2: {  // append
            const uint64_t n = rng() % 71;
            CHECK(l.can_append(n) == m.fits(n));
            if (!m.fits(n)) { ++cov.full; break; }
            CHECK(l.append(n) == m.next);
            m.append(n);
            if (emptied && n) { ++cov.appends_after_emptied; emptied = false; }
            break;
        }
        case 3: case 4: {  // remove: live, dead, reclaimed and never-issued ids, ids below id_base, 0xFFFFFFFF, duplicates
            std::vector<uint32_t> ids;
            if (rng() % 8 == 0) {  // every live row
                for (const ModelRow& r : m.rows)
                    if (r.alive) ids.push_back(r.id);
            }
            const int n = (int)(rng() % 50);
            for (int i = 0; i < n; ++i) {
                const uint64_t kind = rng() % 10;
                if (kind < 6 && issued) ids.push_back((uint32_t)(m.id_base + rng() % issued));  // live, dead or reclaimed
                else if (kind == 6) ids.push_back((uint32_t)std::min<uint64_t>(0xFFFFFFFFull, m.next + rng() % 5));
                else if (kind == 7) ids.push_back(m.id_base ? (uint32_t)(m.id_base - 1 - rng() % std::min<uint64_t>(m.id_base, 700)) : 0u);
                else if (kind == 8) ids.push_back(0xFFFFFFFFu);
                else if (!ids.empty()) ids.push_back(ids[(size_t)(rng() % ids.size())]);
            }
            for (uint32_t id : ids)
                if (id >= m.id_base && id < m.next && m.row_of(id) == kNoRow) ++cov.removes_of_reclaimed;
            CHECK(l.remove(ids.data(), ids.size()) == m.remove(ids));
            break;
        }
        case 5: {  // build
            CHECK(l.wants_reclaim(pct) == m.wants_reclaim(pct));
            if (!m.wants_reclaim(pct)) break;
            reclaim_as_compact(l, 1 + rng() % 97);
            m.reclaim();
            ++cov.reclaims;
            if (m.rows.empty()) { ++cov.emptied; emptied = true; }
            break;
        }
        case 6: {  // set_groups, then perhaps a grouped search's upload
            if (issued) {
                std::vector<uint32_t> ids, groups;
                const int n = 1 + (int)(rng() % 20);
                for (int i = 0; i < n; ++i) {
                    ids.push_back((uint32_t)(m.id_base + rng() % issued));
                    groups.push_back(rng() % 4 == 0 ? NO_GROUP : (uint32_t)(rng() % 6));
                }
                int64_t bad = -1;
                if (rng() % 6 == 0) {  // one id that was never issued: nothing changes
                    bad = (int64_t)(rng() % ids.size());
                    ids[(size_t)bad] = rng() % 2 && m.id_base ? (uint32_t)(m.id_base - 1) : (uint32_t)m.next;
                    ++cov.bad_group_ids;
                }
                CHECK(g.set(ids.data(), groups.data(), ids.size(), l) == bad);
                if (bad < 0)
                    for (size_t i = 0; i < ids.size(); ++i) m.group[(size_t)(ids[i] - m.id_base)] = groups[i];
            }
            if (rng() % 2) dev.upload(g);
            break;
        }
        case 7:  // clear (rare: it ends the history)
            if (rng() % 4) break;
            l.clear();
            g.clear();
            m.clear();
            dev.clear();
            emptied = false;
            break;
        }
        compare(l, g, m, dev, rng);
        if (failures) {
            std::printf("seed %d (id_base %u, dead_pct %u): first failure at operation %d\n", seed, base, pct, op);
            return;
        }
    }
}

// cs_index_build as far as the ledger goes
static void build(IndexLedger& l, uint32_t pct) {
    if (l.wants_reclaim(pct)) l.commit_reclaim();
}

// A reclaim that leaves no row must not return the index to the identity numbering: the ids issued so far stay spent.
static void check_emptied(uint32_t base) {
    IndexLedger l(base);
    CHECK(l.append(300) == base);
    build(l, 10);
    std::vector<uint32_t> all(300);
    for (uint32_t i = 0; i < 300; ++i) all[i] = base + i;
    CHECK(l.remove(all.data(), 300) == 300);
    build(l, 10);
    CHECK(l.stored() == 0 && l.live() == 0 && l.removed() == 0 && l.compacted());
    CHECK(l.next_id() == base + 300);
    CHECK(l.append(200) == base + 300);
    CHECK(l.row_of(base + 300) == 0 && l.row_of(base + 499) == 199);
    CHECK(l.row_of(base) == kNoRow && l.row_of(base + 299) == kNoRow);
    CHECK(l.next_id() == base + 500 && l.stored() == 200);
    if (failures) return;
    for (uint32_t i = 0; i < 200; ++i) CHECK(l.ids_data()[i] == base + 300 + i);
}

static void check_threshold() {
    for (uint32_t rows : {10u, 11u}) {
        IndexLedger l;
        l.append(rows);
        const uint32_t id = 3;
        CHECK(!l.wants_reclaim(10) && !l.wants_reclaim(0));  // nothing dead
        CHECK(l.remove(&id, 1) == 1);
        CHECK(l.wants_reclaim(10) == (rows == 10));  // 1 of 10 is 10 %, 1 of 11 is not
        CHECK(!l.wants_reclaim(0));                  // pct 0: never
        CHECK(l.wants_reclaim(1));
    }
}

static void check_id_space() {
    IndexLedger l(0xFFFFFE00u);
    CHECK(l.can_append(511) && !l.can_append(512));
    CHECK(l.append(511) == 0xFFFFFE00u);
    CHECK(l.next_id() == 0xFFFFFFFFu && !l.issued(0xFFFFFFFFu) && l.row_of(0xFFFFFFFEu) == 510);
    CHECK(l.can_append(0) && !l.can_append(1) && !l.can_append(2));
    IndexLedger z;
    CHECK(z.can_append(0xFFFFFFFFull) && !z.can_append(0x100000000ull));
}

static void check_runs_and_reclaimed() {
    IndexLedger l(640);
    l.append(100);
    CHECK(l.id_run(10, 50).row == 10 && l.id_run(10, 50).len == 50);  // the identity numbering: one run
    CHECK(l.id_run(90, 50).len == 10 && l.id_run(100, 1).row == kNoRow);
    const uint32_t hole[] = {640 + 20, 640 + 21, 640 + 21};
    CHECK(l.remove(hole, 3) == 2);  // the duplicate counts once
    CHECK(l.id_run(10, 50).len == 50);  // tombstoned rows are still stored
    l.commit_reclaim();
    CHECK(l.stored() == 98);
    IndexLedger::Run r = l.id_run(10, 50);
    CHECK(r.row == 10 && r.len == 10);  // up to the hole
    CHECK(l.id_run(20, 5).row == kNoRow && l.id_run(21, 5).row == kNoRow);
    r = l.id_run(22, 500);
    CHECK(r.row == 20 && r.len == 78);
    // an id after its reclaim: nothing to remove, nothing changes
    const std::vector<uint32_t> before = l.dead_words();
    CHECK(l.remove(hole, 3) == 0);
    CHECK(l.removed() == 0 && l.live() == 98 && l.dead_words() == before);
    // clear() returns to the identity numbering
    l.clear();
    CHECK(!l.compacted() && l.next_id() == 640 && l.stored() == 0 && l.dead_words().empty());
    CHECK(l.append(1) == 640 && l.row_of(640) == 0);
}

int main() {
    check_emptied(0);
    check_emptied(640);
    check_threshold();
    check_id_space();
    check_runs_and_reclaimed();
    Coverage cov;
    for (int seed = 0; seed < kSeeds && !failures; ++seed) walk(seed, cov);
    std::printf("walks: %d seeds x %d operations; %d reclaims, %d left no row, %d appends after one, %d removes of reclaimed ids, "
                "%d appends refused at the top of the id space, %d set_groups with an id never issued\n",
                kSeeds, kOps, cov.reclaims, cov.emptied, cov.appends_after_emptied, cov.removes_of_reclaimed, cov.full,
                cov.bad_group_ids);
    if (!failures) {  // the states the walks have to reach
        CHECK(cov.emptied >= 1);
        CHECK(cov.appends_after_emptied >= 1);
        CHECK(cov.removes_of_reclaimed >= 1);
        CHECK(cov.full >= 1);
        CHECK(cov.bad_group_ids >= 1);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("index ledger ok\n");
    return 0;
}
