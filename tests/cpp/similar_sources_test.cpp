// The host side of the similar-chunk search (codesearch_amd/csrc/similar_sources.hpp: source ids -> stored rows, the live
// check, the per-query excluded id and group) against a naive restatement: directed cases (never-issued, tombstoned and
// reclaimed ids, id_base, ids past the group table's end, duplicates) and 5,000 random ledgers.  Plain C++17, no GPU:
// tests/test_similar_host.py builds and runs it once as it is and once under AddressSanitizer + UBSan.
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../../codesearch_amd/csrc/similar_sources.hpp"

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

using namespace cs;

namespace {

// The index the slow way: which ids were issued, which are deleted, the live ids in storage order, every id's group.
struct Model {
    uint32_t id_base = 0;
    uint32_t issued = 0;
    std::set<uint32_t> deleted;            // issued and deleted since (tombstoned or reclaimed alike)
    std::vector<uint32_t> stored;          // the id of each stored row (tombstoned rows included)
    std::map<uint32_t, uint32_t> group;    // ids that were assigned one

    void append(uint32_t n) {
        for (uint32_t i = 0; i < n; ++i) stored.push_back(id_base + issued + i);
        issued += n;
    }
    void remove(uint32_t id) {
        if (id >= id_base && id - id_base < issued) deleted.insert(id);
    }
    void reclaim() {
        std::vector<uint32_t> kept;
        for (uint32_t id : stored)
            if (!deleted.count(id)) kept.push_back(id);
        stored.swap(kept);
    }
    // -> 0 fine, 1 never issued, 2 deleted; *row, *ex_id, *ex_group as the header defines them
    int resolve(uint32_t id, int32_t mode, uint32_t* row, uint32_t* ex_id, uint32_t* ex_group) const {
        if (id < id_base || id - id_base >= issued) return 1;
        if (deleted.count(id)) return 2;
        for (size_t r = 0; r < stored.size(); ++r)
            if (stored[r] == id) *row = (uint32_t)r;
        *ex_id = mode == CS_SIMILAR_EXCLUDE_NONE ? 0xFFFFFFFFu : id;
        const auto g = group.find(id);
        *ex_group = (mode == CS_SIMILAR_EXCLUDE_GROUP && g != group.end()) ? g->second : CS_NO_GROUP;
        return 0;
    }
};

int compare(const Model& m, const IndexLedger& led, const GroupTable& gt, const std::vector<uint32_t>& ids, int32_t mode) {
    const uint32_t nq = (uint32_t)ids.size();
    std::vector<uint32_t> rows(nq, 0xABABABABu), ex_ids(nq, 0xABABABABu), ex_groups(nq, 0xABABABABu);
    int want_fault = 0;
    uint32_t want_at = 0;
    std::vector<uint32_t> wr(nq), wi(nq), wg(nq);
    for (uint32_t q = 0; q < nq && !want_fault; ++q) {
        want_fault = m.resolve(ids[q], mode, &wr[q], &wi[q], &wg[q]);
        if (want_fault) want_at = q;
    }
    const SourceCheck check = resolve_similar_sources(led, gt, ids.data(), nq, mode, nullptr, nullptr, nullptr);
    const SourceCheck full = resolve_similar_sources(led, gt, ids.data(), nq, mode, rows.data(), ex_ids.data(), ex_groups.data());
    REQUIRE((int)check.fault == want_fault && (int)full.fault == want_fault);
    if (want_fault) {
        REQUIRE(check.at == want_at && full.at == want_at);
        return 0;
    }
    REQUIRE(rows == wr && ex_ids == wi && ex_groups == wg);
    return 0;
}

int directed() {
    Model m;
    m.id_base = 5000;
    IndexLedger led(5000);
    GroupTable gt;
    m.append(40);
    led.append(40);
    // groups for the first 20 ids only: the rest lie past the table's end
    std::vector<uint32_t> gi, gg;
    for (uint32_t i = 0; i < 20; ++i) { gi.push_back(5000 + i); gg.push_back(i / 4); m.group[5000 + i] = i / 4; }
    gi.push_back(5007); gg.push_back(CS_NO_GROUP); m.group.erase(5007);  // un-assigned again
    REQUIRE(gt.set(gi.data(), gg.data(), gi.size(), led) == -1);
    REQUIRE(gt.size() == 20);
    for (int32_t mode = 0; mode <= 2; ++mode) {
        REQUIRE(compare(m, led, gt, {5000, 5019, 5020, 5039, 5007, 5000, 5000}, mode) == 0);
        REQUIRE(compare(m, led, gt, {5001, 4999}, mode) == 0);        // below id_base
        REQUIRE(compare(m, led, gt, {5040, 5001}, mode) == 0);        // next_id: not issued yet
        REQUIRE(compare(m, led, gt, {0}, mode) == 0);
        REQUIRE(compare(m, led, gt, {0xFFFFFFFFu}, mode) == 0);
    }
    uint32_t r = 0, ei = 0, eg = 0;
    const uint32_t one = 5021;
    REQUIRE(resolve_similar_sources(led, gt, &one, 1, CS_SIMILAR_EXCLUDE_GROUP, &r, &ei, &eg).fault == SourceFault::None);
    REQUIRE(r == 21 && ei == 5021 && eg == CS_NO_GROUP);  // past the table: EXCLUDE_GROUP is EXCLUDE_SELF
    const uint32_t two = 5006;
    REQUIRE(resolve_similar_sources(led, gt, &two, 1, CS_SIMILAR_EXCLUDE_GROUP, &r, &ei, &eg).fault == SourceFault::None);
    REQUIRE(r == 6 && ei == 5006 && eg == 1);
    REQUIRE(resolve_similar_sources(led, gt, &two, 1, CS_SIMILAR_EXCLUDE_SELF, &r, &ei, &eg).fault == SourceFault::None);
    REQUIRE(ei == 5006 && eg == CS_NO_GROUP);
    REQUIRE(resolve_similar_sources(led, gt, &two, 1, CS_SIMILAR_EXCLUDE_NONE, &r, &ei, &eg).fault == SourceFault::None);
    REQUIRE(ei == kNoExcludedId && eg == CS_NO_GROUP);
    // tombstoned: refused as deleted; the first offender is named
    const std::vector<uint32_t> gone = {5003, 5010, 5011, 5039};
    for (uint32_t id : gone) m.remove(id);
    REQUIRE(led.remove(gone.data(), gone.size()) == 4);
    for (int32_t mode = 0; mode <= 2; ++mode) {
        REQUIRE(compare(m, led, gt, {5000, 5002, 5010, 5003}, mode) == 0);
        REQUIRE(compare(m, led, gt, {5039}, mode) == 0);
        REQUIRE(compare(m, led, gt, {5004, 5012, 5038}, mode) == 0);
    }
    const uint32_t mixed[3] = {5002, 5011, 4000};
    const SourceCheck sc = resolve_similar_sources(led, gt, mixed, 3, 1, nullptr, nullptr, nullptr);
    REQUIRE(sc.fault == SourceFault::Deleted && sc.at == 1);
    // reclaimed: still refused as deleted, and the survivors' rows have moved
    m.reclaim();
    led.commit_reclaim();
    REQUIRE(led.stored() == 36 && led.compacted());
    for (int32_t mode = 0; mode <= 2; ++mode) {
        REQUIRE(compare(m, led, gt, {5000, 5004, 5012, 5038, 5019, 5020}, mode) == 0);
        REQUIRE(compare(m, led, gt, {5004, 5003}, mode) == 0);
        REQUIRE(compare(m, led, gt, {5039}, mode) == 0);
        REQUIRE(compare(m, led, gt, {5040}, mode) == 0);
    }
    const uint32_t moved = 5012;
    REQUIRE(resolve_similar_sources(led, gt, &moved, 1, 1, &r, &ei, &eg).fault == SourceFault::None && r == 9);
    // appended after the reclaim: new ids, rows behind the survivors; then deleted before the next build
    m.append(5);
    led.append(5);
    REQUIRE(compare(m, led, gt, {5040, 5044, 5000}, 2) == 0);
    const uint32_t fresh = 5042;
    m.remove(fresh);
    REQUIRE(led.remove(&fresh, 1) == 1);
    REQUIRE(compare(m, led, gt, {5041, 5042}, 2) == 0);
    // clear(): every id is never-issued again
    led.clear();
    gt.clear();
    m = Model();
    m.id_base = 5000;
    REQUIRE(compare(m, led, gt, {5000}, 1) == 0);
    REQUIRE(!similar_mode_ok(-1) && similar_mode_ok(0) && similar_mode_ok(1) && similar_mode_ok(2) && !similar_mode_ok(3));
    return 0;
}

int random_ledgers(uint32_t rounds) {
    std::mt19937 rng(20261019u);
    auto pick = [&](uint32_t n) { return n ? (uint32_t)(rng() % n) : 0u; };
    for (uint32_t round = 0; round < rounds; ++round) {
        Model m;
        m.id_base = pick(4) == 0 ? 0u : pick(3) == 0 ? 0xFFFFF000u : pick(100000);
        IndexLedger led(m.id_base);
        GroupTable gt;
        const uint32_t steps = 1 + pick(8);
        for (uint32_t s = 0; s < steps; ++s) {
            const uint32_t what = pick(5);
            if (what <= 1 || m.issued == 0) {  // append
                const uint32_t n = 1 + pick(40);
                m.append(n);
                led.append(n);
            } else if (what == 2) {  // remove a few, unknown ids among them
                std::vector<uint32_t> ids;
                for (uint32_t i = 0, n = 1 + pick(12); i < n; ++i) ids.push_back(m.id_base + pick(m.issued + 3));
                std::set<uint32_t> fresh;
                for (uint32_t id : ids)
                    if (id >= m.id_base && id - m.id_base < m.issued && !m.deleted.count(id)) fresh.insert(id);
                for (uint32_t id : ids) m.remove(id);
                REQUIRE(led.remove(ids.data(), ids.size()) == fresh.size());
            } else if (what == 3) {  // a reclaiming build
                m.reclaim();
                led.commit_reclaim();
            } else {  // groups for a few ids
                std::vector<uint32_t> ids, groups;
                for (uint32_t i = 0, n = 1 + pick(10); i < n; ++i) {
                    ids.push_back(m.id_base + pick(m.issued));
                    groups.push_back(pick(5) == 0 ? CS_NO_GROUP : pick(4));
                }
                REQUIRE(gt.set(ids.data(), groups.data(), ids.size(), led) == -1);
                for (size_t i = 0; i < ids.size(); ++i) {
                    if (groups[i] == CS_NO_GROUP) m.group.erase(ids[i]);
                    else m.group[ids[i]] = groups[i];
                }
            }
        }
        REQUIRE(led.stored() == m.stored.size());
        // live sources only (every mode), then a list with whatever the dice say
        std::vector<uint32_t> live;
        for (uint32_t id : m.stored)
            if (!m.deleted.count(id)) live.push_back(id);
        for (int32_t mode = 0; mode <= 2; ++mode) {
            if (!live.empty()) {
                std::vector<uint32_t> ids;
                for (uint32_t i = 0, n = 1 + pick(12); i < n; ++i) ids.push_back(live[pick((uint32_t)live.size())]);
                REQUIRE(compare(m, led, gt, ids, mode) == 0);
            }
            std::vector<uint32_t> ids;
            for (uint32_t i = 0, n = 1 + pick(6); i < n; ++i) {
                const uint32_t dice = pick(10);
                if (dice == 0) ids.push_back(m.id_base + m.issued + pick(3));             // not issued yet
                else if (dice == 1) ids.push_back(m.id_base - 1 - pick(3));               // below id_base (wraps at base 0)
                else ids.push_back(m.id_base + pick(m.issued));                           // issued: live or deleted
            }
            REQUIRE(compare(m, led, gt, ids, mode) == 0);
        }
    }
    return 0;
}

}  // namespace

int main() {
    if (directed()) return 1;
    if (random_ledgers(5000)) return 1;
    std::printf("similar sources ok\n");
    return 0;
}
