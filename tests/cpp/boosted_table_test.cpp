// The class table of the boosted search (codesearch_amd/csrc/index_ledger.hpp: ClassTable, the GroupTable's sibling from one
// template) on the CPU: 2 B entries, assignment and un-assignment, ids never issued, what a device copy has not seen, and
// that builds' reclaims and appends leave it alone while clear() drops it.  The group table's own walk against a model is
// tests/cpp/index_ledger_test.cpp.
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "../../codesearch_amd/csrc/index_ledger.hpp"

using namespace cs;

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static_assert(std::is_same<decltype(ClassTable().data()), const uint16_t*>::value, "2 B per id");
static_assert(std::is_same<decltype(GroupTable().data()), const uint32_t*>::value, "the group table keeps 4 B per id");
static_assert(CS_NO_CLASS == 0xFFFFu && CS_MAX_CLASSES == 4096u && CS_MAX_CLASSES <= CS_NO_CLASS, "public constants");

// a device copy as index.hip keeps it: grown, refreshed over the pending range only
struct Shadow {
    std::vector<uint16_t> dev;
    uint64_t copied = 0;
    void upload(ClassTable& t) {
        if (t.assigned() == 0) return;  // ensure_classes: no class assigned, a null table
        const uint64_t n = t.size();
        if (n > dev.size()) {
            dev.assign((size_t)n, 0xABCD);  // a fresh allocation holds garbage
            t.uploaded(0);
        }
        uint64_t lo = 0, hi = 0;
        if (t.pending(&lo, &hi)) {
            for (uint64_t i = lo; i < hi; ++i) dev[(size_t)i] = t.data()[i];
            copied += hi - lo;
        }
        t.uploaded(n);
    }
};

static uint16_t class_of(const ClassTable& t, const IndexLedger& l, uint32_t id) {
    const uint32_t i = id - l.id_base();
    return i < t.size() ? t.data()[i] : (uint16_t)CS_NO_CLASS;  // ids past the end read as unassigned
}

int main() {
    IndexLedger led(1000);
    ClassTable t;
    Shadow dev;
    CHECK(led.append(100) == 1000);
    CHECK(t.assigned() == 0 && t.size() == 0);

    // an id never issued: its position is reported and NOTHING of the call is assigned
    const uint32_t bad_ids[3] = {1005, 999, 1006};
    const uint16_t cls3[3] = {1, 2, 3};
    CHECK(t.set(bad_ids, cls3, 3, led) == 1);
    CHECK(t.assigned() == 0 && t.size() == 0);
    const uint32_t past[1] = {1100};
    CHECK(t.set(past, cls3, 1, led) == 0 && t.size() == 0);

    // assignment: the table reaches the highest id touched, the rest of it unassigned
    const uint32_t ids[3] = {1010, 1003, 1040};
    CHECK(t.set(ids, cls3, 3, led) == -1);
    CHECK(t.assigned() == 3 && t.size() == 41);
    CHECK(class_of(t, led, 1010) == 1 && class_of(t, led, 1003) == 2 && class_of(t, led, 1040) == 3);
    CHECK(class_of(t, led, 1000) == CS_NO_CLASS && class_of(t, led, 1041) == CS_NO_CLASS && class_of(t, led, 1099) == CS_NO_CLASS);
    dev.upload(t);
    CHECK(dev.copied == 41);
    uint64_t lo, hi;
    CHECK(!t.pending(&lo, &hi));

    // re-assignment dirties its entry alone; the same value again dirties nothing
    const uint32_t one[1] = {1010};
    const uint16_t nine[1] = {9};
    CHECK(t.set(one, nine, 1, led) == -1 && t.assigned() == 3);
    CHECK(t.pending(&lo, &hi) && lo == 10 && hi == 11);
    dev.upload(t);
    CHECK(dev.copied == 42 && dev.dev[10] == 9);
    CHECK(t.set(one, nine, 1, led) == -1 && !t.pending(&lo, &hi));

    // CS_NO_CLASS un-assigns
    const uint16_t none[1] = {(uint16_t)CS_NO_CLASS};
    CHECK(t.set(one, none, 1, led) == -1 && t.assigned() == 2 && class_of(t, led, 1010) == CS_NO_CLASS);
    dev.upload(t);
    CHECK(dev.dev[10] == CS_NO_CLASS);

    // growth past the device copy: everything is pending again after the reallocation
    const uint32_t far[1] = {1090};
    CHECK(t.set(far, nine, 1, led) == -1 && t.size() == 91);
    dev.upload(t);
    for (uint64_t i = 0; i < t.size(); ++i) CHECK(dev.dev[(size_t)i] == t.data()[i]);

    // deletes, a reclaiming build and appends leave the table alone; a deleted id is still an id
    const uint32_t dead[2] = {1003, 1040};
    CHECK(led.remove(dead, 2) == 2);
    led.commit_reclaim();
    CHECK(led.append(10) == 1100);
    CHECK(t.assigned() == 3 && class_of(t, led, 1003) == 2 && class_of(t, led, 1105) == CS_NO_CLASS);
    CHECK(t.set(dead, cls3, 2, led) == -1);
    CHECK(!t.pending(&lo, &hi) || (lo == 3 && hi == 41));
    const uint32_t fresh[1] = {1105};
    CHECK(t.set(fresh, nine, 1, led) == -1 && t.size() == 106 && t.assigned() == 4);

    // clear() drops it: nothing assigned, nothing pending, and the ledger's ids restart
    t.clear();
    led.clear();
    CHECK(t.assigned() == 0 && t.size() == 0 && !t.pending(&lo, &hi));
    CHECK(led.append(5) == 1000 && t.set(one, nine, 1, led) == 0);  // 1010 is not issued any more

    std::printf("class table ok\n");
    return 0;
}
