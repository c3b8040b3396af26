// The plan and the route of a scoped search through the int8 filter (codesearch_amd/csrc/scoped_filter_plan.hpp) on the
// CPU, over synthetic ascending row lists.  On every case: phase 0's entries and the row ranges of the filter phases
// (tail included) cover every list entry exactly once, in ascending order; P <= c0 < P + 1024; boundaries lie on the
// 1,024 granule; every filter phase keeps the kernel, queries per tile and query tiles plan_filter picks for the same
// (nq, k, dim).  Then the route predicate on both sides of its rules, and the forced routes.
#include <cstdio>
#include <string>
#include <vector>

#include "../../codesearch_amd/csrc/scoped_filter_plan.hpp"

using namespace cs;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++failures;                                   \
            printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
        }                                                 \
    } while (0)

// what a scope keeps on the host of `list`
struct Tables {
    std::vector<uint32_t> head, stride;
    ScopeListView view;
    explicit Tables(const std::vector<uint32_t>& list) {
        for (uint64_t i = 0; i < scope_head_entries(list.size()); ++i) head.push_back(list[i]);
        for (uint64_t j = 0; j < scope_stride_entries(list.size()); ++j) stride.push_back(list[j * 1024]);
        view.live = list.size();
        view.head = head.data();
        view.stride = stride.data();
        view.last = list.empty() ? 0 : list.back();
    }
};

static const FilterKnobs kn;
constexpr int kCus = 256;

// Plans `list` over a store of n_rows rows and checks the invariants; returns the plan.
static ScopedFilterPlan plan_and_check(const char* name, const std::vector<uint32_t>& list, uint64_t n_rows, uint32_t dim,
                                       uint32_t nq, uint32_t k, bool expect_ok) {
    const Tables t(list);
    const uint64_t q8_rows = n_rows / 128 * 128;
    const ScopedFilterPlan s = plan_scoped_filter(dim, n_rows, t.view, nq, k, q8_rows, true, kCus, kn);
    CHECK(s.ok == expect_ok, "%s nq %u k %u: ok = %d", name, nq, k, (int)s.ok);
    if (!s.ok) return s;
    const FilterPlan& p = s.plan;
    const uint32_t P = nq <= 32 ? kFilterPhase0 : 1024u;
    CHECK(s.c0 >= P && s.c0 < P + 1024, "%s: c0 = %u, P = %u", name, s.c0, P);
    CHECK(p.phase0_rows == s.c0, "%s: phase0_rows", name);
    CHECK(s.b0 % 1024 == 0 && s.b0 > 0, "%s: b0 = %llu", name, (unsigned long long)s.b0);
    // phase 0 = exactly the entries below b0
    CHECK(list[s.c0 - 1] < s.b0 && list[s.c0] >= s.b0, "%s: c0 does not split the list at b0", name);
    CHECK(p.nphases >= 2 && p.phase[0].lo == 0 && p.phase[0].hi == s.b0 && p.phase[0].kernel == FilterKernel::None,
          "%s: phase 0", name);
    // what plan_filter picks for this (nq, k, dim): over the live rows, and over the store itself
    const FilterPlan ref = plan_filter(dim, list.size(), nq, k, ~(uint64_t)0, true, kCus, kn);
    const FilterPlan ref_store = plan_filter(dim, n_rows, nq, k, q8_rows, true, kCus, kn);
    CHECK(p.use_q8 && p.two_planes == ref.two_planes && p.two_planes == ref_store.two_planes, "%s: planes", name);
    CHECK(p.phase[0].rk_blocks == ref.phase[0].rk_blocks, "%s: phase 0 refine blocks", name);
    // cover: walk the list once
    uint64_t at = s.c0, prev_hi = s.b0;
    for (uint32_t i = 1; i < p.nphases; ++i) {
        const FilterPhase& f = p.phase[i];
        CHECK(f.lo == prev_hi && f.hi > f.lo, "%s: phase %u is [%llu, %llu) behind %llu", name, i, (unsigned long long)f.lo,
              (unsigned long long)f.hi, (unsigned long long)prev_hi);
        CHECK(f.lo % 1024 == 0, "%s: phase %u starts off the granule", name, i);
        const bool last = i + 1 == p.nphases;
        CHECK(f.hi % 1024 == 0 || (last && f.hi == n_rows), "%s: phase %u ends off the granule at %llu", name, i,
              (unsigned long long)f.hi);
        CHECK(f.hi <= n_rows, "%s: phase %u ends behind the store", name, i);
        // filter rows + tail rows = the phase's rows, the filter on whole 128-row tiles inside the copy
        if (f.kernel != FilterKernel::None) {
            CHECK(f.filter_hi > f.lo && f.filter_hi <= q8_rows && f.filter_hi % 128 == 0 && f.grid > 0, "%s: phase %u filter rows", name, i);
            const FilterPhase& from = ref.phase[s.src[i]];  // the plan_filter phase this one was taken from
            CHECK(s.src[i] >= 1 && s.src[i] < ref.nphases && (i == 1 || s.src[i] > s.src[i - 1]), "%s: phase %u source %u", name, i, s.src[i]);
            CHECK(f.kernel == from.kernel && f.nqt == from.nqt && f.qtiles == from.qtiles,
                  "%s: phase %u kernel differs from plan_filter's over the live rows", name, i);
            CHECK(f.kernel == ref_store.phase[1].kernel && f.nqt == ref_store.phase[1].nqt && f.qtiles == ref_store.phase[1].qtiles,
                  "%s: phase %u kernel differs from plan_filter's over the store", name, i);
            CHECK(f.grid % 8 == 0 && f.grid <= (uint32_t)kCus, "%s: phase %u grid %u", name, i, f.grid);
        }
        CHECK(f.rk_blocks == ref.phase[s.src[i]].rk_blocks, "%s: phase %u refine blocks", name, i);
        const uint64_t fend = f.kernel != FilterKernel::None ? f.filter_hi : f.lo;
        if (fend < f.hi) {
            CHECK(f.tail_lo == fend && f.tail_hi == f.hi && f.tail_hi - f.tail_lo < 128, "%s: phase %u tail [%llu, %llu)", name,
                  i, (unsigned long long)f.tail_lo, (unsigned long long)f.tail_hi);
        } else {
            CHECK(f.tail_hi <= f.tail_lo, "%s: phase %u has a tail inside the filter's rows", name, i);
        }
        uint64_t n_in = 0;
        while (at < list.size() && list[at] < f.hi) {
            CHECK(list[at] >= f.lo, "%s: entry %llu (row %u) lies before phase %u", name, (unsigned long long)at, list[at], i);
            ++at;
            ++n_in;
        }
        CHECK(n_in > 0, "%s: phase %u holds no entry", name, i);
        prev_hi = f.hi;
    }
    CHECK(at == list.size(), "%s: %llu of %llu entries covered", name, (unsigned long long)at, (unsigned long long)list.size());
    CHECK(s.span == prev_hi - s.b0, "%s: span", name);
    return s;
}

static std::vector<uint32_t> range(uint32_t lo, uint32_t hi, uint32_t step = 1) {
    std::vector<uint32_t> v;
    for (uint32_t r = lo; r < hi; r += step) v.push_back(r);
    return v;
}

int main() {
    const uint32_t shapes[][2] = {{1, 10}, {1, 200}, {9, 10}, {9, 200}, {33, 10}, {40, 10}, {200, 10}, {1000, 10}};
    for (const auto& sh : shapes) {
        const uint32_t nq = sh[0], k = sh[1];
        for (uint32_t dim : {384u, 768u, 1024u}) {
            if (dim != 384 && nq > 40) continue;
            // dense from row 0: the boundaries are plan_filter's own
            {
                const ScopedFilterPlan s = plan_and_check("dense from 0", range(0, 1000000), 1000000, dim, nq, k, true);
                const FilterPlan ref = plan_filter(dim, 1000000, nq, k, 1000000 / 128 * 128, true, kCus, kn);
                CHECK(s.plan.nphases == ref.nphases, "dense from 0: %u phases, plan_filter %u", s.plan.nphases, ref.nphases);
                for (uint32_t i = 1; i < ref.nphases && i < s.plan.nphases; ++i) {
                    CHECK(s.plan.phase[i].hi == ref.phase[i].hi && s.plan.phase[i].grid == ref.phase[i].grid &&
                              s.plan.phase[i].filter_hi == ref.phase[i].filter_hi && s.plan.phase[i].tail_lo == ref.phase[i].tail_lo &&
                              s.plan.phase[i].tail_hi == ref.phase[i].tail_hi && s.plan.phase[i].slots == ref.phase[i].slots,
                          "dense from 0 nq %u k %u: phase %u differs from plan_filter's", nq, k, i);
                }
            }
            // dense in the far half: plan_filter's phase 0 would sample nothing of it
            {
                const ScopedFilterPlan s = plan_and_check("far half", range(600037, 1000000), 1000000, dim, nq, k, true);
                CHECK(!s.ok || s.b0 > 600037, "far half: b0");
                CHECK(!s.ok || s.span <= 400000, "far half: span %llu", (unsigned long long)s.span);
            }
            plan_and_check("every other row", range(1, 1000000, 2), 1000000, dim, nq, k, true);
            // the first 3,073 entries inside one granule (rows 2048 .. 3071 + ...): 1,024 rows per granule at most, so
            // "inside one granule" for the phase-0 boundary: the entry P - 1 and the entry P share a granule
            {
                std::vector<uint32_t> l = range(5, 3 * 1024 - 100);          // 2,967 entries
                for (uint32_t r = 7 * 1024; r < 7 * 1024 + 106; ++r) l.push_back(r);  // entries 2,967 .. 3,072 share granule 7
                for (uint32_t r = 7 * 1024 + 500; r < 7 * 1024 + 900; ++r) l.push_back(r);
                for (uint32_t r = 500000; r < 520000; ++r) l.push_back(r);
                const ScopedFilterPlan s = plan_and_check("one granule", l, 600000, dim, nq, k, true);
                if (nq <= 32) CHECK(s.b0 == 8 * 1024 && s.c0 == 2967 + 106 + 400, "one granule: b0 %llu c0 %u", (unsigned long long)s.b0, s.c0);
            }
            // live just above, at and below the phase-0 size (the larger one: only such scopes hold the tables)
            plan_and_check("live = P + 1, spread", range(0, 2 * 3073, 2), 100000, dim, nq, k, true);
            plan_and_check("live = P + 1, dense", range(0, 3073), 100000, dim, nq, k, true);
            plan_and_check("live = P", range(0, 2 * 3072, 2), 100000, dim, nq, k, false);
            plan_and_check("live = P - 1", range(0, 2 * 3071, 2), 100000, dim, nq, k, false);
            // a last entry in the tail behind the last complete tile, the store's last row
            {
                std::vector<uint32_t> l = range(30000, 40000);
                for (uint32_t r = 40000; r < 40037; r += 3) l.push_back(r);
                if (l.back() != 40036) l.push_back(40036);
                const ScopedFilterPlan s = plan_and_check("ragged tail", l, 40037, dim, nq, k, true);
                if (s.ok) {
                    const FilterPhase& f = s.plan.phase[s.plan.nphases - 1];
                    CHECK(f.hi == 40037 && f.tail_lo == 40037 / 128 * 128 && f.tail_hi == 40037, "ragged tail: [%llu, %llu)",
                          (unsigned long long)f.tail_lo, (unsigned long long)f.tail_hi);
                }
            }
            // two far-apart blocks: the span counts the gap
            {
                std::vector<uint32_t> l = range(10000, 60000);
                for (uint32_t r = 900000; r < 950000; ++r) l.push_back(r);
                const ScopedFilterPlan s = plan_and_check("two blocks", l, 1000000, dim, nq, k, true);
                CHECK(!s.ok || s.span > 4 * 100000, "two blocks: span %llu", (unsigned long long)s.span);
            }
        }
    }
    // unsupported dim, no int8 copy
    plan_and_check("dim 100", range(0, 100000), 100000, 100, 9, 10, false);
    {
        const Tables t(range(0, 100000));
        CHECK(!plan_scoped_filter(384, 100000, t.view, 9, 10, 0, true, kCus, kn).ok, "no int8 copy, yet a plan");
    }

    // ---- route ----
    RouteKnobs rk;
    SearchShape shape;
    shape.dim = 384; shape.normed = true; shape.use_split = true; shape.batched = true; shape.prime = true; shape.pinned = true;
    ScopedRouteIn in;
    in.q8_serves = true; in.plan_ok = true;
    auto wants = [&](uint32_t nq, uint32_t k, uint64_t live, uint64_t span, int mode) {
        shape.nq = nq; shape.k = k; shape.n_rows = live;
        in.live = live; in.span = span; in.mode = mode;
        return scoped_wants_filter(rk, shape, in);
    };
    // (b) the row thresholds of one query, in live rows; always from four queries
    CHECK(!wants(1, 10, 20000, 20000, CS_SCOPE_ROUTE_AUTO), "one query over 20,000 live rows took the filter");
    CHECK(wants(1, 10, 32768, 32768, CS_SCOPE_ROUTE_AUTO), "one query over 32,768 live rows did not");
    CHECK(!wants(1, 200, 299999, 299999, CS_SCOPE_ROUTE_AUTO), "one query, k = 200, below 300,000");
    CHECK(wants(1, 200, 300000, 300000, CS_SCOPE_ROUTE_AUTO), "one query, k = 200, at 300,000");
    CHECK(wants(4, 10, 4000, 4000, CS_SCOPE_ROUTE_AUTO) && wants(9, 200, 12000, 12000, CS_SCOPE_ROUTE_AUTO), "four and nine queries");
    // (c) the span, by query count: 2 x live for one query, 4 x for two to eight, 10 x from nine on
    CHECK(wants(1, 10, 100000, 200000, CS_SCOPE_ROUTE_AUTO), "one query, span = 2 x live");
    CHECK(!wants(1, 10, 100000, 200001, CS_SCOPE_ROUTE_AUTO), "one query, span just above 2 x live");
    CHECK(wants(4, 10, 10000, 40000, CS_SCOPE_ROUTE_AUTO) && wants(8, 10, 10000, 40000, CS_SCOPE_ROUTE_AUTO), "span = 4 x live");
    CHECK(!wants(4, 10, 10000, 40001, CS_SCOPE_ROUTE_AUTO) && !wants(8, 10, 10000, 40001, CS_SCOPE_ROUTE_AUTO), "span just above 4 x live");
    CHECK(wants(9, 10, 10000, 100000, CS_SCOPE_ROUTE_AUTO) && wants(40, 10, 10000, 100000, CS_SCOPE_ROUTE_AUTO), "span = 10 x live");
    CHECK(!wants(9, 10, 10000, 100001, CS_SCOPE_ROUTE_AUTO), "span just above 10 x live");
    rk.scope_span_few = 8.0;
    CHECK(wants(4, 10, 10000, 40001, CS_SCOPE_ROUTE_AUTO), "the knob");
    rk.scope_span_few = 4.0;
    // forced routes: _FILTER waives (b) and (c) only; _GATHER never filters
    CHECK(wants(1, 10, 20000, 20000, CS_SCOPE_ROUTE_FILTER) && wants(9, 10, 10000, 400000, CS_SCOPE_ROUTE_FILTER), "forced filter");
    CHECK(!wants(9, 10, 100000, 100000, CS_SCOPE_ROUTE_GATHER), "forced gather");
    in.q8_serves = false;
    CHECK(!wants(9, 10, 100000, 100000, CS_SCOPE_ROUTE_FILTER) && !wants(9, 10, 100000, 100000, CS_SCOPE_ROUTE_AUTO), "(a) waived");
    in.q8_serves = true; in.plan_ok = false;
    CHECK(!wants(9, 10, 100000, 100000, CS_SCOPE_ROUTE_FILTER), "no plan, yet the filter");

    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("scoped filter plan ok\n");
    return 0;
}
