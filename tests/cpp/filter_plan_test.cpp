// The filter plan (codesearch_amd/csrc/filter_plan.hpp) on the CPU: phase boundaries, filter kernels and launch shapes.
// Every expected value below was recorded from the launch sequence of the filter search as it stood before the plan was
// split out of scan_filter.hip (cus = 256, MI355X).  Form of a plan: "q8 <int8 copy> planes <two query planes> p0 <phase-0
// rows>", then per phase "| lo-hi [kernel/nqt/qtiles g<grid> s<slots> f<filter rows' end>] [tail a-b] rk<refine blocks>".
#include <cstdio>
#include <string>

#include "../../codesearch_amd/csrc/filter_plan.hpp"

using namespace cs;

static const char* kernel_name(FilterKernel k) {
    switch (k) {
        case FilterKernel::None: return "None";
        case FilterKernel::Q8Tile256: return "Q8Tile256";
        case FilterKernel::Q8Rq: return "Q8Rq";
        case FilterKernel::Q8Rq1: return "Q8Rq1";
        case FilterKernel::Q8Rw: return "Q8Rw";
        case FilterKernel::Q8Rw2: return "Q8Rw2";
        case FilterKernel::F16Rw: return "F16Rw";
        case FilterKernel::F16Tile256: return "F16Tile256";
        case FilterKernel::F16Tile128: return "F16Tile128";
    }
    return "?";
}

static std::string describe(const FilterPlan& p) {
    char b[256];
    snprintf(b, sizeof b, "q8 %d planes %d p0 %u", (int)p.use_q8, (int)p.two_planes, p.phase0_rows);
    std::string s = b;
    for (uint32_t i = 0; i < p.nphases; ++i) {
        const FilterPhase& f = p.phase[i];
        snprintf(b, sizeof b, " | %llu-%llu", (unsigned long long)f.lo, (unsigned long long)f.hi);
        s += b;
        if (f.kernel != FilterKernel::None) {
            snprintf(b, sizeof b, " %s/%u/%u g%u s%u f%llu", kernel_name(f.kernel), f.nqt, f.qtiles, f.grid, f.slots,
                     (unsigned long long)f.filter_hi);
            s += b;
        }
        if (f.tail_hi > f.tail_lo) {
            snprintf(b, sizeof b, " tail %llu-%llu", (unsigned long long)f.tail_lo, (unsigned long long)f.tail_hi);
            s += b;
        }
        snprintf(b, sizeof b, " rk%u", f.rk_blocks);
        s += b;
    }
    return s;
}

// "<kernel/nqt/qtiles> x<filter phases>[ tail]": the kernel every filter phase of the search takes
static std::string kernel_choice(const FilterPlan& p) {
    std::string k;
    bool tail = false;
    for (uint32_t i = 1; i < p.nphases; ++i) {
        const FilterPhase& f = p.phase[i];
        tail = tail || f.tail_hi > f.tail_lo;
        if (f.kernel == FilterKernel::None) continue;
        const std::string t = std::string(kernel_name(f.kernel)) + "/" + std::to_string(f.nqt) + "/" + std::to_string(f.qtiles);
        if (!k.empty() && k != t) return "mixed";
        k = t;
    }
    return k + " x" + std::to_string(p.nphases - 1) + (tail ? " tail" : "");
}

enum Knobs { kDefault, kGrowth4, kRq0 };

static FilterKnobs knobs(Knobs which) {
    FilterKnobs kn;
    if (which == kGrowth4) kn.growth = 4;  // CS_FILTER_GROWTH=4: round 3's fixed growth
    if (which == kRq0) kn.int8_rq = false;  // CS_FILTER_INT8_RQ=0
    return kn;
}

struct PhaseCase {
    Knobs knobs;
    uint32_t dim;
    uint64_t rows;
    uint32_t nq, k;
    uint64_t q8_rows;
    const char* plan;
};

// one query over 10M / 1M / 100,000 rows at k = 10 and 200, 1,000 queries over 10M; each under the product's knobs,
// CS_FILTER_GROWTH=4 and CS_FILTER_INT8_RQ=0
static const PhaseCase kPhases[] = {
    {kDefault, 384, 10000000, 1, 10, 10000000,
     "q8 1 planes 0 p0 3072 | 0-3072 rk96 | 3072-46080 Q8Rw/1/1 g256 s0 f46080 rk32 | 46080-683008 Q8Rw/1/1 g256 s0 f683008 rk32 | 683008-10000000 Q8Rw/1/1 g256 s0 f10000000 rk32"},
    {kDefault, 384, 1000000, 1, 10, 999936,
     "q8 1 planes 0 p0 3072 | 0-3072 rk96 | 3072-56320 Q8Rw/1/1 g256 s0 f56320 rk32 | 56320-1000000 Q8Rw/1/1 g256 s0 f999936 tail 999936-1000000 rk32"},
    {kDefault, 384, 100000, 1, 10, 99968,
     "q8 1 planes 0 p0 3072 | 0-3072 rk96 | 3072-100000 Q8Rw/1/1 g256 s0 f99968 tail 99968-100000 rk32"},
    {kDefault, 384, 10000000, 1, 200, 10000000,
     "q8 1 planes 1 p0 3072 | 0-3072 rk96 | 3072-16384 Q8Rw2/1/1 g104 s0 f16384 rk32 | 16384-82944 Q8Rw2/1/1 g256 s0 f82944 rk32 | 82944-418816 Q8Rw2/1/1 g256 s0 f418816 rk32 | 418816-2111488 Q8Rw2/1/1 g256 s0 f2111488 rk32 | 2111488-10000000 Q8Rw2/1/1 g256 s0 f10000000 rk32"},
    {kDefault, 384, 1000000, 1, 200, 999936,
     "q8 1 planes 1 p0 3072 | 0-3072 rk96 | 3072-13312 Q8Rw2/1/1 g80 s0 f13312 rk32 | 13312-57344 Q8Rw2/1/1 g256 s0 f57344 rk32 | 57344-243712 Q8Rw2/1/1 g256 s0 f243712 rk32 | 243712-1000000 Q8Rw2/1/1 g256 s0 f999936 tail 999936-1000000 rk32"},
    {kDefault, 384, 100000, 1, 200, 99968,
     "q8 1 planes 1 p0 3072 | 0-3072 rk96 | 3072-10240 Q8Rw2/1/1 g56 s0 f10240 rk32 | 10240-32768 Q8Rw2/1/1 g176 s0 f32768 rk32 | 32768-100000 Q8Rw2/1/1 g256 s0 f99968 tail 99968-100000 rk32"},
    {kDefault, 384, 10000000, 1000, 10, 10000000,
     "q8 1 planes 0 p0 1024 | 0-1024 rk4 | 1024-22528 Q8Rq/8/4 g256 s0 f22528 rk4 | 22528-482304 Q8Rq/8/4 g256 s0 f482304 rk4 | 482304-10000000 Q8Rq/8/4 g256 s0 f10000000 rk4"},
    // CS_FILTER_GROWTH=4 over 10M rows
    {kGrowth4, 384, 10000000, 1, 10, 10000000,
     "q8 1 planes 0 p0 3072 | 0-3072 rk96 | 3072-15360 Q8Rw/1/1 g96 s0 f15360 rk32 | 15360-76800 Q8Rw/1/1 g256 s0 f76800 rk32 | 76800-384000 Q8Rw/1/1 g256 s0 f384000 rk32 | 384000-1920000 Q8Rw/1/1 g256 s0 f1920000 rk32 | 1920000-9600000 Q8Rw/1/1 g256 s0 f9600000 rk32 | 9600000-10000000 Q8Rw/1/1 g256 s0 f10000000 rk32"},
    {kGrowth4, 384, 10000000, 1, 200, 10000000,
     "q8 1 planes 1 p0 3072 | 0-3072 rk96 | 3072-15360 Q8Rw2/1/1 g96 s0 f15360 rk32 | 15360-76800 Q8Rw2/1/1 g256 s0 f76800 rk32 | 76800-384000 Q8Rw2/1/1 g256 s0 f384000 rk32 | 384000-1920000 Q8Rw2/1/1 g256 s0 f1920000 rk32 | 1920000-9600000 Q8Rw2/1/1 g256 s0 f9600000 rk32 | 9600000-10000000 Q8Rw2/1/1 g256 s0 f10000000 rk32"},
    {kGrowth4, 384, 10000000, 9, 200, 10000000,
     "q8 1 planes 1 p0 3072 | 0-3072 rk96 | 3072-15360 Q8Rw2/1/1 g96 s0 f15360 rk32 | 15360-76800 Q8Rw2/1/1 g256 s0 f76800 rk32 | 76800-384000 Q8Rw2/1/1 g256 s0 f384000 rk32 | 384000-1920000 Q8Rw2/1/1 g256 s0 f1920000 rk32 | 1920000-9600000 Q8Rw2/1/1 g256 s0 f9600000 rk32 | 9600000-10000000 Q8Rw2/1/1 g256 s0 f10000000 rk32"},
    {kGrowth4, 384, 10000000, 300, 10, 10000000,
     "q8 1 planes 0 p0 1024 | 0-1024 rk13 | 1024-5120 Q8Rq/8/2 g32 s0 f5120 rk13 | 5120-25600 Q8Rq/8/2 g160 s0 f25600 rk13 | 25600-128000 Q8Rq/8/2 g256 s0 f128000 rk13 | 128000-640000 Q8Rq/8/2 g256 s0 f640000 rk13 | 640000-3200000 Q8Rq/8/2 g256 s0 f3200000 rk13 | 3200000-10000000 Q8Rq/8/2 g256 s0 f10000000 rk13"},
    {kGrowth4, 384, 10000000, 1000, 10, 10000000,
     "q8 1 planes 0 p0 1024 | 0-1024 rk4 | 1024-5120 Q8Rq/8/4 g64 s0 f5120 rk4 | 5120-25600 Q8Rq/8/4 g256 s0 f25600 rk4 | 25600-128000 Q8Rq/8/4 g256 s0 f128000 rk4 | 128000-640000 Q8Rq/8/4 g256 s0 f640000 rk4 | 640000-3200000 Q8Rq/8/4 g256 s0 f3200000 rk4 | 3200000-10000000 Q8Rq/8/4 g256 s0 f10000000 rk4"},
    // CS_FILTER_INT8_RQ=0 over 10M rows (the one-query plans are the default ones)
    {kRq0, 384, 10000000, 300, 10, 10000000,
     "q8 1 planes 0 p0 1024 | 0-1024 rk13 | 1024-22528 Q8Rw/8/2 g256 s0 f22528 rk13 | 22528-482304 Q8Rw/8/2 g256 s0 f482304 rk13 | 482304-10000000 Q8Rw/8/2 g256 s0 f10000000 rk13"},
    {kRq0, 384, 10000000, 1000, 10, 10000000,
     "q8 1 planes 0 p0 1024 | 0-1024 rk4 | 1024-22528 Q8Rw/8/4 g256 s0 f22528 rk4 | 22528-482304 Q8Rw/8/4 g256 s0 f482304 rk4 | 482304-10000000 Q8Rw/8/4 g256 s0 f10000000 rk4"},
};

struct KernelCase {
    uint32_t dim, nq, k;
    uint64_t q8_rows;  // 1,000,000: the int8 copy covers the corpus; 0: the f16 copy; 200,000: int8 copy + tail
    const char* choice;
};

// 1M rows, two-plane query buffers present
static const KernelCase kKernels[] = {
    {384, 2, 10, 1000000, "Q8Rw/1/1 x2"},
    {384, 2, 10, 0, "F16Rw/1/1 x2"},
    {384, 2, 10, 200000, "Q8Rw/1/1 x2 tail"},
    {384, 2, 200, 1000000, "Q8Rw2/1/1 x4"},
    {384, 2, 200, 0, "F16Rw/1/1 x4"},
    {384, 2, 200, 200000, "Q8Rw2/1/1 x4 tail"},
    {384, 32, 10, 1000000, "Q8Rw/1/1 x2"},
    {384, 32, 10, 0, "F16Rw/1/1 x2"},
    {384, 32, 10, 200000, "Q8Rw/1/1 x2 tail"},
    {384, 32, 200, 1000000, "Q8Rw2/1/1 x4"},
    {384, 32, 200, 0, "F16Rw/1/1 x4"},
    {384, 32, 200, 200000, "Q8Rw2/1/1 x4 tail"},
    {384, 33, 10, 1000000, "Q8Rw/2/1 x3"},
    {384, 33, 10, 0, "F16Rw/2/1 x3"},
    {384, 33, 10, 200000, "Q8Rw/2/1 x3 tail"},
    {384, 33, 200, 1000000, "Q8Rw/2/1 x5"},
    {384, 33, 200, 0, "F16Rw/2/1 x5"},
    {384, 33, 200, 200000, "Q8Rw/2/1 x5 tail"},
    {384, 64, 10, 1000000, "Q8Rw/2/1 x3"},
    {384, 64, 10, 0, "F16Rw/2/1 x3"},
    {384, 64, 10, 200000, "Q8Rw/2/1 x3 tail"},
    {384, 64, 200, 1000000, "Q8Rw/2/1 x5"},
    {384, 64, 200, 0, "F16Rw/2/1 x5"},
    {384, 64, 200, 200000, "Q8Rw/2/1 x5 tail"},
    {384, 65, 10, 1000000, "Q8Rw/4/1 x3"},
    {384, 65, 10, 0, "F16Tile128/0/0 x3"},
    {384, 65, 10, 200000, "Q8Rw/4/1 x3 tail"},
    {384, 65, 200, 1000000, "Q8Rw/4/1 x5"},
    {384, 65, 200, 0, "F16Tile128/0/0 x5"},
    {384, 65, 200, 200000, "Q8Rw/4/1 x5 tail"},
    {384, 128, 10, 1000000, "Q8Rw/4/1 x3"},
    {384, 128, 10, 0, "F16Tile128/0/0 x3"},
    {384, 128, 10, 200000, "Q8Rw/4/1 x3 tail"},
    {384, 128, 200, 1000000, "Q8Rw/4/1 x5"},
    {384, 128, 200, 0, "F16Tile128/0/0 x5"},
    {384, 128, 200, 200000, "Q8Rw/4/1 x5 tail"},
    {384, 129, 10, 1000000, "Q8Rq1/8/1 x3"},
    {384, 129, 10, 0, "F16Tile256/0/0 x3"},
    {384, 129, 10, 200000, "Q8Rq1/8/1 x3 tail"},
    {384, 129, 200, 1000000, "Q8Rq1/8/1 x5"},
    {384, 129, 200, 0, "F16Tile256/0/0 x5"},
    {384, 129, 200, 200000, "Q8Rq1/8/1 x5 tail"},
    {384, 300, 10, 1000000, "Q8Rq/8/2 x3"},
    {384, 300, 10, 0, "F16Tile256/0/0 x3"},
    {384, 300, 10, 200000, "Q8Rq/8/2 x3 tail"},
    {384, 300, 200, 1000000, "Q8Rq/8/2 x5"},
    {384, 300, 200, 0, "F16Tile256/0/0 x5"},
    {384, 300, 200, 200000, "Q8Rq/8/2 x5 tail"},
    {384, 1000, 10, 1000000, "Q8Rq/8/4 x3"},
    {384, 1000, 10, 0, "F16Tile256/0/0 x3"},
    {384, 1000, 10, 200000, "Q8Rq/8/4 x3 tail"},
    {384, 1000, 200, 1000000, "Q8Rq/8/4 x5"},
    {384, 1000, 200, 0, "F16Tile256/0/0 x5"},
    {384, 1000, 200, 200000, "Q8Rq/8/4 x5 tail"},
    {768, 2, 10, 1000000, "Q8Rw/1/1 x2"},
    {768, 2, 10, 0, "F16Rw/1/1 x2"},
    {768, 2, 10, 200000, "Q8Rw/1/1 x2 tail"},
    {768, 2, 200, 1000000, "Q8Rw2/1/1 x4"},
    {768, 2, 200, 0, "F16Rw/1/1 x4"},
    {768, 2, 200, 200000, "Q8Rw2/1/1 x4 tail"},
    {768, 32, 10, 1000000, "Q8Rw/1/1 x2"},
    {768, 32, 10, 0, "F16Rw/1/1 x2"},
    {768, 32, 10, 200000, "Q8Rw/1/1 x2 tail"},
    {768, 32, 200, 1000000, "Q8Rw2/1/1 x4"},
    {768, 32, 200, 0, "F16Rw/1/1 x4"},
    {768, 32, 200, 200000, "Q8Rw2/1/1 x4 tail"},
    {768, 33, 10, 1000000, "Q8Rw/2/1 x3"},
    {768, 33, 10, 0, "F16Rw/2/1 x3"},
    {768, 33, 10, 200000, "Q8Rw/2/1 x3 tail"},
    {768, 33, 200, 1000000, "Q8Rw/2/1 x5"},
    {768, 33, 200, 0, "F16Rw/2/1 x5"},
    {768, 33, 200, 200000, "Q8Rw/2/1 x5 tail"},
    {768, 64, 10, 1000000, "Q8Rw/2/1 x3"},
    {768, 64, 10, 0, "F16Rw/2/1 x3"},
    {768, 64, 10, 200000, "Q8Rw/2/1 x3 tail"},
    {768, 64, 200, 1000000, "Q8Rw/2/1 x5"},
    {768, 64, 200, 0, "F16Rw/2/1 x5"},
    {768, 64, 200, 200000, "Q8Rw/2/1 x5 tail"},
    {768, 65, 10, 1000000, "Q8Rw/4/1 x3"},
    {768, 65, 10, 0, "F16Tile128/0/0 x3"},
    {768, 65, 10, 200000, "Q8Rw/4/1 x3 tail"},
    {768, 65, 200, 1000000, "Q8Rw/4/1 x5"},
    {768, 65, 200, 0, "F16Tile128/0/0 x5"},
    {768, 65, 200, 200000, "Q8Rw/4/1 x5 tail"},
    {768, 128, 10, 1000000, "Q8Rw/4/1 x3"},
    {768, 128, 10, 0, "F16Tile128/0/0 x3"},
    {768, 128, 10, 200000, "Q8Rw/4/1 x3 tail"},
    {768, 128, 200, 1000000, "Q8Rw/4/1 x5"},
    {768, 128, 200, 0, "F16Tile128/0/0 x5"},
    {768, 128, 200, 200000, "Q8Rw/4/1 x5 tail"},
    {768, 129, 10, 1000000, "Q8Rw/4/2 x3"},
    {768, 129, 10, 0, "F16Tile256/0/0 x3"},
    {768, 129, 10, 200000, "Q8Rw/4/2 x3 tail"},
    {768, 129, 200, 1000000, "Q8Rw/4/2 x5"},
    {768, 129, 200, 0, "F16Tile256/0/0 x5"},
    {768, 129, 200, 200000, "Q8Rw/4/2 x5 tail"},
    {768, 300, 10, 1000000, "Q8Rw/4/3 x3"},
    {768, 300, 10, 0, "F16Tile256/0/0 x3"},
    {768, 300, 10, 200000, "Q8Rw/4/3 x3 tail"},
    {768, 300, 200, 1000000, "Q8Rw/4/3 x5"},
    {768, 300, 200, 0, "F16Tile256/0/0 x5"},
    {768, 300, 200, 200000, "Q8Rw/4/3 x5 tail"},
    {768, 1000, 10, 1000000, "Q8Rw/4/8 x3"},
    {768, 1000, 10, 0, "F16Tile256/0/0 x3"},
    {768, 1000, 10, 200000, "Q8Rw/4/8 x3 tail"},
    {768, 1000, 200, 1000000, "Q8Rw/4/8 x5"},
    {768, 1000, 200, 0, "F16Tile256/0/0 x5"},
    {768, 1000, 200, 200000, "Q8Rw/4/8 x5 tail"},
    {1024, 2, 10, 1000000, "Q8Rw/1/1 x2"},
    {1024, 2, 10, 0, "F16Rw/1/1 x2"},
    {1024, 2, 10, 200000, "Q8Rw/1/1 x2 tail"},
    {1024, 2, 200, 1000000, "Q8Rw/1/1 x4"},
    {1024, 2, 200, 0, "F16Rw/1/1 x4"},
    {1024, 2, 200, 200000, "Q8Rw/1/1 x4 tail"},
    {1024, 32, 10, 1000000, "Q8Rw/1/1 x2"},
    {1024, 32, 10, 0, "F16Rw/1/1 x2"},
    {1024, 32, 10, 200000, "Q8Rw/1/1 x2 tail"},
    {1024, 32, 200, 1000000, "Q8Rw/1/1 x4"},
    {1024, 32, 200, 0, "F16Rw/1/1 x4"},
    {1024, 32, 200, 200000, "Q8Rw/1/1 x4 tail"},
    {1024, 33, 10, 1000000, "Q8Rw/2/1 x3"},
    {1024, 33, 10, 0, "F16Tile128/0/0 x3"},
    {1024, 33, 10, 200000, "Q8Rw/2/1 x3 tail"},
    {1024, 33, 200, 1000000, "Q8Rw/2/1 x5"},
    {1024, 33, 200, 0, "F16Tile128/0/0 x5"},
    {1024, 33, 200, 200000, "Q8Rw/2/1 x5 tail"},
    {1024, 64, 10, 1000000, "Q8Rw/2/1 x3"},
    {1024, 64, 10, 0, "F16Tile128/0/0 x3"},
    {1024, 64, 10, 200000, "Q8Rw/2/1 x3 tail"},
    {1024, 64, 200, 1000000, "Q8Rw/2/1 x5"},
    {1024, 64, 200, 0, "F16Tile128/0/0 x5"},
    {1024, 64, 200, 200000, "Q8Rw/2/1 x5 tail"},
    {1024, 65, 10, 1000000, "Q8Rw/2/2 x3"},
    {1024, 65, 10, 0, "F16Tile128/0/0 x3"},
    {1024, 65, 10, 200000, "Q8Rw/2/2 x3 tail"},
    {1024, 65, 200, 1000000, "Q8Rw/2/2 x5"},
    {1024, 65, 200, 0, "F16Tile128/0/0 x5"},
    {1024, 65, 200, 200000, "Q8Rw/2/2 x5 tail"},
    {1024, 128, 10, 1000000, "Q8Rw/2/2 x3"},
    {1024, 128, 10, 0, "F16Tile128/0/0 x3"},
    {1024, 128, 10, 200000, "Q8Rw/2/2 x3 tail"},
    {1024, 128, 200, 1000000, "Q8Rw/2/2 x5"},
    {1024, 128, 200, 0, "F16Tile128/0/0 x5"},
    {1024, 128, 200, 200000, "Q8Rw/2/2 x5 tail"},
    {1024, 129, 10, 1000000, "Q8Rw/2/3 x3"},
    {1024, 129, 10, 0, "F16Tile256/0/0 x3"},
    {1024, 129, 10, 200000, "Q8Rw/2/3 x3 tail"},
    {1024, 129, 200, 1000000, "Q8Rw/2/3 x5"},
    {1024, 129, 200, 0, "F16Tile256/0/0 x5"},
    {1024, 129, 200, 200000, "Q8Rw/2/3 x5 tail"},
    {1024, 300, 10, 1000000, "Q8Rw/2/5 x3"},
    {1024, 300, 10, 0, "F16Tile256/0/0 x3"},
    {1024, 300, 10, 200000, "Q8Rw/2/5 x3 tail"},
    {1024, 300, 200, 1000000, "Q8Rw/2/5 x5"},
    {1024, 300, 200, 0, "F16Tile256/0/0 x5"},
    {1024, 300, 200, 200000, "Q8Rw/2/5 x5 tail"},
    {1024, 1000, 10, 1000000, "Q8Rw/2/16 x3"},
    {1024, 1000, 10, 0, "F16Tile256/0/0 x3"},
    {1024, 1000, 10, 200000, "Q8Rw/2/16 x3 tail"},
    {1024, 1000, 200, 1000000, "Q8Rw/2/16 x5"},
    {1024, 1000, 200, 0, "F16Tile256/0/0 x5"},
    {1024, 1000, 200, 200000, "Q8Rw/2/16 x5 tail"},
    {1024, 2100, 10, 1000000, "Q8Tile256/0/0 x3"},
    {1024, 2100, 10, 0, "F16Tile256/0/0 x3"},
    {1024, 2100, 10, 200000, "Q8Tile256/0/0 x3 tail"},
    {1024, 2100, 200, 1000000, "Q8Tile256/0/0 x5"},
    {1024, 2100, 200, 0, "F16Tile256/0/0 x5"},
    {1024, 2100, 200, 200000, "Q8Tile256/0/0 x5 tail"},
};

int main() {
    int bad = 0;
    const auto check = [&](const std::string& got, const char* want, const char* what) {
        if (got == want) return;
        ++bad;
        printf("MISMATCH %s\n  want %s\n  got  %s\n", what, want, got.c_str());
    };
    for (const PhaseCase& c : kPhases) {
        char what[128];
        snprintf(what, sizeof what, "knobs %d dim %u rows %llu nq %u k %u q8 %llu", (int)c.knobs, c.dim,
                 (unsigned long long)c.rows, c.nq, c.k, (unsigned long long)c.q8_rows);
        check(describe(plan_filter(c.dim, c.rows, c.nq, c.k, c.q8_rows, true, 256, knobs(c.knobs))), c.plan, what);
    }
    for (const KernelCase& c : kKernels) {
        char what[128];
        snprintf(what, sizeof what, "dim %u nq %u k %u q8 %llu", c.dim, c.nq, c.k, (unsigned long long)c.q8_rows);
        check(kernel_choice(plan_filter(c.dim, 1000000, c.nq, c.k, c.q8_rows, true, 256, FilterKnobs())), c.choice, what);
    }
    // the counts DESIGN.md and filter_plan.hpp quote: 10M rows take 5 filter phases at k = 200 and 3 at k = 10, 1M rows 2
    // at k = 10, 100,000 rows one round
    const FilterKnobs kn;
    const uint32_t quoted[][3] = {{10000000, 200, 5}, {10000000, 10, 3}, {1000000, 10, 2}, {100000, 10, 1}};
    for (const auto& q : quoted)
        if (plan_filter(384, q[0], 1, q[1], q[0] / 128 * 128, true, 256, kn).nphases != q[2] + 1) {
            ++bad;
            printf("MISMATCH %u rows k = %u: not %u filter phases\n", q[0], q[1], q[2]);
        }
    if (bad) return 1;
    printf("filter plan ok: %zu plans, %zu kernel choices\n", sizeof kPhases / sizeof kPhases[0],
           sizeof kKernels / sizeof kKernels[0]);
    return 0;
}
