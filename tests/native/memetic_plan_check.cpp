// The launch plan of a memetic call (pick_ik_amd/csrc/pik_memetic_plan.hpp): candidates, range tables, marks, what a
// pass enqueues, the scratch layout and the grid formula, held to values worked out by hand from the rules the three
// launchers had written out each (a chip of 256 CUs = 1024 SIMDs, wavefronts of 64 lanes).  Host only: compiled by
// tests/test_build_cpu.py as HIP host code (the header reaches hip_runtime.h), no device needed to run it.
#include <cstdio>
#include <initializer_list>
#include <memory>
#include <vector>

#include "../../pick_ik_amd/csrc/pik_memetic_plan.hpp"

static int bad = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("line %d: %s\n", __LINE__, #cond);               \
            ++bad;                                                       \
        }                                                                \
    } while (0)

using namespace pik;
constexpr long long ANY = 0xffffffffll;

struct Setup {
    std::unique_ptr<pikamd_solver> s{new pikamd_solver()};
    pikamd_params p{};
    ParamsK pk{};
    explicit Setup(int elites = 4, int species = 1) {
        s->num_cu = 256;
        s->chain.dof = 7;
        s->chain.bounded_mask = 0x7fu;
        p.mode = 0;
        p.memetic_num_threads = species;
        pk.elites = elites;
        pk.population = 16;
        pk.max_generations = 100;
    }
    MemeticPlan plan(bool wide_ok, bool two_per_simd_built = true, bool exact = false) const {
        MemeticPlan pl;
        plan_begin(s.get(), &p, pk, pl);
        plan_candidates(s.get(), pl, wide_ok, two_per_simd_built, exact);
        return pl;
    }
};

static std::vector<int> ids(const MemeticPlan& pl) {
    std::vector<int> v;
    for (int i = 0; i < pl.n_var; ++i) v.push_back(pl.var[i].id);
    return v;
}
static std::vector<int> ids(const MemeticPlan& pl, const RangeTable& t) {
    std::vector<int> v;
    for (int i = 0; i < t.n; ++i) v.push_back(pl.var[t.var[i]].id);
    return v;
}
static std::vector<long long> his(const RangeTable& t) { return std::vector<long long>(t.hi, t.hi + t.n); }
static std::vector<long long> los(const RangeTable& t) { return std::vector<long long>(t.lo, t.lo + t.n); }
static RangeTable ranges(const Setup& c, const MemeticPlan& pl, bool throughput) {
    RangeTable t;
    plan_ranges(c.s.get(), pl, throughput, t);
    return t;
}
using VI = std::vector<int>;
using VL = std::vector<long long>;

int main() {
    {   // four elites, one species, one tip, every width allowed, default options, D <= 9
        Setup c;
        const MemeticPlan lat = c.plan(true);
        CHECK(lat.gs == 4 && lat.S == 1 && lat.sp == 1 && !lat.multi && lat.sc.n_sched == 0);
        CHECK(ids(lat) == (VI{5, 4, 3, 2, 1, 7}));
        const RangeTable tl = ranges(c, lat, false);
        CHECK(ids(lat, tl) == (VI{5, 4, 3, 2, 1, 7}));
        CHECK(his(tl) == (VL{1024, 2048, 4096, 8192, 18431, ANY})); // 18431 = 256 * 4 * 9 / 8 * 64 / 4 - 1
        CHECK(los(tl) == (VL{0, 1024, 2048, 4096, 8192, 18431}));
        // throughput: the host rule has the one-lane candidates only; the routed launcher all, and a table without the wide
        const MemeticPlan thr = c.plan(false);
        CHECK(ids(thr) == (VI{1, 7}));
        CHECK(his(ranges(c, thr, true)) == (VL{10239, ANY})); // 10239 = 256 * 4 * 5 / 8 * 16 - 1
        const RangeTable tt = ranges(c, lat, true);
        CHECK(ids(lat, tt) == (VI{1, 7}) && his(tt) == (VL{10239, ANY}) && los(tt) == (VL{0, 10239}));
        CHECK(tt.var[0] == 4 && tt.var[1] == 5); // (the routed launcher's counters are indexed by candidate)
        // the regime and its two thresholds
        CHECK(!plan_throughput(c.s.get(), false) && plan_throughput(c.s.get(), true));
        CHECK(plan_occ2_from(c.s.get(), lat.sc, false) == 1152 && plan_occ2_from(c.s.get(), lat.sc, true) == 640);
        c.s->opt.regime = 1;
        CHECK(!plan_throughput(c.s.get(), true));
        c.s->opt.regime = 2;
        CHECK(plan_throughput(c.s.get(), false));
        c.s->opt.regime = 0;

        // pass 0 of the host rule: one launch, for any count
        const int want0[][2] = {{1, 5}, {1024, 5}, {1025, 4}, {8193, 1}, {18432, 7}};
        for (const auto& w : want0) {
            PassLaunch q[PLAN_MAX_VARIANTS];
            const int n = plan_pass(lat, tl, 0, w[0], w[0], false, q);
            CHECK(n == 1 && lat.var[q[0].var].id == w[1] && q[0].sel_lo == 0u && q[0].sel_hi == 0xffffffffu);
        }
        {   // a later pass of a call of 3000 problems: every variant 3000 survivors can reach, nothing narrower
            PassLaunch q[PLAN_MAX_VARIANTS];
            const int n = plan_pass(lat, tl, 8, 3000, 0, true, q);
            CHECK(n == 3);
            const unsigned want[][3] = {{5, 0, 1024}, {4, 1024, 2048}, {3, 2048, 4096}};
            for (int i = 0; i < 3 && i < n; ++i)
                CHECK((unsigned)lat.var[q[i].var].id == want[i][0] && q[i].sel_lo == want[i][1] && q[i].sel_hi == want[i][2]);
            // pass 0 of a restart attempt: from a counted list -- the one variant for a known size, with its range
            CHECK(plan_pass(lat, tl, 0, 1500, 1500, true, q) == 1 && lat.var[q[0].var].id == 4 && q[0].sel_lo == 1024u && q[0].sel_hi == 2048u);
            // ... and every reachable one when the host does not know it
            CHECK(plan_pass(lat, tl, 0, 1500, 0, true, q) == 2 && lat.var[q[1].var].id == 4);
        }
        // marks: a call the widest variant serves in one round has none; a restart attempt has 8 and 32
        int m[16];
        CHECK(plan_marks(c.s.get(), lat, false, 1024, false, m) == 0);
        CHECK(plan_marks(c.s.get(), lat, false, 1024, true, m) == 0);
        CHECK(plan_marks(c.s.get(), lat, false, 1025, false, m) == 11);
        CHECK((VI(m, m + 11) == VI{2, 4, 8, 12, 16, 24, 32, 40, 48, 64, 80}));
        CHECK(plan_marks(c.s.get(), lat, false, 1025, true, m) == 2 && m[0] == 8 && m[1] == 32);
        CHECK(plan_marks(c.s.get(), lat, true, 1, false, m) == 11); // (throughput regime: re-packing keeps the wavefronts full)
        c.pk.max_generations = 30;
        const MemeticPlan few = c.plan(true);
        CHECK(plan_marks(c.s.get(), few, false, 1025, false, m) == 6 && m[5] == 24);
        CHECK(plan_marks(c.s.get(), few, false, 1025, true, m) == 1 && m[0] == 8);
        c.pk.max_generations = 100;
        c.s->opt.passes_set = true; // option "passes": the caller's marks, for every size and for restart attempts too
        c.s->opt.n_marks = 2;
        c.s->opt.marks[0] = 5;
        c.s->opt.marks[1] = 10;
        const MemeticPlan own = c.plan(true);
        CHECK(plan_marks(c.s.get(), own, false, 1, false, m) == 2 && m[0] == 5 && m[1] == 10);
        CHECK(plan_marks(c.s.get(), own, false, 1, true, m) == 2 && m[0] == 5 && m[1] == 10);
    }
    {   // no two-per-SIMD build (D >= 10) or option two_per_simd = 0: no id 7, id 1 takes the rest
        Setup c;
        const MemeticPlan long_chain = c.plan(true, false);
        CHECK(ids(long_chain) == (VI{5, 4, 3, 2, 1}));
        CHECK(his(ranges(c, long_chain, false)) == (VL{1024, 2048, 4096, 8192, ANY}));
        c.s->opt.two_per_simd = 0;
        const MemeticPlan never = c.plan(true);
        CHECK(ids(never) == (VI{5, 4, 3, 2, 1}));
        CHECK(his(ranges(c, never, false)) == (VL{1024, 2048, 4096, 8192, ANY}));
        CHECK(his(ranges(c, c.plan(false), true)) == (VL{ANY}));
        c.s->opt.two_per_simd = 700; // an explicit threshold holds in both regimes: 700 * 16 - 1
        const MemeticPlan at700 = c.plan(true);
        CHECK(ids(at700) == (VI{5, 4, 3, 2, 1, 7}));
        CHECK(his(ranges(c, at700, false)) == (VL{1024, 2048, 4096, 8192, 11199, ANY}));
        CHECK(his(ranges(c, at700, true)) == (VL{11199, ANY}));
        c.s->opt.two_per_simd = -1;
        c.s->opt.disabled_lanes = 1u | 8u; // the self test switched the two-per-SIMD build and 8 lanes off
        CHECK(ids(c.plan(true)) == (VI{5, 3, 2, 1}));
        CHECK(ids(c.plan(true, true, true)) == (VI{5, 4, 3, 2, 1, 7})); // (the exact flavour keeps its own set)
        c.s->opt.disabled_lanes = 0u;
        c.s->chain.n_mimic = 1; // a mimic joint: the exact flavours' literal descent, one per SIMD only
        CHECK(ids(c.plan(true, true, true)) == (VI{5, 4, 3, 2, 1}) && ids(c.plan(true)) == (VI{5, 4, 3, 2, 1, 7}));
    }
    {   // force_occ2 (the self test): id 1's range is empty, id 7 takes everything behind the last wide variant
        Setup c;
        c.s->opt.force_occ2 = true;
        const MemeticPlan pl = c.plan(true);
        const RangeTable tl = ranges(c, pl, false), tt = ranges(c, pl, true);
        CHECK(his(tl) == (VL{1024, 2048, 4096, 8192, 8192, ANY}) && tl.lo[5] == 8192);
        CHECK(his(tt) == (VL{0, ANY}) && tt.lo[1] == 0);
        PassLaunch q[PLAN_MAX_VARIANTS];
        CHECK(plan_pass(pl, tl, 0, 8193, 8193, false, q) == 1 && pl.var[q[0].var].id == 7);
        CHECK(plan_pass(pl, tl, 8, 100000, 0, true, q) == 5 && pl.var[q[4].var].id == 7 && q[4].sel_lo == 8192u);
    }
    {   // a forced schedule: one pick per pass; one lane per elite and a call that fills the chip: the two-per-SIMD build
        Setup c;
        c.s->opt.lpe = 1;
        const MemeticPlan pl = c.plan(true);
        CHECK(pl.sc.n_sched == 1);
        const RangeTable tl = ranges(c, pl, false);
        PassLaunch q[PLAN_MAX_VARIANTS];
        CHECK(plan_pass(pl, tl, 0, 18432, 18432, false, q) == 1 && pl.var[q[0].var].id == 7 && q[0].sel_lo == 0u && q[0].sel_hi == 0xffffffffu);
        CHECK(plan_pass(pl, tl, 0, 18431, 18431, false, q) == 1 && pl.var[q[0].var].id == 1);
        CHECK(plan_pass(pl, tl, 12, 18432, 0, true, q) == 1 && pl.var[q[0].var].id == 7 && q[0].sel_hi == 0xffffffffu);
        int m[16];
        CHECK(plan_marks(c.s.get(), pl, false, 1, false, m) == 11); // (forced: the passes stay)
        c.s->opt.lpe = 0; // "lanes_per_elite_schedule": 8 lanes, 2 from generation 12 on
        c.s->opt.n_sched = 2;
        c.s->opt.sched_of[0] = 8;
        c.s->opt.sched_from[1] = 12;
        c.s->opt.sched_of[1] = 2;
        const MemeticPlan two = c.plan(true);
        CHECK(two.sc.n_sched == 2);
        CHECK(plan_pass(two, tl, 8, 5, 0, true, q) == 1 && two.var[q[0].var].id == 4);
        CHECK(plan_pass(two, tl, 12, 5, 0, true, q) == 1 && two.var[q[0].var].id == 2);
    }
    {   // larger elite groups: the widths that fit a wavefront
        Setup c16(16), c9(9), c64(64);
        const MemeticPlan p16 = c16.plan(true), p9 = c9.plan(true), p64 = c64.plan(true);
        CHECK(p16.gs == 16 && p9.gs == 16 && p64.gs == 64);
        CHECK(ids(p16) == (VI{3, 2, 1, 7}) && ids(p9) == (VI{3, 2, 1, 7}));
        CHECK(his(ranges(c16, p16, false)) == (VL{1024, 2048, 4607, ANY})); // 1152 * 64 / 16 - 1
        CHECK(his(ranges(c16, p16, true)) == (VL{2559, ANY}));              // 640 * 64 / 16 - 1
        CHECK(ids(p64) == (VI{1, 7}));
        CHECK(his(ranges(c64, p64, false)) == (VL{1151, ANY}) && his(ranges(c64, p64, true)) == (VL{639, ANY}));
        int m[16];
        CHECK(plan_marks(c16.s.get(), p16, false, 1024, false, m) == 0 && plan_marks(c16.s.get(), p16, false, 1025, false, m) == 11);
        CHECK(plan_marks(c64.s.get(), p64, false, 1, false, m) == 11); // (no wide variant: nothing to gain)
        // two species: a pair of groups per problem; no two-per-SIMD build
        Setup sp(4, 2);
        const MemeticPlan p2 = sp.plan(true);
        CHECK(p2.S == 2 && p2.sp == 2 && ids(p2) == (VI{4, 3, 2, 1}));
        CHECK(his(ranges(sp, p2, false)) == (VL{1024, 2048, 4096, ANY}));
        CHECK(p2.groups_per_wave(0) == 1 && p2.groups_per_wave(3) == 8);
    }
    {   // several tip frames: the cooperative 16 / 8 lanes of the product flavours, the pair, one lane
        Setup c;
        c.s->n_tips = 2;
        CHECK(ids(c.plan(true)) == (VI{10, 9, 8, 6}) && ids(c.plan(true, true, true)) == (VI{8, 6}) && ids(c.plan(false)) == (VI{6}));
        const MemeticPlan pl = c.plan(true);
        CHECK(his(ranges(c, pl, false)) == (VL{1024, 2048, 8192, ANY}));
    }
    {   // the scratch layout: 10 problems, records of 100 doubles + 3 long longs + 5 ints, population 16, 7 variables
        const MemeticScratch b(10, 1, 16, 7, false, 100, 3, 5), u(10, 1, 16, 7, true, 100, 3, 5), u2(10, 2, 16, 7, true, 100, 3, 5);
        CHECK(b.off_d == 0 && b.off_l == 8000 && b.off_i == 8240 && b.off_list == 8440 && b.off_pop == 8640);
        CHECK(b.pop_stride == 136 && b.total == 8640 && !b.has_unbounded);
        CHECK(u.off_l == 8000 && u.off_i == 8240 && u.off_list == 8440 && u.off_pop == 8640 && u.total == 8640 + 21760 && u.has_unbounded);
        CHECK(u2.off_l == 16000 && u2.off_i == 16480 && u2.off_list == 16880 && u2.off_pop == 17024 && u2.total == 17024 + 43520);
        Setup c;
        CHECK(!chain_has_unbounded(c.s.get()));
        c.s->chain.bounded_mask = 0x3fu;
        CHECK(chain_has_unbounded(c.s.get()));
    }
    // the grid: what the problems need, at most what the chip holds
    CHECK(plan_grid(100, 4, 10) == 10 && plan_grid(100, 4, 1000) == 25 && plan_grid(101, 4, 1000) == 26 && plan_grid(1, 16, 2048) == 1);
    if (bad) return 1;
    std::printf("memetic plan check OK\n");
    return 0;
}
