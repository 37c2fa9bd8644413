// pik_memetic_plan.hpp -- how a memetic call is enqueued, stated once for the three launchers that enqueue one:
// launch_solve (pik_launch.hpp), the routed launcher (pik_route.hpp) and the launcher of a restart attempt
// (pik_restart.hpp).  The slot's scratch layout, the schedule the handle's options ask for, the regime's thresholds,
// the candidate kernel variants with their ids, the range table of a regime, the rule that a small call has no
// passes, and which variants a pass enqueues.  Host arithmetic only: no kernel, no device function and no HIP call,
// so a host-only program can include it (tests/native/memetic_plan_check.cpp), and pick_ik_amd/build.py flavour_sha
// does not read it.  No result depends on anything decided here: the variants and the passes re-order the same
// arithmetic.
#pragma once

#include "pik_solver.hpp"

namespace pik {

constexpr int PLAN_WAVE = 64;           // lanes of a wavefront (pik_kernels.hpp WAVE)
constexpr int PLAN_MAX_VARIANTS = 8;
constexpr long long PLAN_ANY = 0xffffffffll; // the upper end of the last range: every survivor count

inline int pow2ceil_log2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// Per-slot scratch of a memetic call of B problems, S species: parked state (one record per problem and species,
// d_rows doubles + l_rows long longs + i_rows ints: StateRows<D> of pik_kernels.hpp), two survivor lists and, for
// chains with unbounded variables, the stored population: 2 parities x (P fitness + P*D genes + P ints order) per
// problem and species.
inline bool chain_has_unbounded(const pikamd_solver* s) { return s->chain.bounded_mask != ((1u << s->chain.dof) - 1u); }

struct MemeticScratch {
    size_t off_d, off_l, off_i, off_list, off_pop, pop_stride, total;
    bool has_unbounded;
    MemeticScratch(long long B, int S, int population, int D, bool unbounded, size_t d_rows, size_t l_rows, size_t i_rows) {
        const size_t recs = (size_t)B * (size_t)S;
        off_d = 0;
        off_l = off_d + sizeof(double) * d_rows * recs;
        off_i = off_l + sizeof(long long) * l_rows * recs;
        off_list = off_i + sizeof(int) * i_rows * recs;
        const size_t off_cnt = off_list + sizeof(int) * 2 * (size_t)B;
        has_unbounded = unbounded;
        pop_stride = (size_t)population * (1 + D) + ((size_t)population + 1) / 2;
        off_pop = (off_cnt + 64 + 63) / 64 * 64;
        total = off_pop + (has_unbounded ? sizeof(double) * 2 * pop_stride * (size_t)B * (size_t)S : 0);
    }
};

// launch schedule of a memetic call
struct Schedule {
    // forced lanes per elite (experiments / tests): passes starting at generation >= lpe_from[i] run
    // with lpe_of[i]; n_sched == 0: adaptive (the default, see plan_pass)
    int lpe_from[4] = {0, 0, 0, 0}, lpe_of[4] = {1, 1, 1, 1}, n_sched = 0;
    int marks[16], n_marks = 0;
    bool occ2_ok = true;
    long long occ2_from = 0;
};

// the handle's scheduling options (pikamd_set_option) -> the launch schedule of one call
inline void make_schedule(const pikamd_solver* s, const ParamsK& pk, int gs, int S, Schedule& sc) {
    const bool multi = s->n_tips > 1;
    const SolverOptions& o = s->opt;
    auto ok = [&](int v) { return lpe_allowed(s, v, gs, S, multi); };
    if (o.lpe > 0 && ok(o.lpe)) {
        sc.lpe_of[0] = o.lpe;
        sc.n_sched = 1;
    }
    if (o.n_sched > 0) {
        bool good = true;
        for (int i = 0; i < o.n_sched; ++i) good = good && ok(o.sched_of[i]);
        if (good) {
            sc.n_sched = o.n_sched;
            for (int i = 0; i < o.n_sched; ++i) {
                sc.lpe_from[i] = o.sched_from[i];
                sc.lpe_of[i] = o.sched_of[i];
            }
        }
    }
    if (S != 1 && sc.n_sched > 1) sc.n_sched = 1; // (species: one choice for all passes when forced)
    if (multi && sc.n_sched > 0 && !ok(sc.lpe_of[0])) sc.n_sched = 0; // (a request several tips cannot serve: adaptive)
    if (multi && sc.n_sched > 1) sc.n_sched = 1;
    (void)ok;
    // Compaction passes: generation marks at which still-running problems are parked in HBM and
    // re-packed densely for the next launch (results do not depend on the marks).  Dense in the
    // tail: the survivor count halves every ~10 generations, and every pass re-chooses the lanes
    // per elite for the survivors it gets.
    {
        static const int default_marks[] = {2, 4, 8, 12, 16, 24, 32, 40, 48, 64, 80};
        const int* m = o.passes_set ? o.marks : default_marks;
        const int n = o.passes_set ? o.n_marks : (int)(sizeof default_marks / sizeof default_marks[0]);
        (void)S; // (several species park and resume like one: a record per (problem, species))
        for (int i = 0; i < n && sc.n_marks < 15; ++i)
            if (m[i] > 0 && m[i] < pk.max_generations && (sc.n_marks == 0 || m[i] > sc.marks[sc.n_marks - 1]))
                sc.marks[sc.n_marks++] = m[i];
    }
    sc.occ2_ok = S == 1;
    // first-pass wavefronts from which the two-per-SIMD variant pays (measured crossover with
    // overlapped batches on 1024 SIMDs: slower at 512, +3 % at 640, +5 % at 768, +26 % at 1024)
    sc.occ2_from = (long long)s->num_cu * 4 * 5 / 8;
    if (o.two_per_simd >= 0) {
        sc.occ2_ok = sc.occ2_ok && o.two_per_simd != 0;
        if (o.two_per_simd > 1) sc.occ2_from = o.two_per_simd; // (explicit threshold)
    }
    if (o.force_occ2) sc.occ2_from = 0;
}

// one kernel variant: lanes per elite, its id (5 / 4 / 3 / 2 = 16 / 8 / 4 / 2 lanes, 1 = one lane, 7 = one lane compiled
// for two wavefronts per SIMD; several tip frames: 10 / 9 / 8 = 16 / 8 / 2 lanes, 6 = one), wavefronts the chip holds of it
struct MemeticVariant {
    int lpe, id;
    long long capacity;
};

struct MemeticPlan {
    int gs_log2, sp_log2;
    int gs, S, sp; // lanes of an elite group, species, groups of a wavefront per problem (pow2ceil(S))
    bool multi;
    Schedule sc;
    MemeticVariant var[PLAN_MAX_VARIANTS]; // candidates, widest first (plan_candidates)
    int n_var;
    long long groups_per_wave(int v) const { return PLAN_WAVE / (gs * var[v].lpe * sp); }
};

// groups of GS * LPE lanes per problem; species: pow2ceil(S) groups per problem share a wavefront and park / resume together
inline void plan_begin(const pikamd_solver* s, const pikamd_params* p, const ParamsK& pk, MemeticPlan& pl) {
    pl.gs_log2 = pow2ceil_log2(pk.elites);
    pl.gs = 1 << pl.gs_log2;
    pl.S = p->memetic_num_threads > 1 ? p->memetic_num_threads : 1;
    pl.sp_log2 = pow2ceil_log2(pl.S);
    pl.sp = 1 << pl.sp_log2;
    pl.multi = s->n_tips > 1;
    pl.n_var = 0;
    make_schedule(s, pk, pl.gs, pl.S, pl.sc);
}

// Regime.  More lanes per elite buy latency with throughput (a problem-generation costs 31 us of
// SIMD time at one lane per elite, 68 / 95 / 158 us at 4 / 8 / 16): right when the chip would
// otherwise idle behind this call's long-running problems, wrong when other calls are queued up
// to use it.  Measured (512 x 4096-problem steps in pools of 64): 2 calls in flight 4.14 (adaptive)
// vs 3.84 M solves/s (one lane per elite everywhere), 4 calls in flight 4.32 vs 4.69.  So: with
// three or more OTHER calls of this handle still in flight (others_busy, asked by the launcher), every pass
// uses one lane per elite -- unless the option "regime" forces one.
inline bool plan_throughput(const pikamd_solver* s, bool others_busy) {
    return s->opt.regime != 0 ? s->opt.regime == 2 : others_busy;
}

// First-pass wavefronts from which the two-per-SIMD variant of the one-lane kernel is taken: the schedule's figure
// (5/8 of the SIMD count) with other calls queued up; a call with the chip to itself takes it only when its
// wavefronts outnumber the SIMDs (measured on the driver's 20-batch pool: threshold 5/8 -> 9/8 of the SIMD count:
// 2.85 -> 2.90 M solves/s).
inline long long plan_occ2_from(const pikamd_solver* s, const Schedule& sc, bool throughput) {
    if (!throughput && s->opt.two_per_simd < 2 && !s->opt.force_occ2) return (long long)s->num_cu * 4 * 9 / 8;
    return sc.occ2_from;
}

// Candidate variants, widest first.  wide_ok: the variants with several lanes per elite are candidates (not in the
// throughput regime, unless a forced schedule may ask for any); two_per_simd_built: the kernels have that build
// (D <= 9: its LDS footprint, 6 D rows, lets 5..8 wavefronts share a CU up to D = 9; beyond that the register cap
// would cost scratch traffic for nothing.  The exact flavours have it too: their descent and evaluations are calls
// that need fewer than 256 registers, and a second wavefront per SIMD hides the latencies a lone one waits out).
inline void plan_candidates(const pikamd_solver* s, MemeticPlan& pl, bool wide_ok, bool two_per_simd_built,
                            bool exact = EXACT_FLAVOUR) {
    auto add = [&](int lpe, int id) { pl.var[pl.n_var++] = MemeticVariant{lpe, id, 0}; };
    auto ok = [&](int v) { return wide_ok && lpe_allowed(s, v, pl.gs, pl.S, pl.multi, exact); };
    pl.n_var = 0;
    if (pl.multi) {
        // (16 / 8 lanes for several tips: the product flavours' cooperative descent)
        if (!exact && ok(16)) add(16, 10);
        if (!exact && ok(8)) add(8, 9);
        if (ok(2)) add(2, 8);
        add(1, 6);
        return;
    }
    if (ok(16)) add(16, 5);
    if (ok(8)) add(8, 4);
    if (ok(4)) add(4, 3);
    if (ok(2)) add(2, 2);
    add(1, 1);
    bool occ2 = two_per_simd_built && pl.sc.occ2_ok && !(disabled_lanes_of(s, exact) & 1u);
    // (the exact flavours, a floating or a mimic joint: the literal descent, one per SIMD only)
    if (exact) occ2 = occ2 && s->chain.float_mask == 0u && s->chain.n_mimic == 0;
    if (occ2) add(1, 7);
}

// The range table of one regime.  Adaptive rule: a pass runs with the MOST lanes per elite whose wavefronts still
// fit the chip in one round for the problems it has (fewest generations' latency without queueing); the one-lane
// variant takes everything larger, compiled for two wavefronts per SIMD from the measured crossover on.  Entry i
// is candidate var[i] and serves problem counts in (lo[i], hi[i]] -- lo is the hi of the entry before, an entry
// with hi == lo serves none; the throughput regime has the one-lane variants only.
struct RangeTable {
    int n;
    int var[PLAN_MAX_VARIANTS];
    long long lo[PLAN_MAX_VARIANTS], hi[PLAN_MAX_VARIANTS];
    long long occ2_from_problems;
};

inline void plan_ranges(const pikamd_solver* s, const MemeticPlan& pl, bool throughput, RangeTable& t) {
    t.occ2_from_problems = plan_occ2_from(s, pl.sc, throughput) * PLAN_WAVE / pl.gs; // first-pass wavefronts -> problems
    t.n = 0;
    long long lo = 0;
    for (int i = 0; i < pl.n_var; ++i) {
        const MemeticVariant& v = pl.var[i];
        if (throughput && v.lpe > 1) continue;
        long long hi = (v.lpe > 1) ? (long long)s->num_cu * 4 * pl.groups_per_wave(i) // one wavefront per SIMD
                       : (v.id == 7 || i == pl.n_var - 1) ? PLAN_ANY
                                                          : t.occ2_from_problems - 1;
        if (hi < lo) hi = lo;
        if (hi > PLAN_ANY) hi = PLAN_ANY;
        t.var[t.n] = i;
        t.lo[t.n] = lo;
        t.hi[t.n] = hi;
        ++t.n;
        lo = hi;
    }
}

// The passes of a restart attempt when the option "passes" is not set: two of the default marks.  The problems of
// a restart attempt are the few a whole solve has failed on; what a pass re-packs is the tail of a tail, and every
// mark costs an empty dispatch per candidate variant when nothing is left.
inline bool restart_default_mark(int generation) { return generation == 8 || generation == 32; }

// The generation marks of a call that can have n problems; returns their number.  A call whose problems each get a
// wavefront of the widest variant in one round gains nothing from compaction (there is nothing to re-pack into):
// one launch, no passes -- 3-6 % off the latency of the plugin-style calls (B = 1 .. 256).  Not in the throughput
// regime, where the one-lane wavefronts hold 16 problems each and re-packing is what keeps them full.
inline int plan_marks(const pikamd_solver* s, const MemeticPlan& pl, bool throughput, long long n, bool restart,
                      int marks[16]) {
    int n_marks = 0;
    for (int i = 0; i < pl.sc.n_marks; ++i)
        if (!restart || s->opt.passes_set || restart_default_mark(pl.sc.marks[i])) marks[n_marks++] = pl.sc.marks[i];
    if (!throughput && pl.sc.n_sched == 0 && !s->opt.passes_set) {
        int widest = 1;
        for (int l : {16, 8, 4, 2})
            if (widest == 1 && lpe_allowed(s, l, pl.gs, pl.S, pl.multi)) widest = l;
        if (widest > 1 && n <= (long long)s->num_cu * 4 * (PLAN_WAVE / (pl.gs * widest * pl.sp))) n_marks = 0;
    }
    return n_marks;
}

// wavefronts of a launch: what n problems need, at most what the chip holds of the variant
inline long long plan_grid(long long n, long long groups_per_wave, long long capacity) {
    const long long waves_needed = (n + groups_per_wave - 1) / groups_per_wave;
    return waves_needed < capacity ? waves_needed : capacity;
}

// What a pass that starts at generation start_gen enqueues under the host's rule: candidates (indices into pl.var)
// with the survivor counts sel_lo < n <= sel_hi each runs for.  `size`: the most problems the pass can have;
// `known` > 0: the host knows how many it has; `counted`: the kernels find the count on the device (without one a
// variant cannot select itself: it runs for any).
// Forced schedule: one pick -- with one lane per elite and a call that fills the chip, the two-per-SIMD build.
// Adaptive: the one variant whose range holds the known size, or every variant `size` problems can reach.
struct PassLaunch {
    int var;
    unsigned sel_lo, sel_hi;
};

inline int plan_pass(const MemeticPlan& pl, const RangeTable& t, int start_gen, long long size, long long known,
                     bool counted, PassLaunch out[PLAN_MAX_VARIANTS]) {
    const Schedule& sc = pl.sc;
    if (sc.n_sched > 0) {
        int lpe_k = sc.lpe_of[0];
        for (int i = 1; i < sc.n_sched; ++i)
            if (start_gen >= sc.lpe_from[i]) lpe_k = sc.lpe_of[i];
        int pick = -1;
        for (int i = 0; i < pl.n_var && pick < 0; ++i)
            if (pl.var[i].lpe == lpe_k) pick = i; // (one lane per elite: the one-per-SIMD build comes first)
        if (pick < 0) pick = pl.n_var - 1;
        if (pl.var[pick].lpe == 1 && pl.var[pl.n_var - 1].id == 7 && size >= t.occ2_from_problems) pick = pl.n_var - 1;
        out[0] = PassLaunch{pick, 0u, (unsigned)PLAN_ANY};
        return 1;
    }
    int n = 0;
    for (int i = 0; i < t.n; ++i) {
        // (a pass cannot have more problems than `size`: narrower variants whose range starts beyond that are not enqueued)
        if (!(size > t.lo[i] && t.hi[i] > t.lo[i]) || (known > 0 && known > t.hi[i])) continue;
        out[n++] = counted ? PassLaunch{t.var[i], (unsigned)t.lo[i], (unsigned)t.hi[i]}
                           : PassLaunch{t.var[i], 0u, (unsigned)PLAN_ANY};
    }
    return n;
}

} // namespace pik
