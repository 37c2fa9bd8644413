// pik_search.hpp -- local IK with random restarts in one launch (pikamd_search_batch).
//
// searchPositionIK (src/pick_ik_plugin.cpp:145-291) solves, and when no solution came back draws a random valid
// configuration and solves again from there.  As a host loop that is up to max_attempts pikamd_solve_batch round
// trips.  Local mode draws no random numbers and the restart states are keyed by (seed, problem, attempt), so the
// attempts of one problem are independent computations: the kernels here wrap the EXISTING local-mode descents
// (pik_kernels.hpp: PIK_DESCENT(GD_LOCAL, ...), gd_wide, gd_wide_multi) in a loop over the attempts of a WORK UNIT
// (problem b, first attempt a0, number of attempts n):
//   sequential schedule: one unit per problem, n = max_attempts -- a lane (or a team of lanes) walks its problem's
//                        attempts, writes the primary outputs while the problem is open and leaves the loop when no
//                        unit of the wavefront is open;
//   parallel schedule:   max_attempts units per problem, n = 1 -- every attempt of every problem is on the chip at
//                        once and writes one row; search_finalize_kernel, stream-ordered behind them, applies the
//                        loop's rule per problem (the first attempt with status > 0 wins).
// A unit loads its goal once and per attempt computes the attempt's start (the validity test of the initial guess
// and the draws in front of the attempt) and runs GradientIk::from + the loop + the post-loop exactly as
// ik_gradient_kernel does, including the cost of the attempt's start on failure.
//
// The result is defined as what the loop of pikamd_solve_batch calls returns (include/pick_ik_amd.h), and every
// variant below performs the arithmetic of the one-lane kernel, so all of them return the same bits.
//
// Across a descent a unit keeps what the path loop keeps -- the seed, the goal, the problem index -- plus the attempt
// counter, the open flag and the two counter sums.  The attempt's start is NOT kept: a failed attempt reports its
// cost, and it is computed again from the initial guess and the draws (search_start) -- one draw per bounded
// variable, the draws 1 .. a of an unbounded one, whose draw is centred on the previous start.
//
// Compiled in translation units of its own (pik_search_inst.hip), for the flavours fast, exact and strict: nothing
// here is read by pik_inst.hip, whose kernels are compiled from the text they had before this file existed.
#pragma once

#include "pik_path.hpp"
#include "pik_search_ops.hpp"
#if defined(PIK_STRICT)
#include "pik_validity.hpp"
#endif

namespace pik {

constexpr uint32_t STREAM_RESTART = 3u; // (streams 1 and 2: pik_math.hpp)
constexpr int PIKAMD_GATE_REFUSED_K = -1002; // PIKAMD_GATE_REFUSED

#if defined(PIK_STRICT)
// The validity step of an attempt (src/pick_ik_plugin.cpp:269-274, the solution callback's place): the sphere test of
// pik_validity.hpp on the attempt's answer.  A real call with the lane's centres in private memory (96 doubles at the
// most, indexed by sphere): the descents around it keep their registers, and a call without a model never gets here.
template <int D>
__device__ __noinline__ bool search_valid(CK<D> c_in, const void* image, const double (&q)[D]) {
    CK<D> c = scalar_ref(c_in);
    VM m = scalar_ref(((const PIK_CONSTANT ValidityImage<D>*)image)->model);
    double store[3 * VALIDITY_MAX_SPHERES];
    double clearance;
    return validity_clear<D>(c, m, q, store, 1, clearance);
}
#endif

// (hi - lo) * u + lo with every operation rounded on its own, whatever contraction the flavour is compiled with
// (the fast flavour's uniform_real is one fused expression): the restart states are the same doubles in all flavours
__device__ __forceinline__ double restart_value(double lo, double hi, double u) {
#pragma clang fp contract(off)
    const double width = hi - lo;
    const double scaled = width * u;
    const double v = scaled + lo;
    return v;
}

// draw(b, e, q) of the header: Robot::set_random_valid_configuration (src/robot.cpp:87-95, 23-30) from the RESTART
// stream, key (rng_seed, problem_offset + b), epoch e, individual 0, slot j
// (bounded_too = false: only the unbounded variables -- a bounded one does not depend on the previous start, so of a
//  chain of draws only the last one matters for it)
template <int D>
__device__ __forceinline__ void restart_draw(CK<D> c, const SearchArgs& a, long long b, unsigned e, bool bounded_too,
                                             double (&q)[D]) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
        if (!bounded_too && ((c.bounded_mask >> j) & 1u) != 0) continue;
        const U4 w = rng_block(a.rng_seed, STREAM_RESTART, (uint64_t)(a.problem_offset + b), e, 0u, (unsigned)(j >> 1));
        const double u = (j & 1) ? u01_from_words(w.z, w.w) : u01_from_words(w.x, w.y);
        const bool bounded = ((c.bounded_mask >> j) & 1u) != 0;
        double lo, hi;
        {
#pragma clang fp contract(off)
            lo = q[j] - M_PI;
            hi = q[j] + M_PI;
        }
        q[j] = restart_value(bounded ? c.qmin[j] : lo, bounded ? c.qmax[j] : hi, u);
    }
}

// Where attempt `att` of problem b starts: the initial guess, re-drawn at epoch 0 when a bounded variable is outside
// its limits (src/pick_ik_plugin.cpp:152-159; a NaN is outside), then the draws 1 .. att that the failures in front of
// the attempt made.
template <int D>
__device__ __forceinline__ void search_start(CK<D> c, const SearchArgs& a, long long b, int att, double (&cur)[D]) {
    bool valid = true;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        cur[j] = a.guess[b * D + j];
        const bool bounded = ((c.bounded_mask >> j) & 1u) != 0;
        valid = valid && (!bounded || (cur[j] <= c.qmax[j] && cur[j] >= c.qmin[j]));
    }
    // (the epochs are those of the lane's own problem; lanes whose guess is valid skip epoch 0)
    for (int e = 0; e <= att; ++e) {
        double next[D];
#pragma unroll
        for (int j = 0; j < D; ++j) next[j] = cur[j];
        restart_draw<D>(c, a, b, (unsigned)e, e == att, next);
        const bool take = e > 0 || !valid;
#pragma unroll
        for (int j = 0; j < D; ++j) cur[j] = take ? next[j] : cur[j];
    }
}

// The unit a lane owns -- one lane per unit, or a team of LPE adjacent lanes -- and its seed.  A lane without a unit
// runs masked on unit 0's data.  Returns whether the lane has a unit.
template <int D, int LPE>
__device__ __forceinline__ bool search_begin(const SearchArgs& a, long long& b, int& a0, int& n, double (&sd)[D]) {
    const long long u = (long long)blockIdx.x * (WAVE / LPE) + threadIdx.x / LPE;
    const long long units = a.parallel ? a.B * a.K : a.B;
    const bool mine = u < units;
    const long long uu = mine ? u : 0;
    b = a.parallel ? uu / a.K : uu;
    a0 = a.parallel ? (int)(uu - b * a.K) : 0;
    n = a.parallel ? 1 : a.K;
#pragma unroll
    for (int j = 0; j < D; ++j) sd[j] = a.seed[b * D + j];
    return mine;
}

// GradientIk::from for an attempt: the search starts at the attempt's start
template <int D>
__device__ __forceinline__ void search_state(CK<D> c, const SearchArgs& a, long long b, int att, GdState<D>& s) {
    double cur[D];
    search_start<D>(c, a, b, att, cur);
    path_state<D>(cur, s);
}

// Behind the descent of attempt `att` of problem b: the post-loop of ik_gradient (src/ik_gradient.cpp:130-138) as
// ik_gradient_kernel has it, the approximate-solution gate where the handle has one (a refused answer is
// PIKAMD_GATE_REFUSED and the seed; everything below -- the row, the primary outputs, whether the problem stays open,
// and with the row search_finalize_kernel's winner -- uses the gated status), the attempt's row (stored by the lanes
// with `store`: the unit's first lane), in the sequential schedule the primary outputs while the problem is open.
// `run`: the unit ran this attempt (it is open, or every attempt is wanted).  All lanes of the wavefront call this
// together.
template <int D, typename G>
__device__ __forceinline__ void search_attempt(CK<D> c, PK p, const SearchArgs& a, const G& g, const double (&sd)[D],
                                               const GdState<D>& s, long long b, int att, bool store, bool run,
                                               bool& open, long long& evals, int& gens) {
    int status = PIKAMD_NO_IK_SOLUTION_K;
    if (s.found) {
        status = 1;
    } else if (!p.stop_on_valid && s.best_sol) {
        status = 1;
    } else if (p.approx) {
        status = 2;
    }
    // One evaluation per attempt at the most, with operands chosen by what the call needs: the cost of the attempt's
    // start, reported on failure, or -- a.gate -- the approximate-solution gate on the attempt's answer
    // (src/pick_ik_plugin.cpp:219-267) under the parameters p' of pikamd_gate_batch.  The host sets a.gate only with
    // return_approximate_solution, and then every status is > 0: a call needs the one or the other, never both.
    const bool solved = status > 0;
    double first_cost = 0.0;
    if (__any(run && (a.gate != 0 || !solved))) {
        double cur[D];
        if (a.gate == 0) {
            search_start<D>(c, a, b, att, cur);
        } else {
#pragma unroll
            for (int j = 0; j < D; ++j) cur[j] = s.best[j];
        }
        const PIK_CONSTANT ParamsK* pe = a.gate != 0 ? (const PIK_CONSTANT ParamsK*)a.gate_params : &p;
        EvalOut e;
        evaluate<D>(c, *pe, g, sd, cur, e);
        first_cost = e.cost;
        if (a.gate != 0 && solved) {
            bool pass = e.sol;
            if (a.gate_joint > 0.0) {
#pragma unroll
                for (int j = 0; j < D; ++j) pass = pass && !(fabs(s.best[j] - sd[j]) > a.gate_joint);
            }
            status = pass ? status : PIKAMD_GATE_REFUSED_K;
        }
    }
#if defined(PIK_STRICT)
    // The validity step, behind the gate and whether or not the call is gated: an answer the handle's sphere model
    // refuses is PIKAMD_VALIDITY_REFUSED and the seed -- the row, the primary outputs, whether the problem stays open
    // and search_finalize_kernel's winner use the tested status; cost and counters stay, no evaluation is counted.
    if (a.validity != nullptr && __any(run && status > 0)) {
        const bool ok = search_valid<D>(c, a.validity, s.best);
        status = (status > 0 && !ok) ? PIKAMD_VALIDITY_REFUSED_K : status;
    }
#endif
    StatsK st;
    st.cost_evals = (s.found == 2) ? 0 : 1 + (long long)s.steps * (2 * D + 3);
    st.generations = s.iters;
    st.wipeouts = 0;
    st.pool_erasures = 0;
    st.reserved = 0;
    const double cost = solved ? s.best_cost : first_cost; // (a refused answer keeps the cost the solve returned)
    if (run && store) {
        const long long row = b * a.K + att;
        if (a.row_solution) {
#pragma unroll
            for (int j = 0; j < D; ++j) a.row_solution[row * D + j] = (status > 0) ? s.best[j] : sd[j];
        }
        if (a.row_status) a.row_status[row] = status;
        if (a.parallel) {
            a.row_cost[row] = cost;
            static_cast<StatsK*>(a.row_stats)[row] = st;
        }
    }
    if (!a.parallel) {
        if (open) {
            evals += st.cost_evals;
            gens += st.generations;
        }
        if (open && store) {
#pragma unroll
            for (int j = 0; j < D; ++j) a.solution[b * D + j] = (status > 0) ? s.best[j] : sd[j];
            a.status[b] = status;
            if (a.cost) a.cost[b] = cost;
            if (a.stats) {
                StatsK sum = st;
                sum.cost_evals = evals;
                sum.generations = gens;
                static_cast<StatsK*>(a.stats)[b] = sum;
            }
            if (a.attempts) a.attempts[b] = att + 1;
        }
        open = open && !(status > 0);
    }
}

// one lane per unit, one tip frame or several (every flavour)
template <int D, bool MULTI = false>
__global__ __launch_bounds__(WAVE) void ik_search_kernel(const ConstsK<D>* __restrict__ kc, SearchArgs a) {
    PIK_CONSTS(kc);
    __shared__ double frames[GD_ROWS(D) * WAVE];
    long long b, evals = 0;
    int a0, n, gens = 0;
    double sd[D];
    const bool mine = search_begin<D, 1>(a, b, a0, n, sd);
    bool open = mine;
    typename GoalSel<MULTI>::type g;
    load_goals<D>(c, a.goal, b, g);
    for (int k = 0; k < n && __any(mine && (a.every || open)); ++k) {
        const bool run = mine && (a.every || open);
        GdState<D> s;
        search_state<D>(c, a, b, a0 + k, s);
        PIK_DESCENT(GD_LOCAL, 1, g, sd, nullptr, s, run, p.local_max_iters, frames, (int)threadIdx.x, 0);
        search_attempt<D>(c, p, a, g, sd, s, b, a0 + k, true, run, open, evals, gens);
    }
}

#if !defined(PIK_STRICT)
// LPE lanes per unit: the cooperative descent (gd_wide / gd_wide_multi), as ik_gradient_wide_kernel.  Its probes read
// the seed by a per-lane joint index from memory: the problem's seed is the same for every attempt.
template <int D, int LPE, bool MULTI = false>
__global__ __launch_bounds__(WAVE) void ik_search_wide_kernel(const ConstsK<D>* __restrict__ kc, SearchArgs a) {
    PIK_CONSTS(kc);
    constexpr int GDR = GD_ROWS(D, LPE, !MULTI);
    constexpr int TCR = MULTI ? (MAX_TIPS * (7 * D + 24) + WAVE - 1) / WAVE : 0; // (several tips: the chains' constants)
    __shared__ double lds[(GDR + TCR) * WAVE];
    const int lane = threadIdx.x;
    const int sub = lane % LPE;
    long long b, evals = 0;
    int a0, n, gens = 0;
    double sd[D];
    const bool mine = search_begin<D, LPE>(a, b, a0, n, sd);
    bool open = mine;
    typename GoalSel<MULTI>::type g;
    load_goals<D>(c, a.goal, b, g);
    if constexpr (MULTI) stage_tip_constants<D>(c, lds + GDR * WAVE, lane);
    for (int k = 0; k < n && __any(mine && (a.every || open)); ++k) {
        const bool run = mine && (a.every || open);
        GdState<D> s;
        search_state<D>(c, a, b, a0 + k, s);
        if constexpr (MULTI) {
            gd_wide_multi<D, LPE, GD_LOCAL>(c, p, g, sd, a.seed + b * D, s, run, p.local_max_iters, lds,
                                            lds + GDR * WAVE, lane, sub);
        } else {
            gd_wide<D, LPE, GD_LOCAL>(c, p, g, sd, a.seed + b * D, s, run, p.local_max_iters, lds, lane, sub);
        }
        search_attempt<D>(c, p, a, g, sd, s, b, a0 + k, sub == 0, run, open, evals, gens);
    }
}
#endif

#if defined(PIK_STRICT)
// exact flavours, one tip frame, LPE lanes per unit: the team forms of the memoised descent, as
// ik_gradient_team_kernel (every lane of a unit holds the same state; its first lane stores)
template <int D, int LPE>
__global__ __launch_bounds__(WAVE) void ik_search_team_kernel(const ConstsK<D>* __restrict__ kc, SearchArgs a) {
    PIK_CONSTS(kc);
    __shared__ double lds[GD_ROWS(D, LPE) * WAVE];
    const int lane = threadIdx.x;
    const int sub = lane % LPE;
    long long b, evals = 0;
    int a0, n, gens = 0;
    double sd[D];
    const bool mine = search_begin<D, LPE>(a, b, a0, n, sd);
    bool open = mine;
    GoalK g;
    load_goals<D>(c, a.goal, b, g);
    for (int k = 0; k < n && __any(mine && (a.every || open)); ++k) {
        const bool run = mine && (a.every || open);
        GdState<D> s;
        search_state<D>(c, a, b, a0 + k, s);
        PIK_DESCENT(GD_LOCAL, LPE, g, sd, nullptr, s, run, p.local_max_iters, lds, lane, sub);
        search_attempt<D>(c, p, a, g, sd, s, b, a0 + k, sub == 0, run, open, evals, gens);
    }
}
#endif

// Parallel schedule, behind the descents: the loop's rule per problem.  The winner is the first attempt with
// status > 0, with none the last one; the counters are summed up to and including the winner.
template <int D>
__global__ __launch_bounds__(WAVE) void search_finalize_kernel(SearchArgs a) {
    const long long b = (long long)blockIdx.x * WAVE + threadIdx.x;
    if (b >= a.B) return;
    const long long row0 = b * a.K;
    int win = a.K - 1;
    for (int k = 0; k < a.K; ++k) {
        if (a.row_status[row0 + k] > 0) {
            win = k;
            break;
        }
    }
    StatsK sum;
    sum.cost_evals = 0;
    sum.generations = 0;
    sum.wipeouts = 0;
    sum.pool_erasures = 0;
    sum.reserved = 0;
    for (int k = 0; k <= win; ++k) {
        const StatsK st = static_cast<const StatsK*>(a.row_stats)[row0 + k];
        sum.cost_evals += st.cost_evals;
        sum.generations += st.generations;
        sum.wipeouts += st.wipeouts;
        sum.pool_erasures += st.pool_erasures;
    }
    const long long row = row0 + win;
#pragma unroll
    for (int j = 0; j < D; ++j) a.solution[b * D + j] = a.row_solution[row * D + j];
    a.status[b] = a.row_status[row];
    if (a.cost) a.cost[b] = a.row_cost[row];
    if (a.stats) static_cast<StatsK*>(a.stats)[b] = sum;
    if (a.attempts) a.attempts[b] = win + 1;
}

// One launch for the whole call (two in the parallel schedule); schedule and width by search_plan
// (pik_search_ops.hpp), which the caller has applied: a.parallel, a.lanes.  Stream-ordered: nothing here waits unless
// the slot's constants change (upload_consts).
template <int D>
int launch_search(pikamd_solver* s, const ParamsK& pk, const SearchArgs& a, hipStream_t st, int slot) {
    if (a.B == 0) return 0;
    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, &pk, slot, st, &kc)) return rc;
    const bool multi = s->n_tips > 1;
    const int lpe = a.lanes;
    const long long per_wave = WAVE / lpe, units = a.parallel ? a.B * a.K : a.B;
    const dim3 g((unsigned)((units + per_wave - 1) / per_wave)), b(WAVE);
#if !defined(PIK_STRICT)
    if (lpe == 16 && multi) hipLaunchKernelGGL((ik_search_wide_kernel<D, 16, true>), g, b, 0, st, kc, a);
    else if (lpe == 8 && multi) hipLaunchKernelGGL((ik_search_wide_kernel<D, 8, true>), g, b, 0, st, kc, a);
    else if (lpe == 16) hipLaunchKernelGGL((ik_search_wide_kernel<D, 16>), g, b, 0, st, kc, a);
    else if (lpe == 8) hipLaunchKernelGGL((ik_search_wide_kernel<D, 8>), g, b, 0, st, kc, a);
#else
    if (lpe == 16) hipLaunchKernelGGL((ik_search_team_kernel<D, 16>), g, b, 0, st, kc, a);
    else if (lpe == 4) hipLaunchKernelGGL((ik_search_team_kernel<D, 4>), g, b, 0, st, kc, a);
#endif
    else if (lpe != 1) return fail(PIKAMD_EINVAL, "search: no kernel with %d lanes per unit", lpe);
    else if (multi) hipLaunchKernelGGL((ik_search_kernel<D, true>), g, b, 0, st, kc, a);
    else hipLaunchKernelGGL(ik_search_kernel<D>, g, b, 0, st, kc, a);
    HIP_TRY(hipGetLastError());
    if (a.parallel) {
        hipLaunchKernelGGL(search_finalize_kernel<D>, dim3((unsigned)((a.B + WAVE - 1) / WAVE)), b, 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

template <int D>
const SearchOps* make_search_ops() {
    static const SearchOps ops = {&launch_search<D>};
    return &ops;
}

} // namespace pik
