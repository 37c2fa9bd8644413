// pik_startpath.hpp -- Cartesian paths from a pose: restart the start state until the path holds
// (pikamd_search_paths).
//
// A planner has a Cartesian motion and a pose to start it from, but no joint state: it solves waypoint 0 with restarts,
// runs the path from that answer, looks how far it got, and when the path broke draws another start and does both
// again.  As a host loop that is up to 2 * max_attempts dependent launches and copies.  The kernels here wrap the
// EXISTING local-mode descents (pik_kernels.hpp: PIK_DESCENT(GD_LOCAL, ...), gd_wide, gd_wide_multi) in two loops: a
// lane (or a team of lanes) owns one path; the attempt loop wraps the waypoint loop.  Waypoint 0 of attempt a starts
// from search_start(..., a) with the caller's seed as the minimal-displacement reference, as an attempt of
// ik_search_kernel does; the waypoints behind it run exactly as ik_path_kernel's (path_state, path_waypoint, path_tail).
// The attempt that held the most waypoints is kept, the first among equals; a path that held throughout is closed, and
// the attempt loop ends when no path of the wavefront is open.
//
// The rows of attempt 0 go straight to the outputs.  The rows of a later attempt go to the slot's scratch and are
// copied over the outputs, by the lane that wrote them, only when the attempt held more waypoints than every one
// before it.
//
// The result is defined as what the loop of pikamd_solve_batch / pikamd_solve_paths calls returns
// (include/pick_ik_amd.h), and every variant below performs the arithmetic of the one-lane kernel, so all of them
// return the same bits.
//
// Across a descent a path keeps what the path loop keeps -- the seed, the goal, the path index, the waypoint counter,
// the held flag and the count of held waypoints -- plus the attempt counter, the open flag, the best count and the two
// counter sums.  The caller's seed is read again at the start of every attempt and the attempt's start is computed
// again where a failed waypoint 0 reports its cost (search_start), as in pik_search.hpp.
//
// Compiled in translation units of its own (pik_startpath_inst.hip), for the flavours fast, exact and strict: nothing
// here is read by pik_inst.hip, pik_path_inst.hip or pik_search_inst.hip.
#pragma once

#include "pik_search.hpp"
#include "pik_startpath_ops.hpp"

namespace pik {

// What path_waypoint and path_tail read and write for one attempt: the outputs (attempt 0) or the slot's scratch.
// reached is the kernel's to write, behind the last attempt.
__device__ __forceinline__ PathArgs startpath_rows(const StartPathArgs& a, bool first) {
    PathArgs r;
    r.P = a.P;
    r.W = a.W;
    r.pad_ = 0;
    r.goal = a.goal;
    r.start = a.seed;
    r.max_step = a.max_step;
    r.solution = first ? a.solution : a.row_solution;
    r.status = first ? a.status : a.row_status;
    r.cost = first ? a.cost : a.row_cost;
    r.stats = first ? a.stats : a.row_stats;
    r.reached = nullptr;
    return r;
}

// ... and what search_start reads: the initial guesses and the key of the draws
__device__ __forceinline__ SearchArgs startpath_draws(const StartPathArgs& a) {
    SearchArgs r = {};
    r.B = a.P;
    r.K = a.K;
    r.seed = a.seed;
    r.guess = a.guess;
    r.rng_seed = a.rng_seed;
    r.problem_offset = a.problem_offset;
    return r;
}

// The path a lane owns -- one lane per path, or a team of LPE adjacent lanes.  A lane without a path runs masked on
// path 0's data.  Returns whether the lane has a path.
template <int LPE>
__device__ __forceinline__ bool startpath_begin(const StartPathArgs& a, long long& path) {
    const long long i = (long long)blockIdx.x * (WAVE / LPE) + threadIdx.x / LPE;
    const bool mine = i < a.P;
    path = mine ? i : 0;
    return mine;
}

// the caller's seed of a path: the minimal-displacement reference of waypoint 0 and what a failed waypoint 0 returns
template <int D>
__device__ __forceinline__ void startpath_seed(const StartPathArgs& a, long long path, double (&sd)[D]) {
#pragma unroll
    for (int j = 0; j < D; ++j) sd[j] = a.seed[path * D + j];
}

// Behind the descent of waypoint 0 of attempt `att`: the post-loop of ik_gradient as ik_gradient_kernel has it and the
// row pikamd_solve_batch returns -- on failure the seed and the cost of the attempt's start; NO joint-step test --,
// stored by the lanes with `store`, and what the path carries on: the answer as the next seed, or the end of the
// attempt.  All lanes of the wavefront call this together.
template <int D, typename G>
__device__ __forceinline__ void startpath_first(CK<D> c, PK p, const PathArgs& a, const SearchArgs& sa, const G& g,
                                                double (&sd)[D], const GdState<D>& s, long long path, int att,
                                                bool store, bool& active, int& reached) {
    int status = PIKAMD_NO_IK_SOLUTION_K;
    if (s.found) {
        status = 1;
    } else if (!p.stop_on_valid && s.best_sol) {
        status = 1;
    } else if (p.approx) {
        status = 2;
    }
    const bool solved = status > 0;
    double first_cost = 0.0; // cost of the attempt's start, reported on failure
    if (__any(active && !solved)) {
        double cur[D];
        search_start<D>(c, sa, path, att, cur);
        EvalOut e;
        evaluate<D>(c, p, g, sd, cur, e);
        first_cost = e.cost;
    }
    if (active && store) {
        const long long row = path * a.W;
#pragma unroll
        for (int j = 0; j < D; ++j) a.solution[row * D + j] = solved ? s.best[j] : sd[j];
        a.status[row] = status;
        if (a.cost) a.cost[row] = solved ? s.best_cost : first_cost;
        if (a.stats) {
            StatsK st;
            st.cost_evals = (s.found == 2) ? 0 : 1 + (long long)s.steps * (2 * D + 3);
            st.generations = s.iters;
            st.wipeouts = 0;
            st.pool_erasures = 0;
            st.reserved = 0;
            static_cast<StatsK*>(a.stats)[row] = st;
        }
    }
    if (active && solved) {
#pragma unroll
        for (int j = 0; j < D; ++j) sd[j] = s.best[j];
        ++reached;
    }
    active = active && solved;
}

// the counters of a descent the path ran, into the sums over every row of every attempt
template <int D>
__device__ __forceinline__ void startpath_count(const GdState<D>& s, bool ran, long long& evals, int& gens) {
    if (ran) {
        evals += (s.found == 2) ? 0 : 1 + (long long)s.steps * (2 * D + 3);
        gens += s.iters;
    }
}

// Behind the rows of attempt `att` (`ran`: the path was open for it): the attempt is kept when it held more waypoints
// than every one before it -- its rows are copied from the scratch over the outputs by the lanes with `store`, which
// wrote them --, and a path that held throughout is closed.
template <int D>
__device__ __forceinline__ void startpath_keep(const StartPathArgs& a, long long path, int att, bool ran, bool store,
                                               int reached, int& best, bool& open) {
    const bool better = ran && reached > best;
    if (better && store && att > 0) {
        for (int k = 0; k < a.W; ++k) {
            const long long row = path * a.W + k;
#pragma unroll
            for (int j = 0; j < D; ++j) a.solution[row * D + j] = a.row_solution[row * D + j];
            a.status[row] = a.row_status[row];
            if (a.cost) a.cost[row] = a.row_cost[row];
            if (a.stats) static_cast<StatsK*>(a.stats)[row] = static_cast<const StatsK*>(a.row_stats)[row];
        }
    }
    if (ran && store && a.attempts) a.attempts[path] = att + 1;
    best = better ? reached : best;
    open = open && reached != a.W;
}

// behind the last attempt: the count of held waypoints of the kept attempt and the sums of the counters
__device__ __forceinline__ void startpath_end(const StartPathArgs& a, long long path, bool store, int best,
                                              long long evals, int gens) {
    if (!store) return;
    if (a.reached) a.reached[path] = best;
    if (a.totals) {
        StatsK st;
        st.cost_evals = evals;
        st.generations = gens;
        st.wipeouts = 0;
        st.pool_erasures = 0;
        st.reserved = 0;
        static_cast<StatsK*>(a.totals)[path] = st;
    }
}

// one lane per path, one tip frame or several (every flavour)
template <int D, bool MULTI = false>
__global__ __launch_bounds__(WAVE) void ik_startpath_kernel(const ConstsK<D>* __restrict__ kc, StartPathArgs a) {
    PIK_CONSTS(kc);
    __shared__ double frames[GD_ROWS(D) * WAVE];
    const SearchArgs sa = startpath_draws(a);
    long long ii, evals = 0;
    int gens = 0, best = -1;
    const bool mine = startpath_begin<1>(a, ii);
    bool open = mine;
    for (int att = 0; att < a.K && __any(open); ++att) {
        const PathArgs rows = startpath_rows(a, att == 0);
        double sd[D];
        startpath_seed<D>(a, ii, sd);
        bool active = open;
        int reached = 0;
        for (int k = 0; k < a.W && __any(active); ++k) {
            const long long row = ii * a.W + k;
            typename GoalSel<MULTI>::type g;
            load_goals<D>(c, a.goal, row, g);
            GdState<D> s;
            if (k == 0) search_state<D>(c, sa, ii, att, s);
            else path_state<D>(sd, s);
            const bool ran = active;
            PIK_DESCENT(GD_LOCAL, 1, g, sd, nullptr, s, active, p.local_max_iters, frames, (int)threadIdx.x, 0);
            if (k == 0) startpath_first<D>(c, p, rows, sa, g, sd, s, ii, att, true, active, reached);
            else path_waypoint<D>(c, p, rows, g, sd, s, row, true, active, reached);
            startpath_count<D>(s, ran, evals, gens);
        }
        path_tail<D>(rows, sd, ii, open, reached);
        startpath_keep<D>(a, ii, att, open, true, reached, best, open);
    }
    startpath_end(a, ii, mine, best, evals, gens);
}

#if !defined(PIK_STRICT)
// LPE lanes per path: the cooperative descent (gd_wide / gd_wide_multi), as ik_path_wide_kernel.  Its probes read the
// seed by a per-lane joint index from memory: the team keeps a copy of its path's current seed in LDS.
template <int D, int LPE, bool MULTI = false>
__global__ __launch_bounds__(WAVE) void ik_startpath_wide_kernel(const ConstsK<D>* __restrict__ kc, StartPathArgs a) {
    PIK_CONSTS(kc);
    constexpr int GDR = GD_ROWS(D, LPE, !MULTI);
    constexpr int TCR = MULTI ? (MAX_TIPS * (7 * D + 24) + WAVE - 1) / WAVE : 0; // (several tips: the chains' constants)
    constexpr int PER_WAVE = WAVE / LPE;
    __shared__ double lds[(GDR + TCR) * WAVE + PER_WAVE * D];
    const int lane = threadIdx.x;
    const int sub = lane % LPE;
    double* const seed_l = lds + (GDR + TCR) * WAVE + (lane / LPE) * D;
    const SearchArgs sa = startpath_draws(a);
    long long ii, evals = 0;
    int gens = 0, best = -1;
    const bool mine = startpath_begin<LPE>(a, ii);
    bool open = mine;
    if constexpr (MULTI) stage_tip_constants<D>(c, lds + GDR * WAVE, lane);
    for (int att = 0; att < a.K && __any(open); ++att) {
        const PathArgs rows = startpath_rows(a, att == 0);
        double sd[D];
        startpath_seed<D>(a, ii, sd);
        bool active = open;
        int reached = 0;
        for (int k = 0; k < a.W && __any(active); ++k) {
            const long long row = ii * a.W + k;
            typename GoalSel<MULTI>::type g;
            load_goals<D>(c, a.goal, row, g);
            GdState<D> s;
            if (k == 0) search_state<D>(c, sa, ii, att, s);
            else path_state<D>(sd, s);
            const bool ran = active;
            wave_sync(); // (the previous waypoint's probes have read the copy)
            if (sub == 0) {
#pragma unroll
                for (int j = 0; j < D; ++j) seed_l[j] = sd[j];
            }
            wave_sync();
            if constexpr (MULTI) {
                gd_wide_multi<D, LPE, GD_LOCAL>(c, p, g, sd, seed_l, s, active, p.local_max_iters, lds, lds + GDR * WAVE,
                                                lane, sub);
            } else {
                gd_wide<D, LPE, GD_LOCAL>(c, p, g, sd, seed_l, s, active, p.local_max_iters, lds, lane, sub);
            }
            if (k == 0) startpath_first<D>(c, p, rows, sa, g, sd, s, ii, att, sub == 0, active, reached);
            else path_waypoint<D>(c, p, rows, g, sd, s, row, sub == 0, active, reached);
            startpath_count<D>(s, ran, evals, gens);
        }
        path_tail<D>(rows, sd, ii, open && sub == 0, reached);
        startpath_keep<D>(a, ii, att, open, sub == 0, reached, best, open);
    }
    startpath_end(a, ii, mine && sub == 0, best, evals, gens);
}
#endif

#if defined(PIK_STRICT)
// exact flavours, one tip frame, LPE lanes per path: the team forms of the memoised descent, as ik_path_team_kernel
// (every lane of a path holds the same state; its first lane stores)
template <int D, int LPE>
__global__ __launch_bounds__(WAVE) void ik_startpath_team_kernel(const ConstsK<D>* __restrict__ kc, StartPathArgs a) {
    PIK_CONSTS(kc);
    __shared__ double lds[GD_ROWS(D, LPE) * WAVE];
    const int lane = threadIdx.x;
    const int sub = lane % LPE;
    const SearchArgs sa = startpath_draws(a);
    long long ii, evals = 0;
    int gens = 0, best = -1;
    const bool mine = startpath_begin<LPE>(a, ii);
    bool open = mine;
    for (int att = 0; att < a.K && __any(open); ++att) {
        const PathArgs rows = startpath_rows(a, att == 0);
        double sd[D];
        startpath_seed<D>(a, ii, sd);
        bool active = open;
        int reached = 0;
        for (int k = 0; k < a.W && __any(active); ++k) {
            const long long row = ii * a.W + k;
            GoalK g;
            load_goals<D>(c, a.goal, row, g);
            GdState<D> s;
            if (k == 0) search_state<D>(c, sa, ii, att, s);
            else path_state<D>(sd, s);
            const bool ran = active;
            PIK_DESCENT(GD_LOCAL, LPE, g, sd, nullptr, s, active, p.local_max_iters, lds, lane, sub);
            if (k == 0) startpath_first<D>(c, p, rows, sa, g, sd, s, ii, att, sub == 0, active, reached);
            else path_waypoint<D>(c, p, rows, g, sd, s, row, sub == 0, active, reached);
            startpath_count<D>(s, ran, evals, gens);
        }
        path_tail<D>(rows, sd, ii, open && sub == 0, reached);
        startpath_keep<D>(a, ii, att, open, sub == 0, reached, best, open);
    }
    startpath_end(a, ii, mine && sub == 0, best, evals, gens);
}
#endif

// One launch for the whole call; the variant by path_lanes (pik_path_ops.hpp).  Stream-ordered: nothing here waits
// unless the slot's constants change (upload_consts).
template <int D>
int launch_startpaths(pikamd_solver* s, const ParamsK& pk, const StartPathArgs& a, hipStream_t st, int slot) {
    if (a.P == 0) return 0;
    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, &pk, slot, st, &kc)) return rc;
    const bool multi = s->n_tips > 1;
    const int lpe = path_lanes(s, a.P, EXACT_FLAVOUR);
    const long long per_wave = WAVE / lpe;
    const dim3 g((unsigned)((a.P + per_wave - 1) / per_wave)), b(WAVE);
#if !defined(PIK_STRICT)
    if (lpe == 16 && multi) hipLaunchKernelGGL((ik_startpath_wide_kernel<D, 16, true>), g, b, 0, st, kc, a);
    else if (lpe == 8 && multi) hipLaunchKernelGGL((ik_startpath_wide_kernel<D, 8, true>), g, b, 0, st, kc, a);
    else if (lpe == 16) hipLaunchKernelGGL((ik_startpath_wide_kernel<D, 16>), g, b, 0, st, kc, a);
    else if (lpe == 8) hipLaunchKernelGGL((ik_startpath_wide_kernel<D, 8>), g, b, 0, st, kc, a);
#else
    if (lpe == 16) hipLaunchKernelGGL((ik_startpath_team_kernel<D, 16>), g, b, 0, st, kc, a);
    else if (lpe == 4) hipLaunchKernelGGL((ik_startpath_team_kernel<D, 4>), g, b, 0, st, kc, a);
#endif
    else if (multi) hipLaunchKernelGGL((ik_startpath_kernel<D, true>), g, b, 0, st, kc, a);
    else hipLaunchKernelGGL(ik_startpath_kernel<D>, g, b, 0, st, kc, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int D>
const StartPathOps* make_startpath_ops() {
    static const StartPathOps ops = {&launch_startpaths<D>};
    return &ops;
}

} // namespace pik
