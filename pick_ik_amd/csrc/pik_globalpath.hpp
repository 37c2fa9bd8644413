// pik_globalpath.hpp -- Cartesian paths from a pose with a memetic start (pikamd_search_global_paths).
//
// pikamd_search_paths restarts a LOCAL descent for waypoint 0.  Waypoint 0 is the one waypoint with no neighbouring
// joint state -- a cold query from a pose alone, which is what the memetic solver is for.  Here attempt a of a call is
// the memetic solve of waypoint 0 for the paths still open (the EXISTING launches: pikamd_solve_batches' for attempt 0,
// launch_restart_attempt of pik_restart.hpp behind it, one batch record whose outputs are a row per path in the slot's
// scratch) and, stream-ordered behind it, ONE tail kernel of this file.  A lane (or a team of lanes) of the tail kernel
// owns path i of all P and reads open[i]; for an open path it copies the memetic row to row 0, walks the waypoints
// behind it from that answer exactly as ik_path_kernel does (path_state, the UNCHANGED local-mode descents,
// path_waypoint, path_tail), applies the keep-the-furthest rule (startpath_keep), adds the attempt's counters to the
// sums, and closes the path or draws its next start (restart_draw) and appends it to the next attempt's list -- the
// ballot and atomic append of restart_fold_kernel, so no fold kernel of its own runs.  What the loop carries from one
// attempt to the next -- the starts, the open flags, the best counts, the sums -- lives in memory, not in registers.
//
// `reached` is written behind EVERY attempt a path ran, not only behind the last one: the value only changes when the
// path ran, so the result is that of one write at the end, and the host-pointer entry point stops enqueuing attempts
// once no path is open -- the attempt that turns out to be the last is not known when its tail kernel is enqueued
// (`last` says only that the attempt is max_attempts - 1).  Writing it under `last` alone would lose the paths that
// closed earlier.
//
// The rows of attempt 0 go straight to the outputs.  The rows of a later attempt go to the slot's scratch and are
// copied over the outputs, by the lane that wrote them, only when the attempt held more waypoints than every one
// before it.
//
// The result is defined as what the loop of pikamd_solve_batches / pikamd_solve_paths calls returns
// (include/pick_ik_amd.h), and every variant below performs the arithmetic of the one-lane kernel, so all of them
// return the same bits.  Iterating over all P with the open flags needs no second counter and changes no result.
//
// Compiled in translation units of its own (pik_globalpath_inst.hip), for the flavours fast, exact and strict: nothing
// here is read by the translation units of the other families.
#pragma once

#include "pik_globalpath_ops.hpp"
#include "pik_startpath.hpp"

namespace pik {

// the two fields restart_draw reads of a search call
__device__ __forceinline__ SearchArgs globalpath_draw_key(const GlobalPathArgs& a) {
    SearchArgs k = {};
    k.rng_seed = a.rng_seed;
    k.problem_offset = a.problem_offset;
    return k;
}

// What path_waypoint and path_tail read and write for the attempt: the outputs (attempt 0) or the slot's scratch.
__device__ __forceinline__ PathArgs globalpath_rows(const GlobalPathArgs& a) {
    const bool first = a.attempt == 0;
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

// ... and what startpath_keep reads: the outputs, the scratch rows and the attempts
__device__ __forceinline__ StartPathArgs globalpath_keep_view(const GlobalPathArgs& a) {
    StartPathArgs r = {};
    r.P = a.P;
    r.W = a.W;
    r.K = a.K;
    r.solution = a.solution;
    r.status = a.status;
    r.cost = a.cost;
    r.stats = a.stats;
    r.attempts = a.attempts;
    r.row_solution = a.row_solution;
    r.row_status = a.row_status;
    r.row_cost = a.row_cost;
    r.row_stats = a.row_stats;
    return r;
}

// In front of attempt 0, one thread per path: the goals of waypoint 0 gathered into the contiguous array a batch record
// wants; init[p] = the initial guess, re-drawn at epoch 0 when a bounded variable is outside its limits (a NaN is
// outside); no attempt kept yet, the sums zero, every path open.
template <int D>
__global__ __launch_bounds__(WAVE) void ik_globalpath_prepare_kernel(const ConstsK<D>* __restrict__ kc, GlobalPathArgs a) {
    PIK_CONSTS(kc);
    const long long i = (long long)blockIdx.x * WAVE + threadIdx.x;
    if (i >= a.P) return;
    for (int j = 0; j < a.g7; ++j) a.goal0[i * a.g7 + j] = a.goal[i * a.W * a.g7 + j];
    const SearchArgs key = globalpath_draw_key(a);
    double q[D], drawn[D];
    bool valid = true;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        q[j] = a.user_guess[i * D + j];
        drawn[j] = q[j];
        const bool bounded = ((c.bounded_mask >> j) & 1u) != 0;
        valid = valid && (!bounded || (q[j] <= c.qmax[j] && q[j] >= c.qmin[j]));
    }
    restart_draw<D>(c, key, i, 0u, true, drawn);
#pragma unroll
    for (int j = 0; j < D; ++j) a.guess[i * D + j] = valid ? q[j] : drawn[j];
    a.best[i] = -1;
    a.open[i] = 1;
    if (a.totals) {
        StatsK z;
        z.cost_evals = 0;
        z.generations = 0;
        z.wipeouts = 0;
        z.pool_erasures = 0;
        z.reserved = 0;
        static_cast<StatsK*>(a.totals)[i] = z;
    }
}

// The path a lane owns -- one lane per path, or a team of LPE adjacent lanes -- and whether the loop still has it open.
// A lane without an open path runs masked on path 0's data.
template <int LPE>
__device__ __forceinline__ bool globalpath_begin(const GlobalPathArgs& a, long long& path) {
    const long long i = (long long)blockIdx.x * (WAVE / LPE) + threadIdx.x / LPE;
    const bool open = i < a.P && a.open[i < a.P ? i : 0] != 0;
    path = open ? i : 0;
    return open;
}

// Row 0 of the attempt: what the memetic solve returned (on failure the seed and the cost of the attempt's start; NO
// joint-step test), stored by the lanes with `store`, and what the path carries on: the answer as the seed of waypoint
// 1, or the caller's seed and the end of the attempt.
template <int D>
__device__ __forceinline__ void globalpath_first(const GlobalPathArgs& a, const PathArgs& rows, long long path, bool open,
                                                 bool store, double (&sd)[D], bool& active, int& reached) {
    const bool solved = open && a.m_status[path] > 0;
    if (open && store) {
        const long long row = path * a.W;
#pragma unroll
        for (int j = 0; j < D; ++j) rows.solution[row * D + j] = a.m_solution[path * D + j];
        rows.status[row] = a.m_status[path];
        if (rows.cost) rows.cost[row] = a.m_cost[path];
        if (rows.stats) static_cast<StatsK*>(rows.stats)[row] = static_cast<const StatsK*>(a.m_stats)[path];
    }
#pragma unroll
    for (int j = 0; j < D; ++j) sd[j] = solved ? a.m_solution[path * D + j] : a.seed[path * D + j];
    active = solved;
    reached = solved ? 1 : 0;
}

// Behind the rows of the attempt (`ran`: the path was open for it; every lane of the wavefront calls this together): the
// keep rule, the sums, the count of held waypoints, and for a path that stays open the next start and its place in the
// next attempt's list.
template <int D>
__device__ __forceinline__ void globalpath_fold(CK<D> c, const GlobalPathArgs& a, long long path, bool ran, bool store,
                                                int reached, long long evals, int gens) {
    int best = ran ? a.best[path] : -1;
    bool open = ran;
    startpath_keep<D>(globalpath_keep_view(a), path, a.attempt, ran, store, reached, best, open);
    const bool write = ran && store;
    if (write) {
        a.best[path] = best;
        if (a.reached) a.reached[path] = best; // (behind EVERY attempt: see the header comment)
        if (a.totals) {
            // every row of the attempt: the memetic row, and the descents behind it
            const StatsK m = static_cast<const StatsK*>(a.m_stats)[path];
            StatsK sum = static_cast<const StatsK*>(a.totals)[path];
            sum.cost_evals += m.cost_evals + evals;
            sum.generations += m.generations + gens;
            sum.wipeouts += m.wipeouts;
            sum.pool_erasures += m.pool_erasures;
            sum.reserved += m.reserved;
            static_cast<StatsK*>(a.totals)[path] = sum;
        }
        if (!open) a.open[path] = 0;
    }
    // the next attempt's paths: the start is drawn around the start of the attempt that did not hold
    const bool next = !a.last && write && open;
    if (next) {
        const SearchArgs key = globalpath_draw_key(a);
        double q[D];
#pragma unroll
        for (int j = 0; j < D; ++j) q[j] = a.guess[path * D + j];
        restart_draw<D>(c, key, path, (unsigned)(a.attempt + 1), true, q);
#pragma unroll
        for (int j = 0; j < D; ++j) a.guess[path * D + j] = q[j];
    }
    // ... and their list: a ballot, the lane's rank among the set bits, one atomic per wavefront
    const unsigned long long mask = __ballot(next);
    if (mask == 0ull) return;
    const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    unsigned base = 0u;
    if (threadIdx.x == 0) base = atomicAdd(a.n_list, (unsigned)__popcll(mask));
    base = (unsigned)__shfl((int)base, 0);
    if (next) a.list[base + rank] = (int)path;
}

// one lane per path, one tip frame or several (every flavour)
template <int D, bool MULTI = false>
__global__ __launch_bounds__(WAVE) void ik_globalpath_kernel(const ConstsK<D>* __restrict__ kc, GlobalPathArgs a) {
    PIK_CONSTS(kc);
    __shared__ double frames[GD_ROWS(D) * WAVE];
    long long ii, evals = 0;
    int gens = 0, reached;
    const bool open = globalpath_begin<1>(a, ii);
    if (!__any(open)) return;
    const PathArgs rows = globalpath_rows(a);
    double sd[D];
    bool active;
    globalpath_first<D>(a, rows, ii, open, true, sd, active, reached);
    for (int k = 1; k < a.W && __any(active); ++k) {
        const long long row = ii * a.W + k;
        typename GoalSel<MULTI>::type g;
        load_goals<D>(c, a.goal, row, g);
        GdState<D> s;
        path_state<D>(sd, s);
        const bool ran = active;
        PIK_DESCENT(GD_LOCAL, 1, g, sd, nullptr, s, active, p.local_max_iters, frames, (int)threadIdx.x, 0);
        path_waypoint<D>(c, p, rows, g, sd, s, row, true, active, reached);
        startpath_count<D>(s, ran, evals, gens);
    }
    path_tail<D>(rows, sd, ii, open, reached);
    globalpath_fold<D>(c, a, ii, open, true, reached, evals, gens);
}

#if !defined(PIK_STRICT)
// LPE lanes per path: the cooperative descent (gd_wide / gd_wide_multi), as ik_path_wide_kernel.  Its probes read the
// seed by a per-lane joint index from memory: the team keeps a copy of its path's current seed in LDS.
template <int D, int LPE, bool MULTI = false>
__global__ __launch_bounds__(WAVE) void ik_globalpath_wide_kernel(const ConstsK<D>* __restrict__ kc, GlobalPathArgs a) {
    PIK_CONSTS(kc);
    constexpr int GDR = GD_ROWS(D, LPE, !MULTI);
    constexpr int TCR = MULTI ? (MAX_TIPS * (7 * D + 24) + WAVE - 1) / WAVE : 0; // (several tips: the chains' constants)
    constexpr int PER_WAVE = WAVE / LPE;
    __shared__ double lds[(GDR + TCR) * WAVE + PER_WAVE * D];
    const int lane = threadIdx.x;
    const int sub = lane % LPE;
    double* const seed_l = lds + (GDR + TCR) * WAVE + (lane / LPE) * D;
    long long ii, evals = 0;
    int gens = 0, reached;
    const bool open = globalpath_begin<LPE>(a, ii);
    if (!__any(open)) return;
    const PathArgs rows = globalpath_rows(a);
    double sd[D];
    bool active;
    globalpath_first<D>(a, rows, ii, open, sub == 0, sd, active, reached);
    if constexpr (MULTI) stage_tip_constants<D>(c, lds + GDR * WAVE, lane);
    for (int k = 1; k < a.W && __any(active); ++k) {
        const long long row = ii * a.W + k;
        typename GoalSel<MULTI>::type g;
        load_goals<D>(c, a.goal, row, g);
        GdState<D> s;
        path_state<D>(sd, s);
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
        path_waypoint<D>(c, p, rows, g, sd, s, row, sub == 0, active, reached);
        startpath_count<D>(s, ran, evals, gens);
    }
    path_tail<D>(rows, sd, ii, open && sub == 0, reached);
    globalpath_fold<D>(c, a, ii, open, sub == 0, reached, evals, gens);
}
#endif

#if defined(PIK_STRICT)
// exact flavours, one tip frame, LPE lanes per path: the team forms of the memoised descent, as ik_path_team_kernel
// (every lane of a path holds the same state; its first lane stores)
template <int D, int LPE>
__global__ __launch_bounds__(WAVE) void ik_globalpath_team_kernel(const ConstsK<D>* __restrict__ kc, GlobalPathArgs a) {
    PIK_CONSTS(kc);
    __shared__ double lds[GD_ROWS(D, LPE) * WAVE];
    const int lane = threadIdx.x;
    const int sub = lane % LPE;
    long long ii, evals = 0;
    int gens = 0, reached;
    const bool open = globalpath_begin<LPE>(a, ii);
    if (!__any(open)) return;
    const PathArgs rows = globalpath_rows(a);
    double sd[D];
    bool active;
    globalpath_first<D>(a, rows, ii, open, sub == 0, sd, active, reached);
    for (int k = 1; k < a.W && __any(active); ++k) {
        const long long row = ii * a.W + k;
        GoalK g;
        load_goals<D>(c, a.goal, row, g);
        GdState<D> s;
        path_state<D>(sd, s);
        const bool ran = active;
        PIK_DESCENT(GD_LOCAL, LPE, g, sd, nullptr, s, active, p.local_max_iters, lds, lane, sub);
        path_waypoint<D>(c, p, rows, g, sd, s, row, sub == 0, active, reached);
        startpath_count<D>(s, ran, evals, gens);
    }
    path_tail<D>(rows, sd, ii, open && sub == 0, reached);
    globalpath_fold<D>(c, a, ii, open, sub == 0, reached, evals, gens);
}
#endif

template <int D>
int launch_globalpath_prepare(pikamd_solver* s, const ParamsK& pk, const GlobalPathArgs& a, hipStream_t st, int slot) {
    if (a.P == 0) return 0;
    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, &pk, slot, st, &kc)) return rc;
    hipLaunchKernelGGL(ik_globalpath_prepare_kernel<D>, dim3((unsigned)((a.P + WAVE - 1) / WAVE)), dim3(WAVE), 0, st, kc, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// One launch per attempt; the variant by path_lanes (pik_path_ops.hpp).  Stream-ordered: nothing here waits unless the
// slot's constants change (upload_consts).
template <int D>
int launch_globalpath_tail(pikamd_solver* s, const ParamsK& pk, const GlobalPathArgs& a, hipStream_t st, int slot) {
    if (a.P == 0) return 0;
    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, &pk, slot, st, &kc)) return rc;
    const bool multi = s->n_tips > 1;
    const int lpe = path_lanes(s, a.P, EXACT_FLAVOUR);
    const long long per_wave = WAVE / lpe;
    const dim3 g((unsigned)((a.P + per_wave - 1) / per_wave)), b(WAVE);
#if !defined(PIK_STRICT)
    if (lpe == 16 && multi) hipLaunchKernelGGL((ik_globalpath_wide_kernel<D, 16, true>), g, b, 0, st, kc, a);
    else if (lpe == 8 && multi) hipLaunchKernelGGL((ik_globalpath_wide_kernel<D, 8, true>), g, b, 0, st, kc, a);
    else if (lpe == 16) hipLaunchKernelGGL((ik_globalpath_wide_kernel<D, 16>), g, b, 0, st, kc, a);
    else if (lpe == 8) hipLaunchKernelGGL((ik_globalpath_wide_kernel<D, 8>), g, b, 0, st, kc, a);
#else
    if (lpe == 16) hipLaunchKernelGGL((ik_globalpath_team_kernel<D, 16>), g, b, 0, st, kc, a);
    else if (lpe == 4) hipLaunchKernelGGL((ik_globalpath_team_kernel<D, 4>), g, b, 0, st, kc, a);
#endif
    else if (multi) hipLaunchKernelGGL((ik_globalpath_kernel<D, true>), g, b, 0, st, kc, a);
    else hipLaunchKernelGGL(ik_globalpath_kernel<D>, g, b, 0, st, kc, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int D>
const GlobalPathOps* make_globalpath_ops() {
    static const GlobalPathOps ops = {&launch_globalpath_prepare<D>, &launch_globalpath_tail<D>};
    return &ops;
}

} // namespace pik
