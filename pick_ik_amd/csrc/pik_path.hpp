// pik_path.hpp -- Cartesian waypoint paths: chained local IK in one launch (pikamd_solve_paths).
//
// computeCartesianPath, servoing and straight-line approach sampling solve every waypoint of a path from the
// previous waypoint's answer.  As a host loop that is W dependent pikamd_solve_batch calls -- each one copies in,
// launches, copies out and synchronises for one short descent from a seed that is already close.  The kernels here
// wrap the EXISTING local-mode descents (pik_kernels.hpp: PIK_DESCENT(GD_LOCAL, ...), gd_wide, gd_wide_multi) in a
// per-path waypoint loop: a lane (or a team of lanes) owns one path, loads waypoint k's goal, runs GradientIk::from +
// the loop + the post-loop exactly as ik_gradient_kernel does, applies the joint-step test, stores the waypoint's row
// and carries the answer on as the next seed in registers.  A path that stops goes on masked (the descents take the
// mask) and fills its remaining rows behind the loop; the loop ends when no path of the wavefront is held.
//
// The result is defined as what the loop of pikamd_solve_batch calls returns (include/pick_ik_amd.h), and every
// variant below performs the arithmetic of the one-lane kernel, so all of them return the same bits.
//
// Across a descent the loop itself keeps only the seed, the path index, the waypoint counter, the held flag and the
// count of held waypoints live (the goal too, as in ik_gradient_kernel: a failed waypoint reports the cost of its
// seed): the descents sit at the register cap.
//
// Compiled in translation units of its own (pik_path_inst.hip), for the flavours fast, exact and strict: nothing
// here is read by pik_inst.hip, whose kernels are compiled from the text they had before this file existed.
#pragma once

#include "pik_launch.hpp"
#include "pik_path_ops.hpp"

namespace pik {

constexpr int PIKAMD_PATH_JUMP_K = -1001; // PIKAMD_PATH_JUMP

// Behind the descent of waypoint `row` (= path * W + k): the post-loop of ik_gradient (src/ik_gradient.cpp:130-138)
// as ik_gradient_kernel has it, the joint-step test, the waypoint's row (stored by the lanes with `store`: the
// path's first lane) and what the path carries on -- the answer as the next seed, or the end of the path.
// All lanes of the wavefront call this together.
template <int D, typename G>
__device__ __forceinline__ void path_waypoint(CK<D> c, PK p, const PathArgs& a, const G& g, double (&sd)[D],
                                              const GdState<D>& s, long long row, bool store, bool& active,
                                              int& reached) {
    int status = PIKAMD_NO_IK_SOLUTION_K;
    if (s.found) {
        status = 1;
    } else if (!p.stop_on_valid && s.best_sol) {
        status = 1;
    } else if (p.approx) {
        status = 2;
    }
    double first_cost = 0.0; // cost of the initial guess (= the seed), reported on failure
    if (__any(active && status < 0)) {
        EvalOut e;
        evaluate<D>(c, p, g, sd, sd, e);
        first_cost = e.cost;
    }
    // a variable that moved further than its limit: the waypoint is solved but refused (plain IEEE compares; a
    // limit that is 0 or less, or not a number, is none)
    bool jump = false;
    if (a.max_step) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const double lim = a.max_step[j];
            jump = jump || (lim > 0.0 && fabs(s.best[j] - sd[j]) > lim);
        }
    }
    jump = jump && status > 0;
    const bool held = status > 0 && !jump;
    if (active && store) {
#pragma unroll
        for (int j = 0; j < D; ++j) a.solution[row * D + j] = held ? s.best[j] : sd[j];
        a.status[row] = jump ? PIKAMD_PATH_JUMP_K : status;
        if (a.cost) a.cost[row] = (status > 0) ? s.best_cost : first_cost;
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
    if (active && held) {
#pragma unroll
        for (int j = 0; j < D; ++j) sd[j] = s.best[j];
        ++reached;
    }
    active = active && held;
}

// Behind the waypoint loop: the rows behind the waypoint the path stopped at (the last held configuration, not
// attempted, cost 0, no statistics) and the count of held waypoints.  A path that held throughout has none.
template <int D>
__device__ __forceinline__ void path_tail(const PathArgs& a, const double (&sd)[D], long long path, bool store,
                                          int reached) {
    if (!store) return;
    for (int k = reached + 1; k < a.W; ++k) {
        const long long row = path * a.W + k;
#pragma unroll
        for (int j = 0; j < D; ++j) a.solution[row * D + j] = sd[j];
        a.status[row] = 0; // PIKAMD_NOT_ATTEMPTED
        if (a.cost) a.cost[row] = 0.0;
        if (a.stats) {
            StatsK st;
            st.cost_evals = 0;
            st.generations = 0;
            st.wipeouts = 0;
            st.pool_erasures = 0;
            st.reserved = 0;
            static_cast<StatsK*>(a.stats)[row] = st;
        }
    }
    if (a.reached) a.reached[path] = reached;
}

// The path a lane owns -- one lane per path, or a team of LPE adjacent lanes -- and its first seed.  A lane without a
// path runs masked on path 0's data.  Returns whether the lane has a path.
template <int D, int LPE>
__device__ __forceinline__ bool path_begin(const PathArgs& a, long long& path, double (&sd)[D]) {
    const long long i = (long long)blockIdx.x * (WAVE / LPE) + threadIdx.x / LPE;
    const bool mine = i < a.P;
    path = mine ? i : 0;
#pragma unroll
    for (int j = 0; j < D; ++j) sd[j] = a.start[path * D + j];
    return mine;
}

// GradientIk::from for a waypoint: the search starts at the seed
template <int D>
__device__ __forceinline__ void path_state(const double (&sd)[D], GdState<D>& s) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
        s.local[j] = sd[j];
        s.best[j] = sd[j];
        s.grad[j] = 0.0;
    }
    s.local_cost = 0.0;
    s.best_cost = 0.0;
    s.best_sol = false;
}

// one lane per path, one tip frame or several (every flavour)
template <int D, bool MULTI = false>
__global__ __launch_bounds__(WAVE) void ik_path_kernel(const ConstsK<D>* __restrict__ kc, PathArgs a) {
    PIK_CONSTS(kc);
    __shared__ double frames[GD_ROWS(D) * WAVE];
    long long ii;
    double sd[D];
    const bool mine = path_begin<D, 1>(a, ii, sd);
    bool active = mine;
    int reached = 0;
    for (int k = 0; k < a.W && __any(active); ++k) {
        const long long row = ii * a.W + k;
        typename GoalSel<MULTI>::type g;
        load_goals<D>(c, a.goal, row, g);
        GdState<D> s;
        path_state<D>(sd, s);
        PIK_DESCENT(GD_LOCAL, 1, g, sd, nullptr, s, active, p.local_max_iters, frames, (int)threadIdx.x, 0);
        path_waypoint<D>(c, p, a, g, sd, s, row, true, active, reached);
    }
    path_tail<D>(a, sd, ii, mine, reached);
}

#if !defined(PIK_STRICT)
// LPE lanes per path: the cooperative descent (gd_wide / gd_wide_multi), as ik_gradient_wide_kernel.  Its probes
// read the seed by a per-lane joint index from memory: the team keeps a copy of its path's current seed in LDS.
template <int D, int LPE, bool MULTI = false>
__global__ __launch_bounds__(WAVE) void ik_path_wide_kernel(const ConstsK<D>* __restrict__ kc, PathArgs a) {
    PIK_CONSTS(kc);
    constexpr int GDR = GD_ROWS(D, LPE, !MULTI);
    constexpr int TCR = MULTI ? (MAX_TIPS * (7 * D + 24) + WAVE - 1) / WAVE : 0; // (several tips: the chains' constants)
    constexpr int PER_WAVE = WAVE / LPE;
    __shared__ double lds[(GDR + TCR) * WAVE + PER_WAVE * D];
    const int lane = threadIdx.x;
    const int sub = lane % LPE;
    double* const seed_l = lds + (GDR + TCR) * WAVE + (lane / LPE) * D;
    long long ii;
    double sd[D];
    const bool mine = path_begin<D, LPE>(a, ii, sd);
    bool active = mine;
    int reached = 0;
    if constexpr (MULTI) stage_tip_constants<D>(c, lds + GDR * WAVE, lane);
    for (int k = 0; k < a.W && __any(active); ++k) {
        const long long row = ii * a.W + k;
        typename GoalSel<MULTI>::type g;
        load_goals<D>(c, a.goal, row, g);
        GdState<D> s;
        path_state<D>(sd, s);
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
        path_waypoint<D>(c, p, a, g, sd, s, row, sub == 0, active, reached);
    }
    path_tail<D>(a, sd, ii, mine && sub == 0, reached);
}
#endif

#if defined(PIK_STRICT)
// exact flavours, one tip frame, LPE lanes per path: the team forms of the memoised descent, as
// ik_gradient_team_kernel (every lane of a path holds the same state; its first lane stores)
template <int D, int LPE>
__global__ __launch_bounds__(WAVE) void ik_path_team_kernel(const ConstsK<D>* __restrict__ kc, PathArgs a) {
    PIK_CONSTS(kc);
    __shared__ double lds[GD_ROWS(D, LPE) * WAVE];
    const int lane = threadIdx.x;
    const int sub = lane % LPE;
    long long ii;
    double sd[D];
    const bool mine = path_begin<D, LPE>(a, ii, sd);
    bool active = mine;
    int reached = 0;
    for (int k = 0; k < a.W && __any(active); ++k) {
        const long long row = ii * a.W + k;
        GoalK g;
        load_goals<D>(c, a.goal, row, g);
        GdState<D> s;
        path_state<D>(sd, s);
        PIK_DESCENT(GD_LOCAL, LPE, g, sd, nullptr, s, active, p.local_max_iters, lds, lane, sub);
        path_waypoint<D>(c, p, a, g, sd, s, row, sub == 0, active, reached);
    }
    path_tail<D>(a, sd, ii, mine && sub == 0, reached);
}
#endif

// One launch for the whole call; the variant by path_lanes (pik_path_ops.hpp).  Stream-ordered: nothing here
// waits unless the slot's constants change (upload_consts).
template <int D>
int launch_paths(pikamd_solver* s, const ParamsK& pk, const PathArgs& a, hipStream_t st, int slot) {
    if (a.P == 0) return 0;
    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, &pk, slot, st, &kc)) return rc;
    const bool multi = s->n_tips > 1;
    const int lpe = path_lanes(s, a.P, EXACT_FLAVOUR);
    const long long per_wave = WAVE / lpe;
    const dim3 g((unsigned)((a.P + per_wave - 1) / per_wave)), b(WAVE);
#if !defined(PIK_STRICT)
    if (lpe == 16 && multi) hipLaunchKernelGGL((ik_path_wide_kernel<D, 16, true>), g, b, 0, st, kc, a);
    else if (lpe == 8 && multi) hipLaunchKernelGGL((ik_path_wide_kernel<D, 8, true>), g, b, 0, st, kc, a);
    else if (lpe == 16) hipLaunchKernelGGL((ik_path_wide_kernel<D, 16>), g, b, 0, st, kc, a);
    else if (lpe == 8) hipLaunchKernelGGL((ik_path_wide_kernel<D, 8>), g, b, 0, st, kc, a);
#else
    if (lpe == 16) hipLaunchKernelGGL((ik_path_team_kernel<D, 16>), g, b, 0, st, kc, a);
    else if (lpe == 4) hipLaunchKernelGGL((ik_path_team_kernel<D, 4>), g, b, 0, st, kc, a);
#endif
    else if (multi) hipLaunchKernelGGL((ik_path_kernel<D, true>), g, b, 0, st, kc, a);
    else hipLaunchKernelGGL(ik_path_kernel<D>, g, b, 0, st, kc, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int D>
const PathOps* make_path_ops() {
    static const PathOps ops = {&launch_paths<D>};
    return &ops;
}

} // namespace pik
