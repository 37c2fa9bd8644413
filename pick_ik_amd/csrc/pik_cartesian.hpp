// pik_cartesian.hpp -- computeCartesianPath in one call (pikamd_cartesian_paths): P Cartesian motions, each a start
// joint state and a target, walked for their own number of steps, with the absolute and the relative jump test and
// MoveIt's fraction.
//
// Two steps on the stream.  The PREPARE kernel, one lane per path, runs forward kinematics on the start exactly as
// fk_kernel does (the bits of pikamd_fk_batch), then the interpolation header (pik_interp.hpp: the bits of
// pikamd_interpolate_poses) and writes the path's step count and its W goal rows.  The WALK kernels are the three
// variants of the path family (pik_path.hpp) around the unchanged descents, path_waypoint and load_goals, with three
// differences: the loop of a path runs while k < steps[path], a path with more steps than W never becomes active,
// and a tail of their own fills the rows behind the stop, applies the relative jump test to the rows the path's
// storing lane wrote and stores reached and fraction.
//
// The result is defined by pikamd_fk_batch, pikamd_interpolate_poses and pikamd_solve_paths (include/pick_ik_amd.h),
// and every variant performs the arithmetic of the one-lane kernel, so all of them return the same bits.
//
// Across a descent the loop keeps live what ik_path_kernel keeps, and the step count: the descents sit at the
// register cap.  The goal row is loaded from memory per waypoint.
//
// Compiled in translation units of its own (pik_cartesian_inst.hip), for the flavours fast, exact and strict: nothing
// here is read by pik_inst.hip.
#pragma once

#include "pik_cartesian_ops.hpp"
#include "pik_interp.hpp"
#include "pik_path.hpp"

namespace pik {

constexpr int PIKAMD_PATH_RELATIVE_JUMP_K = -1003; // PIKAMD_PATH_RELATIVE_JUMP

// one lane per path: the start's pose (fk_kernel's statements), the step count and the goal rows
template <int D>
__global__ __launch_bounds__(256) void cartesian_prepare_kernel(const ConstsK<D>* __restrict__ kc, CartesianArgs a) {
    PIK_CONSTS(kc);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.path.P) return;
    double qq[D];
#pragma unroll
    for (int j = 0; j < D; ++j) qq[j] = a.path.start[i * D + j];
    double R[9], t[3], qt[4];
    fk<D, false>(c, qq, R, t, nullptr, 0);
    matrix_to_quat(R, qt);
    const double pose[7] = {t[0], t[1], t[2], qt[0], qt[1], qt[2], qt[3]};
    double tg[7];
#pragma unroll
    for (int e = 0; e < 7; ++e) tg[e] = a.target[7 * i + e];
    const pik_interp::Motion m = {a.frame, a.min_steps, a.max_translation, a.max_rotation};
    a.steps[i] = pik_interp::interpolate_path(m, a.path.W, pose, tg, a.goals + 7 * i * a.path.W);
}

// a row nobody solved: the configuration `q`, not attempted, cost 0, no statistics
template <int D>
__device__ __forceinline__ void cartesian_blank_row(const PathArgs& a, long long row, const double* q) {
#pragma unroll
    for (int j = 0; j < D; ++j) a.solution[row * D + j] = q[j];
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

// the distance of two configurations for the relative test: the sum over the variables, ascending, of the absolute
// differences
template <int D>
__device__ __forceinline__ double cartesian_dist(const double* from, const double* to) {
#pragma clang fp contract(off)
    double d = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) d = d + fabs(to[j] - from[j]);
    return d;
}

// Behind the waypoint loop, by the lane that stored the path's rows (`store`).  n: the path's steps; reached: the
// waypoints held; sd: the last held configuration (the start when none).  Fills the rows behind the stop, applies the
// relative jump test (MoveIt's checkRelativeJointSpaceJump over the start and the held rows) and stores reached and
// fraction.
template <int D>
__device__ __forceinline__ void cartesian_tail(const CartesianArgs& ca, const double (&sd)[D], long long path,
                                               bool store, int n, int reached) {
#pragma clang fp contract(off)
    if (!store) return;
    const PathArgs& a = ca.path;
    const long long row0 = path * a.W;
    // too long: every row blank; complete: the rows behind the last step; stopped: the rows behind the refused one
    const int behind = n > a.W ? 0 : (reached == n ? n : reached + 1);
    for (int k = behind; k < a.W; ++k) cartesian_blank_row<D>(a, row0 + k, sd);
    double fraction = n > a.W ? 0.0 : (double)reached / (double)n;
    if (ca.jump_factor > 0.0 && reached >= 1) {
        // traj[0] = the start, traj[i] = row i - 1
        const double* const first = a.start + path * D;
        const double* const rows = a.solution + row0 * D;
        double total = 0.0;
        for (int i = 0; i < reached; ++i)
            total = total + cartesian_dist<D>(i == 0 ? first : rows + (long long)(i - 1) * D, rows + (long long)i * D);
        const double thres = ca.jump_factor * (total / (double)reached);
        for (int i = 0; i < reached; ++i) {
            const double* const from = i == 0 ? first : rows + (long long)(i - 1) * D;
            if (!(cartesian_dist<D>(from, rows + (long long)i * D) > thres)) continue;
            fraction = fraction * ((double)(i + 1) / (double)(reached + 1));
            double keep[D];
#pragma unroll
            for (int j = 0; j < D; ++j) keep[j] = from[j];
            // row i: refused, its cost and counters stay; behind it: blank
#pragma unroll
            for (int j = 0; j < D; ++j) a.solution[(row0 + i) * D + j] = keep[j];
            a.status[row0 + i] = PIKAMD_PATH_RELATIVE_JUMP_K;
            for (int k = i + 1; k < a.W; ++k) cartesian_blank_row<D>(a, row0 + k, keep);
            reached = i;
            break;
        }
    }
    if (a.reached) a.reached[path] = reached;
    if (ca.fraction) ca.fraction[path] = fraction;
}

// the steps of the lane's path, and whether it is walked at all
__device__ __forceinline__ int cartesian_begin(const CartesianArgs& ca, long long path, bool mine, bool& active) {
    const int n = ca.steps[path];
    active = mine && n <= ca.path.W;
    return n;
}

// one lane per path (every flavour)
template <int D>
__global__ __launch_bounds__(WAVE) void ik_cartesian_kernel(const ConstsK<D>* __restrict__ kc, CartesianArgs ca) {
    PIK_CONSTS(kc);
    __shared__ double frames[GD_ROWS(D) * WAVE];
    const PathArgs& a = ca.path;
    long long ii;
    double sd[D];
    const bool mine = path_begin<D, 1>(a, ii, sd);
    bool active;
    const int n = cartesian_begin(ca, ii, mine, active);
    int reached = 0;
    for (int k = 0; __any(active && k < n); ++k) {
        active = active && k < n;
        const long long row = ii * a.W + k; // (k < W: some active lane's steps are above k, and they are at most W)
        GoalK g;
        load_goals<D>(c, a.goal, row, g);
        GdState<D> s;
        path_state<D>(sd, s);
        PIK_DESCENT(GD_LOCAL, 1, g, sd, nullptr, s, active, p.local_max_iters, frames, (int)threadIdx.x, 0);
        path_waypoint<D>(c, p, a, g, sd, s, row, true, active, reached);
    }
    cartesian_tail<D>(ca, sd, ii, mine, n, reached);
}

#if !defined(PIK_STRICT)
// LPE lanes per path: the cooperative descent, as ik_path_wide_kernel (one tip frame)
template <int D, int LPE>
__global__ __launch_bounds__(WAVE) void ik_cartesian_wide_kernel(const ConstsK<D>* __restrict__ kc, CartesianArgs ca) {
    PIK_CONSTS(kc);
    constexpr int GDR = GD_ROWS(D, LPE, true);
    constexpr int PER_WAVE = WAVE / LPE;
    __shared__ double lds[GDR * WAVE + PER_WAVE * D];
    const PathArgs& a = ca.path;
    const int lane = threadIdx.x;
    const int sub = lane % LPE;
    double* const seed_l = lds + GDR * WAVE + (lane / LPE) * D;
    long long ii;
    double sd[D];
    const bool mine = path_begin<D, LPE>(a, ii, sd);
    bool active;
    const int n = cartesian_begin(ca, ii, mine, active);
    int reached = 0;
    for (int k = 0; __any(active && k < n); ++k) {
        active = active && k < n;
        const long long row = ii * a.W + k;
        GoalK g;
        load_goals<D>(c, a.goal, row, g);
        GdState<D> s;
        path_state<D>(sd, s);
        wave_sync(); // (the previous waypoint's probes have read the copy)
        if (sub == 0) {
#pragma unroll
            for (int j = 0; j < D; ++j) seed_l[j] = sd[j];
        }
        wave_sync();
        gd_wide<D, LPE, GD_LOCAL>(c, p, g, sd, seed_l, s, active, p.local_max_iters, lds, lane, sub);
        path_waypoint<D>(c, p, a, g, sd, s, row, sub == 0, active, reached);
    }
    cartesian_tail<D>(ca, sd, ii, mine && sub == 0, n, reached);
}
#endif

#if defined(PIK_STRICT)
// exact flavours, LPE lanes per path: the team forms of the memoised descent, as ik_path_team_kernel
template <int D, int LPE>
__global__ __launch_bounds__(WAVE) void ik_cartesian_team_kernel(const ConstsK<D>* __restrict__ kc, CartesianArgs ca) {
    PIK_CONSTS(kc);
    __shared__ double lds[GD_ROWS(D, LPE) * WAVE];
    const PathArgs& a = ca.path;
    const int lane = threadIdx.x;
    const int sub = lane % LPE;
    long long ii;
    double sd[D];
    const bool mine = path_begin<D, LPE>(a, ii, sd);
    bool active;
    const int n = cartesian_begin(ca, ii, mine, active);
    int reached = 0;
    for (int k = 0; __any(active && k < n); ++k) {
        active = active && k < n;
        const long long row = ii * a.W + k;
        GoalK g;
        load_goals<D>(c, a.goal, row, g);
        GdState<D> s;
        path_state<D>(sd, s);
        PIK_DESCENT(GD_LOCAL, LPE, g, sd, nullptr, s, active, p.local_max_iters, lds, lane, sub);
        path_waypoint<D>(c, p, a, g, sd, s, row, sub == 0, active, reached);
    }
    cartesian_tail<D>(ca, sd, ii, mine && sub == 0, n, reached);
}
#endif

// the prepare step: one launch, stream-ordered
template <int D>
int launch_cartesian_prepare(pikamd_solver* s, const ParamsK& pk, const CartesianArgs& a, hipStream_t st, int slot) {
    if (a.path.P == 0) return 0;
    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, &pk, slot, st, &kc)) return rc;
    const int block = 256;
    const long long grid = (a.path.P + block - 1) / block;
    hipLaunchKernelGGL(cartesian_prepare_kernel<D>, dim3((unsigned)grid), dim3(block), 0, st, kc, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the walk: one launch; the variant by path_lanes (pik_path_ops.hpp)
template <int D>
int launch_cartesian_walk(pikamd_solver* s, const ParamsK& pk, const CartesianArgs& a, hipStream_t st, int slot) {
    if (a.path.P == 0) return 0;
    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, &pk, slot, st, &kc)) return rc;
    const int lpe = path_lanes(s, a.path.P, EXACT_FLAVOUR);
    const long long per_wave = WAVE / lpe;
    const dim3 g((unsigned)((a.path.P + per_wave - 1) / per_wave)), b(WAVE);
#if !defined(PIK_STRICT)
    if (lpe == 16) hipLaunchKernelGGL((ik_cartesian_wide_kernel<D, 16>), g, b, 0, st, kc, a);
    else if (lpe == 8) hipLaunchKernelGGL((ik_cartesian_wide_kernel<D, 8>), g, b, 0, st, kc, a);
#else
    if (lpe == 16) hipLaunchKernelGGL((ik_cartesian_team_kernel<D, 16>), g, b, 0, st, kc, a);
    else if (lpe == 4) hipLaunchKernelGGL((ik_cartesian_team_kernel<D, 4>), g, b, 0, st, kc, a);
#endif
    else hipLaunchKernelGGL(ik_cartesian_kernel<D>, g, b, 0, st, kc, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int D>
const CartesianOps* make_cartesian_ops() {
    static const CartesianOps ops = {&launch_cartesian_prepare<D>, &launch_cartesian_walk<D>};
    return &ops;
}

} // namespace pik
