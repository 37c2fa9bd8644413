// pik_polyline.hpp -- computeCartesianPath through a list of waypoints (pikamd_cartesian_waypoints): P motions, each a
// start joint state and up to S targets.  Segment i starts at the tip pose of the joint state segment i-1 ended in --
// not at target i-1 --, so its poses and its step count exist only once segment i-1 has been solved.
//
// S passes and a finish on the stream, no host round trip.  Pass i: the SEGMENT kernel, one lane per path, runs forward
// kinematics on the path's current state exactly as fk_kernel does (the bits of pikamd_fk_batch), then the
// interpolation header (pik_interp.hpp: the bits of pikamd_interpolate_poses) into the rows the path has left, and
// writes the segment's step count; a segment with more steps than rows closes the path.  The WALK kernels are the loops
// of ik_cartesian_*_kernel (pik_cartesian.hpp) around the unchanged descents, load_goals, path_state and path_waypoint:
// the row base is the path's first free row, the start its current state (the start, or the last row of the previous
// segment -- no copy), the bound the segment's steps.  Behind the loop the storing lane updates the path's state.  The
// FINISH kernel fills the rows behind the stop, applies the relative jump test to the stitched rows (cartesian_dist and
// the statements of cartesian_tail) and stores reached, steps and fraction.  A wavefront none of whose paths is open
// finds no step to walk and returns.
//
// The passes are not fused into one walk launch: the boundary forward kinematics must return pikamd_fk_batch's bits, and
// the flavour of the parity hooks can differ from the walk's; and the descents have no registers to spare.
//
// The result is defined by pikamd_cartesian_paths (include/pick_ik_amd.h), and every variant performs the arithmetic of
// the one-lane kernel, so all of them return the same bits.
//
// Across a descent the loop keeps live what ik_cartesian_kernel keeps -- the row base stands where the path index
// stood --: the descents sit at the register cap.  The path index is computed again behind the loop.
//
// Compiled in translation units of its own (pik_polyline_inst.hip), for the flavours fast, exact and strict: nothing
// here is read by pik_inst.hip.  Reading pik_cartesian.hpp instantiates none of its kernels.
#pragma once

#include "pik_cartesian.hpp"
#include "pik_polyline_ops.hpp"

namespace pik {

// the targets of a path: n_targets clamped to 0..S
__device__ __forceinline__ int polyline_targets(const PolylineArgs& pa, long long path) {
    if (!pa.n_targets) return pa.S;
    const int v = pa.n_targets[path];
    return v < 0 ? 0 : (v > pa.S ? pa.S : v);
}

// one lane per path: the state of the first pass; for an open path with a target left the current state's pose
// (fk_kernel's statements), the segment's step count and its goal rows
template <int D>
__global__ __launch_bounds__(256) void polyline_segment_kernel(const ConstsK<D>* __restrict__ kc, PolylineArgs pa) {
    PIK_CONSTS(kc);
    const PathArgs& a = pa.path;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.P) return;
    const int sp = polyline_targets(pa, i);
    int off = 0, open = sp > 0 ? 1 : 0;
    if (pa.seg == 0) {
        pa.st.off[i] = 0;
        pa.st.held[i] = 0;
        pa.st.behind[i] = 0;
        pa.st.need[i] = 0;
        pa.st.open[i] = open;
        pa.st.frac[i] = 0.0;
        if (!open) // (no target: no pose is ever made -- the rows are zero)
            for (long long e = 0; e < 7ll * a.W; ++e) pa.goals[7 * i * a.W + e] = 0.0;
    } else {
        off = pa.st.off[i];
        open = pa.st.open[i];
    }
    int n_i = 0, walk = 0;
    if (open && pa.seg < sp) {
        const long long row0 = i * a.W + off;
        const double* const cur = off == 0 ? a.start + i * D : a.solution + (row0 - 1) * D;
        double qq[D];
#pragma unroll
        for (int j = 0; j < D; ++j) qq[j] = cur[j];
        double R[9], t[3], qt[4];
        fk<D, false>(c, qq, R, t, nullptr, 0);
        matrix_to_quat(R, qt);
        const double pose[7] = {t[0], t[1], t[2], qt[0], qt[1], qt[2], qt[3]};
        double tg[7];
#pragma unroll
        for (int e = 0; e < 7; ++e) tg[e] = pa.targets[7 * (i * pa.S + pa.seg) + e];
        const pik_interp::Motion m = {pa.frame, pa.min_steps, pa.max_translation, pa.max_rotation};
        const int room = a.W - off; // (no room: the count only, no pose is written)
        n_i = pik_interp::interpolate_path(m, room, pose, tg, pa.goals + 7 * row0);
        pa.st.need[i] = n_i > 2147483647 - off ? 2147483647 : off + n_i;
        if (n_i > room) pa.st.open[i] = 0; // did not fit: the rows from `off` stay blank
        else walk = n_i;
    }
    pa.st.n[i] = walk;
    if (pa.segment_steps) pa.segment_steps[i * pa.S + pa.seg] = n_i;
}

// The path a lane owns (as path_begin), the steps its segment has in this pass (0: none), its first free row and its
// current state: the start, or the last row of the previous segment (no segment: row 0 and the start, never read for
// a result).  A lane without a path runs masked on path 0's data.  Returns whether the lane has a path.
template <int D, int LPE>
__device__ __forceinline__ bool polyline_begin(const PolylineArgs& pa, long long& row0, double (&sd)[D], int& n) {
    const PathArgs& a = pa.path;
    const long long i = (long long)blockIdx.x * (WAVE / LPE) + threadIdx.x / LPE;
    const bool mine = i < a.P;
    const long long path = mine ? i : 0;
    n = pa.st.n[path];
    // (a path without a segment in this pass walks nothing, but its lane loads a goal row as long as a neighbour
    // walks: it is given its first row -- `off` may be W, a row behind the path's last)
    const int off = n > 0 ? pa.st.off[path] : 0;
    row0 = path * a.W + off;
    const double* const cur = off == 0 ? a.start + path * D : a.solution + (row0 - 1) * D;
#pragma unroll
    for (int j = 0; j < D; ++j) sd[j] = cur[j];
    return mine;
}

// Behind the waypoint loop, by the lane that stored the segment's rows: what the path carries into the next pass.
// n: the segment's steps (0: the path had none in this pass); reached: the waypoints of it held.
template <int LPE>
__device__ __forceinline__ void polyline_tail(const PolylineArgs& pa, long long row0, bool store, int n, int reached) {
#pragma clang fp contract(off)
    if (!store || n == 0) return;
    const long long path = (long long)blockIdx.x * (WAVE / LPE) + threadIdx.x / LPE;
    const int off = (int)(row0 - path * pa.path.W);
    const double sp = (double)polyline_targets(pa, path);
    pa.st.held[path] = off + reached;
    if (reached == n) {
        pa.st.behind[path] = off + n;
        pa.st.off[path] = off + n;
        pa.st.frac[path] = (double)(pa.seg + 1) / sp;
    } else {
        pa.st.behind[path] = off + reached + 1; // (the refused row is the segment's)
        pa.st.open[path] = 0;
        pa.st.frac[path] = (double)pa.seg / sp + ((double)reached / (double)n) / sp;
    }
}

// one lane per path (every flavour)
template <int D>
__global__ __launch_bounds__(WAVE) void ik_polyline_kernel(const ConstsK<D>* __restrict__ kc, PolylineArgs pa) {
    PIK_CONSTS(kc);
    __shared__ double frames[GD_ROWS(D) * WAVE];
    const PathArgs& a = pa.path;
    long long row0;
    double sd[D];
    int n;
    const bool mine = polyline_begin<D, 1>(pa, row0, sd, n);
    bool active = mine && n > 0;
    int reached = 0;
    for (int k = 0; __any(active && k < n); ++k) {
        active = active && k < n;
        // (an active lane: k < n <= the rows the path has left; a masked lane loads its goal too, so it stays on the
        // first row of its segment -- polyline_begin keeps that one inside the path)
        const long long row = row0 + (k < n ? k : 0);
        GoalK g;
        load_goals<D>(c, a.goal, row, g);
        GdState<D> s;
        path_state<D>(sd, s);
        PIK_DESCENT(GD_LOCAL, 1, g, sd, nullptr, s, active, p.local_max_iters, frames, (int)threadIdx.x, 0);
        path_waypoint<D>(c, p, a, g, sd, s, row, true, active, reached);
    }
    polyline_tail<1>(pa, row0, mine, n, reached);
}

#if !defined(PIK_STRICT)
// LPE lanes per path: the cooperative descent, as ik_cartesian_wide_kernel (one tip frame)
template <int D, int LPE>
__global__ __launch_bounds__(WAVE) void ik_polyline_wide_kernel(const ConstsK<D>* __restrict__ kc, PolylineArgs pa) {
    PIK_CONSTS(kc);
    constexpr int GDR = GD_ROWS(D, LPE, true);
    constexpr int PER_WAVE = WAVE / LPE;
    __shared__ double lds[GDR * WAVE + PER_WAVE * D];
    const PathArgs& a = pa.path;
    const int lane = threadIdx.x;
    const int sub = lane % LPE;
    double* const seed_l = lds + GDR * WAVE + (lane / LPE) * D;
    long long row0;
    double sd[D];
    int n;
    const bool mine = polyline_begin<D, LPE>(pa, row0, sd, n);
    bool active = mine && n > 0;
    int reached = 0;
    for (int k = 0; __any(active && k < n); ++k) {
        active = active && k < n;
        const long long row = row0 + (k < n ? k : 0); // (a masked lane stays inside its path, see ik_polyline_kernel)
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
    polyline_tail<LPE>(pa, row0, mine && sub == 0, n, reached);
}
#endif

#if defined(PIK_STRICT)
// exact flavours, LPE lanes per path: the team forms of the memoised descent, as ik_cartesian_team_kernel
template <int D, int LPE>
__global__ __launch_bounds__(WAVE) void ik_polyline_team_kernel(const ConstsK<D>* __restrict__ kc, PolylineArgs pa) {
    PIK_CONSTS(kc);
    __shared__ double lds[GD_ROWS(D, LPE) * WAVE];
    const PathArgs& a = pa.path;
    const int lane = threadIdx.x;
    const int sub = lane % LPE;
    long long row0;
    double sd[D];
    int n;
    const bool mine = polyline_begin<D, LPE>(pa, row0, sd, n);
    bool active = mine && n > 0;
    int reached = 0;
    for (int k = 0; __any(active && k < n); ++k) {
        active = active && k < n;
        const long long row = row0 + (k < n ? k : 0); // (a masked lane stays inside its path, see ik_polyline_kernel)
        GoalK g;
        load_goals<D>(c, a.goal, row, g);
        GdState<D> s;
        path_state<D>(sd, s);
        PIK_DESCENT(GD_LOCAL, LPE, g, sd, nullptr, s, active, p.local_max_iters, lds, lane, sub);
        path_waypoint<D>(c, p, a, g, sd, s, row, sub == 0, active, reached);
    }
    polyline_tail<LPE>(pa, row0, mine && sub == 0, n, reached);
}
#endif

// one lane per path, behind the last pass: the rows behind the stop, the relative jump test over the start and the
// held rows of every segment (the statements of cartesian_tail), reached, steps and fraction
template <int D>
__global__ __launch_bounds__(256) void polyline_finish_kernel(PolylineArgs pa) {
#pragma clang fp contract(off)
    const PathArgs& a = pa.path;
    const long long path = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (path >= a.P) return;
    const long long row0 = path * a.W;
    const double* const first = a.start + path * D;
    const double* const rows = a.solution + row0 * D;
    int reached = pa.st.held[path];
    double fraction = pa.st.frac[path];
    {
        // the last held configuration: the start when none
        const double* const last = reached == 0 ? first : rows + (long long)(reached - 1) * D;
        double sd[D];
#pragma unroll
        for (int j = 0; j < D; ++j) sd[j] = last[j];
        for (int k = pa.st.behind[path]; k < a.W; ++k) cartesian_blank_row<D>(a, row0 + k, sd);
    }
    if (pa.jump_factor > 0.0 && reached >= 1) {
        // traj[0] = the start, traj[i] = row i - 1
        double total = 0.0;
        for (int i = 0; i < reached; ++i)
            total = total + cartesian_dist<D>(i == 0 ? first : rows + (long long)(i - 1) * D, rows + (long long)i * D);
        const double thres = pa.jump_factor * (total / (double)reached);
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
    pa.steps[path] = pa.st.need[path];
    if (pa.fraction) pa.fraction[path] = fraction;
}

// the segment step of a pass: one launch, stream-ordered
template <int D>
int launch_polyline_segment(pikamd_solver* s, const ParamsK& pk, const PolylineArgs& a, hipStream_t st, int slot) {
    if (a.path.P == 0) return 0;
    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, &pk, slot, st, &kc)) return rc;
    const int block = 256;
    const long long grid = (a.path.P + block - 1) / block;
    hipLaunchKernelGGL(polyline_segment_kernel<D>, dim3((unsigned)grid), dim3(block), 0, st, kc, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the walk of a pass: one launch; the variant by path_lanes (pik_path_ops.hpp)
template <int D>
int launch_polyline_walk(pikamd_solver* s, const ParamsK& pk, const PolylineArgs& a, hipStream_t st, int slot) {
    if (a.path.P == 0) return 0;
    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, &pk, slot, st, &kc)) return rc;
    const int lpe = path_lanes(s, a.path.P, EXACT_FLAVOUR);
    const long long per_wave = WAVE / lpe;
    const dim3 g((unsigned)((a.path.P + per_wave - 1) / per_wave)), b(WAVE);
#if !defined(PIK_STRICT)
    if (lpe == 16) hipLaunchKernelGGL((ik_polyline_wide_kernel<D, 16>), g, b, 0, st, kc, a);
    else if (lpe == 8) hipLaunchKernelGGL((ik_polyline_wide_kernel<D, 8>), g, b, 0, st, kc, a);
#else
    if (lpe == 16) hipLaunchKernelGGL((ik_polyline_team_kernel<D, 16>), g, b, 0, st, kc, a);
    else if (lpe == 4) hipLaunchKernelGGL((ik_polyline_team_kernel<D, 4>), g, b, 0, st, kc, a);
#endif
    else hipLaunchKernelGGL(ik_polyline_kernel<D>, g, b, 0, st, kc, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the finish: one launch behind the last pass
template <int D>
int launch_polyline_finish(pikamd_solver* s, const ParamsK& pk, const PolylineArgs& a, hipStream_t st, int slot) {
    (void)s, (void)pk, (void)slot;
    if (a.path.P == 0) return 0;
    const int block = 256;
    const long long grid = (a.path.P + block - 1) / block;
    hipLaunchKernelGGL(polyline_finish_kernel<D>, dim3((unsigned)grid), dim3(block), 0, st, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int D>
const PolylineOps* make_polyline_ops() {
    static const PolylineOps ops = {&launch_polyline_segment<D>, &launch_polyline_walk<D>, &launch_polyline_finish<D>};
    return &ops;
}

} // namespace pik
