// pik_pathvalid.hpp -- the validity step of the path entry points (pikamd_set_path_validity): the sphere model of the
// handle cuts a path at the first waypoint whose answer it refuses, where computeCartesianPath hands its validity
// callback to setFromIK.
//
// A post-pass, not a change to the walks.  A refused waypoint only ends its path, and nothing behind it is a result,
// so "stop walking at the first refused answer" returns the bits of: walk as ever, test the held rows, cut at the
// first refused one.  The kernels here run between the existing launches; the descents, path_waypoint and the tails of
// the walk families are compiled from the text they had before this file existed.
//
// A team of T adjacent lanes owns one path (T: a power of two up to 64, chosen from W by pathvalid_team; 64 / T paths
// per wavefront).  The held rows are taken in rounds of T, ascending, one row per lane, each lane running
// validity_clear (pik_validity.hpp: pikamd_validity_batch's bits) with its centres in its own LDS column; the first
// round with a refusal ends the path's loop, and the first set bit of the team's share of the ballot is the refused
// row f.  The team's first lane then rewrites the path: row f becomes the held state (row f - 1, or the start) with
// PIKAMD_VALIDITY_REFUSED, its cost and counters stay; what lies behind it is blank.
//
//   pathvalid_paths_kernel      pikamd_solve_paths*: the cut, the blank rows, reached
//   pathvalid_motion_kernel     pikamd_cartesian_paths*: the walk ran with jump_factor 0; the cut, then cartesian_tail
//                               itself with the caller's jump_factor (blank rows, fraction, the relative test over the
//                               cut path, reached).  A path with more steps than W is left alone.
//   pathvalid_segment_kernel    pikamd_cartesian_waypoints*, behind each segment's walk: the cut over the rows the pass
//                               walked, and the pass state polyline_tail would have left for reached = f
//
// Compiled in translation units of its own (pik_pathvalid_inst.hip) with the exact flavours' flags only, as
// pik_validity_inst.hip.  Reading pik_validity.hpp and pik_polyline.hpp instantiates none of their kernels.
#pragma once

#include "pik_validity.hpp"
#include "pik_polyline.hpp"
#include "pik_pathvalid_ops.hpp"

namespace pik {

// The first refused row of `count` rows (rows[k * D + j]), or -1.  Called by all lanes of the wavefront together; a
// lane without rows passes count = 0.  sub: the lane's place in its team, first: the team's first lane, col: the
// lane's LDS column.
template <int D>
__device__ __forceinline__ int pathvalid_first(CK<D> c, VM m, const double* rows, int count, int T, int sub, int first,
                                               double* col) {
    const unsigned long long team = T >= 64 ? ~0ull : ((1ull << T) - 1ull);
    int f = -1;
    bool going = count > 0;
    for (int base = 0; __any(going); base += T) {
        const int k = base + sub;
        bool refused = false;
        if (going && k < count) {
            double qq[D];
#pragma unroll
            for (int j = 0; j < D; ++j) qq[j] = rows[(long long)k * D + j];
            double clear;
            refused = !validity_clear<D>(c, m, qq, col, VALIDITY_WAVE, clear);
        }
        const unsigned long long bits = (__ballot(refused) >> first) & team;
        if (going) {
            if (bits != 0ull) {
                f = base + (__ffsll((long long)bits) - 1);
                going = false;
            } else if (count - base <= T) {
                going = false;
            }
        }
    }
    return f;
}

// Row r of a path (r counted from the path's first row) is refused: it becomes the held state -- row r - 1, or the
// start -- with PIKAMD_VALIDITY_REFUSED; its cost and counters stay.  sd: the held state.
template <int D>
__device__ __forceinline__ void pathvalid_refuse_row(const PathArgs& a, long long path, int r, double (&sd)[D]) {
    const long long row0 = path * a.W;
    const double* const held = r == 0 ? a.start + path * D : a.solution + (row0 + r - 1) * D;
#pragma unroll
    for (int j = 0; j < D; ++j) sd[j] = held[j];
#pragma unroll
    for (int j = 0; j < D; ++j) a.solution[(row0 + r) * D + j] = sd[j];
    a.status[row0 + r] = PIKAMD_VALIDITY_REFUSED_K;
}

// the path of a lane (a lane without one runs masked on path 0's indices and reads nothing)
__device__ __forceinline__ bool pathvalid_begin(long long P, int T, long long& path, int& sub) {
    const int lane = threadIdx.x;
    sub = lane & (T - 1);
    const long long i = (long long)blockIdx.x * (VALIDITY_WAVE / T) + lane / T;
    path = i < P ? i : 0;
    return i < P;
}

template <int D>
__global__ __launch_bounds__(VALIDITY_WAVE) void pathvalid_paths_kernel(const ValidityImage<D>* __restrict__ img,
                                                                        PathArgs a, const int* reached_in, int T) {
    extern __shared__ double validity_lds[];
    PIK_VALIDITY_IMAGE(img);
    long long path;
    int sub;
    const bool mine = pathvalid_begin(a.P, T, path, sub);
    int reached = mine ? reached_in[path] : 0;
    if (reached > a.W) reached = a.W;
    const int f = pathvalid_first<D>(c, m, a.solution + path * a.W * D, reached, T, sub, (int)threadIdx.x - sub,
                                     validity_lds + threadIdx.x);
    if (f < 0 || sub != 0) return;
    double sd[D];
    pathvalid_refuse_row<D>(a, path, f, sd);
    for (int k = f + 1; k < a.W; ++k) cartesian_blank_row<D>(a, path * a.W + k, sd);
    if (a.reached) a.reached[path] = f;
}

template <int D>
__global__ __launch_bounds__(VALIDITY_WAVE) void pathvalid_motion_kernel(const ValidityImage<D>* __restrict__ img,
                                                                         CartesianArgs ca, const int* reached_in,
                                                                         int T) {
    extern __shared__ double validity_lds[];
    PIK_VALIDITY_IMAGE(img);
    const PathArgs& a = ca.path;
    long long path;
    int sub;
    const bool mine = pathvalid_begin(a.P, T, path, sub);
    const int n = mine ? ca.steps[path] : 0;
    const bool walked = mine && n <= a.W; // (more steps than rows: not walked, left alone)
    int reached = walked ? reached_in[path] : 0;
    if (reached > a.W) reached = a.W;
    const int f = pathvalid_first<D>(c, m, a.solution + path * a.W * D, reached, T, sub, (int)threadIdx.x - sub,
                                     validity_lds + threadIdx.x);
    if (!walked || sub != 0) return;
    if (f < 0 && !(ca.jump_factor > 0.0)) return; // (nothing cut, no relative test: the walk's tail stands)
    double sd[D];
    if (f >= 0) {
        pathvalid_refuse_row<D>(a, path, f, sd);
        reached = f;
    } else {
        const double* const last = reached == 0 ? a.start + path * D : a.solution + (path * a.W + reached - 1) * D;
#pragma unroll
        for (int j = 0; j < D; ++j) sd[j] = last[j];
    }
    // the walk's own tail over the cut path, now with the caller's jump_factor
    cartesian_tail<D>(ca, sd, path, true, n, reached);
}

template <int D>
__global__ __launch_bounds__(VALIDITY_WAVE) void pathvalid_segment_kernel(const ValidityImage<D>* __restrict__ img,
                                                                          PolylineArgs pa, int T) {
#pragma clang fp contract(off)
    extern __shared__ double validity_lds[];
    PIK_VALIDITY_IMAGE(img);
    const PathArgs& a = pa.path;
    long long path;
    int sub;
    const bool mine = pathvalid_begin(a.P, T, path, sub);
    // the segment this pass walked: n steps from row off0, `reached` of them held.  The walk advanced `off` only when
    // the segment was completed, and only then left the path open.
    const int n = mine ? pa.st.n[path] : 0;
    int off0 = 0, reached = 0;
    if (n > 0) {
        const int off = pa.st.off[path];
        off0 = pa.st.open[path] ? off - n : off;
        reached = pa.st.held[path] - off0;
        if (off0 < 0 || reached < 0 || off0 + reached > a.W) reached = 0; // (never: the rows stay inside the path)
    }
    const int f = pathvalid_first<D>(c, m, a.solution + (path * a.W + off0) * D, reached, T, sub,
                                     (int)threadIdx.x - sub, validity_lds + threadIdx.x);
    if (f < 0 || sub != 0) return;
    double sd[D];
    pathvalid_refuse_row<D>(a, path, off0 + f, sd);
    // what polyline_tail writes for a segment stopped at its row f
    const double sp = (double)polyline_targets(pa, path);
    pa.st.held[path] = off0 + f;
    pa.st.behind[path] = off0 + f + 1;
    pa.st.off[path] = off0;
    pa.st.open[path] = 0;
    pa.st.frac[path] = (double)pa.seg / sp + ((double)f / (double)n) / sp;
}

// the grid of a launch of P paths with teams of T lanes; 0: more than one launch holds
inline unsigned pathvalid_grid(long long P, int T) {
    const long long per_wave = VALIDITY_WAVE / T;
    const long long grid = (P + per_wave - 1) / per_wave;
    return grid > 0x7fffffffLL ? 0u : (unsigned)grid;
}

template <int D>
int launch_pathvalid_paths(const void* d_image, int n_spheres, const PathArgs& a, const int* reached_in, hipStream_t st) {
    if (a.P == 0) return 0;
    const int T = pathvalid_team(a.W);
    const unsigned grid = pathvalid_grid(a.P, T);
    if (!grid) return fail(PIKAMD_EINVAL, "pikamd_solve_paths: P = %lld is more than the validity step's launch holds", a.P);
    hipLaunchKernelGGL(pathvalid_paths_kernel<D>, dim3(grid), dim3(VALIDITY_WAVE), validity_lds_bytes(n_spheres), st,
                       static_cast<const ValidityImage<D>*>(d_image), a, reached_in, T);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int D>
int launch_pathvalid_cartesian(const void* d_image, int n_spheres, const CartesianArgs& a, const int* reached_in,
                               hipStream_t st) {
    if (a.path.P == 0) return 0;
    const int T = pathvalid_team(a.path.W);
    const unsigned grid = pathvalid_grid(a.path.P, T);
    if (!grid)
        return fail(PIKAMD_EINVAL, "pikamd_cartesian_paths: P = %lld is more than the validity step's launch holds", a.path.P);
    hipLaunchKernelGGL(pathvalid_motion_kernel<D>, dim3(grid), dim3(VALIDITY_WAVE), validity_lds_bytes(n_spheres), st,
                       static_cast<const ValidityImage<D>*>(d_image), a, reached_in, T);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int D>
int launch_pathvalid_segment(const void* d_image, int n_spheres, const PolylineArgs& a, hipStream_t st) {
    if (a.path.P == 0) return 0;
    const int T = pathvalid_team(a.path.W);
    const unsigned grid = pathvalid_grid(a.path.P, T);
    if (!grid)
        return fail(PIKAMD_EINVAL, "pikamd_cartesian_waypoints: P = %lld is more than the validity step's launch holds", a.path.P);
    hipLaunchKernelGGL(pathvalid_segment_kernel<D>, dim3(grid), dim3(VALIDITY_WAVE), validity_lds_bytes(n_spheres), st,
                       static_cast<const ValidityImage<D>*>(d_image), a, T);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int D>
const PathValidOps* make_pathvalid_ops() {
    static const PathValidOps ops = {&launch_pathvalid_paths<D>, &launch_pathvalid_cartesian<D>,
                                     &launch_pathvalid_segment<D>};
    return &ops;
}

} // namespace pik
