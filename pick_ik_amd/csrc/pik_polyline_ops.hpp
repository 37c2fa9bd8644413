// pik_polyline_ops.hpp -- host side of the waypoint-list kernels (pik_polyline.hpp): the arguments of a
// pikamd_cartesian_waypoints call, the per-path state the passes hand on, its layout in the slot's scratch and the ops
// table a per-length translation unit of pik_polyline_inst.hip exports.  The kernel variant is the path family's choice
// (path_lanes, pik_path_ops.hpp), shared by the launch (launch_polyline_walk) and
// pikamd_cartesian_waypoints_kernel_name.  No device code here; not read by pik_inst.hip.
#pragma once

#include <cstddef>

#include "pik_path_ops.hpp"

namespace pik {

// What a path carries from pass to pass ([P] each, in the slot's scratch).  off: the rows the complete segments took
// (the next segment's first row); held: the rows held so far; behind: the first row nobody solved; n: the steps of
// the segment the walk of THIS pass has to walk (0: none); need: off + the steps of the last segment started,
// saturating; open: 0 once the path has stopped; frac: the fraction so far.
struct PolylineState {
    int *off, *held, *behind, *n, *need, *open;
    double* frac;
};

constexpr size_t POLYLINE_STATE_INTS = 6;
// bytes of the state of P paths (the int arrays padded to 8 bytes together, the fractions behind them)
inline size_t polyline_state_bytes(long long P) {
    const size_t ints = (POLYLINE_STATE_INTS * (size_t)P * sizeof(int) + 7) & ~(size_t)7;
    return ints + (size_t)P * sizeof(double);
}
inline PolylineState polyline_state_at(void* base, long long P) {
    int* const i = static_cast<int*>(base);
    const size_t ints = (POLYLINE_STATE_INTS * (size_t)P * sizeof(int) + 7) & ~(size_t)7;
    return {i, i + P, i + 2 * P, i + 3 * P, i + 4 * P, i + 5 * P, reinterpret_cast<double*>(static_cast<char*>(base) + ints)};
}

// one call (device pointers): see pikamd_cartesian_waypoints in include/pick_ik_amd.h
struct PolylineArgs {
    // the walk, as a path call sees it: goal = the interpolated poses [P][W][7] (the caller's `goals`, or the slot's
    // scratch), start, max_step and the per-row outputs; reached [P] or null
    PathArgs path;
    const double* targets; // [P][S][7]
    const int* n_targets;  // [P] or null: S for every path
    double* goals;         // = path.goal, for the segment step to write
    int* steps;            // [P]
    int* segment_steps;    // [P][S] or null
    double* fraction;      // [P] or null
    PolylineState st;
    int S;         // targets per path at most
    int seg;       // the pass: the index of the segment it starts and walks
    int frame;     // PIKAMD_CARTESIAN_*
    int min_steps; // resolved: >= 1 (a waypoint list is walked with no jump test per segment: 0 gives 1)
    double max_translation, max_rotation, jump_factor;
};

// segment: forward kinematics of the state the previous segment ended in, the poses and the step count of segment
// `seg`, in the flavour of the handle's parity hooks (the bits of pikamd_fk_batch); walk: the waypoint loop of the
// segment; finish: the blank rows, the relative test, reached, steps and fraction -- both in the flavour of a path
// call.  All enqueue on the stream and return.
struct PolylineOps {
    int (*segment)(pikamd_solver*, const ParamsK&, const PolylineArgs&, hipStream_t, int slot);
    int (*walk)(pikamd_solver*, const ParamsK&, const PolylineArgs&, hipStream_t, int slot);
    int (*finish)(pikamd_solver*, const ParamsK&, const PolylineArgs&, hipStream_t, int slot);
};

PIK_DECLARE_OPS_FAMILY(PolylineOps, polyline) // polyline_ops_d<N>(), polyline_ops(dof)

} // namespace pik
