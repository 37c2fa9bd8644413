// pik_cartesian_ops.hpp -- host side of the Cartesian-motion kernels (pik_cartesian.hpp): the arguments of a
// pikamd_cartesian_paths call and the ops table a per-length translation unit of pik_cartesian_inst.hip exports.  The
// kernel variant is the path family's choice (path_lanes, pik_path_ops.hpp), shared by the launch (launch_cartesian)
// and pikamd_cartesian_kernel_name.  No device code here; not read by pik_inst.hip.
#pragma once

#include "pik_path_ops.hpp"

namespace pik {

// one call (device pointers): see pikamd_cartesian_paths in include/pick_ik_amd.h
struct CartesianArgs {
    // the walk, as a path call sees it: goal = the interpolated poses [P][W][7] (the caller's `goals`, or the slot's
    // scratch), start, max_step and the per-waypoint outputs; reached [P] or null
    PathArgs path;
    const double* target; // [P][7]
    double* goals;        // = path.goal, for the prepare step to write
    int* steps;           // [P]: written by the prepare step, read by the walk
    double* fraction;     // [P] or null
    int frame;            // PIKAMD_CARTESIAN_*
    int min_steps;        // resolved (MoveIt's rule applied): >= 1
    double max_translation, max_rotation, jump_factor;
};

// the minimum step count of a call: MoveIt's rule where the caller gave none
inline int cartesian_min_steps(int min_steps, double jump_factor) {
    return min_steps > 0 ? min_steps : (jump_factor > 0.0 ? 10 : 1);
}

// prepare: forward kinematics of the starts and the interpolated poses, in the flavour of the handle's parity hooks
// (the bits of pikamd_fk_batch); walk: the waypoint loop and the tail, in the flavour of a path call.  Both enqueue on
// the stream and return.
struct CartesianOps {
    int (*prepare)(pikamd_solver*, const ParamsK&, const CartesianArgs&, hipStream_t, int slot);
    int (*walk)(pikamd_solver*, const ParamsK&, const CartesianArgs&, hipStream_t, int slot);
};

PIK_DECLARE_OPS_FAMILY(CartesianOps, cartesian) // cartesian_ops_d<N>(), cartesian_ops(dof)

} // namespace pik
