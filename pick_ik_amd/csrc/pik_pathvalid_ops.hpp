// pik_pathvalid_ops.hpp -- host side of the validity step of the path entry points (pik_pathvalid.hpp,
// pikamd_set_path_validity): the choice of the team width and the ops table a per-length translation unit of
// pik_pathvalid_inst.hip exports.  No device code here; not read by pik_inst.hip.
#pragma once

#include "pik_cartesian_ops.hpp"
#include "pik_polyline_ops.hpp"

namespace pik {

// Lanes per path of the step: the power of two that holds the W rows of a path in one round, 64 at the most (a longer
// path takes ceil(W / 64) rounds).
inline int pathvalid_team(int W) {
    int t = 1;
    while (t < W && t < 64) t *= 2;
    return t;
}

// All three enqueue one kernel on the stream and return.  d_image: the handle's model image (ValidityImage, the exact
// flavour's layout); the arguments are the walk's, with the caller's outputs.
struct PathValidOps {
    // behind the walk of pikamd_solve_paths*; reached_in [P]: what the walk stored (the caller's array, or scratch)
    int (*paths)(const void* d_image, int n_spheres, const PathArgs&, const int* reached_in, hipStream_t);
    // behind the walk of pikamd_cartesian_paths*, which ran with jump_factor 0; the arguments carry the caller's
    int (*cartesian)(const void* d_image, int n_spheres, const CartesianArgs&, const int* reached_in, hipStream_t);
    // behind the walk of segment a.seg of pikamd_cartesian_waypoints*, in front of the next segment kernel
    int (*segment)(const void* d_image, int n_spheres, const PolylineArgs&, hipStream_t);
};

PIK_DECLARE_OPS_FAMILY(PathValidOps, pathvalid) // pathvalid_ops_d<N>(), pathvalid_ops(dof)

} // namespace pik
