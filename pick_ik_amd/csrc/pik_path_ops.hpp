// pik_path_ops.hpp -- host side of the waypoint-path kernels (pik_path.hpp): the arguments of a path call, the
// ops table a per-length translation unit of pik_path_inst.hip exports, and the choice of kernel variant, shared by
// the launch (launch_paths) and pikamd_path_kernel_name.  No device code here; not read by pik_inst.hip.
#pragma once

#include "pik_dofs.hpp"
#include "pik_solver.hpp"

namespace pik {

// one path call (device pointers): see pikamd_solve_paths in include/pick_ik_amd.h
struct PathArgs {
    long long P;            // paths
    int W;                  // waypoints per path
    int pad_;
    const double* goal;     // [P][W][n_tips][7]
    const double* start;    // [P][D]
    const double* max_step; // [D], or null: no step limit
    double* solution;       // [P][W][D]
    int* status;            // [P][W]
    double* cost;           // [P][W] or null
    void* stats;            // [P][W] StatsK, or null
    int* reached;           // [P] or null
};

struct PathOps {
    int (*solve)(pikamd_solver*, const ParamsK&, const PathArgs&, hipStream_t, int slot);
};

PIK_DECLARE_OPS_FAMILY(PathOps, path) // path_ops_d<N>(), path_ops(dof)

// Lanes per path of a call of P paths: the rule launch_solve has for the problems of a local-mode call
// (pik_launch.hpp).  Exact flavours, one tip frame: the team kernels with 16 (or 4) lanes as long as every path gets
// its wavefront share in one round; product flavour: the cooperative descent with 16 (or 8), for one and for several
// tips.  The option lanes_per_elite forces a choice (a width the handle is not served falls to one lane).
inline int path_lanes(const pikamd_solver* s, long long P, bool exact) {
    constexpr int WAVE_LANES = 64;
    const long long simds = (long long)s->num_cu * 4;
    const bool multi = s->n_tips > 1;
    if (exact && multi) return 1;
    const int narrow = exact ? 4 : 8;
    int lpe = 0;
    if (lpe_allowed(s, 16, 1, 1, multi, exact) && P <= simds * (WAVE_LANES / 16)) lpe = 16;
    else if (lpe_allowed(s, narrow, 1, 1, multi, exact) && P <= simds * (WAVE_LANES / narrow)) lpe = narrow;
    if (s->opt.lpe > 0) {
        const int v = s->opt.lpe;
        lpe = ((v == 16 || v == narrow) && lpe_allowed(s, v, 1, 1, multi, exact)) ? v : 0;
    }
    return lpe ? lpe : 1;
}

} // namespace pik
