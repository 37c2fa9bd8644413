// pik_startpath_ops.hpp -- host side of the start-search path kernels (pik_startpath.hpp): the arguments of a
// pikamd_search_paths call and the ops table a per-length translation unit of pik_startpath_inst.hip exports.  The
// kernel variant is the path family's choice (path_lanes, pik_path_ops.hpp), shared by the launch
// (launch_startpaths) and pikamd_search_paths_kernel_name.  No device code here; not read by pik_inst.hip.
#pragma once

#include "pik_search_ops.hpp"

namespace pik {

// one call (device pointers): see pikamd_search_paths in include/pick_ik_amd.h
struct StartPathArgs {
    long long P;                  // paths
    int W;                        // waypoints per path
    int K;                        // max_attempts
    const double* goal;           // [P][W][n_tips][7]
    const double* seed;           // [P][D]
    const double* guess;          // [P][D] (the host passes seed when the caller gave none)
    const double* max_step;       // [D], or null: no step limit
    unsigned long long rng_seed;
    long long problem_offset;
    double* solution;             // [P][W][D]
    int* status;                  // [P][W]
    double* cost;                 // [P][W] or null
    void* stats;                  // [P][W] StatsK, or null
    int* reached;                 // [P] or null
    int* attempts;                // [P] or null
    void* totals;                 // [P] StatsK, or null
    // the rows of an attempt behind the first, in the slot's scratch: copied over the outputs when the attempt holds
    // more waypoints than every one before it (null with K = 1; the costs and counters only where the call has them)
    double* row_solution;         // [P][W][D]
    int* row_status;              // [P][W]
    double* row_cost;             // [P][W] or null
    void* row_stats;              // [P][W] StatsK, or null
};

// the bytes of the slot's scratch a call needs, and where its pieces lie: stats | cost | solution | status
struct StartPathScratch {
    size_t off_stats, off_cost, off_solution, off_status, total;
};
inline StartPathScratch startpath_scratch(long long P, int W, int K, int dof, bool cost, bool stats) {
    StartPathScratch l = {0, 0, 0, 0, 0};
    if (K <= 1) return l;
    const size_t rows = (size_t)P * (size_t)W;
    l.off_cost = l.off_stats + (stats ? sizeof(pikamd_stats) * rows : 0);
    l.off_solution = l.off_cost + (cost ? sizeof(double) * rows : 0);
    l.off_status = l.off_solution + sizeof(double) * (size_t)dof * rows;
    l.total = l.off_status + ((sizeof(int) * rows + 7) & ~(size_t)7);
    return l;
}

struct StartPathOps {
    int (*solve)(pikamd_solver*, const ParamsK&, const StartPathArgs&, hipStream_t, int slot);
};

PIK_DECLARE_OPS_FAMILY(StartPathOps, startpath) // startpath_ops_d<N>(), startpath_ops(dof)

} // namespace pik
