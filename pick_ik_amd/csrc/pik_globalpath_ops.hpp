// pik_globalpath_ops.hpp -- host side of the memetic-start path kernels (pik_globalpath.hpp): the arguments of a
// pikamd_search_global_paths call, the layout of its scratch and the ops table a per-length translation unit of
// pik_globalpath_inst.hip exports.  The variant of the tail kernel is the path family's choice (path_lanes,
// pik_path_ops.hpp), shared by the launch (launch_globalpath_tail) and pikamd_search_global_paths_kernel_name.  No
// kernel code here; not read by pik_inst.hip.
#pragma once

#include "pik_startpath_ops.hpp"

namespace pik {

// What the prepare kernel and the tail kernel get (device pointers): see pikamd_search_global_paths in
// include/pick_ik_amd.h.  The memetic attempt between them is a pikamd_solve_batches launch with ONE record, whose goal
// is goal0, whose guess is `guess` and whose outputs are the m_* rows.
struct GlobalPathArgs {
    long long P;                  // paths
    int W;                        // waypoints per path
    int K;                        // max_attempts
    int attempt;                  // tail: the attempt whose memetic solve has just finished
    int last;                     // tail: no attempt follows -- nothing is drawn, no list is built
    int g7;                       // doubles of one waypoint's goal: 7 * n_tips
    int pad_;
    const double* goal;           // [P][W][n_tips][7]
    const double* seed;           // [P][D]
    const double* user_guess;     // prepare: [P][D] the caller's initial guess (or seed)
    const double* max_step;       // [D], or null: no step limit
    unsigned long long rng_seed;  // the CALLER's seed: the key of the restart draws
    long long problem_offset;
    double* solution;             // [P][W][D]
    int* status;                  // [P][W]
    double* cost;                 // [P][W] or null
    void* stats;                  // [P][W] StatsK, or null
    int* reached;                 // [P] or null
    int* attempts;                // [P] or null
    void* totals;                 // [P] StatsK, or null
    // the slot's scratch: the rows of an attempt behind the first (null with K = 1; the costs and counters only where
    // the call has them) ...
    double* row_solution;         // [P][W][D]
    int* row_status;              // [P][W]
    double* row_cost;             // [P][W] or null
    void* row_stats;              // [P][W] StatsK, or null
    // ... the waypoint-0 goals, the starts, the row the memetic attempt writes per path, and the state of the loop
    double* goal0;                // [P][n_tips][7]
    double* guess;                // [P][D]: init[p]
    const double* m_solution;     // [P][D]
    const int* m_status;          // [P]
    const double* m_cost;         // [P]
    const void* m_stats;          // [P] StatsK
    int* best;                    // [P]: waypoints held by the kept attempt (-1: none yet)
    int* open;                    // [P]: 1 while the loop has not closed the path
    int* list;                    // [P]: the paths of the next attempt
    unsigned* n_list;             // their number (the slot's n_list[0]: zero when the tail starts)
};

// the bytes of the slot's scratch a call needs, and where its pieces lie (every piece 8-byte aligned)
struct GlobalPathScratch {
    size_t off_row_stats, off_row_cost, off_row_solution, off_row_status;
    size_t off_goal0, off_guess, off_m_solution, off_m_cost, off_m_stats, off_m_status, off_best, off_open, off_list, total;
};
inline GlobalPathScratch globalpath_scratch(long long P, int W, int K, int dof, int g7, bool cost, bool stats) {
    auto ints = [](size_t n) { return (sizeof(int) * n + 7) & ~(size_t)7; };
    const size_t n = (size_t)P, rows = K > 1 ? n * (size_t)W : 0, d = (size_t)dof;
    GlobalPathScratch l;
    l.off_row_stats = 0;
    l.off_row_cost = l.off_row_stats + (stats ? sizeof(pikamd_stats) * rows : 0);
    l.off_row_solution = l.off_row_cost + (cost ? sizeof(double) * rows : 0);
    l.off_row_status = l.off_row_solution + sizeof(double) * d * rows;
    l.off_goal0 = l.off_row_status + ints(rows);
    l.off_guess = l.off_goal0 + sizeof(double) * (size_t)g7 * n;
    l.off_m_solution = l.off_guess + sizeof(double) * d * n;
    l.off_m_cost = l.off_m_solution + sizeof(double) * d * n;
    l.off_m_stats = l.off_m_cost + sizeof(double) * n;
    l.off_m_status = l.off_m_stats + sizeof(pikamd_stats) * n;
    l.off_best = l.off_m_status + ints(n);
    l.off_open = l.off_best + ints(n);
    l.off_list = l.off_open + ints(n);
    l.total = l.off_list + ints(n);
    return l;
}

struct GlobalPathOps {
    // in front of attempt 0: the waypoint-0 goals gathered, init[p], every path open
    int (*prepare)(pikamd_solver*, const ParamsK&, const GlobalPathArgs&, hipStream_t, int slot);
    // behind the memetic solve of attempt a.attempt: the waypoints behind the first, the keep rule, the sums, the next
    // attempt's starts and list
    int (*tail)(pikamd_solver*, const ParamsK&, const GlobalPathArgs&, hipStream_t, int slot);
};

PIK_DECLARE_OPS_FAMILY(GlobalPathOps, globalpath) // globalpath_ops_d<N>(), globalpath_ops(dof)

} // namespace pik
