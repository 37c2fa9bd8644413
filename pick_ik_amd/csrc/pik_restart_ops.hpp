// pik_restart_ops.hpp -- host side of the restart launcher (pik_restart.hpp, pikamd_search_global_batch): the
// arguments of its two small kernels and the ops table a per-length translation unit of pik_restart_inst.hip exports.
// No device code here; not read by pik_inst.hip.
#pragma once

#include "pik_search_ops.hpp"

namespace pik {

// What restart_prepare_kernel and restart_fold_kernel get (device pointers).  The slot's scratch holds the guess
// buffer, the rows of ONE attempt -- what the attempt's batch table points its outputs at --, the open flags and the
// list of the problems the next attempt solves.
struct RestartArgs {
    long long B;                  // problems
    int K;                        // max_attempts
    int attempt;                  // the attempt that has just finished (fold)
    int every;                    // all_* wanted: every attempt of every problem runs, no early exit
    int last;                     // fold: no attempt follows -- nothing is drawn, no list is built
    const double* user_guess;     // prepare: [B][D] the caller's initial guess (or seed)
    double* guess;                // [B][D] scratch: init[b]
    unsigned long long rng_seed;  // the CALLER's seed: the key of the restart draws
    long long problem_offset;
    double* row_solution;         // [B][D] the finished attempt's outputs (restart_gate_kernel rewrites a refused row)
    int* row_status;              // [B]
    const double* row_cost;       // [B]
    const void* row_stats;        // [B] StatsK
    double* solution;             // [B][D] primary outputs
    int* status;                  // [B]
    double* cost;                 // [B] or null
    void* stats;                  // [B] StatsK, or null
    int* attempts;                // [B] or null
    double* all_solution;         // [B][K][D] or null
    int* all_status;              // [B][K] or null
    int* open;                    // [B] scratch: 1 while the loop has not closed the problem
    int* list;                    // [B] scratch: the problems of the next attempt
    unsigned* n_list;             // their number (the slot's n_list[0]: zero when the fold starts)
    // the approximate-solution gate (restart_gate_kernel, in front of the fold): SearchArgs has the same three fields
    const double* goal;           // [B][n_tips][7]
    const double* seed;           // [B][D]
    int gate;                     // 0: no gate, the gate kernel is not launched
    double gate_joint;
    const ParamsK* gate_params;
};

struct RestartOps {
    // the slot's solver scratch for a call of B problems, in front of attempt 0 (so that no attempt grows it while
    // kernels of an earlier one use it)
    int (*reserve)(pikamd_solver*, const pikamd_params*, const ParamsK&, long long B, int slot);
    int (*prepare)(pikamd_solver*, const ParamsK&, const RestartArgs&, hipStream_t, int slot);
    int (*fold)(pikamd_solver*, const ParamsK&, const RestartArgs&, hipStream_t, int slot);
    // between an attempt and its fold when the call is gated (r.gate): the attempt's rows through the gate
    int (*gate)(pikamd_solver*, const ParamsK&, const RestartArgs&, hipStream_t, int slot);
    // one attempt a >= 1: the pass loop over the problems of `list` (device memory, their number in the slot's
    // n_list[0]); `rec`: ONE record of B problems (host copy, device pointers); n_hint: the number of listed
    // problems where the host knows it (sizes grids, changes no result), else < 0
    int (*attempt)(pikamd_solver*, const pikamd_params*, const ParamsK&, BatchRecord* rec, unsigned long long rng_seed_a,
                   const int* list, long long n_hint, hipStream_t, int slot);
};

PIK_DECLARE_OPS_FAMILY(RestartOps, restart) // restart_ops_d<N>(), restart_ops(dof)

// rng_seed_a of the header: attempt a's seed is the caller's with a added to its HIGH word (mod 2^64)
inline unsigned long long restart_attempt_seed(unsigned long long rng_seed, int a) {
    return rng_seed + ((unsigned long long)(unsigned)a << 32);
}

} // namespace pik
