// pik_search_ops.hpp -- host side of the restart-search kernels (pik_search.hpp): the arguments of a search call, the
// ops table a per-length translation unit of pik_search_inst.hip exports, and the choice of schedule and kernel
// variant, shared by the launch (launch_search) and pikamd_search_kernel_name.  No device code here; not read by
// pik_inst.hip.
#pragma once

#include "pik_path_ops.hpp"

namespace pik {

constexpr int SEARCH_MAX_ATTEMPTS = PIKAMD_MAX_ATTEMPTS;

// one search call (device pointers): see pikamd_search_batch in include/pick_ik_amd.h
struct SearchArgs {
    long long B;                  // problems
    int K;                        // max_attempts
    int parallel;                 // 0: one unit per problem walks its attempts; 1: one unit per (problem, attempt)
    int every;                    // all_* wanted: every attempt is run and recorded, no early exit
    int lanes;                    // lanes per unit (search_plan)
    const double* goal;           // [B][n_tips][7]
    const double* seed;           // [B][D]
    const double* guess;          // [B][D] (the host passes seed when the caller gave none)
    unsigned long long rng_seed;
    long long problem_offset;
    double* solution;             // [B][D]
    int* status;                  // [B]
    double* cost;                 // [B] or null
    void* stats;                  // [B] StatsK, or null
    int* attempts;                // [B] or null
    // one row per attempt: the caller's all_* arrays where given; in the parallel schedule the slot's scratch
    // otherwise, and always for the costs and counters (what search_finalize_kernel reads)
    double* row_solution;         // [B][K][D] or null (sequential schedule without all_solution)
    int* row_status;              // [B][K] or null
    double* row_cost;             // [B][K], parallel schedule only
    void* row_stats;              // [B][K] StatsK, parallel schedule only
    // The approximate-solution gate of the handle (pikamd_set_approximate_gate), applied behind every attempt.  The
    // host sets `gate` only for a call with return_approximate_solution.  gate_params: the parameters p' of
    // pikamd_gate_batch in device memory -- the evaluation reads its parameters through the constant address space,
    // where a kernel cannot make a copy; they are not in ConstsK, which every other kernel reads.
    int gate;                     // 0: no gate (the fields below are not read)
    double gate_joint;            // approximate_solution_joint_threshold (not > 0: no limit)
    const ParamsK* gate_params;
    // The sphere validity model of the handle (pikamd_set_validity_model), applied behind the gate: the device image
    // of pik_validity_ops.hpp, or null -- no model, and always null in a call of the path-from-pose families.  Read by
    // the exact flavours' kernels only (the host refuses a model on a call the fast kernels serve).
    const void* validity;
};

// p' of pikamd_gate_batch, from the call's converted parameters: the gate's cost threshold in place of the call's when
// it is > 0, else no joint goal (src/pick_ik_plugin.cpp:240-242: no goal is tested; the frame tests stay)
inline ParamsK gate_params_k(const ParamsK& pk, double cost_threshold) {
#pragma clang fp contract(off)
    ParamsK g = pk;
    if (cost_threshold > 0.0) {
        g.cost_thr_sq = cost_threshold * cost_threshold;
    } else {
        g.goal_mask = 0;
        g.w_center_sq = g.w_limits_sq = g.w_disp_sq = 0.0;
    }
    return g;
}

struct SearchOps {
    int (*solve)(pikamd_solver*, const ParamsK&, const SearchArgs&, hipStream_t, int slot);
};

PIK_DECLARE_OPS_FAMILY(SearchOps, search) // search_ops_d<N>(), search_ops(dof)

// option search_schedule
constexpr int SEARCH_ADAPTIVE = 0, SEARCH_SEQUENTIAL = 1, SEARCH_PARALLEL = 2;

// How a call of B problems with K attempts runs: the schedule and the lanes per unit.  A unit is (problem, first
// attempt, number of attempts): one per problem in the sequential schedule, K per problem in the parallel one; its
// width is what path_lanes gives that many units (the rule launch_solve has for the problems of a local-mode call).
// Adaptive: parallel while all B * K units at their width fit the chip in one round (num_cu * 4 wavefronts) -- a
// plugin-style query with 16 attempts then costs about one descent --, else sequential: a lane or team leaves its
// problem at the first success, and the throughput is that of the descents actually needed.
struct SearchPlan {
    bool parallel;
    int lanes;
    long long units;
};
inline SearchPlan search_plan(const pikamd_solver* s, int schedule, long long B, int K, bool exact) {
    constexpr int WAVE_LANES = 64;
    const long long simds = (long long)s->num_cu * 4;
    const long long all = B * (long long)K;
    const int wide = path_lanes(s, all, exact);
    bool parallel = all <= simds * (WAVE_LANES / wide);
    if (schedule == SEARCH_SEQUENTIAL) parallel = false;
    if (schedule == SEARCH_PARALLEL) parallel = true;
    if (K == 1) parallel = false; // (one attempt: the same work either way, and nothing to finalize)
    if (parallel) return {true, wide, all};
    return {false, path_lanes(s, B, exact), B};
}

} // namespace pik
