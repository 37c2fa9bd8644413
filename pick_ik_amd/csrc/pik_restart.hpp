// pik_restart.hpp -- memetic IK with random restarts (pikamd_search_global_batch): the launcher of a restart attempt
// and the small kernels that run between the attempts.
//
// searchPositionIK (src/pick_ik_plugin.cpp:145-291) solves, and when no solution came back draws a random valid
// configuration and solves again from there.  Attempt 0 of a call is the existing launch of pikamd_solve_batches
// (launch_solve or the routed launcher), with a batch table whose guess is the slot's guess buffer and whose outputs
// are the slot's attempt rows.  An attempt a >= 1 (launch_restart_attempt) is launch_solve's plan and pass loop (the
// shared pik_memetic_plan.hpp and MemeticCall of pik_launch.hpp, not a copy) with a
// first pass the two existing launchers never enqueue: fresh = 1 AND list_in = the problems still open, n_in = their
// device-side number.  memetic_kernel already serves that combination (it reads `prob` from list_in, its size from
// *n_in, starts from the batch's guess when `fresh`, picks its variant by sel_lo < *n_in <= sel_hi and re-arms
// *n_in when it ends); the later passes run as they do today.  The kernels are the ones pik_inst.hip compiles
// (pik_restart_inst.hip declares them `extern template`: no second copy of their code).
//
// Between the attempts restart_fold_kernel applies the loop's rule per problem -- the attempt's row goes to the
// primary outputs while the problem is open, the counters are summed, a success closes the problem -- and, for a
// problem that stays open, draws the next start (restart_draw of pik_search.hpp: the draw of pikamd_search_batch)
// and appends the problem to the next attempt's list.  restart_prepare_kernel, in front of attempt 0, tests the
// initial guess and re-draws an invalid one at epoch 0.  The order of the list cannot change a result: every random
// stream and every output row is keyed by the problem index.
#pragma once

#include "pik_launch.hpp"
#include "pik_restart_ops.hpp"
#include "pik_search.hpp"

namespace pik {

// the two fields restart_draw reads of a search call
__device__ __forceinline__ SearchArgs restart_draw_key(const RestartArgs& r) {
    SearchArgs k = {};
    k.rng_seed = r.rng_seed;
    k.problem_offset = r.problem_offset;
    return k;
}

// In front of attempt 0, one thread per problem: init[b] = the initial guess, re-drawn at epoch 0 when a bounded
// variable is outside its limits (a NaN is outside); every problem is open.
template <int D>
__global__ __launch_bounds__(WAVE) void restart_prepare_kernel(const ConstsK<D>* __restrict__ kc, RestartArgs r) {
    PIK_CONSTS(kc);
    const long long b = (long long)blockIdx.x * WAVE + threadIdx.x;
    if (b >= r.B) return;
    const SearchArgs key = restart_draw_key(r);
    double q[D], drawn[D];
    bool valid = true;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        q[j] = r.user_guess[b * D + j];
        drawn[j] = q[j];
        const bool bounded = ((c.bounded_mask >> j) & 1u) != 0;
        valid = valid && (!bounded || (q[j] <= c.qmax[j] && q[j] >= c.qmin[j]));
    }
    restart_draw<D>(c, key, b, 0u, true, drawn);
#pragma unroll
    for (int j = 0; j < D; ++j) r.guess[b * D + j] = valid ? q[j] : drawn[j];
    r.open[b] = 1;
}

// The approximate-solution gate (src/pick_ik_plugin.cpp:219-267), between attempt r.attempt and its fold when the call
// is gated, one thread per problem: a row the attempt wrote with status > 0 is evaluated under p' (r.gate_params: the
// flavour's own evaluate, the routine cost_kernel calls) and held to the joint threshold; a refused row becomes
// PIKAMD_GATE_REFUSED and the seed, its cost and counters stay, and the fold -- which is what it was -- reads the gated
// row.  A kernel of its own: the fold runs in every call, gated or not, without a stack, and the exact flavours'
// evaluation of a long chain is a call.
template <int D, bool MULTI = false>
__global__ __launch_bounds__(WAVE) void restart_gate_kernel(const ConstsK<D>* __restrict__ kc, RestartArgs r) {
    PIK_CONSTS(kc);
    const long long b = (long long)blockIdx.x * WAVE + threadIdx.x;
    if (b >= r.B) return;
    const bool ran = r.every != 0 || r.open[b] != 0;
    if (!ran || !(r.row_status[b] > 0)) return;
    typename GoalSel<MULTI>::type g;
    load_goals<D>(c, r.goal, b, g);
    double q[D], sd[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        q[j] = r.row_solution[b * D + j];
        sd[j] = r.seed[b * D + j];
    }
    EvalOut e;
    evaluate<D>(c, *(const PIK_CONSTANT ParamsK*)r.gate_params, g, sd, q, e);
    bool pass = e.sol;
    if (r.gate_joint > 0.0) {
#pragma unroll
        for (int j = 0; j < D; ++j) pass = pass && !(fabs(q[j] - sd[j]) > r.gate_joint);
    }
    if (pass) return;
    r.row_status[b] = PIKAMD_GATE_REFUSED_K;
#pragma unroll
    for (int j = 0; j < D; ++j) r.row_solution[b * D + j] = sd[j];
}

// Behind attempt r.attempt, one thread per problem, one wavefront per block.
template <int D>
__global__ __launch_bounds__(WAVE) void restart_fold_kernel(const ConstsK<D>* __restrict__ kc, RestartArgs r) {
    PIK_CONSTS(kc);
    const long long b = (long long)blockIdx.x * WAVE + threadIdx.x;
    const bool in = b < r.B;
    const long long bb = in ? b : 0;
    const bool was_open = in && r.open[bb] != 0;
    const bool ran = in && (r.every != 0 || was_open);
    const int st = ran ? r.row_status[bb] : 0;
    if (ran) {
        const long long row = bb * r.K + r.attempt;
        if (r.all_solution) {
#pragma unroll
            for (int j = 0; j < D; ++j) r.all_solution[row * D + j] = r.row_solution[bb * D + j];
        }
        if (r.all_status) r.all_status[row] = st;
    }
    if (was_open) {
#pragma unroll
        for (int j = 0; j < D; ++j) r.solution[bb * D + j] = r.row_solution[bb * D + j];
        r.status[bb] = st;
        if (r.cost) r.cost[bb] = r.row_cost[bb];
        if (r.stats) {
            StatsK sum = static_cast<const StatsK*>(r.row_stats)[bb];
            if (r.attempt > 0) {
                const StatsK before = static_cast<const StatsK*>(r.stats)[bb];
                sum.cost_evals += before.cost_evals;
                sum.generations += before.generations;
                sum.wipeouts += before.wipeouts;
                sum.pool_erasures += before.pool_erasures;
                sum.reserved += before.reserved;
            }
            static_cast<StatsK*>(r.stats)[bb] = sum;
        }
        if (r.attempts) r.attempts[bb] = r.attempt + 1;
        if (st > 0) r.open[bb] = 0;
    }
    // the next attempt's problems: the start is drawn around the start of the attempt that failed
    const bool next = !r.last && in && (r.every != 0 || (was_open && !(st > 0)));
    if (next) {
        const SearchArgs key = restart_draw_key(r);
        double q[D];
#pragma unroll
        for (int j = 0; j < D; ++j) q[j] = r.guess[bb * D + j];
        restart_draw<D>(c, key, bb, (unsigned)(r.attempt + 1), true, q);
#pragma unroll
        for (int j = 0; j < D; ++j) r.guess[bb * D + j] = q[j];
    }
    // ... and their list: a ballot, the lane's rank among the set bits, one atomic per wavefront
    const unsigned long long mask = __ballot(next);
    if (mask == 0ull) return;
    const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    unsigned base = 0u;
    if (threadIdx.x == 0) base = atomicAdd(r.n_list, (unsigned)__popcll(mask));
    base = (unsigned)__shfl((int)base, 0);
    if (next) r.list[base + rank] = (int)bb;
}

template <int D>
int launch_restart_prepare(pikamd_solver* s, const ParamsK& pk, const RestartArgs& r, hipStream_t st, int slot) {
    if (r.B == 0) return 0;
    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, &pk, slot, st, &kc)) return rc;
    hipLaunchKernelGGL(restart_prepare_kernel<D>, dim3((unsigned)((r.B + WAVE - 1) / WAVE)), dim3(WAVE), 0, st, kc, r);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int D>
int launch_restart_fold(pikamd_solver* s, const ParamsK& pk, const RestartArgs& r, hipStream_t st, int slot) {
    if (r.B == 0) return 0;
    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, &pk, slot, st, &kc)) return rc;
    hipLaunchKernelGGL(restart_fold_kernel<D>, dim3((unsigned)((r.B + WAVE - 1) / WAVE)), dim3(WAVE), 0, st, kc, r);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int D>
int launch_restart_gate(pikamd_solver* s, const ParamsK& pk, const RestartArgs& r, hipStream_t st, int slot) {
    if (r.B == 0 || !r.gate) return 0;
    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, &pk, slot, st, &kc)) return rc;
    const dim3 g((unsigned)((r.B + WAVE - 1) / WAVE)), b(WAVE);
    if (s->n_tips > 1) hipLaunchKernelGGL((restart_gate_kernel<D, true>), g, b, 0, st, kc, r);
    else hipLaunchKernelGGL(restart_gate_kernel<D>, g, b, 0, st, kc, r);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the slot's solver scratch for a call of B problems, in front of attempt 0: no attempt grows it under kernels in flight
template <int D>
int restart_reserve(pikamd_solver* s, const pikamd_params* p, const ParamsK& pk, long long B, int slot) {
    if (B == 0) return 0;
    const int S = p->memetic_num_threads > 1 ? p->memetic_num_threads : 1;
    return s->slot_state[slot].ensure(memetic_scratch<D>(s, pk, B, S).total);
}

// Attempt a >= 1: the shared plan and launches of a memetic call (pik_memetic_plan.hpp, MemeticCall of pik_launch.hpp)
// with what only a restart attempt has -- pass 0 starts from the device-side list of the open problems, a fresh start
// each; the grids are sized for the n_hint problems the host knows to be open (n_hint < 0: it does not know, B);
// the marks are the restart filter's; dirty counters are refused, because the open count in n_list[0] goes with them.
template <int D>
int launch_restart_attempt(pikamd_solver* s, const pikamd_params* p, const ParamsK& pk, BatchRecord* rec,
                           unsigned long long rng_seed_a, const int* list, long long n_hint, hipStream_t st, int slot) {
    const long long B = rec->B;
    if (B == 0 || n_hint == 0) return 0;
    if (p->mode != 0) return fail(PIKAMD_EINVAL, "restart attempts are memetic calls");
    const long long Bh = (n_hint > 0 && n_hint < B) ? n_hint : B; // problems the attempt can have
    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, &pk, slot, st, &kc)) return rc;
    SolveArgs a;
    TableSlot table; // (declared before any launch: its destructor records the event behind the last one)
    std::memset(&a, 0, sizeof a);
    a.n_batches = 1;
    a.rng_seed = rng_seed_a;
    a.B = B;
    MemeticCall<D> m(s, p, pk, st, slot, a);
    m.kc = kc;
    const bool throughput_regime = plan_throughput(s, others_busy(s, slot));
    int marks[16];
    const int n_marks = plan_marks(s, m.pl, throughput_regime, Bh, true, marks);
    const MemeticScratch lay = m.scratch(pk, B);
    if (n_marks > 0 || lay.has_unbounded) {
        if (int rc = s->slot_state[slot].ensure(lay.total)) return rc; // (restart_reserve has: nothing grows here)
    }
    if (int rc = upload_batch_table(s, rec, 1, st, &m.a.batches, &m.a.B, table)) return rc;
    m.bind(lay, n_marks > 0);
    // (a failed launch leaves the slot's counters dirty; the open count in n_list[0] goes with them, so the caller
    //  gives the call up)
    if (s->counters_dirty[slot]) return fail(PIKAMD_EHIP, "restart attempt: an earlier launch on slot %d failed", slot);
    s->counters_dirty[slot] = true;
    plan_candidates(s, m.pl, !throughput_regime || m.pl.sc.n_sched > 0, D <= 9);
    RangeTable t;
    plan_ranges(s, m.pl, throughput_regime, t);
    if (int rc = m.capacities()) return rc;
    for (int k = 0; k <= n_marks; ++k) {
        m.pass(k, marks, n_marks);
        if (k == 0) {
            m.a.list_in = list;
            m.a.n_in = m.c_nlist;
        }
        // (where the host knows the attempt's size pass 0 is one launch)
        if (int rc = m.launch_pass(t, k == 0 ? 0 : marks[k - 1], Bh, (k == 0 && n_hint > 0) ? n_hint : 0, true)) return rc;
    }
    return m.finish();
}

template <int D>
const RestartOps* make_restart_ops() {
    static const RestartOps ops = {&restart_reserve<D>, &launch_restart_prepare<D>, &launch_restart_fold<D>,
                                   &launch_restart_gate<D>, &launch_restart_attempt<D>};
    return &ops;
}

} // namespace pik
