// pik_restart.hpp -- memetic IK with random restarts (pikamd_search_global_batch): the launcher of a restart attempt
// and the small kernels that run between the attempts.
//
// searchPositionIK (src/pick_ik_plugin.cpp:145-291) solves, and when no solution came back draws a random valid
// configuration and solves again from there.  Attempt 0 of a call is the existing launch of pikamd_solve_batches
// (launch_solve or the routed launcher), with a batch table whose guess is the slot's guess buffer and whose outputs
// are the slot's attempt rows.  An attempt a >= 1 (launch_restart_attempt) is launch_solve's pass loop again with a
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

// launch_solve's per-slot scratch for a memetic call of B problems
template <int D>
struct RestartScratch {
    size_t off_d, off_l, off_i, off_list, off_pop, pop_stride, total;
    bool has_unbounded;
    RestartScratch(const pikamd_solver* s, const ParamsK& pk, long long B, int S) {
        const size_t recs = (size_t)B * (size_t)S;
        const size_t d_rows = (size_t)StateRows<D>::D_ROWS(pk.elites);
        off_d = 0;
        off_l = off_d + sizeof(double) * d_rows * recs;
        off_i = off_l + sizeof(long long) * StateRows<D>::L_ROWS * recs;
        off_list = off_i + sizeof(int) * StateRows<D>::I_ROWS * recs;
        const size_t off_cnt = off_list + sizeof(int) * 2 * (size_t)B;
        has_unbounded = s->chain.bounded_mask != ((1u << s->chain.dof) - 1u);
        pop_stride = (size_t)pk.population * (1 + D) + ((size_t)pk.population + 1) / 2;
        off_pop = (off_cnt + 64 + 63) / 64 * 64;
        total = off_pop + (has_unbounded ? sizeof(double) * 2 * pop_stride * (size_t)B * (size_t)S : 0);
    }
};

template <int D>
int restart_reserve(pikamd_solver* s, const pikamd_params* p, const ParamsK& pk, long long B, int slot) {
    if (B == 0) return 0;
    const int S = p->memetic_num_threads > 1 ? p->memetic_num_threads : 1;
    const RestartScratch<D> sc(s, pk, B, S);
    return s->slot_state[slot].ensure(sc.total);
}

// The passes of a restart attempt when the option "passes" is not set: two of launch_solve's default marks.  The
// problems of a restart attempt are the few a whole solve has failed on; what a pass re-packs is the tail of a tail,
// and every mark costs an empty dispatch per candidate variant when nothing is left.  (Scheduling: no result
// depends on the marks.)
inline bool restart_default_mark(int generation) { return generation == 8 || generation == 32; }

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
    a.gs_log2 = pow2ceil_log2(pk.elites);
    const int gs = 1 << a.gs_log2;
    const int S = p->memetic_num_threads > 1 ? p->memetic_num_threads : 1;
    a.species = S;
    a.sp_log2 = pow2ceil_log2(S);
    const bool multi = s->n_tips > 1;
    Schedule sc;
    make_schedule(s, pk, gs, S, sc);
    // the regime: launch_solve's rule
    bool throughput_regime = false;
    {
        int others = 0;
        for (int k = 0; k < N_DEVICE_SLOTS + N_HOST_JOBS; ++k)
            if (k != slot && s->slot_event_used[k] && hipEventQuery(s->slot_event[k]) == hipErrorNotReady) ++others;
        (void)hipGetLastError(); // (hipErrorNotReady is an answer, not a failure)
        throughput_regime = others >= 3;
        if (s->opt.regime != 0) throughput_regime = s->opt.regime == 2;
    }
    if (!throughput_regime && s->opt.two_per_simd < 2 && !s->opt.force_occ2) sc.occ2_from = (long long)s->num_cu * 4 * 9 / 8;
    int marks[16], n_marks = 0;
    for (int i = 0; i < sc.n_marks; ++i)
        if (s->opt.passes_set || restart_default_mark(sc.marks[i])) marks[n_marks++] = sc.marks[i];
    if (!throughput_regime && sc.n_sched == 0 && !s->opt.passes_set) {
        int widest = 1;
        for (int l : {16, 8, 4, 2})
            if (widest == 1 && lpe_allowed(s, l, gs, S, multi)) widest = l;
        if (widest > 1 && Bh <= (long long)s->num_cu * 4 * (WAVE / (gs * widest * (1 << a.sp_log2)))) n_marks = 0;
    }
    const RestartScratch<D> lay(s, pk, B, S);
    if (n_marks > 0 || lay.has_unbounded) {
        if (int rc = s->slot_state[slot].ensure(lay.total)) return rc; // (restart_reserve has: nothing grows here)
    }
    if (int rc = upload_batch_table(s, rec, 1, st, &a.batches, &a.B, table)) return rc;
    char* base = (char*)s->slot_state[slot].p;
    a.pop = lay.has_unbounded ? (double*)(base + lay.off_pop) : nullptr;
    a.pop_stride = (long long)lay.pop_stride;
    a.cap = B;
    a.st_d = n_marks ? (double*)(base + lay.off_d) : nullptr;
    a.st_l = n_marks ? (long long*)(base + lay.off_l) : nullptr;
    a.st_i = n_marks ? (int*)(base + lay.off_i) : nullptr;
    int* lists[2] = {n_marks ? (int*)(base + lay.off_list) : nullptr, n_marks ? (int*)(base + lay.off_list) + B : nullptr};
    unsigned char* cblk = s->counters + COUNTER_BLOCK * (size_t)slot;
    unsigned long long* c_work = (unsigned long long*)cblk;
    unsigned* c_nlist = (unsigned*)(cblk + 128);
    unsigned* c_done = (unsigned*)(cblk + 256);
    // (a failed launch leaves the slot's counters dirty; the open count in n_list[0] goes with them, so the caller
    //  gives the call up)
    if (s->counters_dirty[slot]) return fail(PIKAMD_EHIP, "restart attempt: an earlier launch on slot %d failed", slot);
    s->counters_dirty[slot] = true;

    auto capacity_of = [&](auto kernel, int variant, long long* cap_out) -> int {
        int per_cu = s->occupancy_cache[PIK_OCC_ROW][variant];
        if (per_cu == 0) {
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, WAVE, 0));
            if (per_cu < 1) per_cu = 1;
            s->occupancy_cache[PIK_OCC_ROW][variant] = per_cu;
        }
        *cap_out = (long long)s->num_cu * per_cu;
        return 0;
    };
    struct Variant {
        int lpe, id;
        long long capacity; // wavefronts the chip holds of it
        long long hi;       // largest problem count it is chosen for (adaptive schedule)
    };
    Variant var[8];
    int n_var = 0;
    auto add_variant = [&](auto kernel, int lpe_, int id) -> int {
        Variant v{lpe_, id, 0, 0};
        if (int rc = capacity_of(kernel, id, &v.capacity)) return rc;
        var[n_var++] = v;
        return 0;
    };
    auto launch_variant = [&](const Variant& v, unsigned lo, unsigned hi) -> int {
        const long long groups_per_wave = WAVE / (gs * v.lpe * (1 << a.sp_log2));
        const long long waves_needed = (Bh + groups_per_wave - 1) / groups_per_wave;
        const long long grid = waves_needed < v.capacity ? waves_needed : v.capacity;
        a.sel_lo = lo;
        a.sel_hi = hi;
        const dim3 g((unsigned)grid), b(WAVE);
        switch (v.id) {
            case 5: hipLaunchKernelGGL((memetic_kernel<D, 16>), g, b, 0, st, kc, a); break;
            case 4: hipLaunchKernelGGL((memetic_kernel<D, 8>), g, b, 0, st, kc, a); break;
            case 3: hipLaunchKernelGGL((memetic_kernel<D, 4>), g, b, 0, st, kc, a); break;
            case 2: hipLaunchKernelGGL((memetic_kernel<D, 2>), g, b, 0, st, kc, a); break;
            case 7:
                if constexpr (D <= 9) hipLaunchKernelGGL((memetic_kernel<D, 1, false, 2>), g, b, 0, st, kc, a);
                break;
#if !defined(PIK_STRICT)
            case 10: hipLaunchKernelGGL((memetic_kernel<D, 16, true>), g, b, 0, st, kc, a); break;
            case 9: hipLaunchKernelGGL((memetic_kernel<D, 8, true>), g, b, 0, st, kc, a); break;
#endif
            case 8: hipLaunchKernelGGL((memetic_kernel<D, 2, true>), g, b, 0, st, kc, a); break;
            case 6: hipLaunchKernelGGL((memetic_kernel<D, 1, true>), g, b, 0, st, kc, a); break;
            default: hipLaunchKernelGGL((memetic_kernel<D, 1>), g, b, 0, st, kc, a); break;
        }
        HIP_TRY(hipGetLastError());
        return 0;
    };
    // launch_solve's candidates and range table
    const long long occ2_from_problems = sc.occ2_from * WAVE / gs;
    const bool wide_ok = !throughput_regime || sc.n_sched > 0;
    if (multi) {
#if !defined(PIK_STRICT)
        if (wide_ok && lpe_allowed(s, 16, gs, S, multi))
            if (int rc = add_variant(memetic_kernel<D, 16, true>, 16, 10)) return rc;
        if (wide_ok && lpe_allowed(s, 8, gs, S, multi))
            if (int rc = add_variant(memetic_kernel<D, 8, true>, 8, 9)) return rc;
#endif
        if (wide_ok && lpe_allowed(s, 2, gs, S, multi))
            if (int rc = add_variant(memetic_kernel<D, 2, true>, 2, 8)) return rc;
        if (int rc = add_variant(memetic_kernel<D, 1, true>, 1, 6)) return rc;
    } else {
        if (wide_ok && lpe_allowed(s, 16, gs, S, multi))
            if (int rc = add_variant(memetic_kernel<D, 16>, 16, 5)) return rc;
        if (wide_ok && lpe_allowed(s, 8, gs, S, multi))
            if (int rc = add_variant(memetic_kernel<D, 8>, 8, 4)) return rc;
        if (wide_ok && lpe_allowed(s, 4, gs, S, multi))
            if (int rc = add_variant(memetic_kernel<D, 4>, 4, 3)) return rc;
        if (wide_ok && lpe_allowed(s, 2, gs, S, multi))
            if (int rc = add_variant(memetic_kernel<D, 2>, 2, 2)) return rc;
        if (int rc = add_variant(memetic_kernel<D, 1>, 1, 1)) return rc;
        if constexpr (D <= 9) {
            bool occ2 = sc.occ2_ok && !(disabled_lanes_of(s, EXACT_FLAVOUR) & 1u);
#if defined(PIK_STRICT)
            occ2 = occ2 && s->chain.float_mask == 0u && s->chain.n_mimic == 0;
#endif
            if (occ2)
                if (int rc = add_variant(memetic_kernel<D, 1, false, 2>, 1, 7)) return rc;
        }
    }
    for (int i = 0; i < n_var; ++i) {
        const long long per_wave = WAVE / (gs * var[i].lpe * (1 << a.sp_log2));
        var[i].hi = (var[i].lpe > 1) ? (long long)s->num_cu * 4 * per_wave // one wavefront per SIMD
                    : (var[i].id == 7 || i == n_var - 1) ? 0xffffffffll
                                                         : occ2_from_problems - 1;
    }
    for (int k = 0; k <= n_marks; ++k) {
        // every pass starts from a device-side list: pass 0 from the open problems, a fresh start each
        a.fresh = (k == 0);
        a.pause_gen = (k < n_marks) ? marks[k] : 0x7fffffff;
        a.list_in = (k == 0) ? list : lists[(k - 1) & 1];
        a.n_in = c_nlist + k;
        a.list_out = n_marks ? lists[k & 1] : nullptr;
        a.n_out = n_marks ? c_nlist + (k + 1) : nullptr;
        a.work_counter = c_work + k;
        a.done = c_done + k;
        const int start_gen = (k == 0) ? 0 : marks[k - 1];
        if (sc.n_sched > 0) {
            // forced lanes per elite
            int lpe_k = sc.lpe_of[0];
            for (int i = 1; i < sc.n_sched; ++i)
                if (start_gen >= sc.lpe_from[i]) lpe_k = sc.lpe_of[i];
            int pick = -1;
            for (int i = 0; i < n_var && pick < 0; ++i)
                if (var[i].lpe == lpe_k) pick = i;
            if (pick < 0) pick = n_var - 1;
            if (var[pick].lpe == 1 && var[n_var - 1].id == 7 && Bh >= occ2_from_problems) pick = n_var - 1;
            if (int rc = launch_variant(var[pick], 0u, 0xffffffffu)) return rc;
            continue;
        }
        // adaptive: variant i serves problem counts in (hi of the next wider one, its own hi]; a pass cannot have
        // more problems than the attempt, and where the host knows the attempt's size pass 0 is one launch
        long long lo = 0;
        for (int i = 0; i < n_var; ++i) {
            const long long hi = var[i].hi < lo ? lo : var[i].hi;
            const bool reachable = Bh > lo && hi > lo;
            const bool exact_size = k == 0 && n_hint > 0;
            if (reachable && (!exact_size || n_hint <= hi))
                if (int rc = launch_variant(var[i], (unsigned)lo, (unsigned)(hi > 0xffffffffll ? 0xffffffffll : hi))) return rc;
            lo = hi;
        }
    }
    s->counters_dirty[slot] = false;
    if (!s->slot_event[slot]) HIP_TRY(hipEventCreateWithFlags(&s->slot_event[slot], hipEventDisableTiming));
    HIP_TRY(hipEventRecord(s->slot_event[slot], st));
    s->slot_event_used[slot] = true;
    return 0;
}

template <int D>
const RestartOps* make_restart_ops() {
    static const RestartOps ops = {&restart_reserve<D>, &launch_restart_prepare<D>, &launch_restart_fold<D>,
                                   &launch_restart_gate<D>, &launch_restart_attempt<D>};
    return &ops;
}

} // namespace pik
