// pik_launch.hpp -- kernel launches for one chain length D (templates; instantiated by pik_inst.hip
// once per D so that the per-DOF kernels compile in parallel translation units).
#pragma once

#include <new>

#include "pik_kernels.hpp"
#include "pik_solver.hpp"
#include "pik_memetic_plan.hpp"

namespace pik {

static_assert(sizeof(StatsK) == sizeof(pikamd_stats), "stats layout");
static_assert(sizeof(BatchRecord) == sizeof(BatchK), "batch record layout");
static_assert(offsetof(BatchRecord, completed) == offsetof(BatchK, completed), "batch record layout");

// Makes the slot's device constants buffer hold this call's chain + params.  The upload is
// skipped when the slot already holds the same bytes (the common case: same robot, same params
// every call), so steady-state launches cost one table copy + the kernels.  When the contents
// change, the slot's previous stream is drained first so no in-flight kernel can observe the rewrite.
template <int D>
int upload_consts(pikamd_solver* s, const ParamsK* pk, int slot, hipStream_t st, const ConstsK<D>** out) {
    static_assert(sizeof(ConstsK<D>) <= CONSTS_STRIDE, "constants slot too small");
    static_assert(MAX_TIPS == PIKAMD_MAX_TIPS, "tip limit");
    // staging copy: per handle (handles are used from one thread at a time, different handles may
    // be used concurrently)
    ConstsK<D>& want = *reinterpret_cast<ConstsK<D>*>(s->consts_tmp);
    // only the chains in use are compared / uploaded
    const size_t used = offsetof(ConstsK<D>, more) + sizeof(ChainK<D>) * (size_t)(s->n_tips - 1);
    std::memset(&want, 0, used);
    want.chain = make_chain_k<D>(s->chain);
    for (int k = 1; k < s->n_tips; ++k) want.more[k - 1] = make_chain_k<D>(s->more[k - 1]);
    want.n_tips = s->n_tips;
    if (pk) want.params = *pk;
    char* host = s->consts_host + (size_t)slot * CONSTS_STRIDE;
    char* dev = s->consts_dev + (size_t)slot * CONSTS_STRIDE;
    if (!s->consts_valid[slot] || std::memcmp(host, &want, used) != 0) {
        if (s->consts_valid[slot]) HIP_TRY(hipStreamSynchronize(s->consts_stream[slot]));
        s->consts_valid[slot] = false;
        std::memcpy(host, &want, used);
        HIP_TRY(hipMemcpyAsync(dev, host, used, hipMemcpyHostToDevice, st));
        // later calls on OTHER streams may reuse these bytes without copying: make them visible
        HIP_TRY(hipStreamSynchronize(st));
        s->consts_valid[slot] = true;
    }
    s->consts_stream[slot] = st;
    *out = reinterpret_cast<const ConstsK<D>*>(dev);
    return 0;
}

template <int D>
int launch_fk(pikamd_solver* s, long long n, const double* d_q, double* d_out, hipStream_t st) {
    if (n == 0) return 0;
    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, nullptr, SLOT_HOOKS, st, &kc)) return rc;
    const int block = 256;
    const long long grid = (n + block - 1) / block;
    if (s->n_tips > 1)
        hipLaunchKernelGGL((fk_kernel<D, true>), dim3((unsigned)grid), dim3(block), 0, st, kc, n, d_q, d_out);
    else
        hipLaunchKernelGGL(fk_kernel<D>, dim3((unsigned)grid), dim3(block), 0, st, kc, n, d_q, d_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int D>
int launch_cost(pikamd_solver* s, const ParamsK& pk, long long n, const double* d_goal, const double* d_seed,
                const double* d_q, double* d_cost, int* d_sol, hipStream_t st) {
    if (n == 0) return 0;
    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, &pk, SLOT_HOOKS, st, &kc)) return rc;
    const int block = 64;
    const long long grid = (n + block - 1) / block;
    if (s->n_tips > 1)
        hipLaunchKernelGGL((cost_kernel<D, true>), dim3((unsigned)grid), dim3(block), 0, st, kc, n, d_goal,
                           d_seed, d_q, d_cost, d_sol);
    else
        hipLaunchKernelGGL(cost_kernel<D>, dim3((unsigned)grid), dim3(block), 0, st, kc, n, d_goal, d_seed, d_q,
                           d_cost, d_sol);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int D>
int launch_step(pikamd_solver* s, const ParamsK& pk, long long n, const double* d_goal, const double* d_seed,
                double* d_local, double* d_best, double* d_lc, double* d_bc, double* d_grad, int* d_imp,
                hipStream_t st) {
    if (n == 0) return 0;
    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, &pk, SLOT_HOOKS, st, &kc)) return rc;
    const int block = 64;
    const long long grid = (n + block - 1) / block;
    if (s->n_tips > 1)
        hipLaunchKernelGGL((gd_step_kernel<D, true>), dim3((unsigned)grid), dim3(block), 0, st, kc, n, d_goal,
                           d_seed, d_local, d_best, d_lc, d_bc, d_grad, d_imp);
    else
        hipLaunchKernelGGL(gd_step_kernel<D>, dim3((unsigned)grid), dim3(block), 0, st, kc, n, d_goal, d_seed,
                           d_local, d_best, d_lc, d_bc, d_grad, d_imp);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The call's batch table goes to the device through a ring of table slots.  The kernels of the call
// read their table whenever a problem starts, resumes or finishes (find_batch), so a slot may only be
// rewritten once the LAST kernel of the call that used it has run: TableSlot records the slot's event
// when launch_solve returns -- behind every launch of the call, on whichever path it leaves -- and the
// ring waits for that event when it comes round (practically never blocks: 256 calls in flight).
struct TableSlot {
    pikamd_solver* s = nullptr;
    int slot = -1;
    hipStream_t st = nullptr;
    TableSlot() = default;
    TableSlot(const TableSlot&) = delete;
    TableSlot& operator=(const TableSlot&) = delete;
    ~TableSlot() {
        if (slot < 0) return;
        // (if the record fails the slot stays marked unused-but-unsafe: drain the stream instead)
        if (hipEventRecord(s->table_event[slot], st) != hipSuccess) (void)hipStreamSynchronize(st);
        s->table_used[slot] = true;
    }
};

inline int upload_batch_table(pikamd_solver* s, BatchRecord* batches, int n, hipStream_t st, const BatchK** out,
                              long long* total, TableSlot& guard) {
    long long start = 0;
    for (int k = 0; k < n; ++k) {
        batches[k].start = start;
        start += batches[k].B;
    }
    *total = start;
    const int slot = s->table_next;
    s->table_next = (slot + 1) % TABLE_RING;
    if (s->table_used[slot]) HIP_TRY(hipEventSynchronize(s->table_event[slot]));
    BatchRecord* host = s->tables_host + (size_t)slot * PIKAMD_MAX_BATCHES;
    BatchRecord* dev = s->tables_dev + (size_t)slot * PIKAMD_MAX_BATCHES;
    std::memcpy(host, batches, sizeof(BatchRecord) * (size_t)n);
    s->table_used[slot] = false;
    guard.s = s;
    guard.slot = slot;
    guard.st = st;
    HIP_TRY(hipMemcpyAsync(dev, host, sizeof(BatchRecord) * (size_t)n, hipMemcpyHostToDevice, st));
    *out = reinterpret_cast<const BatchK*>(dev);
    return 0;
}

// ---- a memetic call: what its three launchers -- launch_solve below, the routed launcher (pik_route.hpp), the
// launcher of a restart attempt (pik_restart.hpp) -- share besides the plan (pik_memetic_plan.hpp) ----
static_assert(WAVE == PLAN_WAVE, "the plan's wavefront");

// the plan's regime input: are three or more OTHER calls of this handle still in flight?
inline bool others_busy(pikamd_solver* s, int slot) {
    int others = 0;
    for (int k = 0; k < N_DEVICE_SLOTS + N_HOST_JOBS; ++k)
        if (k != slot && s->slot_event_used[k] && hipEventQuery(s->slot_event[k]) == hipErrorNotReady) ++others;
    (void)hipGetLastError(); // (hipErrorNotReady is an answer, not a failure)
    return others >= 3;
}

// f(the memetic kernel with this variant id)
template <int D, class F>
int with_variant_kernel(int id, F f) {
    switch (id) {
        case 5: return f(memetic_kernel<D, 16>);
        case 4: return f(memetic_kernel<D, 8>);
        case 3: return f(memetic_kernel<D, 4>);
        case 2: return f(memetic_kernel<D, 2>);
        case 7:
            if constexpr (D <= 9) return f(memetic_kernel<D, 1, false, 2>);
            return 0;
#if !defined(PIK_STRICT)
        case 10: return f(memetic_kernel<D, 16, true>);
        case 9: return f(memetic_kernel<D, 8, true>);
#endif
        case 8: return f(memetic_kernel<D, 2, true>);
        case 6: return f(memetic_kernel<D, 1, true>);
        default: return f(memetic_kernel<D, 1>);
    }
}

// waves per CU of each kernel variant: asked once per handle and FLAVOUR (the general and the exact kernels are
// different code with different register counts: a handle switched between them by the option "arithmetic"
// must not size one flavour's grids by the other's figure)
#define PIK_OCC_ROW (PIK_COMMON ? (PIK_NO_GOALS ? 1 : 2) : (PIK_XF ? 3 : 0))

// the slot's scratch for a memetic call of B problems, S species (the plan's layout with this length's record rows)
template <int D>
MemeticScratch memetic_scratch(const pikamd_solver* s, const ParamsK& pk, long long B, int S) {
    return MemeticScratch(B, S, pk.population, D, chain_has_unbounded(s), (size_t)StateRows<D>::D_ROWS(pk.elites),
                          StateRows<D>::L_ROWS, StateRows<D>::I_ROWS);
}

template <int D>
struct MemeticCall {
    pikamd_solver* s;
    hipStream_t st;
    int slot;
    const ConstsK<D>* kc = nullptr;
    SolveArgs a; // the caller's (batches, seed, B) + what the plan and the pass fill in
    MemeticPlan pl;
    int* lists[2] = {nullptr, nullptr};
    unsigned char* cblk = nullptr; // the slot's counter block: u64 work[16] | u32 n_list[17] @128 | u32 done[16] @256
    unsigned long long* c_work = nullptr;
    unsigned* c_nlist = nullptr;
    unsigned* c_done = nullptr;

    MemeticCall(pikamd_solver* s_, const pikamd_params* p, const ParamsK& pk, hipStream_t st_, int slot_, const SolveArgs& a0)
        : s(s_), st(st_), slot(slot_), a(a0) {
        plan_begin(s, p, pk, pl);
        a.gs_log2 = pl.gs_log2;
        a.species = pl.S;
        a.sp_log2 = pl.sp_log2;
    }
    MemeticScratch scratch(const ParamsK& pk, long long B) const { return memetic_scratch<D>(s, pk, B, pl.S); }
    // the slot's scratch (parked state and survivor lists only for a call with passes) and its counter block
    void bind(const MemeticScratch& lay, bool passes) {
        char* base = (char*)s->slot_state[slot].p;
        a.pop = lay.has_unbounded ? (double*)(base + lay.off_pop) : nullptr;
        a.pop_stride = (long long)lay.pop_stride;
        a.cap = a.B;
        a.st_d = passes ? (double*)(base + lay.off_d) : nullptr;
        a.st_l = passes ? (long long*)(base + lay.off_l) : nullptr;
        a.st_i = passes ? (int*)(base + lay.off_i) : nullptr;
        lists[0] = passes ? (int*)(base + lay.off_list) : nullptr;
        lists[1] = passes ? lists[0] + a.cap : nullptr;
        cblk = s->counters + COUNTER_BLOCK * (size_t)slot;
        c_work = (unsigned long long*)cblk;
        c_nlist = (unsigned*)(cblk + 128);
        c_done = (unsigned*)(cblk + 256);
    }
    // wavefronts the chip holds of every candidate
    int capacities() {
        for (int i = 0; i < pl.n_var; ++i) {
            int& per_cu = s->occupancy_cache[PIK_OCC_ROW][pl.var[i].id];
            if (per_cu == 0) {
                int asked = 0;
                if (int rc = with_variant_kernel<D>(pl.var[i].id, [&](auto kernel) -> int {
                        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&asked, kernel, WAVE, 0));
                        return 0;
                    }))
                    return rc;
                per_cu = asked < 1 ? 1 : asked;
            }
            pl.var[i].capacity = (long long)s->num_cu * per_cu;
        }
        return 0;
    }
    // pass k of n_marks + 1: from the survivors of pass k - 1 (pass 0: every problem) to the list of its own
    void pass(int k, const int* marks, int n_marks) {
        a.fresh = (k == 0);
        a.pause_gen = (k < n_marks) ? marks[k] : 0x7fffffff;
        a.list_in = (k == 0) ? nullptr : lists[(k - 1) & 1];
        a.n_in = (k == 0) ? nullptr : c_nlist + k;
        a.list_out = n_marks ? lists[k & 1] : nullptr;
        a.n_out = n_marks ? c_nlist + (k + 1) : nullptr;
        a.work_counter = c_work + k;
        a.done = c_done + k;
    }
    // candidate v for survivor counts in (lo, hi], its grid sized for n problems
    int launch(int v, long long n, unsigned lo, unsigned hi) {
        a.sel_lo = lo;
        a.sel_hi = hi;
        const dim3 g((unsigned)plan_grid(n, pl.groups_per_wave(v), pl.var[v].capacity)), b(WAVE);
        return with_variant_kernel<D>(pl.var[v].id, [&](auto kernel) -> int {
            hipLaunchKernelGGL(kernel, g, b, 0, st, kc, a);
            HIP_TRY(hipGetLastError());
            return 0;
        });
    }
    // what the host's rule enqueues for the pass (plan_pass)
    int launch_pass(const RangeTable& t, int start_gen, long long size, long long known, bool counted) {
        PassLaunch q[PLAN_MAX_VARIANTS];
        const int n = plan_pass(pl, t, start_gen, size, known, counted, q);
        for (int i = 0; i < n; ++i)
            if (int rc = launch(q[i].var, size, q[i].sel_lo, q[i].sel_hi)) return rc;
        return 0;
    }
    // behind the last launch: the kernels have re-armed the counters; the slot's event
    int finish() {
        s->counters_dirty[slot] = false;
        if (!s->slot_event[slot]) HIP_TRY(hipEventCreateWithFlags(&s->slot_event[slot], hipEventDisableTiming));
        HIP_TRY(hipEventRecord(s->slot_event[slot], st));
        s->slot_event_used[slot] = true;
        return 0;
    }
};

template <int D>
int launch_solve(pikamd_solver* s, const pikamd_params* p, const ParamsK& pk, BatchRecord* batches, int n_batches,
                 unsigned long long rng_seed, hipStream_t st, int slot, bool reserve_only) {
    long long B = 0;
    for (int k = 0; k < n_batches; ++k) B += batches[k].B;
    if (B == 0) return 0;
    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, &pk, slot, st, &kc)) return rc;
    SolveArgs a;
    TableSlot table; // (declared before any launch: its destructor records the event behind the last one)
    std::memset(&a, 0, sizeof a);
    a.n_batches = n_batches;
    for (int k = 0; k < n_batches; ++k) a.signal |= batches[k].completed != nullptr;
    a.rng_seed = rng_seed;
    a.B = B;
    if (p->mode == 1) {
        if (reserve_only) return 0;
        if (int rc = upload_batch_table(s, batches, n_batches, st, &a.batches, &a.B, table)) return rc;
        const int block = 64;
        const long long grid = (a.B + block - 1) / block;
#if !defined(PIK_STRICT)
        // few targets: the cooperative descent with 16 (or 8) lanes per problem, as long as every
        // problem gets its wavefront share in one round -- a third of the one-lane latency (the
        // plugin's local mode is called with one target at a time); option lanes_per_elite=1 forces one lane
        {
            int lpe = 0;
            const long long simds = (long long)s->num_cu * 4;
            const bool multi = s->n_tips > 1;
            if (lpe_allowed(s, 16, 1, 1, multi) && a.B <= simds * (WAVE / 16)) lpe = 16;
            else if (lpe_allowed(s, 8, 1, 1, multi) && a.B <= simds * (WAVE / 8)) lpe = 8;
            if (s->opt.lpe > 0) { // forced lanes per problem (1 = the one-lane kernel)
                const int v = s->opt.lpe;
                lpe = (v == 16 && lpe_allowed(s, 16, 1, 1, multi)) ? 16 : (v == 8 && lpe_allowed(s, 8, 1, 1, multi)) ? 8 : 0;
            }
            if (lpe) {
                const long long per_wave = WAVE / lpe;
                const dim3 g((unsigned)((a.B + per_wave - 1) / per_wave));
                if (multi) {
                    if (lpe == 16) hipLaunchKernelGGL((ik_gradient_wide_kernel<D, 16, true>), g, dim3(block), 0, st, kc, a);
                    else hipLaunchKernelGGL((ik_gradient_wide_kernel<D, 8, true>), g, dim3(block), 0, st, kc, a);
                } else if (lpe == 16) hipLaunchKernelGGL((ik_gradient_wide_kernel<D, 16>), g, dim3(block), 0, st, kc, a);
                else hipLaunchKernelGGL((ik_gradient_wide_kernel<D, 8>), g, dim3(block), 0, st, kc, a);
                HIP_TRY(hipGetLastError());
                return 0;
            }
        }
#else
        // exact flavours, one tip frame: the team forms of the memoised descent with 16 (or 4) lanes per problem, as long
        // as every problem gets its wavefront share in one round (pik_kernels.hpp ik_gradient_team_kernel); option
        // lanes_per_elite = 1 forces one lane, 16 / 4 one of the team kernels whatever the size of the call
        if (s->n_tips == 1) {
            int lpe = 0;
            const long long simds = (long long)s->num_cu * 4;
            if (lpe_allowed(s, 16, 1, 1, false) && a.B <= simds * (WAVE / 16)) lpe = 16;
            else if (lpe_allowed(s, 4, 1, 1, false) && a.B <= simds * (WAVE / 4)) lpe = 4;
            if (s->opt.lpe > 0) {
                const int v = s->opt.lpe;
                lpe = ((v == 16 || v == 4) && lpe_allowed(s, v, 1, 1, false)) ? v : 0;
            }
            if (lpe) {
                const long long per_wave = WAVE / lpe;
                const dim3 g((unsigned)((a.B + per_wave - 1) / per_wave));
                if (lpe == 16) hipLaunchKernelGGL((ik_gradient_team_kernel<D, 16>), g, dim3(block), 0, st, kc, a);
                else hipLaunchKernelGGL((ik_gradient_team_kernel<D, 4>), g, dim3(block), 0, st, kc, a);
                HIP_TRY(hipGetLastError());
                return 0;
            }
        }
#endif
        if (s->n_tips > 1)
            hipLaunchKernelGGL((ik_gradient_kernel<D, true>), dim3((unsigned)grid), dim3(block), 0, st, kc, a);
        else
            hipLaunchKernelGGL(ik_gradient_kernel<D>, dim3((unsigned)grid), dim3(block), 0, st, kc, a);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // memetic: groups of GS * LPE lanes per problem, one wavefront per workgroup, persistent waves.  The host's rule:
    // the regime is the one at the time of the call, the first pass knows its size and is one launch, every later
    // pass enqueues each variant the call's problems can reach and the variants select themselves by the count.
    MemeticCall<D> m(s, p, pk, st, slot, a);
    m.kc = kc;
    const bool throughput_regime = plan_throughput(s, others_busy(s, slot));
    int marks[16];
    const int n_marks = plan_marks(s, m.pl, throughput_regime, B, false, marks);
    const MemeticScratch lay = m.scratch(pk, B);
    // (a reservation is for calls in either regime: as if the call had every pass of the schedule)
    if (n_marks > 0 || lay.has_unbounded || (reserve_only && m.pl.sc.n_marks > 0)) {
        if (int rc = s->slot_state[slot].ensure(lay.total)) return rc;
    }
    if (reserve_only) return 0;
    if (int rc = upload_batch_table(s, batches, n_batches, st, &m.a.batches, &m.a.B, table)) return rc;
    m.bind(lay, n_marks > 0);
    if (s->counters_dirty[slot]) HIP_TRY(hipMemsetAsync(m.cblk, 0, COUNTER_BLOCK, st)); // after a failed launch
    s->counters_dirty[slot] = true;
    plan_candidates(s, m.pl, !throughput_regime || m.pl.sc.n_sched > 0, D <= 9);
    RangeTable t;
    plan_ranges(s, m.pl, throughput_regime, t);
    if (int rc = m.capacities()) return rc;
    for (int k = 0; k <= n_marks; ++k) {
        m.pass(k, marks, n_marks);
        if (int rc = m.launch_pass(t, k == 0 ? 0 : marks[k - 1], m.a.B, k == 0 ? m.a.B : 0, k > 0)) return rc;
    }
    return m.finish();
}

template <int D>
const LaunchOps* make_ops() {
    static const LaunchOps ops = {&launch_fk<D>, &launch_cost<D>, &launch_step<D>, &launch_solve<D>};
    return &ops;
}

} // namespace pik
