// pik_route.hpp -- the routed launcher: launch_solve's memetic branch (pik_launch.hpp) with the regime -- latency or
// throughput schedule -- chosen per pass ON THE DEVICE, when the pass starts, instead of on the host when the call is
// enqueued.  It launches the memetic kernels pik_inst.hip compiles (pik_route_inst.hip declares them `extern template`:
// no second copy of their code); the only kernel of its own is route_kernel below.
//
// launch_solve enqueues every candidate variant of a pass and lets each compare the survivor count with its own range
// (SolveArgs::sel_lo / sel_hi), because the host cannot know how many problems survive.  Neither can it know, when it
// enqueues a call, what ELSE will be on the chip when a pass of that call starts: a burst of calls enqueued within a
// millisecond all count "others in flight" before any of them runs, and the pools that finish last keep the schedule
// chosen for a full chip when they have it to themselves.  Here every slot publishes the problems its call still
// has; in front of every pass a one-wavefront router reads the pass's survivor count, publishes it, sums what the
// other slots published, picks the regime (throughput when the others hold at least `threshold` problems: by default
// half of what gives every SIMD a one-lane wavefront -- measured best of 1/2 x, 1 x and 2 x that figure, DESIGN.md
// section 9), applies the host's range table of that regime and hands the count to the ONE
// variant it chose -- through that variant's own counter; the others find 0 and return.  The kernels, their
// arguments' layout, the scratch, the batch table and the marks are launch_solve's, by construction: the schedule,
// the candidates and both regimes' range tables come from the plan every launcher of a memetic call uses
// (pik_memetic_plan.hpp), the launches from MemeticCall (pik_launch.hpp); what is written here is the router, its
// tables' device form, the per-variant counters and the pruning of variants no table can reach.  A stale load changes
// which variant runs, never a result: the variants re-order the same arithmetic (tests/test_gpu_device_regime.py).
#pragma once

#include "pik_launch.hpp"
#include "pik_route_ops.hpp"

namespace pik {

// the range table of one regime: entry i is chosen for survivor counts in (hi[i - 1], hi[i]]
struct RouteTable {
    int n;
    int var[ROUTE_MAX_VARIANTS];      // index of the variant's counter
    int id[ROUTE_MAX_VARIANTS];       // its id (launch_solve: 5 / 4 / 3 / 2 = 16 / 8 / 4 / 2 lanes, 1 and 7 = one lane)
    unsigned hi[ROUTE_MAX_VARIANTS];
};

struct RouteArgs {
    unsigned* count;        // survivor count of the pass (the previous pass's n_out); null: `fixed_n`
    unsigned fixed_n;       // pass 0: the call's problems ...
    int fixed_id;           // ... and the variant the host launched for them
    unsigned* vc;           // the pass's variant counters [ROUTE_MAX_VARIANTS]
    unsigned* loads;        // [n_slots]
    unsigned* record;       // the pass's record [4], or null
    int slot, n_slots;
    int clear;              // behind the last pass: the slot's load back to 0, nothing else
    unsigned long long threshold;
    RouteTable lat, thr;
};

// (a template over the chain length only so that every per-length object carries its own instance, as the kernels do)
template <int D>
__global__ __launch_bounds__(WAVE) void route_kernel(RouteArgs r) {
    __shared__ unsigned long long part[WAVE];
    const int lane = threadIdx.x;
    // (relaxed, agent scope: the other slots' routers run on other queues; a value one pass old is as good)
    unsigned long long mine = 0ull;
    for (int i = lane; i < r.n_slots; i += WAVE)
        if (i != r.slot) mine += __hip_atomic_load(r.loads + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    part[lane] = mine;
    __syncthreads();
    if (lane != 0) return;
    if (r.clear) {
        __hip_atomic_store(r.loads + r.slot, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    unsigned long long others = 0ull;
    for (int i = 0; i < WAVE; ++i) others += part[i];
    const unsigned n = r.count ? *r.count : r.fixed_n;
    __hip_atomic_store(r.loads + r.slot, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int id = r.fixed_id;
    if (r.count) {
        const RouteTable& t = (others >= r.threshold) ? r.thr : r.lat;
        int pick = -1;
        for (int i = 0; i < t.n; ++i)
            if (pick < 0 && n > 0u && n <= t.hi[i]) pick = i;
        id = 0;
        if (pick >= 0) {
            r.vc[t.var[pick]] = n; // (the chosen variant's epilogue zeroes it again)
            id = t.id[pick];
        }
        *r.count = 0u; // re-armed for the next call on the slot
    }
    if (r.record) {
        r.record[0] = n;
        r.record[1] = others > 0xffffffffull ? 0xffffffffu : (unsigned)others;
        r.record[2] = (unsigned)id;
        r.record[3] = 1u;
    }
}

static_assert(ROUTE_MAX_VARIANTS == PLAN_MAX_VARIANTS, "a counter per candidate");
static_assert(sizeof(Schedule::marks) / sizeof(int) <= ROUTE_MAX_PASSES, "a record per pass");

// the plan's range table of one regime as the router reads it; lo_of[i]: the fewest survivors that can bring a pass
// to candidate i in either regime
inline void route_table(const MemeticPlan& pl, const RangeTable& t, RouteTable& r, long long* lo_of) {
    r.n = t.n;
    for (int j = 0; j < t.n; ++j) {
        r.var[j] = t.var[j];
        r.id[j] = pl.var[t.var[j]].id;
        r.hi[j] = (unsigned)t.hi[j];
        if (t.hi[j] > t.lo[j] && t.lo[j] < lo_of[t.var[j]]) lo_of[t.var[j]] = t.lo[j];
    }
}

template <int D>
int launch_solve_routed(pikamd_solver* s, const pikamd_params* p, const ParamsK& pk, BatchRecord* batches,
                        int n_batches, unsigned long long rng_seed, hipStream_t st, int slot, RouteCtx* ctx) {
    ctx->served = false;
    ctx->n_passes = 0;
    long long B = 0;
    for (int k = 0; k < n_batches; ++k) B += batches[k].B;
    // (the caller has checked: memetic mode, one tip frame, one species, nothing forced)
    if (B == 0 || p->mode != 0 || s->n_tips != 1 || p->memetic_num_threads > 1) return 0;
    SolveArgs a;
    std::memset(&a, 0, sizeof a);
    a.n_batches = n_batches;
    for (int k = 0; k < n_batches; ++k) a.signal |= batches[k].completed != nullptr;
    a.rng_seed = rng_seed;
    a.B = B;
    MemeticCall<D> m(s, p, pk, st, slot, a);
    if (m.pl.sc.n_sched > 0 || s->opt.regime != 0) return 0;
    // the host's view of the regime: it still decides pass 0 (whose size is known) and whether a small call is cut
    // into passes at all
    const bool host_throughput = others_busy(s, slot);
    int marks[16];
    const int n_marks = plan_marks(s, m.pl, host_throughput, B, false, marks);
    if (n_marks == 0) return 0; // one launch, no pass to route: launch_solve

    if (int rc = upload_consts<D>(s, &pk, slot, st, &m.kc)) return rc;
    TableSlot table; // (declared before any launch: its destructor records the event behind the last one)
    const MemeticScratch lay = m.scratch(pk, B);
    if (int rc = s->slot_state[slot].ensure(lay.total)) return rc;
    if (int rc = upload_batch_table(s, batches, n_batches, st, &m.a.batches, &m.a.B, table)) return rc;
    m.bind(lay, true);
    unsigned* vc = route_vc(s, slot);
    if (s->counters_dirty[slot]) { // after a failed launch
        HIP_TRY(hipMemsetAsync(m.cblk, 0, COUNTER_BLOCK, st));
        HIP_TRY(hipMemsetAsync(vc, 0, ROUTE_VC_BLOCK, st));
    }
    s->counters_dirty[slot] = true;
    // every candidate for one tip frame and both regimes' tables: which regime a pass runs in is the router's decision
    plan_candidates(s, m.pl, true, D <= 9);
    if (int rc = m.capacities()) return rc;
    RangeTable lat, thr;
    plan_ranges(s, m.pl, false, lat);
    plan_ranges(s, m.pl, true, thr);
    RouteArgs r;
    std::memset(&r, 0, sizeof r);
    long long lo_of[ROUTE_MAX_VARIANTS];
    for (long long& v : lo_of) v = 0x7fffffffffffffffll;
    route_table(m.pl, lat, r.lat, lo_of);
    route_table(m.pl, thr, r.thr, lo_of);
    r.loads = route_loads(s);
    r.slot = slot;
    r.n_slots = N_SLOTS;
    r.threshold = ctx->threshold > 0 ? (unsigned long long)ctx->threshold
                                     : (unsigned long long)((long long)s->num_cu * 4 * WAVE / m.pl.gs / 2);
    auto launch_router = [&](int k, unsigned* count, int fixed_id, bool clear) -> int {
        r.count = count;
        r.fixed_n = (unsigned)(m.a.B > 0xffffffffll ? 0xffffffffll : m.a.B);
        r.fixed_id = fixed_id;
        r.vc = vc + (size_t)k * ROUTE_MAX_VARIANTS;
        r.record = clear ? nullptr : route_record(s, slot) + (size_t)k * 4;
        r.clear = clear ? 1 : 0;
        hipLaunchKernelGGL(route_kernel<D>, dim3(1), dim3(WAVE), 0, st, r);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    for (int k = 0; k <= n_marks; ++k) {
        m.pass(k, marks, n_marks);
        if (k == 0) {
            // the first pass knows its size: one launch, chosen by the host's view of the regime
            PassLaunch q[PLAN_MAX_VARIANTS];
            const int v = plan_pass(m.pl, host_throughput ? thr : lat, 0, m.a.B, m.a.B, false, q) ? q[0].var : m.pl.n_var - 1;
            if (int rc = launch_router(0, nullptr, m.pl.var[v].id, false)) return rc; // (publishes the call's size)
            if (int rc = m.launch(v, m.a.B, 0u, 0xffffffffu)) return rc;
            continue;
        }
        // the survivors of pass k - 1 -> the counter of the variant this pass runs with
        if (int rc = launch_router(k, m.c_nlist + k, 0, false)) return rc;
        for (int i = 0; i < m.pl.n_var; ++i) {
            // (a pass cannot have more survivors than the call has problems: variants no regime's table can reach
            //  with that many are not enqueued)
            if (m.a.B <= lo_of[i]) continue;
            m.a.n_in = vc + (size_t)k * ROUTE_MAX_VARIANTS + i;
            if (int rc = m.launch(i, m.a.B, 0u, 0xffffffffu)) return rc;
        }
    }
    if (int rc = launch_router(0, nullptr, 0, true)) return rc;
    if (int rc = m.finish()) return rc;
    ctx->served = true;
    ctx->n_passes = n_marks + 1;
    return 0;
}

template <int D>
const RouteOps* make_route_ops() {
    static const RouteOps ops = {&launch_solve_routed<D>};
    return &ops;
}

} // namespace pik
