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
// arguments' layout, the scratch, the batch table and the marks are launch_solve's.  A stale load changes which
// variant runs, never a result: the variants re-order the same arithmetic (tests/test_gpu_device_regime.py).
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
    a.gs_log2 = pow2ceil_log2(pk.elites);
    const int gs = 1 << a.gs_log2;
    const int S = 1;
    a.species = S;
    a.sp_log2 = 0;
    Schedule sc;
    make_schedule(s, pk, gs, S, sc);
    if (sc.n_sched > 0 || s->opt.regime != 0) return 0;
    // the host's view of the regime, as launch_solve has it: it still decides pass 0 (whose size is known) and
    // whether a small call is cut into passes at all
    bool host_throughput = false;
    {
        int others = 0;
        for (int k = 0; k < N_DEVICE_SLOTS + N_HOST_JOBS; ++k)
            if (k != slot && s->slot_event_used[k] && hipEventQuery(s->slot_event[k]) == hipErrorNotReady) ++others;
        (void)hipGetLastError(); // (hipErrorNotReady is an answer, not a failure)
        host_throughput = others >= 3;
    }
    // the one-lane kernel's two-per-SIMD build: from 9/8 of the SIMD count with the chip to itself, from the
    // schedule's threshold (5/8) with other calls queued up -- launch_solve's two figures, one per regime
    const long long occ2_from_thr = sc.occ2_from;
    const long long occ2_from_lat =
        (s->opt.two_per_simd < 2 && !s->opt.force_occ2) ? (long long)s->num_cu * 4 * 9 / 8 : sc.occ2_from;
    int n_marks = sc.n_marks;
    if (!host_throughput && !s->opt.passes_set) {
        int widest = 1;
        for (int l : {16, 8, 4, 2})
            if (widest == 1 && lpe_allowed(s, l, gs, S, false)) widest = l;
        if (widest > 1 && B <= (long long)s->num_cu * 4 * (WAVE / (gs * widest))) n_marks = 0;
    }
    if (n_marks == 0) return 0; // one launch, no pass to route: launch_solve
    static_assert(sizeof(Schedule::marks) / sizeof(int) <= ROUTE_MAX_PASSES, "a record per pass");

    const ConstsK<D>* kc = nullptr;
    if (int rc = upload_consts<D>(s, &pk, slot, st, &kc)) return rc;
    TableSlot table; // (declared before any launch: its destructor records the event behind the last one)
    a.n_batches = n_batches;
    for (int k = 0; k < n_batches; ++k) a.signal |= batches[k].completed != nullptr;
    a.rng_seed = rng_seed;
    a.B = B;
    // per-slot scratch: launch_solve's layout
    const long long cap = B;
    const size_t recs = (size_t)B * (size_t)S;
    const size_t d_rows = (size_t)StateRows<D>::D_ROWS(pk.elites);
    const size_t off_d = 0;
    const size_t off_l = off_d + sizeof(double) * d_rows * recs;
    const size_t off_i = off_l + sizeof(long long) * StateRows<D>::L_ROWS * recs;
    const size_t off_list = off_i + sizeof(int) * StateRows<D>::I_ROWS * recs;
    const size_t off_cnt = off_list + sizeof(int) * 2 * (size_t)cap;
    const bool has_unbounded = s->chain.bounded_mask != ((1u << s->chain.dof) - 1u);
    const size_t pop_stride = (size_t)pk.population * (1 + D) + ((size_t)pk.population + 1) / 2;
    const size_t off_pop = (off_cnt + 64 + 63) / 64 * 64;
    const size_t total = off_pop + (has_unbounded ? sizeof(double) * 2 * pop_stride * (size_t)cap * (size_t)S : 0);
    if (int rc = s->slot_state[slot].ensure(total)) return rc;
    if (int rc = upload_batch_table(s, batches, n_batches, st, &a.batches, &a.B, table)) return rc;
    char* base = (char*)s->slot_state[slot].p;
    a.pop = has_unbounded ? (double*)(base + off_pop) : nullptr;
    a.pop_stride = (long long)pop_stride;
    a.cap = cap;
    a.st_d = (double*)(base + off_d);
    a.st_l = (long long*)(base + off_l);
    a.st_i = (int*)(base + off_i);
    int* lists[2] = {(int*)(base + off_list), (int*)(base + off_list) + cap};
    unsigned char* cblk = s->counters + COUNTER_BLOCK * (size_t)slot;
    unsigned long long* c_work = (unsigned long long*)cblk;
    unsigned* c_nlist = (unsigned*)(cblk + 128);
    unsigned* c_done = (unsigned*)(cblk + 256);
    unsigned* vc = route_vc(s, slot);
    if (s->counters_dirty[slot]) { // after a failed launch
        HIP_TRY(hipMemsetAsync(cblk, 0, COUNTER_BLOCK, st));
        HIP_TRY(hipMemsetAsync(vc, 0, ROUTE_VC_BLOCK, st));
    }
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
    };
    Variant var[ROUTE_MAX_VARIANTS];
    int n_var = 0;
    auto add_variant = [&](auto kernel, int lpe_, int id) -> int {
        Variant v{lpe_, id, 0};
        if (int rc = capacity_of(kernel, id, &v.capacity)) return rc;
        var[n_var++] = v;
        return 0;
    };
    auto launch_variant = [&](const Variant& v) -> int {
        const long long groups_per_wave = WAVE / (gs * v.lpe);
        const long long waves_needed = (a.B + groups_per_wave - 1) / groups_per_wave;
        const long long grid = waves_needed < v.capacity ? waves_needed : v.capacity;
        a.sel_lo = 0u;
        a.sel_hi = 0xffffffffu;
        const dim3 g((unsigned)grid), b(WAVE);
        switch (v.id) {
            case 5: hipLaunchKernelGGL((memetic_kernel<D, 16>), g, b, 0, st, kc, a); break;
            case 4: hipLaunchKernelGGL((memetic_kernel<D, 8>), g, b, 0, st, kc, a); break;
            case 3: hipLaunchKernelGGL((memetic_kernel<D, 4>), g, b, 0, st, kc, a); break;
            case 2: hipLaunchKernelGGL((memetic_kernel<D, 2>), g, b, 0, st, kc, a); break;
            case 7:
                if constexpr (D <= 9) hipLaunchKernelGGL((memetic_kernel<D, 1, false, 2>), g, b, 0, st, kc, a);
                break;
            default: hipLaunchKernelGGL((memetic_kernel<D, 1>), g, b, 0, st, kc, a); break;
        }
        HIP_TRY(hipGetLastError());
        return 0;
    };
    // launch_solve's candidates for one tip frame, widest first -- all of them: which regime a pass runs in is
    // the router's decision
    if (lpe_allowed(s, 16, gs, S, false))
        if (int rc = add_variant(memetic_kernel<D, 16>, 16, 5)) return rc;
    if (lpe_allowed(s, 8, gs, S, false))
        if (int rc = add_variant(memetic_kernel<D, 8>, 8, 4)) return rc;
    if (lpe_allowed(s, 4, gs, S, false))
        if (int rc = add_variant(memetic_kernel<D, 4>, 4, 3)) return rc;
    if (lpe_allowed(s, 2, gs, S, false))
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
    // the range tables: launch_solve's `hi` of every variant and its running `lo`, once per regime (the throughput
    // regime has the one-lane variants only)
    auto make_table = [&](bool throughput, RouteTable& t, long long* lo_of) {
        const long long occ2_from_problems = (throughput ? occ2_from_thr : occ2_from_lat) * WAVE / gs;
        t.n = 0;
        long long lo = 0;
        for (int i = 0; i < n_var; ++i) {
            if (throughput && var[i].lpe > 1) continue;
            const long long per_wave = WAVE / (gs * var[i].lpe);
            long long hi = (var[i].lpe > 1) ? (long long)s->num_cu * 4 * per_wave // one wavefront per SIMD
                           : (var[i].id == 7 || i == n_var - 1) ? 0xffffffffll
                                                                : occ2_from_problems - 1;
            if (hi < lo) hi = lo;
            if (hi > 0xffffffffll) hi = 0xffffffffll;
            t.var[t.n] = i;
            t.id[t.n] = var[i].id;
            t.hi[t.n] = (unsigned)hi;
            ++t.n;
            if (hi > lo && lo < lo_of[i]) lo_of[i] = lo; // (the fewest survivors that can bring a pass to variant i)
            lo = hi;
        }
    };
    RouteArgs r;
    std::memset(&r, 0, sizeof r);
    long long lo_of[ROUTE_MAX_VARIANTS];
    for (long long& v : lo_of) v = 0x7fffffffffffffffll;
    make_table(false, r.lat, lo_of);
    make_table(true, r.thr, lo_of);
    r.loads = route_loads(s);
    r.slot = slot;
    r.n_slots = N_SLOTS;
    r.threshold = ctx->threshold > 0 ? (unsigned long long)ctx->threshold
                                     : (unsigned long long)((long long)s->num_cu * 4 * WAVE / gs / 2);
    auto launch_router = [&](int k, unsigned* count, int fixed_id, bool clear) -> int {
        r.count = count;
        r.fixed_n = (unsigned)(a.B > 0xffffffffll ? 0xffffffffll : a.B);
        r.fixed_id = fixed_id;
        r.vc = vc + (size_t)k * ROUTE_MAX_VARIANTS;
        r.record = clear ? nullptr : route_record(s, slot) + (size_t)k * 4;
        r.clear = clear ? 1 : 0;
        hipLaunchKernelGGL(route_kernel<D>, dim3(1), dim3(WAVE), 0, st, r);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    for (int k = 0; k <= n_marks; ++k) {
        a.fresh = (k == 0);
        a.pause_gen = (k < n_marks) ? sc.marks[k] : 0x7fffffff;
        a.list_in = (k == 0) ? nullptr : lists[(k - 1) & 1];
        a.list_out = lists[k & 1];
        a.n_out = c_nlist + (k + 1);
        a.work_counter = c_work + k;
        a.done = c_done + k;
        if (k == 0) {
            // the first pass knows its size: one launch, chosen by the host's view of the regime
            const RouteTable& t = host_throughput ? r.thr : r.lat;
            int pick = t.n - 1;
            for (int i = t.n - 1; i >= 0; --i)
                if ((unsigned long long)a.B <= t.hi[i]) pick = i;
            a.n_in = nullptr;
            if (int rc = launch_router(0, nullptr, t.id[pick], false)) return rc; // (publishes the call's size)
            if (int rc = launch_variant(var[t.var[pick]])) return rc;
            continue;
        }
        // the survivors of pass k - 1 -> the counter of the variant this pass runs with
        if (int rc = launch_router(k, c_nlist + k, 0, false)) return rc;
        for (int i = 0; i < n_var; ++i) {
            // (a pass cannot have more survivors than the call has problems: variants no regime's table can reach
            //  with that many are not enqueued)
            if (a.B <= lo_of[i]) continue;
            a.n_in = vc + (size_t)k * ROUTE_MAX_VARIANTS + i;
            if (int rc = launch_variant(var[i])) return rc;
        }
    }
    if (int rc = launch_router(0, nullptr, 0, true)) return rc;
    s->counters_dirty[slot] = false;
    if (!s->slot_event[slot]) HIP_TRY(hipEventCreateWithFlags(&s->slot_event[slot], hipEventDisableTiming));
    HIP_TRY(hipEventRecord(s->slot_event[slot], st));
    s->slot_event_used[slot] = true;
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
