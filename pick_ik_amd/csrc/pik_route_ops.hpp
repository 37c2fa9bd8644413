// pik_route_ops.hpp -- host side of the routed launcher (pik_route.hpp): the device state it keeps behind the
// handle's counter blocks, the context pik_amd.hip hands it, the ops table a per-length translation unit of
// pik_route_inst.hip exports, and the parser of the option device_regime.  No device code here; not read by
// pik_inst.hip.
#pragma once

#include "pik_dofs.hpp"
#include "pik_solver.hpp"

namespace pik {

// Device state of the routed launcher, in the handle's counter allocation (pikamd_solver::counters) behind the
// N_SLOTS counter blocks:
//   per slot  u32 variant counters [ROUTE_MAX_PASSES][ROUTE_MAX_VARIANTS]  -- the survivor count of a pass, written by
//             the router into the counter of the variant it chose; zero whenever no call is in flight on the slot
//             (the chosen variant re-arms its own, the others are never written)
//   u32 load [N_SLOTS]  -- problems the call in flight on a slot still has, as its last router published them
//             (0: nothing routed in flight)
//   per slot  u32 record [ROUTE_MAX_PASSES][4]  -- survivors, others' load seen, variant id, 1: what the routers of
//             the last call on the slot decided (pikamd_debug_regime)
constexpr int ROUTE_MAX_PASSES = 16;
constexpr int ROUTE_MAX_VARIANTS = 8;
constexpr size_t ROUTE_VC_BLOCK = sizeof(unsigned) * ROUTE_MAX_PASSES * ROUTE_MAX_VARIANTS;
constexpr size_t ROUTE_RECORD_BLOCK = sizeof(unsigned) * ROUTE_MAX_PASSES * 4;
constexpr size_t ROUTE_OFF_VC = COUNTER_BLOCK * (size_t)N_SLOTS;
constexpr size_t ROUTE_OFF_LOADS = ROUTE_OFF_VC + ROUTE_VC_BLOCK * (size_t)N_SLOTS;
constexpr size_t ROUTE_OFF_RECORD = ROUTE_OFF_LOADS + sizeof(unsigned) * (size_t)N_SLOTS;
// the whole counter allocation: the counter blocks the kernels use + the routed launcher's state
constexpr size_t COUNTERS_BYTES = ROUTE_OFF_RECORD + ROUTE_RECORD_BLOCK * (size_t)N_SLOTS;

inline unsigned* route_vc(const pikamd_solver* s, int slot) {
    return reinterpret_cast<unsigned*>(s->counters + ROUTE_OFF_VC + ROUTE_VC_BLOCK * (size_t)slot);
}
inline unsigned* route_loads(const pikamd_solver* s) { return reinterpret_cast<unsigned*>(s->counters + ROUTE_OFF_LOADS); }
inline unsigned* route_record(const pikamd_solver* s, int slot) {
    return reinterpret_cast<unsigned*>(s->counters + ROUTE_OFF_RECORD + ROUTE_RECORD_BLOCK * (size_t)slot);
}

// what pik_amd.hip hands one routed call, and what it gets back
struct RouteCtx {
    long long threshold = 0; // others' load from which a pass takes the throughput schedule (0: SIMD count * 64 / gs / 2)
    bool served = false;     // out: the call was enqueued (false: not this launcher's kind of call -- launch_solve)
    int n_passes = 0;        // out: passes of the call (each with a record)
};

struct RouteOps {
    // launch_solve's arguments (never reserve_only) + the context; returns 0 with ctx->served == false, and nothing
    // enqueued, for a call that has no compaction pass
    int (*solve)(pikamd_solver*, const pikamd_params*, const ParamsK&, BatchRecord* batches, int n_batches,
                 unsigned long long rng_seed, hipStream_t, int slot, RouteCtx* ctx);
};

PIK_DECLARE_OPS_FAMILY(RouteOps, route) // route_ops_d<N>(), route_ops(dof)

// option device_regime: "1" (or "", the default) / "0"; anything else is refused
inline bool parse_device_regime(const char* value, int* out) {
    if (!value || !value[0] || (value[0] == '1' && !value[1])) {
        *out = 1;
        return true;
    }
    if (value[0] == '0' && !value[1]) {
        *out = 0;
        return true;
    }
    return false;
}

} // namespace pik
