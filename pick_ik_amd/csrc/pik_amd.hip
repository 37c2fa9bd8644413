// pik_amd.hip -- C ABI (include/pick_ik_amd.h) of the gfx950 solver library.
//
// Host side of the drop-in boundary: model extraction (pik_host.hpp), handle life cycle, staging
// for the host-pointer entry points.  The kernels and their launches live in one translation unit
// per chain length (pik_inst.hip -> pik_launch.hpp), reached through pik::launch_ops(dof).
// No CPU compute path exists here: without a HIP device every entry point fails with
// PIKAMD_ENODEVICE.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "pik_cartesian_ops.hpp"
#include "pik_globalpath_ops.hpp"
#include "pik_interp.hpp"
#include "pik_path_ops.hpp"
#include "pik_polyline_ops.hpp"
#include "pik_restart_ops.hpp"
#include "pik_route_ops.hpp"
#include "pik_search_ops.hpp"
#include "pik_solver.hpp"
#include "pik_startpath_ops.hpp"
#include "pik_urdf.hpp"
#include "pik_pathvalid_ops.hpp"
#include "pik_validity_ops.hpp"

namespace pik {
char* error_buffer() {
    static thread_local char buf[ERROR_BUFFER_SIZE] = "";
    return buf;
}
} // namespace pik

using pik::fail;

#if !defined(PIK_STRICT)
// All flavours are compiled from the same headers, so the handle, parameter and batch-record layouts -- and the ops
// tables -- are the same types under several namespace names; the tables of the other namespaces are declared
// `const void*` here (PIK_DECLARE_OPS_FAMILY with the type void) and reached through their mangled names.  The
// waypoint-path and restart-search kernels are built for the general and the exact flavour only: the kernels of the
// common configuration return the general ones' bits, a path or search call of theirs is served by the general ones.
namespace pik_exact {
char* error_buffer() { return ::pik::error_buffer(); }
PIK_DECLARE_OPS_FAMILY(void, launch)
PIK_DECLARE_OPS_FAMILY(void, path)
PIK_DECLARE_OPS_FAMILY(void, search)
PIK_DECLARE_OPS_FAMILY(void, route)
PIK_DECLARE_OPS_FAMILY(void, restart)
PIK_DECLARE_OPS_FAMILY(void, startpath)
PIK_DECLARE_OPS_FAMILY(void, globalpath)
PIK_DECLARE_OPS_FAMILY(void, cartesian)
PIK_DECLARE_OPS_FAMILY(void, polyline)
PIK_DECLARE_OPS_FAMILY(void, validity)
PIK_DECLARE_OPS_FAMILY(void, pathvalid)
} // namespace pik_exact
namespace pik_common {
char* error_buffer() { return ::pik::error_buffer(); }
PIK_DECLARE_OPS_FAMILY(void, launch)
PIK_DECLARE_OPS_FAMILY(void, route)
PIK_DECLARE_OPS_FAMILY(void, restart)
} // namespace pik_common
namespace pik_common_goals {
char* error_buffer() { return ::pik::error_buffer(); }
PIK_DECLARE_OPS_FAMILY(void, launch)
PIK_DECLARE_OPS_FAMILY(void, route)
PIK_DECLARE_OPS_FAMILY(void, restart)
} // namespace pik_common_goals
#endif

namespace {

// The flavours of kernels this library links, and the families of per-length ops tables each may have.  The product
// library: the Denavit-Hartenberg kernels (namespace pik), the EXACT kernels (-DPIK_STRICT -DPIK_EXACT_FMA, namespace
// pik_exact: MoveIt's chain product, the literal 2 dof + 3 cost evaluations per gradient step with the accept
// evaluation's work re-used, IEEE square roots and divisions, fused multiply-adds at stated places -- bit-identical to
// the oracle's math mode "fma"; they solve the chains the Denavit-Hartenberg kernels cannot express and every call of
// a handle whose option `arithmetic` is `exact`), and the kernels specialised for the common configuration
// (-DPIK_COMMON=1, namespace pik_common; pik_math.hpp says what that is and what it buys), without and with the joint
// goals (-DPIK_NO_GOALS=0, namespace pik_common_goals: BASELINE config 3's kind of call).  The verification library:
// its one flavour (namespace pik_strict, which `pik` names there).
enum Flavour {
    FL_HOME, // the namespace this file is compiled in: the general kernels (product) / the strict ones (verification)
#if !defined(PIK_STRICT)
    FL_EXACT,
    FL_COMMON,
    FL_COMMON_GOALS,
#endif
    N_FLAVOURS
};
enum Family { FAM_LAUNCH, FAM_PATH, FAM_SEARCH, FAM_ROUTE, FAM_RESTART, FAM_STARTPATH, FAM_GLOBALPATH, FAM_CARTESIAN, FAM_POLYLINE, FAM_VALIDITY, FAM_PATHVALID, N_FAMILIES };

// What a handle keeps for pikamd_search_batch*: the option search_schedule and, per slot, the per-attempt rows of the
// parallel schedule.  Every handle is allocated as one of these (create_solver); pikamd_solver itself is read by the
// kernels' translation units and stays as it is.
struct SolverExt : pikamd_solver {
    int search_schedule = pik::SEARCH_ADAPTIVE;
    pik::DevBuf search_rows[pik::N_SLOTS];
    // the routed launcher (pik_route.hpp): the option device_regime (1: the regime of a pass is chosen on the device
    // when the pass starts; 0: on the host when the call is enqueued, launch_solve's rule), the option
    // regime_threshold (0: the default) and, per slot, the passes the routed launcher enqueued for the last call
    // (-1: the call was launch_solve's) -- what pikamd_debug_regime reads the slot's record by
    int device_regime = 1;
    long long regime_threshold = 0;
    int routed_passes[pik::N_SLOTS];
    // pikamd_search_global_batch*: per slot the starts, the rows of one attempt, the open flags and the open list
    pik::DevBuf restart_rows[pik::N_SLOTS];
    // pikamd_set_approximate_gate: the gate of both search families, and per slot the parameters p' its evaluation
    // reads on the device (gate_for_call)
    bool gate_set = false;
    pikamd_gate gate = {0.0, 0.0};
    pik::DevBuf gate_params_dev; // [N_SLOTS] ParamsK, GATE_PARAMS_STRIDE apart
    pik::ParamsK gate_params_host[pik::N_SLOTS];
    bool gate_params_valid[pik::N_SLOTS] = {};
    // pikamd_search_paths*: per slot the rows of an attempt behind the first (pik_startpath.hpp)
    pik::DevBuf startpath_rows[pik::N_SLOTS];
    // pikamd_search_global_paths*: per slot the scratch of a call (globalpath_scratch, pik_globalpath_ops.hpp)
    pik::DevBuf globalpath_rows[pik::N_SLOTS];
    // pikamd_cartesian_paths_device: per slot the interpolated poses of a call whose caller keeps none
    pik::DevBuf cartesian_goals[pik::N_SLOTS];
    // pikamd_cartesian_waypoints*: per slot the per-path state of the passes and, for a call whose caller keeps none,
    // the interpolated poses
    pik::DevBuf polyline_rows[pik::N_SLOTS];
    // pikamd_set_validity_model: the sphere model as the kernels read it, its device image (the chain's constants in
    // the exact flavour's layout + the model: pik_validity_ops.hpp) and, from pikamd_create, the variables that are
    // the _X / _Y slot of a planar joint (no chain can be cut behind them)
    bool validity_set = false;
    pik::ValidityModelK validity_model;
    pik::DevBuf validity_dev;
    uint32_t planar_xy_mask = 0;
    // pikamd_set_path_validity: the switch, and per slot the `reached` of a path call whose caller keeps none (the
    // validity step reads it)
    int path_validity = 0;
    pik::DevBuf pathvalid_rows[pik::N_SLOTS];
    SolverExt() {
        for (int& v : routed_passes) v = -1;
    }
};
SolverExt* ext_of(pikamd_solver* s) { return static_cast<SolverExt*>(s); }
const SolverExt* ext_of(const pikamd_solver* s) { return static_cast<const SolverExt*>(s); }

// Every ops table of the library: [flavour][family] -> the lookup by chain length (<stem>_ops(dof), pik_dofs.hpp), or
// null where the flavour has no such family.  A lookup gives null for a length outside 1..16 and for one built as a
// stub (PIK_ONLY_D).
using OpsLookup = const void* (*)(int dof);
template <class Ops, const Ops* (*lookup)(int)>
const void* untyped(int dof) {
    return lookup(dof);
}
const OpsLookup OPS_TABLE[N_FLAVOURS][N_FAMILIES] = {
    {untyped<pik::LaunchOps, pik::launch_ops>, untyped<pik::PathOps, pik::path_ops>, untyped<pik::SearchOps, pik::search_ops>,
#if defined(PIK_STRICT)
     nullptr, // (no routed launcher)
#else
     untyped<pik::RouteOps, pik::route_ops>,
#endif
     untyped<pik::RestartOps, pik::restart_ops>, untyped<pik::StartPathOps, pik::startpath_ops>,
     untyped<pik::GlobalPathOps, pik::globalpath_ops>, untyped<pik::CartesianOps, pik::cartesian_ops>,
     untyped<pik::PolylineOps, pik::polyline_ops>,
#if defined(PIK_STRICT)
     untyped<pik::ValidityOps, pik::validity_ops>, untyped<pik::PathValidOps, pik::pathvalid_ops>},
#else
     nullptr, nullptr}, // (the sphere validity test is the exact flavour's for every handle: validity_ops_of)
    {pik_exact::launch_ops, pik_exact::path_ops, pik_exact::search_ops, pik_exact::route_ops, pik_exact::restart_ops,
     pik_exact::startpath_ops, pik_exact::globalpath_ops, pik_exact::cartesian_ops, pik_exact::polyline_ops,
     pik_exact::validity_ops, pik_exact::pathvalid_ops},
    {pik_common::launch_ops, nullptr, nullptr, pik_common::route_ops, pik_common::restart_ops, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr},
    {pik_common_goals::launch_ops, nullptr, nullptr, pik_common_goals::route_ops, pik_common_goals::restart_ops, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr},
#endif
};
// ... and the namespace each flavour's kernels carry in profiles (what the *_kernel_name entry points report)
const char* const FLAVOUR_NAMESPACE[N_FLAVOURS] = {
#if defined(PIK_STRICT)
    "pik_strict",
#else
    "pik", "pik_exact", "pik_common", "pik_common_goals",
#endif
};

template <class Ops>
const Ops* ops_at(Flavour f, Family family, int dof) {
    const OpsLookup lookup = OPS_TABLE[f][family];
    return lookup ? static_cast<const Ops*>(lookup(dof)) : nullptr;
}

int check_solver(const pikamd_solver* s) {
    if (!s) return fail(PIKAMD_EINVAL, "solver handle is NULL");
    return 0;
}

// the kernels of a handle: Denavit-Hartenberg (product arithmetic) unless the chain needs the literal ones
[[maybe_unused]] bool needs_literal(const pikamd_solver* s) {
    bool f = s->opt.exact || s->chain.float_mask != 0u || s->chain.n_mimic != 0; // (option arithmetic = exact, a floating or a mimic joint)
    for (int k = 1; k < s->n_tips; ++k) f = f || s->more[k - 1].float_mask != 0u || s->more[k - 1].n_mimic != 0;
    return f;
}
// ... and for a gradient step: the Denavit-Hartenberg kernels' probes (pik_math.hpp probe_joint) take the arcsine of
// a half-angle difference as a 4-term series, exact to rounding for gd_step_size <= 1e-2 and 1e-12 .. 1e-4 of the
// gradient off at 0.1 .. 1 (tests/test_gpu_step_accuracy.py).  A larger step is served by the literal kernels, which
// take the central differences as the reference does.  (Measured: an exact arcsine inside probe_joint -- the
// arctangent form behind a ParamsK flag -- grew the spilled scalar registers of 10 of the 44 general kernels of
// lengths 2 and 3 past profiles/r06_kernel_resources.csv, e.g. memetic_kernel<2,2,false,1> 192 -> 210 and
// gd_step_kernel<3,false> 54 -> 62; loading the flag at its use, keying it on line_delta or selecting by |x| grew
// them as well, and a non-inlined arcsine added 32 bytes of scratch per lane.)
[[maybe_unused]] bool needs_literal(const pikamd_solver* s, const pikamd_params* p) {
    return needs_literal(s) || (p && p->gd_step_size > 1.0e-2);
}

// Does this call have the common configuration (pik_math.hpp PIK_COMMON)?  Chain: every variable a bounded
// revolute joint, no general Denavit-Hartenberg step -- on every tip's path; parameters: both pose-cost terms
// on, the line-search angle addition applicable, and for the memetic solver four elites and one species.  (Two
// flavours of it: joint goals compiled out -- the default parameters -- and left in.)
[[maybe_unused]] bool common_eligible(const pikamd_solver* s, const pikamd_params* p, const pik::ParamsK& pk) {
    if (!s->opt.specialised || needs_literal(s)) return false;
    const uint32_t all = (s->chain.dof >= 32) ? ~0u : ((1u << s->chain.dof) - 1u);
    auto chain_ok = [&](const pik::ChainHost& c) {
        return c.prismatic_mask == 0u && c.dh_general_mask == 0u && c.bounded_mask == all;
    };
    if (!chain_ok(s->chain)) return false;
    for (int k = 1; k < s->n_tips; ++k)
        if (!chain_ok(s->more[k - 1])) return false;
    if (pk.line_delta == 0 || !(pk.pos_scale > 0.0) || !(pk.rot_scale > 0.0)) return false;
    if (p->mode == 0 && (pk.elites != 4 || p->memetic_num_threads > 1)) return false;
    return true;
}

// THE flavour of a call: everything that picks kernels or reports their name asks here.  pk: the call's converted
// parameters -- or null, for a call the common flavours never serve (the parity hooks, paths, searches) or whose
// parameters do not convert.
//
// The common flavours are asked for first, the literal kernels second.  The order does not matter: a call cannot
// qualify for both.  common_eligible requires pk.line_delta != 0, which make_params_k (pik_host.hpp) sets only for
// gd_step_size <= 1e-3; needs_literal(s, p) beyond needs_literal(s) -- which common_eligible excludes itself -- asks
// for gd_step_size > 1e-2.  So common_eligible implies !needs_literal(s, p) as long as the first threshold is not
// above the second (tests/test_build_cpu.py reads both from the sources and holds them to that).
Flavour flavour_of(const pikamd_solver* s, const pikamd_params* p, const pik::ParamsK* pk) {
#if defined(PIK_STRICT)
    (void)s, (void)p, (void)pk;
    return FL_HOME;
#else
    if (pk && common_eligible(s, p, *pk)) return pk->goal_mask != 0 ? FL_COMMON_GOALS : FL_COMMON;
    return needs_literal(s, p) ? FL_EXACT : FL_HOME;
#endif
}
// is it one of the common-configuration flavours; the flavour that serves the call where those have no kernels (a
// length built as a stub -- a path or a search never asks for them); does it run the exact flavours' kernel variants
bool is_common(Flavour f) {
#if defined(PIK_STRICT)
    (void)f;
    return false;
#else
    return f == FL_COMMON || f == FL_COMMON_GOALS;
#endif
}
Flavour unspecialised(Flavour f) { return is_common(f) ? FL_HOME : f; }
bool is_exact(Flavour f) { return pik::EXACT_FLAVOUR || (f != FL_HOME && !is_common(f)); }

// the kernels of the parity hooks (no ParamsK: never the common flavours) ...
const pik::LaunchOps* ops_of(const pikamd_solver* s, const pikamd_params* p = nullptr) {
    return ops_at<pik::LaunchOps>(flavour_of(s, p, nullptr), FAM_LAUNCH, s->chain.dof);
}
// ... and of one solve call
const pik::LaunchOps* solve_ops_of(const pikamd_solver* s, const pikamd_params* p, const pik::ParamsK& pk) {
    const Flavour f = flavour_of(s, p, &pk);
    if (const pik::LaunchOps* o = ops_at<pik::LaunchOps>(f, FAM_LAUNCH, s->chain.dof)) return o;
    return ops_at<pik::LaunchOps>(unspecialised(f), FAM_LAUNCH, s->chain.dof);
}

// The routed launcher of one solve call (pik_route.hpp: the regime of every pass chosen on the device), in the
// flavour solve_ops_of picks -- or null: the call is launch_solve's.  Routed are memetic calls on one tip frame with
// one species, nothing forced (lanes per elite, their schedule, the regime) and the option device_regime on; whether
// the call has a compaction pass to route the launcher finds out itself (RouteCtx::served).  The verification library
// has no routed launcher.
const pik::RouteOps* route_ops_of(const pikamd_solver* s, const pikamd_params* p, const pik::ParamsK& pk) {
    const pik::SolverOptions& o = s->opt;
    if (!ext_of(s)->device_regime || p->mode != 0 || s->n_tips != 1 || p->memetic_num_threads > 1 || o.lpe != 0 ||
        o.n_sched != 0 || o.regime != 0)
        return nullptr;
    return ops_at<pik::RouteOps>(flavour_of(s, p, &pk), FAM_ROUTE, s->chain.dof);
}

// one solve call: the routed launcher where the call is of its kind, launch_solve otherwise
int run_solve(pikamd_solver* s, const pikamd_params* p, const pik::ParamsK& pk, pik::BatchRecord* rec, int n,
              unsigned long long rng_seed, hipStream_t stream, int slot) {
    SolverExt* x = ext_of(s);
    if (const pik::RouteOps* r = route_ops_of(s, p, pk)) {
        pik::RouteCtx ctx;
        ctx.threshold = x->regime_threshold;
        if (int rc = r->solve(s, p, pk, rec, n, rng_seed, stream, slot, &ctx)) return rc;
        if (ctx.served) {
            x->routed_passes[slot] = ctx.n_passes;
            return 0;
        }
    }
    x->routed_passes[slot] = -1;
    return solve_ops_of(s, p, pk)->solve(s, p, pk, rec, n, rng_seed, stream, slot, false);
}

int no_kernels(int dof) {
    return fail(PIKAMD_EUNSUPPORTED, "dof %d: kernels are instantiated for 1..16", dof);
}

// the waypoint-path kernels of a call, the restart-search kernels of a call: the flavour ops_of picks (a call with the
// common configuration: the general one) ...
const pik::PathOps* path_ops_of(const pikamd_solver* s, const pikamd_params* p) {
    return ops_at<pik::PathOps>(flavour_of(s, p, nullptr), FAM_PATH, s->chain.dof);
}
const pik::SearchOps* search_ops_of(const pikamd_solver* s, const pikamd_params* p) {
    return ops_at<pik::SearchOps>(flavour_of(s, p, nullptr), FAM_SEARCH, s->chain.dof);
}
const pik::StartPathOps* startpath_ops_of(const pikamd_solver* s, const pikamd_params* p) {
    return ops_at<pik::StartPathOps>(flavour_of(s, p, nullptr), FAM_STARTPATH, s->chain.dof);
}
// (the tail kernels of pikamd_search_global_paths: they walk in local mode, so the flavour is a path call's)
const pik::GlobalPathOps* globalpath_ops_of(const pikamd_solver* s, const pikamd_params* p) {
    return ops_at<pik::GlobalPathOps>(flavour_of(s, p, nullptr), FAM_GLOBALPATH, s->chain.dof);
}
// ... and the restart launcher of a global-mode call (pik_restart.hpp), in the flavour solve_ops_of picks
const pik::RestartOps* restart_ops_of(const pikamd_solver* s, const pikamd_params* p, const pik::ParamsK& pk) {
    return ops_at<pik::RestartOps>(flavour_of(s, p, &pk), FAM_RESTART, s->chain.dof);
}

size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

// The approximate-solution gate of a search call on `slot`: on when the handle has one and the call sets
// return_approximate_solution (src/pick_ik_plugin.cpp:222).  Then the slot's copy of p' (gate_params_k) is made current,
// by upload_consts' rule: nothing is copied when the slot holds the same bytes, and when they change the slot's previous
// stream is drained first and the copy is complete before the call goes on.
constexpr size_t GATE_PARAMS_STRIDE = 256;
static_assert(sizeof(pik::ParamsK) <= GATE_PARAMS_STRIDE, "gate parameters slot too small");
int gate_for_call(pikamd_solver* s, const pik::ParamsK& pk, int slot, hipStream_t st, int* on, double* joint,
                  const pik::ParamsK** dev) {
    SolverExt* x = ext_of(s);
    *on = (x->gate_set && pk.approx) ? 1 : 0;
    *joint = x->gate.joint_threshold;
    *dev = nullptr;
    if (!*on) return 0;
    if (int rc = x->gate_params_dev.ensure(GATE_PARAMS_STRIDE * (size_t)pik::N_SLOTS)) return rc;
    char* d = (char*)x->gate_params_dev.p + GATE_PARAMS_STRIDE * (size_t)slot;
    const pik::ParamsK want = pik::gate_params_k(pk, x->gate.cost_threshold);
    if (!x->gate_params_valid[slot] || std::memcmp(&x->gate_params_host[slot], &want, sizeof want) != 0) {
        if (s->consts_valid[slot]) HIP_TRY(hipStreamSynchronize(s->consts_stream[slot]));
        x->gate_params_valid[slot] = false;
        std::memcpy(&x->gate_params_host[slot], &want, sizeof want);
        HIP_TRY(hipMemcpyAsync(d, &x->gate_params_host[slot], sizeof want, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        x->gate_params_valid[slot] = true;
    }
    *dev = reinterpret_cast<const pik::ParamsK*>(d);
    return 0;
}

// The kernels of the sphere validity test: the exact flavour's in the product library, whatever serves the handle's
// solves (the verification library: its own) -- one arithmetic for every handle.
const pik::ValidityOps* validity_ops_of(const pikamd_solver* s) {
#if defined(PIK_STRICT)
    return ops_at<pik::ValidityOps>(FL_HOME, FAM_VALIDITY, s->chain.dof);
#else
    return ops_at<pik::ValidityOps>(FL_EXACT, FAM_VALIDITY, s->chain.dof);
#endif
}

// what the test cannot walk: several tip frames, a floating joint, mimic joints (they may be set after the model)
int validity_chain_ok(const pikamd_solver* s, const char* who) {
    if (s->n_tips != 1) return fail(PIKAMD_EUNSUPPORTED, "%s: the validity model is for handles with one tip frame", who);
    if ((s->chain.float_mask | s->chain.skip_mask) != 0u)
        return fail(PIKAMD_EUNSUPPORTED, "%s: the validity model does not know floating joints", who);
    if (s->chain.n_mimic != 0) return fail(PIKAMD_EUNSUPPORTED, "%s: the validity model does not know mimic joints", who);
    return 0;
}

// The validity step of a global-mode search call: the handle's model, or null ops where it has none.
int validity_for_call(pikamd_solver* s, const char* who, const pik::ValidityOps** ops) {
    *ops = nullptr;
    if (!ext_of(s)->validity_set) return 0;
    if (int rc = validity_chain_ok(s, who)) return rc;
    *ops = validity_ops_of(s);
    return *ops ? 0 : no_kernels(s->chain.dof);
}

// The validity step of a path call that starts from a joint state (pikamd_set_path_validity): the kernels of
// pik_pathvalid.hpp in the flavour of the validity test, or null ops where the switch is off or the handle has no model.
int path_validity_for_call(pikamd_solver* s, const char* who, const pik::PathValidOps** ops) {
    *ops = nullptr;
    if (!ext_of(s)->path_validity || !ext_of(s)->validity_set) return 0;
    if (int rc = validity_chain_ok(s, who)) return rc;
#if defined(PIK_STRICT)
    *ops = ops_at<pik::PathValidOps>(FL_HOME, FAM_PATHVALID, s->chain.dof);
#else
    *ops = ops_at<pik::PathValidOps>(FL_EXACT, FAM_PATHVALID, s->chain.dof);
#endif
    return *ops ? 0 : no_kernels(s->chain.dof);
}

// `reached` of a path call for the validity step to read: the caller's array, or the slot's scratch, which grows only
// past the largest earlier call on the slot
int path_validity_reached(pikamd_solver* s, int slot, int64_t P, int32_t* callers, int32_t** out) {
    *out = callers;
    if (callers) return 0;
    pik::DevBuf& buf = ext_of(s)->pathvalid_rows[slot];
    if (int rc = buf.ensure(sizeof(int32_t) * (size_t)P)) return rc;
    *out = (int32_t*)buf.p;
    return 0;
}

} // namespace

extern "C" {

void pikamd_default_params(pikamd_params* p) {
    if (!p) return;
    // src/pick_ik_parameters.yaml defaults
    p->mode = 0;
    p->gd_step_size = 0.0001;
    p->gd_max_iters = 100;
    p->gd_min_cost_delta = 1.0e-12;
    p->position_threshold = 0.001;
    p->orientation_threshold = 0.001;
    p->cost_threshold = 0.001;
    p->position_scale = 1.0;
    p->rotation_scale = 0.5;
    p->center_joints_weight = 0.0;
    p->avoid_joint_limits_weight = 0.0;
    p->minimal_displacement_weight = 0.0;
    p->stop_optimization_on_valid_solution = 1;
    p->memetic_num_threads = 1;
    p->memetic_stop_on_first_solution = 1;
    p->memetic_population_size = 16;
    p->memetic_elite_size = 4;
    p->memetic_wipeout_fitness_tol = 0.00001;
    p->memetic_max_generations = 100;
    p->memetic_gd_max_iters = 25;
    p->return_approximate_solution = 0;
}

const char* pikamd_last_error(void) { return pik::error_buffer(); }

const char* pikamd_version(void) { return "pick_ik_amd 0.3.0 (gfx950)"; }

static int32_t create_solver(const pik::ChainHost* chains, int n_tips, int32_t device_ordinal,
                             pikamd_solver** out) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1)
        return fail(PIKAMD_ENODEVICE, "no HIP device available (this library has no CPU path)");
    if (device_ordinal < 0 || device_ordinal >= count)
        return fail(PIKAMD_EINVAL, "device_ordinal %d out of range [0, %d)", device_ordinal, count);
    if (!ops_at<pik::LaunchOps>(FL_HOME, FAM_LAUNCH, chains[0].dof)) return no_kernels(chains[0].dof);
    HIP_TRY(hipSetDevice(device_ordinal));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_ordinal));
    pikamd_solver* s = new (std::nothrow) SolverExt();
    if (!s) return fail(PIKAMD_EHIP, "out of host memory");
    s->device = device_ordinal;
    s->num_cu = prop.multiProcessorCount;
    s->chain = chains[0];
    s->n_tips = n_tips;
    for (int k = 1; k < n_tips; ++k) s->more[k - 1] = chains[k];
    const size_t table_bytes = sizeof(pik::BatchRecord) * PIKAMD_MAX_BATCHES * pik::TABLE_RING;
    // (the counter blocks of the slots + the routed launcher's variant counters, loads and records behind them)
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->counters), pik::COUNTERS_BYTES);
    if (e == hipSuccess) e = hipMemset(s->counters, 0, pik::COUNTERS_BYTES);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->consts_dev), pik::CONSTS_STRIDE * pik::N_SLOTS);
    if (e == hipSuccess)
        e = hipHostMalloc(reinterpret_cast<void**>(&s->consts_host), pik::CONSTS_STRIDE * pik::N_SLOTS, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->tables_dev), table_bytes);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&s->tables_host), table_bytes, hipHostMallocDefault);
    for (int i = 0; i < pik::TABLE_RING && e == hipSuccess; ++i)
        e = hipEventCreateWithFlags(&s->table_event[i], hipEventDisableTiming);
    if (e != hipSuccess) {
        pikamd_destroy(s);
        return fail(PIKAMD_EHIP, "device allocation failed: %s", hipGetErrorString(e));
    }
    for (auto& j : s->jobs) j.host.pinned_host = true;
    *out = s;
    return 0;
}

int32_t pikamd_create(const pikamd_chain* chain, int32_t device_ordinal, pikamd_solver** out) {
    if (!out) return fail(PIKAMD_EINVAL, "out is NULL");
    *out = nullptr;
    pik::ChainHost ch;
    if (const char* msg = pik::build_chain(chain, ch)) return fail(PIKAMD_EINVAL, "%s", msg);
    if (int rc = create_solver(&ch, 1, device_ordinal, out)) return rc;
    for (int j = 0; chain->joint_type && j < chain->dof; ++j)
        if (chain->joint_type[j] == PIKAMD_JOINT_PLANAR_X || chain->joint_type[j] == PIKAMD_JOINT_PLANAR_Y)
            ext_of(*out)->planar_xy_mask |= 1u << j;
    return 0;
}

int32_t pikamd_create_multi(const pikamd_multi_chain* chain, int32_t device_ordinal,
                            pikamd_solver** out) {
    if (!out) return fail(PIKAMD_EINVAL, "out is NULL");
    *out = nullptr;
    if (!chain || !chain->tips) return fail(PIKAMD_EINVAL, "multi-tip chain is NULL");
    if (chain->n_tips < 1 || chain->n_tips > PIKAMD_MAX_TIPS)
        return fail(PIKAMD_EINVAL, "n_tips %d out of range [1, %d]", chain->n_tips, PIKAMD_MAX_TIPS);
    if (!chain->qmin || !chain->qmax) return fail(PIKAMD_EINVAL, "chain has NULL arrays");
    std::vector<pik::ChainHost> ch((size_t)chain->n_tips); // (fresh: build_chain accumulates flag bits)
    uint32_t used = 0;
    for (int k = 0; k < chain->n_tips; ++k) {
        if (const char* msg = pik::build_tip_chain(chain, k, ch[k])) return fail(PIKAMD_EINVAL, "tip %d: %s", k, msg);
        used |= ch[k].active_mask;
    }
    // every variable must move some tip (get_active_variable_indices: the union over the tips)
    if (used != ((chain->dof >= 32) ? ~0u : ((1u << chain->dof) - 1u)))
        return fail(PIKAMD_EINVAL, "a variable is on no tip's path");
    return create_solver(ch.data(), chain->n_tips, device_ordinal, out);
}

int32_t pikamd_urdf_extract(const char* urdf_xml, const char* base_link, const char* const* tip_links,
                            int32_t n_tips, pikamd_urdf_model* out) {
    if (!out) return fail(PIKAMD_EINVAL, "out is NULL");
    const std::string err = pik::urdf::extract(urdf_xml, base_link, tip_links, n_tips, *out);
    if (!err.empty()) return fail(PIKAMD_EINVAL, "%s", err.c_str());
    return 0;
}

int32_t pikamd_create_from_urdf(const char* urdf_xml, const char* base_link, const char* const* tip_links,
                                int32_t n_tips, int32_t device_ordinal, pikamd_solver** out) {
    if (!out) return fail(PIKAMD_EINVAL, "out is NULL");
    *out = nullptr;
    auto m = std::make_unique<pikamd_urdf_model>();
    if (int rc = pikamd_urdf_extract(urdf_xml, base_link, tip_links, n_tips, m.get())) return rc;
    if (m->n_tips == 1) {
        const auto& t = m->tips[0];
        pikamd_chain c{m->dof, &t.origin_xyz_rpy[0][0], &t.axis[0][0], t.joint_type, t.tip_xyz_rpy,
                       m->qmin,  m->qmax,               m->vmax,       m->bounded};
        if (int rc = pikamd_create(&c, device_ordinal, out)) return rc;
        if (m->n_mimic)
            if (int rc = pikamd_set_mimic_joints(*out, m->n_mimic, m->mimic)) {
                pikamd_destroy(*out);
                *out = nullptr;
                return rc;
            }
        return 0;
    }
    pikamd_tip tips[PIKAMD_MAX_TIPS];
    for (int k = 0; k < m->n_tips; ++k) {
        const auto& t = m->tips[k];
        tips[k] = pikamd_tip{t.n_joints, t.variable, &t.origin_xyz_rpy[0][0], &t.axis[0][0], t.joint_type, t.tip_xyz_rpy};
    }
    pikamd_multi_chain c{m->dof, m->n_tips, tips, m->qmin, m->qmax, m->vmax, m->bounded};
    if (int rc = pikamd_create_multi(&c, device_ordinal, out)) return rc;
    if (m->n_mimic)
        if (int rc = pikamd_set_mimic_joints(*out, m->n_mimic, m->mimic)) {
            pikamd_destroy(*out);
            *out = nullptr;
            return rc;
        }
    return 0;
}

int32_t pikamd_n_tips(const pikamd_solver* s) { return s ? s->n_tips : 0; }

int32_t pikamd_set_mimic_joints(pikamd_solver* s, int32_t n, const pikamd_mimic_joint* joints) {
    if (int rc = check_solver(s)) return rc;
    if (n < 0 || (n > 0 && !joints)) return fail(PIKAMD_EINVAL, "bad arguments");
    pik::ChainHost saved[PIKAMD_MAX_TIPS];
    for (int k = 0; k < s->n_tips; ++k) saved[k] = k == 0 ? s->chain : s->more[k - 1];
    auto path = [&](int k) -> pik::ChainHost& { return k == 0 ? s->chain : s->more[k - 1]; };
    for (int k = 0; k < s->n_tips; ++k) pik::clear_mimic_joints(path(k));
    for (int i = 0; i < n; ++i) {
        const pikamd_mimic_joint& m = joints[i];
        const char* msg = (m.tip < 0 || m.tip >= s->n_tips) ? "mimic joint: tip out of range" : pik::add_mimic_joint(path(m.tip), m);
        if (!msg && s->n_tips > 1) { // the variables it names must lie on that tip's path
            const uint32_t act = path(m.tip).active_mask;
            if (!((act >> m.master_variable) & 1u) || (m.after_variable >= 0 && !((act >> m.after_variable) & 1u)))
                msg = "mimic joint: master_variable / after_variable is not on that tip's path";
        }
        if (msg) {
            for (int k = 0; k < s->n_tips; ++k) path(k) = saved[k];
            return fail(PIKAMD_EINVAL, "%s", msg);
        }
    }
    // a different chain: what the self test found out about the old one no longer holds
    s->self_tested.clear();
    s->opt.disabled_lanes = 0;
    s->opt.disabled_lanes_exact = 0;
    return 0;
}

void pikamd_destroy(pikamd_solver* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    if (s->counters) (void)hipFree(s->counters);
    if (s->consts_dev) (void)hipFree(s->consts_dev);
    if (s->consts_host) (void)hipHostFree(s->consts_host);
    if (s->tables_dev) (void)hipFree(s->tables_dev);
    if (s->tables_host) (void)hipHostFree(s->tables_host);
    for (auto& ev : s->table_event)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : s->slot_event)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& b : s->stage) b.release();
    for (auto& b : s->slot_state) b.release();
    for (auto& b : s->slot_soa) b.release();
    for (auto& b : ext_of(s)->search_rows) b.release();
    for (auto& b : ext_of(s)->restart_rows) b.release();
    for (auto& b : ext_of(s)->startpath_rows) b.release();
    for (auto& b : ext_of(s)->cartesian_goals) b.release();
    for (auto& b : ext_of(s)->polyline_rows) b.release();
    for (auto& b : ext_of(s)->globalpath_rows) b.release();
    ext_of(s)->gate_params_dev.release();
    ext_of(s)->validity_dev.release();
    for (auto& b : ext_of(s)->pathvalid_rows) b.release();
    for (auto& j : s->jobs) {
        j.dev.release();
        j.host.release();
        if (j.stream) (void)hipStreamDestroy(j.stream);
    }
    delete ext_of(s);
}

int32_t pikamd_variables(const pikamd_solver* s, double* out) {
    if (int rc = check_solver(s)) return rc;
    if (!out) return fail(PIKAMD_EINVAL, "out is NULL");
    for (int j = 0; j < s->chain.dof; ++j) {
        out[7 * j + 0] = s->chain.qmin[j];
        out[7 * j + 1] = s->chain.qmax[j];
        out[7 * j + 2] = s->chain.mid[j];
        out[7 * j + 3] = s->chain.hspan[j];
        out[7 * j + 4] = s->chain.vrcp[j];
        out[7 * j + 5] = s->chain.mdf[j];
        out[7 * j + 6] = ((s->chain.bounded_mask >> j) & 1u) ? 1.0 : 0.0;
    }
    return 0;
}

int32_t pikamd_fk_batch_device(pikamd_solver* s, int64_t n, const double* d_q, double* d_pos_quat,
                               void* stream) {
    if (int rc = check_solver(s)) return rc;
    if (n < 0 || (n > 0 && (!d_q || !d_pos_quat))) return fail(PIKAMD_EINVAL, "bad arguments");
    HIP_TRY(hipSetDevice(s->device));
    return ops_of(s)->fk(s, n, d_q, d_pos_quat, (hipStream_t)stream);
}

int32_t pikamd_fk_batch(pikamd_solver* s, int64_t n, const double* q, double* pos_quat) {
    if (int rc = check_solver(s)) return rc;
    if (n < 0 || (n > 0 && (!q || !pos_quat))) return fail(PIKAMD_EINVAL, "bad arguments");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(s->device));
    const size_t d = (size_t)s->chain.dof;
    if (int rc = s->stage[0].ensure(sizeof(double) * d * (size_t)n)) return rc;
    if (int rc = s->stage[1].ensure(sizeof(double) * 7 * (size_t)s->n_tips * (size_t)n)) return rc;
    HIP_TRY(hipMemcpy(s->stage[0].p, q, sizeof(double) * d * (size_t)n, hipMemcpyHostToDevice));
    if (int rc = pikamd_fk_batch_device(s, n, (const double*)s->stage[0].p, (double*)s->stage[1].p, nullptr))
        return rc;
    HIP_TRY(hipMemcpy(pos_quat, s->stage[1].p, sizeof(double) * 7 * (size_t)s->n_tips * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

int32_t pikamd_cost_batch(pikamd_solver* s, const pikamd_params* p, int64_t n,
                          const double* goal_pos_quat, const double* seed, const double* q,
                          double* cost, int32_t* is_solution) {
    if (int rc = check_solver(s)) return rc;
    pik::ParamsK pk;
    if (!p) return fail(PIKAMD_EINVAL, "params is NULL");
    if (const char* msg = pik::make_params_k(p, pk)) {
        // the memetic-only constraints do not apply to the cost hooks
        pikamd_params q2 = *p;
        q2.mode = 1;
        if (const char* m2 = pik::make_params_k(&q2, pk)) return fail(PIKAMD_EINVAL, "%s", m2);
        (void)msg;
    }
    if (n < 0 || (n > 0 && (!goal_pos_quat || !seed || !q))) return fail(PIKAMD_EINVAL, "bad arguments");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(s->device));
    const size_t d = (size_t)s->chain.dof, N = (size_t)n;
    if (int rc = s->stage[0].ensure(sizeof(double) * 7 * (size_t)s->n_tips * N)) return rc;
    if (int rc = s->stage[1].ensure(sizeof(double) * d * N)) return rc;
    if (int rc = s->stage[2].ensure(sizeof(double) * d * N)) return rc;
    if (int rc = s->stage[3].ensure(sizeof(double) * N)) return rc;
    if (int rc = s->stage[4].ensure(sizeof(int) * N)) return rc;
    HIP_TRY(hipMemcpy(s->stage[0].p, goal_pos_quat, sizeof(double) * 7 * (size_t)s->n_tips * N, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->stage[1].p, seed, sizeof(double) * d * N, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->stage[2].p, q, sizeof(double) * d * N, hipMemcpyHostToDevice));
    if (int rc = ops_of(s)->cost(s, pk, n, (const double*)s->stage[0].p, (const double*)s->stage[1].p,
                                 (const double*)s->stage[2].p, cost ? (double*)s->stage[3].p : nullptr,
                                 is_solution ? (int*)s->stage[4].p : nullptr, nullptr))
        return rc;
    if (cost) HIP_TRY(hipMemcpy(cost, s->stage[3].p, sizeof(double) * N, hipMemcpyDeviceToHost));
    if (is_solution) HIP_TRY(hipMemcpy(is_solution, s->stage[4].p, sizeof(int) * N, hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

int32_t pikamd_gd_step_batch(pikamd_solver* s, const pikamd_params* p, int64_t n,
                             const double* goal_pos_quat, const double* seed, double* local,
                             double* best, double* local_cost, double* best_cost,
                             double* gradient, int32_t* improved) {
    if (int rc = check_solver(s)) return rc;
    pik::ParamsK pk;
    pikamd_params q2;
    if (!p) return fail(PIKAMD_EINVAL, "params is NULL");
    q2 = *p;
    q2.mode = 1;
    if (const char* msg = pik::make_params_k(&q2, pk)) return fail(PIKAMD_EINVAL, "%s", msg);
    if (n < 0 || (n > 0 && (!goal_pos_quat || !seed || !local || !best || !local_cost || !best_cost || !gradient)))
        return fail(PIKAMD_EINVAL, "bad arguments");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(s->device));
    const size_t d = (size_t)s->chain.dof, N = (size_t)n;
    const size_t sz[8] = {sizeof(double) * 7 * (size_t)s->n_tips * N, sizeof(double) * d * N, sizeof(double) * d * N,
                          sizeof(double) * d * N, sizeof(double) * N,     sizeof(double) * N,
                          sizeof(double) * d * N, sizeof(int) * N};
    for (int i = 0; i < 8; ++i)
        if (int rc = s->stage[i].ensure(sz[i])) return rc;
    HIP_TRY(hipMemcpy(s->stage[0].p, goal_pos_quat, sz[0], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->stage[1].p, seed, sz[1], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->stage[2].p, local, sz[2], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->stage[3].p, best, sz[3], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->stage[4].p, local_cost, sz[4], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->stage[5].p, best_cost, sz[5], hipMemcpyHostToDevice));
    if (int rc = ops_of(s, p)->step(s, pk, n, (const double*)s->stage[0].p, (const double*)s->stage[1].p,
                                 (double*)s->stage[2].p, (double*)s->stage[3].p, (double*)s->stage[4].p,
                                 (double*)s->stage[5].p, (double*)s->stage[6].p, (int*)s->stage[7].p, nullptr))
        return rc;
    HIP_TRY(hipMemcpy(local, s->stage[2].p, sz[2], hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(best, s->stage[3].p, sz[3], hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(local_cost, s->stage[4].p, sz[4], hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(best_cost, s->stage[5].p, sz[5], hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(gradient, s->stage[6].p, sz[6], hipMemcpyDeviceToHost));
    if (improved) HIP_TRY(hipMemcpy(improved, s->stage[7].p, sz[7], hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}


// ---- solvers ---------------------------------------------------------------------------------

// validates the records of a call and converts them (device pointers) for the launch
static int make_records(const pikamd_solver* s, int32_t n_batches, const pikamd_batch* batches,
                        pik::BatchRecord* rec, long long* total) {
    if (n_batches < 0 || n_batches > PIKAMD_MAX_BATCHES)
        return fail(PIKAMD_EINVAL, "n_batches %d out of range [0, %d]", n_batches, PIKAMD_MAX_BATCHES);
    if (n_batches > 0 && !batches) return fail(PIKAMD_EINVAL, "batches is NULL");
    long long sum = 0;
    int n = 0;
    for (int k = 0; k < n_batches; ++k) {
        const pikamd_batch& b = batches[k];
        if (b.B < 0 || (b.B > 0 && (!b.goal_pos_quat || !b.seed || !b.solution || !b.status)))
            return fail(PIKAMD_EINVAL, "batch %d: bad arguments", k);
        if (b.B == 0) continue; // (an empty batch takes no part in the call)
        pik::BatchRecord& r = rec[n++];
        r.start = 0;
        r.B = b.B;
        r.goal = b.goal_pos_quat;
        r.seed = b.seed;
        r.guess = b.initial_guess ? b.initial_guess : b.seed;
        r.problem_offset = b.problem_offset;
        r.solution = b.solution;
        r.status = b.status;
        r.cost = b.final_cost;
        r.stats = b.stats;
        r.completed = b.completed;
        sum += b.B;
    }
    (void)s;
    *total = sum;
    return n;
}

// option joint_layout = soa: [dof][B] <-> [B][dof] (180 bytes per problem against ~5 Mflop of solving: the
// kernels keep the one layout they gather a problem's vector from with a single cache line)
__global__ void pik_joint_layout_kernel(const double* __restrict__ in, double* __restrict__ out, long long B, int D,
                                        int to_aos) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * D) return;
    if (to_aos) { // out [B][D] <- in [D][B]
        const long long b = i / D;
        const int j = (int)(i - b * D);
        out[i] = in[(long long)j * B + b];
    } else { // out [D][B] <- in [B][D]
        const long long j = i / B, b = i - j * B;
        out[i] = in[b * D + j];
    }
}

static int maybe_self_test(pikamd_solver* s, const pikamd_params* p);

static int32_t solve_records(pikamd_solver* s, const pikamd_params* p, pik::BatchRecord* rec, int n,
                             uint64_t rng_seed, hipStream_t stream, int slot) {
    pik::ParamsK pk;
    if (const char* msg = pik::make_params_k(p, pk)) return fail(PIKAMD_EINVAL, "%s", msg);
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(s->device));
    if (!s->opt.soa) return run_solve(s, p, pk, rec, n, rng_seed, stream, slot);
    // joint vectors structure-of-arrays: seed / initial guess are transposed into scratch in front of the
    // kernels, the solutions out of scratch behind them, all on the call's stream
    const int D = s->chain.dof;
    size_t doubles = 0;
    for (int k = 0; k < n; ++k) {
        if (rec[k].completed)
            return fail(PIKAMD_EINVAL, "joint_layout soa: completion counters are not available (the solutions of a "
                                       "batch are in place when the stream has passed the call)");
        doubles += (size_t)rec[k].B * (size_t)D * (rec[k].guess != rec[k].seed ? 3u : 2u);
    }
    if (int rc = s->slot_soa[slot].ensure(sizeof(double) * doubles)) return rc;
    double* w = (double*)s->slot_soa[slot].p;
    double* user_solution[PIKAMD_MAX_BATCHES];
    auto move = [&](const double* in, double* out, long long B, int to_aos) -> int {
        const long long items = B * D;
        hipLaunchKernelGGL(pik_joint_layout_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, in, out, B,
                           D, to_aos);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    for (int k = 0; k < n; ++k) {
        const long long B = rec[k].B;
        const bool own_guess = rec[k].guess != rec[k].seed;
        double* sd = w;
        w += (size_t)B * D;
        if (int rc = move(rec[k].seed, sd, B, 1)) return rc;
        double* gs = sd;
        if (own_guess) {
            gs = w;
            w += (size_t)B * D;
            if (int rc = move(rec[k].guess, gs, B, 1)) return rc;
        }
        user_solution[k] = rec[k].solution;
        rec[k].seed = sd;
        rec[k].guess = gs;
        rec[k].solution = w;
        w += (size_t)B * D;
    }
    if (int rc = run_solve(s, p, pk, rec, n, rng_seed, stream, slot)) return rc;
    for (int k = 0; k < n; ++k)
        if (int rc = move(rec[k].solution, user_solution[k], rec[k].B, 0)) return rc;
    return 0;
}

int32_t pikamd_solve_batches_device(pikamd_solver* s, const pikamd_params* p, int32_t n_batches,
                                    const pikamd_batch* batches, uint64_t rng_seed, void* stream,
                                    int32_t slot) {
    if (int rc = check_solver(s)) return rc;
    if (slot < 0 || slot >= PIKAMD_MAX_SLOTS) return fail(PIKAMD_EINVAL, "slot out of range");
    // (no automatic self test here: this entry point is stream-ordered and must not block or synchronise -- it may
    //  be under stream capture.  pikamd_reserve, which a caller of this entry point runs first, carries it.)
    pik::BatchRecord rec[PIKAMD_MAX_BATCHES];
    long long total = 0;
    const int n = make_records(s, n_batches, batches, rec, &total);
    if (n < 0) return n;
    return solve_records(s, p, rec, n, rng_seed, (hipStream_t)stream, slot);
}

int32_t pikamd_solve_batch_device(pikamd_solver* s, const pikamd_params* p, int64_t B,
                                  const double* d_goal_pos_quat, const double* d_seed,
                                  uint64_t rng_seed, int64_t problem_offset, double* d_solution,
                                  int32_t* d_status, double* d_final_cost, pikamd_stats* d_stats,
                                  void* stream, int32_t slot) {
    const pikamd_batch b = {B,          d_goal_pos_quat, d_seed,       nullptr, problem_offset,
                            d_solution, d_status,        d_final_cost, d_stats, nullptr};
    return pikamd_solve_batches_device(s, p, 1, &b, rng_seed, stream, slot);
}

int32_t pikamd_reserve(pikamd_solver* s, const pikamd_params* p, int64_t B, int32_t slot, void* stream) {
    if (int rc = check_solver(s)) return rc;
    pik::ParamsK pk;
    if (const char* msg = pik::make_params_k(p, pk)) return fail(PIKAMD_EINVAL, "%s", msg);
    if (B < 0) return fail(PIKAMD_EINVAL, "bad arguments");
    if (slot < 0 || slot >= PIKAMD_MAX_SLOTS) return fail(PIKAMD_EINVAL, "slot out of range");
    if (B == 0) return 0;
    if (int rc = maybe_self_test(s, p)) return rc; // (here rather than inside the first timed call)
    HIP_TRY(hipSetDevice(s->device));
    // option joint_layout = soa: the [B][dof] copies of seed, initial guess and solution the kernels work on
    // (sized here so that no enqueue path allocates -- a grow frees, and hipFree synchronises the device)
    if (s->opt.soa)
        if (int rc = s->slot_soa[slot].ensure(sizeof(double) * (size_t)B * (size_t)s->chain.dof * 3u)) return rc;
    pik::BatchRecord rec;
    std::memset(&rec, 0, sizeof rec);
    rec.B = B;
    return solve_ops_of(s, p, pk)->solve(s, p, pk, &rec, 1, 0, (hipStream_t)stream, slot, true);
}

// Host-pointer jobs: inputs -> pinned staging -> one H2D copy, kernels, one D2H copy into pinned
// staging, all on the job's own stream; pikamd_wait copies the results out.  Jobs on different
// slots overlap their transfers and kernels.
static int32_t start_job(pikamd_solver* s, const pikamd_params* p, int32_t n_batches,
                         const pikamd_batch* batches, uint64_t rng_seed, int job) {
    if (int rc = check_solver(s)) return rc;
    if (job < 0 || job > pik::JOB_SELF_TEST) return fail(PIKAMD_EINVAL, "job out of range");
    if (job != pik::JOB_SELF_TEST)
        if (int rc = maybe_self_test(s, p)) return rc;
    pik::HostJob& J = s->jobs[job];
    if (J.pending) return fail(PIKAMD_EINVAL, "job %d is still in flight: call pikamd_wait first", job);
    pik::BatchRecord rec[PIKAMD_MAX_BATCHES];
    long long total = 0;
    const int n = make_records(s, n_batches, batches, rec, &total);
    if (n < 0) return n;
    {
        pik::ParamsK pk;
        if (const char* msg = pik::make_params_k(p, pk)) return fail(PIKAMD_EINVAL, "%s", msg);
    }
    J.n_batches = 0;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(s->device));
    if (!J.stream) HIP_TRY(hipStreamCreateWithFlags(&J.stream, hipStreamNonBlocking));
    const size_t d = (size_t)s->chain.dof, g7 = 7 * (size_t)s->n_tips;
    // layout: [inputs of every batch][outputs of every batch], 8-byte aligned pieces
    size_t off = 0;
    size_t in_goal[PIKAMD_MAX_BATCHES], in_seed[PIKAMD_MAX_BATCHES], in_guess[PIKAMD_MAX_BATCHES];
    for (int k = 0; k < n; ++k) {
        const size_t N = (size_t)rec[k].B;
        in_goal[k] = off;
        off += sizeof(double) * g7 * N;
        in_seed[k] = off;
        off += sizeof(double) * d * N;
        in_guess[k] = (rec[k].guess != rec[k].seed) ? off : in_seed[k];
        if (rec[k].guess != rec[k].seed) off += sizeof(double) * d * N;
    }
    J.in_bytes = off;
    for (int k = 0; k < n; ++k) {
        const size_t N = (size_t)rec[k].B;
        pik::HostJob::Out& o = J.outs[k];
        o.B = rec[k].B;
        o.solution = rec[k].solution;
        o.status = rec[k].status;
        o.final_cost = rec[k].cost;
        o.stats = (pikamd_stats*)rec[k].stats;
        o.off_solution = off;
        off += sizeof(double) * d * N;
        o.off_cost = off;
        off += sizeof(double) * N;
        o.off_stats = off;
        off += sizeof(pikamd_stats) * N;
        o.off_status = off;
        off += align8(sizeof(int32_t) * N);
    }
    J.out_bytes = off - J.in_bytes;
    if (int rc = J.dev.ensure(off)) return rc;
    if (int rc = J.host.ensure(off)) return rc;
    char* hb = (char*)J.host.p;
    char* db = (char*)J.dev.p;
    for (int k = 0; k < n; ++k) {
        const size_t N = (size_t)rec[k].B;
        std::memcpy(hb + in_goal[k], rec[k].goal, sizeof(double) * g7 * N);
        std::memcpy(hb + in_seed[k], rec[k].seed, sizeof(double) * d * N);
        if (in_guess[k] != in_seed[k]) std::memcpy(hb + in_guess[k], rec[k].guess, sizeof(double) * d * N);
        rec[k].goal = (const double*)(db + in_goal[k]);
        rec[k].seed = (const double*)(db + in_seed[k]);
        rec[k].guess = (const double*)(db + in_guess[k]);
        rec[k].solution = (double*)(db + J.outs[k].off_solution);
        rec[k].status = (int*)(db + J.outs[k].off_status);
        rec[k].cost = (double*)(db + J.outs[k].off_cost);
        rec[k].stats = (void*)(db + J.outs[k].off_stats);
        rec[k].completed = nullptr;
    }
    HIP_TRY(hipMemcpyAsync(db, hb, J.in_bytes, hipMemcpyHostToDevice, J.stream));
    // From here on work of this job is (or may be) in flight on its stream.  If a later enqueue fails, the
    // stream is drained before the error is returned: the job stays not-pending, and the next job must not
    // write into staging memory a copy is still reading, nor find kernels of this one still running.
    if (int rc = solve_records(s, p, rec, n, rng_seed, J.stream, pik::N_DEVICE_SLOTS + job)) {
        (void)hipStreamSynchronize(J.stream);
        return rc;
    }
    {
        const hipError_t e = hipMemcpyAsync(hb + J.in_bytes, db + J.in_bytes, J.out_bytes, hipMemcpyDeviceToHost, J.stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(J.stream);
            return fail(PIKAMD_EHIP, "result copy could not be enqueued: %s", hipGetErrorString(e));
        }
    }
    J.n_batches = n;
    J.dof = (int)d;
    J.pending = true;
    return 0;
}

int32_t pikamd_solve_batches_async(pikamd_solver* s, const pikamd_params* p, int32_t n_batches,
                                   const pikamd_batch* batches, uint64_t rng_seed, int32_t job) {
    if (job < 0 || job >= PIKAMD_MAX_HOST_JOBS - 1) // (the last job is the synchronous entry points')
        return fail(PIKAMD_EINVAL, "job out of range [0, %d)", PIKAMD_MAX_HOST_JOBS - 1);
    return start_job(s, p, n_batches, batches, rng_seed, job);
}

static int32_t wait_job(pikamd_solver* s, int job) {
    pik::HostJob& J = s->jobs[job];
    if (!J.pending) return 0;
    HIP_TRY(hipSetDevice(s->device));
    // A failed synchronise ends the job: its results are undefined and are NOT copied out, the error is
    // returned once, and the job index is free again (left pending, every later call on it failed for the life
    // of the handle).
    {
        const hipError_t e = hipStreamSynchronize(J.stream);
        J.pending = false;
        if (e != hipSuccess) return fail(PIKAMD_EHIP, "job %d: %s (its results are lost)", job, hipGetErrorString(e));
    }
    const char* hb = (const char*)J.host.p;
    const size_t d = (size_t)J.dof;
    for (int k = 0; k < J.n_batches; ++k) {
        const pik::HostJob::Out& o = J.outs[k];
        const size_t N = (size_t)o.B;
        std::memcpy(o.solution, hb + o.off_solution, sizeof(double) * d * N);
        std::memcpy(o.status, hb + o.off_status, sizeof(int32_t) * N);
        if (o.final_cost) std::memcpy(o.final_cost, hb + o.off_cost, sizeof(double) * N);
        if (o.stats) std::memcpy(o.stats, hb + o.off_stats, sizeof(pikamd_stats) * N);
    }
    return 0;
}

int32_t pikamd_wait(pikamd_solver* s, int32_t job) {
    if (int rc = check_solver(s)) return rc;
    if (job < 0 || job >= pik::N_HOST_JOBS) return fail(PIKAMD_EINVAL, "job out of range");
    return wait_job(s, job);
}

int32_t pikamd_solve_batches(pikamd_solver* s, const pikamd_params* p, int32_t n_batches,
                             const pikamd_batch* batches, uint64_t rng_seed) {
    const int job = PIKAMD_MAX_HOST_JOBS - 1;
    if (int rc = start_job(s, p, n_batches, batches, rng_seed, job)) return rc;
    return pikamd_wait(s, job);
}

int32_t pikamd_solve_batch(pikamd_solver* s, const pikamd_params* p, int64_t B,
                           const double* goal_pos_quat, const double* seed, uint64_t rng_seed,
                           int64_t problem_offset, double* solution, int32_t* status,
                           double* final_cost, pikamd_stats* stats) {
    const pikamd_batch b = {B,        goal_pos_quat, seed,       nullptr, problem_offset,
                            solution, status,        final_cost, stats,   nullptr};
    const int job = PIKAMD_MAX_HOST_JOBS - 1;
    // (a call with nothing else in flight takes the latency-greedy kernel variants: launch_solve)
    if (int rc = start_job(s, p, 1, &b, rng_seed, job)) return rc;
    return pikamd_wait(s, job);
}

int32_t pikamd_set_option(pikamd_solver* s, const char* name, const char* value) {
    if (int rc = check_solver(s)) return rc;
    if (!name) return fail(PIKAMD_EINVAL, "option name is NULL");
    const std::string n = name, v = value ? value : "";
    pik::SolverOptions& o = s->opt;
    // "a,b,c" -> ints; false on anything that is not a number
    auto ints = [](const std::string& text, char sep, std::vector<int>& out) {
        size_t i = 0;
        while (i < text.size()) {
            char* end = nullptr;
            const long x = std::strtol(text.c_str() + i, &end, 10);
            if (end == text.c_str() + i) return false;
            out.push_back((int)x);
            i = (size_t)(end - text.c_str());
            if (i < text.size()) {
                if (text[i] != sep) return false;
                ++i;
            }
        }
        return true;
    };
    if (n == "lanes_per_elite") {
        if (v.empty()) { o.lpe = 0; return 0; }
        std::vector<int> x;
        if (!ints(v, ',', x) || x.size() != 1 || !(x[0] == 0 || x[0] == 1 || x[0] == 2 || x[0] == 4 || x[0] == 8 || x[0] == 16))
            return fail(PIKAMD_EINVAL, "lanes_per_elite: expected 0 (adaptive), 1, 2, 4, 8 or 16, got '%s'", v.c_str());
        o.lpe = x[0];
        return 0;
    }
    if (n == "lanes_per_elite_schedule") { // "g0:l0,g1:l1,..." ascending generations, the first one 0
        if (v.empty()) { o.n_sched = 0; return 0; }
        int cnt = 0, from[4], of[4];
        size_t i = 0;
        while (i < v.size()) {
            const size_t comma = v.find(',', i), colon = v.find(':', i);
            const size_t end = comma == std::string::npos ? v.size() : comma;
            std::vector<int> a, b;
            if (cnt >= 4 || colon == std::string::npos || colon > end || !ints(v.substr(i, colon - i), ',', a) ||
                !ints(v.substr(colon + 1, end - colon - 1), ',', b) || a.size() != 1 || b.size() != 1 ||
                !(b[0] == 1 || b[0] == 2 || b[0] == 4 || b[0] == 8 || b[0] == 16) ||
                (cnt == 0 ? a[0] != 0 : a[0] <= from[cnt - 1]))
                return fail(PIKAMD_EINVAL, "lanes_per_elite_schedule: expected 'g0:l0,g1:l1,...' with g0 = 0, ascending "
                                           "generations and lanes in {1,2,4,8,16} (at most 4 entries), got '%s'", v.c_str());
            from[cnt] = a[0];
            of[cnt] = b[0];
            ++cnt;
            i = end + (end < v.size() ? 1 : 0);
        }
        o.n_sched = cnt;
        for (int k = 0; k < cnt; ++k) o.sched_from[k] = from[k], o.sched_of[k] = of[k];
        return 0;
    }
    if (n == "passes") { // "2,4,8" generation marks, "none", or "" = the default marks
        if (v.empty()) { o.passes_set = false; return 0; }
        std::vector<int> x;
        if (v != "none" && (!ints(v, ',', x) || x.size() > 15))
            return fail(PIKAMD_EINVAL, "passes: expected 'none' or up to 15 ascending generation marks, got '%s'", v.c_str());
        for (size_t k = 0; k < x.size(); ++k)
            if (x[k] <= 0 || (k > 0 && x[k] <= x[k - 1]))
                return fail(PIKAMD_EINVAL, "passes: marks must be positive and ascending, got '%s'", v.c_str());
        o.passes_set = true;
        o.n_marks = (int)x.size();
        for (size_t k = 0; k < x.size(); ++k) o.marks[k] = x[k];
        return 0;
    }
    if (n == "two_per_simd") {
        if (v.empty()) { o.two_per_simd = -1; return 0; }
        std::vector<int> x;
        if (!ints(v, ',', x) || x.size() != 1 || x[0] < 0)
            return fail(PIKAMD_EINVAL, "two_per_simd: expected 0, 1 or a wavefront threshold, got '%s'", v.c_str());
        o.two_per_simd = x[0];
        return 0;
    }
    if (n == "arithmetic") { // "exact" (default): the exact kernels (oracle math mode "fma"); "fast": the Denavit-Hartenberg kernels (opt-in)
#if defined(PIK_STRICT)
        if (v.empty() || v == "exact") return 0; // (the verification library is exact anyway: oracle math mode "portable")
        return fail(PIKAMD_EINVAL, "arithmetic: the verification library only has 'exact', got '%s'", v.c_str());
#else
        if (v.empty() || v == "exact") { o.exact = true; return 0; }
        if (v == "fast") { o.exact = false; return 0; }
        return fail(PIKAMD_EINVAL, "arithmetic: expected 'fast' or 'exact', got '%s'", v.c_str());
#endif
    }
    if (n == "self_test") { // "auto" (default): see maybe_self_test; "off": only when pikamd_self_test is called
        if (v.empty() || v == "auto") { o.auto_self_test = true; return 0; }
        if (v == "off") { o.auto_self_test = false; return 0; }
        return fail(PIKAMD_EINVAL, "self_test: expected 'auto' or 'off', got '%s'", v.c_str());
    }
    if (n == "specialised") { // "1" (default): the common-configuration kernels for calls that qualify; "0": never
        if (v.empty() || v == "1") { o.specialised = true; return 0; }
        if (v == "0") { o.specialised = false; return 0; }
        return fail(PIKAMD_EINVAL, "specialised: expected '0' or '1', got '%s'", v.c_str());
    }
    if (n == "shard_chunks") { // pikamd_solve_batch_sharded: host jobs per device ("" = default)
        if (v.empty()) { o.shard_chunks = 0; return 0; }
        std::vector<int> x;
        if (!ints(v, ',', x) || x.size() != 1 || x[0] < 1 || x[0] > 8)
            return fail(PIKAMD_EINVAL, "shard_chunks: expected 1..8, got '%s'", v.c_str());
        o.shard_chunks = x[0];
        return 0;
    }
    if (n == "joint_layout") { // "aos" (default): seed / initial_guess / solution are [B][dof]; "soa": [dof][B]
        if (v.empty() || v == "aos") { o.soa = false; return 0; }
        if (v == "soa") { o.soa = true; return 0; }
        return fail(PIKAMD_EINVAL, "joint_layout: expected 'aos' or 'soa', got '%s'", v.c_str());
    }
    if (n == "host_max_time" || n == "host_gd_max_time") { // seconds; "" or "0" = no limit
        double x = 0.0;
        if (!v.empty()) {
            char* end = nullptr;
            x = std::strtod(v.c_str(), &end);
            if (end == v.c_str() || *end != 0 || !(x >= 0.0) || !std::isfinite(x))
                return fail(PIKAMD_EINVAL, "%s: expected a time in seconds >= 0, got '%s'", n.c_str(), v.c_str());
        }
        (n == "host_max_time" ? o.host_max_time : o.host_gd_max_time) = x;
        return 0;
    }
    if (n == "search_schedule") { // pikamd_search_batch*: a problem's attempts one after the other or side by side
        int& sched = ext_of(s)->search_schedule;
        if (v.empty() || v == "adaptive") { sched = pik::SEARCH_ADAPTIVE; return 0; }
        if (v == "sequential") { sched = pik::SEARCH_SEQUENTIAL; return 0; }
        if (v == "parallel") { sched = pik::SEARCH_PARALLEL; return 0; }
        return fail(PIKAMD_EINVAL, "search_schedule: expected 'adaptive', 'sequential' or 'parallel', got '%s'", v.c_str());
    }
    if (n == "device_regime") { // "1" (default): the regime of a pass is chosen on the device when it starts; "0": on the host
        int x = 1;
        if (!pik::parse_device_regime(v.c_str(), &x))
            return fail(PIKAMD_EINVAL, "device_regime: expected '0' or '1', got '%s'", v.c_str());
        ext_of(s)->device_regime = x;
        return 0;
    }
    if (n == "regime_threshold") { // problems the OTHER slots hold from which a pass takes the throughput schedule ("" / 0: default)
        if (v.empty()) { ext_of(s)->regime_threshold = 0; return 0; }
        std::vector<int> x;
        if (!ints(v, ',', x) || x.size() != 1 || x[0] < 0)
            return fail(PIKAMD_EINVAL, "regime_threshold: expected a number of problems >= 0, got '%s'", v.c_str());
        ext_of(s)->regime_threshold = x[0];
        return 0;
    }
    if (n == "regime") {
        if (v.empty() || v == "adaptive") { o.regime = 0; return 0; }
        if (v == "latency") { o.regime = 1; return 0; }
        if (v == "throughput") { o.regime = 2; return 0; }
        return fail(PIKAMD_EINVAL, "regime: expected 'adaptive', 'latency' or 'throughput', got '%s'", v.c_str());
    }
    return fail(PIKAMD_EINVAL, "unknown option '%s'", n.c_str());
}

// ---- several devices ----------------------------------------------------------------------------

void pikamd_shard_bounds(int64_t total, int32_t rank, int32_t world, int64_t* lo, int64_t* hi) {
    if (world < 1) world = 1;
    if (total < 0) total = 0;
    const int64_t base = total / world, rem = total % world;
    const int64_t l = (int64_t)rank * base + (rank < rem ? rank : rem);
    if (lo) *lo = l;
    if (hi) *hi = l + base + (rank < rem ? 1 : 0);
}

int32_t pikamd_solve_batch_sharded(pikamd_solver* const* solvers, int32_t n_devices, const pikamd_params* p,
                                   int64_t B, const double* goal_pos_quat, const double* seed,
                                   const double* initial_guess, uint64_t rng_seed, int64_t problem_offset,
                                   double* solution, int32_t* status, double* final_cost, pikamd_stats* stats) {
    if (!solvers || n_devices < 1) return fail(PIKAMD_EINVAL, "no solver handles");
    if (B < 0 || (B > 0 && (!goal_pos_quat || !seed || !solution || !status))) return fail(PIKAMD_EINVAL, "bad arguments");
    for (int r = 0; r < n_devices; ++r) {
        if (!solvers[r]) return fail(PIKAMD_EINVAL, "solver handle %d is NULL", r);
        if (solvers[r]->chain.dof != solvers[0]->chain.dof || solvers[r]->n_tips != solvers[0]->n_tips)
            return fail(PIKAMD_EINVAL, "solver handle %d describes a different chain", r);
        for (int q = 0; q < r; ++q)
            if (solvers[q] == solvers[r]) return fail(PIKAMD_EINVAL, "solver handle %d is given twice", r);
    }
    if (B == 0) return 0;
    for (int r = 0; r < n_devices; ++r)
        if (solvers[r]->opt.soa)
            return fail(PIKAMD_EINVAL, "joint_layout soa: not with pikamd_solve_batch_sharded (a shard of a [dof][B] "
                                       "array is not contiguous)");
    const size_t d = (size_t)solvers[0]->chain.dof, g7 = 7 * (size_t)solvers[0]->n_tips;
    // host jobs per device: the second one's PCIe copies overlap the first one's kernels.  Measured (Panda, 1 M
    // targets, host arrays in and out): population 128: 166 / 163 / 168 / 193 / 225 ms with 1 / 2 / 3 / 4 / 8 jobs,
    // population 512: 348 / 354 / 361 / 414 / 485 ms -- every job is a call with its own long-running tail, and
    // the tails do not hide each other; option "shard_chunks" overrides
    constexpr int MAX_CHUNKS = 2;
    constexpr int64_t CHUNK_MIN = 32768;     // (no point cutting a shard finer than this)
    std::vector<int> rc((size_t)n_devices, 0);
    std::vector<std::string> msg((size_t)n_devices);
    // one host thread per device: staging copy, enqueue and wait of a shard all happen on it
    auto work = [&](int r) {
        int64_t lo = 0, hi = 0;
        pikamd_shard_bounds(B, r, n_devices, &lo, &hi);
        const int64_t n = hi - lo;
        if (n == 0) return;
        int chunks = (int)((n + CHUNK_MIN - 1) / CHUNK_MIN);
        const int max_chunks = solvers[r]->opt.shard_chunks > 0 ? solvers[r]->opt.shard_chunks : MAX_CHUNKS;
        chunks = chunks < 1 ? 1 : chunks > max_chunks ? max_chunks : chunks;
        int started = 0;
        for (int c = 0; c < chunks && rc[r] == 0; ++c) {
            int64_t clo = 0, chi = 0;
            pikamd_shard_bounds(n, c, chunks, &clo, &chi);
            const int64_t a = lo + clo;
            const pikamd_batch b = {chi - clo,
                                    goal_pos_quat + (size_t)a * g7,
                                    seed + (size_t)a * d,
                                    initial_guess ? initial_guess + (size_t)a * d : nullptr,
                                    problem_offset + a, // random streams keyed by the GLOBAL problem index
                                    solution + (size_t)a * d,
                                    status + a,
                                    final_cost ? final_cost + a : nullptr,
                                    stats ? stats + a : nullptr,
                                    nullptr};
            rc[r] = pikamd_solve_batches_async(solvers[r], p, 1, &b, rng_seed, c);
            if (rc[r] == 0) ++started;
        }
        for (int c = 0; c < started; ++c) {
            const int w = pikamd_wait(solvers[r], c);
            if (rc[r] == 0) rc[r] = w;
        }
        if (rc[r] != 0) msg[r] = pik::error_buffer(); // (thread-local: carried back to the caller below)
    };
    if (n_devices == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        th.reserve((size_t)n_devices);
        for (int r = 0; r < n_devices; ++r) th.emplace_back(work, r);
        for (auto& t : th) t.join();
    }
    for (int r = 0; r < n_devices; ++r)
        if (rc[r] != 0) return fail(rc[r], "device shard %d: %s", r, msg[r].c_str());
    return 0;
}

// ---- host cost functions (pik_host_solve.hpp) -------------------------------------------------
#if defined(PIK_STRICT)
#define PIK_HOST_SOLVE pik_strict_host_solve
#else
#define PIK_HOST_SOLVE pik_exact_host_solve
#endif
} // extern "C"
extern "C" int PIK_HOST_SOLVE(const pikamd_solver* s, const pikamd_params* p, long long B, const double* goal,
                              const double* seed, const double* guess, unsigned long long rng_seed,
                              long long problem_offset, pikamd_cost_fn cb, void* user, double* solution, int32_t* status,
                              double* final_cost, pikamd_stats* stats);
extern "C" {

int32_t pikamd_solve_batch_host(pikamd_solver* s, const pikamd_params* p, int64_t B, const double* goal_pos_quat,
                                const double* seed, const double* initial_guess, uint64_t rng_seed,
                                int64_t problem_offset, pikamd_cost_fn cost_fn, void* user, double* solution,
                                int32_t* status, double* final_cost, pikamd_stats* stats) {
    if (int rc = check_solver(s)) return rc;
    if (!p) return fail(PIKAMD_EINVAL, "params is NULL");
    if (!cost_fn)
        return fail(PIKAMD_EINVAL, "pikamd_solve_batch_host is for queries with a host cost function; without one "
                                   "use pikamd_solve_batch (the GPU)");
    if (B < 0 || (B > 0 && (!goal_pos_quat || !seed || !solution || !status))) return fail(PIKAMD_EINVAL, "bad arguments");
    if (p->mode == 0 && (p->memetic_elite_size < 1 || p->memetic_population_size <= p->memetic_elite_size))
        return fail(PIKAMD_EINVAL, "memetic_population_size must exceed memetic_elite_size >= 1");
    if (s->opt.soa)
        return fail(PIKAMD_EINVAL, "joint_layout soa: not with pikamd_solve_batch_host (its arrays are [B][dof])");
    return PIK_HOST_SOLVE(s, p, B, goal_pos_quat, seed, initial_guess, rng_seed, problem_offset, cost_fn, user, solution,
                          status, final_cost, stats);
}

// ---- self test -------------------------------------------------------------------------------
int32_t pikamd_self_test(pikamd_solver* s, const pikamd_params* p, int32_t n, uint32_t* disabled_out) {
    if (int rc = check_solver(s)) return rc;
    if (!p) return fail(PIKAMD_EINVAL, "params is NULL");
    if (n < 1 || n > 4096) return fail(PIKAMD_EINVAL, "n out of range [1, 4096]");
    // the flavour under test: the exact kernels (this library is the verification build, the option "arithmetic" =
    // exact, or a chain only they serve) or the product flavours' -- each keeps its own mask of switched-off widths
    const bool exact_now = is_exact(flavour_of(s, p, nullptr));
    auto mask_of = [exact_now](pik::SolverOptions& o) -> unsigned& { return exact_now ? o.disabled_lanes_exact : o.disabled_lanes; };
    if (disabled_out) *disabled_out = mask_of(s->opt);
    const int d = s->chain.dof, tips = s->n_tips;
    // reachable targets: joint vectors drawn inside the limits (a plain 64-bit LCG: nothing here needs to
    // be reproducible across machines), their forward kinematics as goals, the range midpoints as seeds
    std::vector<double> q((size_t)n * d), goal((size_t)n * 7 * tips), seed((size_t)n * d);
    unsigned long long x = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < d; ++j) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            const double u = (double)(x >> 11) * (1.0 / 9007199254740992.0);
            const bool bounded = (s->chain.bounded_mask >> j) & 1u;
            const double lo = bounded ? s->chain.qmin[j] : -3.0, hi = bounded ? s->chain.qmax[j] : 3.0;
            q[(size_t)i * d + j] = lo + (hi - lo) * u;
            seed[(size_t)i * d + j] = bounded ? 0.5 * (lo + hi) : 0.0;
        }
    if (int rc = pikamd_fk_batch(s, n, q.data(), goal.data())) return rc;
    struct Out {
        std::vector<double> sol, cost;
        std::vector<int32_t> st;
        std::vector<pikamd_stats> stats;
    };
    pik::SolverOptions saved = s->opt;
    auto run = [&](int lanes, bool passes, bool occ2, Out& o) -> int {
        s->opt = saved;
        s->opt.soa = false; // (the test's own arrays are [n][dof])
        s->opt.lpe = lanes;
        s->opt.n_sched = 0;
        s->opt.passes_set = true;
        s->opt.n_marks = 0;
        if (passes) {
            const int m[] = {1, 2, 3, 4, 7, 11, 16, 24, 40, 64};
            for (int v : m) s->opt.marks[s->opt.n_marks++] = v;
        }
        s->opt.two_per_simd = occ2 ? 1 : 0;
        s->opt.force_occ2 = occ2; // (whatever the call's size)
        s->opt.regime = 1;
        o.sol.assign((size_t)n * d, 0.0);
        o.cost.assign((size_t)n, 0.0);
        o.st.assign((size_t)n, 0);
        o.stats.assign((size_t)n, pikamd_stats{});
        const pikamd_batch b = {n,            goal.data(), seed.data(),   nullptr,        0,
                                o.sol.data(), o.st.data(), o.cost.data(), o.stats.data(), nullptr};
        int rc = start_job(s, p, 1, &b, 12345, pik::JOB_SELF_TEST); // (a job of its own: no caller's staging touched)
        if (!rc) rc = wait_job(s, pik::JOB_SELF_TEST);
        s->opt = saved;
        return rc;
    };
    auto same = [&](const Out& a, const Out& b) {
        return std::memcmp(a.sol.data(), b.sol.data(), sizeof(double) * a.sol.size()) == 0 &&
               std::memcmp(a.cost.data(), b.cost.data(), sizeof(double) * a.cost.size()) == 0 &&
               std::memcmp(a.st.data(), b.st.data(), sizeof(int32_t) * a.st.size()) == 0 &&
               std::memcmp(a.stats.data(), b.stats.data(), sizeof(pikamd_stats) * a.stats.size()) == 0;
    };
    // would the launcher serve `lanes` lanes per elite (per problem in local mode) for this chain and these
    // parameters?  The widths it would not serve fall back to the adaptive choice, which is not what is tested.
    const bool multi = tips > 1;
    const int S = (p->mode == 0 && p->memetic_num_threads > 1) ? p->memetic_num_threads : 1;
    int gs = 1;
    while (p->mode == 0 && gs < p->memetic_elite_size) gs <<= 1;
    auto served = [&](int lanes) -> bool {
        if (mask_of(saved) & (unsigned)lanes) return false;
        return pik::lpe_allowed(s, lanes, gs, S, multi, exact_now);
    };
    Out ref, got;
    unsigned disabled = 0;
    if (p->mode != 0) {
        // local mode: the cooperative descent with 8 / 16 lanes per problem against the one-lane kernel
        if (int rc = run(1, false, false, ref)) return rc;
#if !defined(PIK_STRICT)
        if (!needs_literal(s) && !exact_now)
            for (int lanes : {8, 16}) {
                if (!served(lanes)) continue;
                if (int rc = run(lanes, false, false, got)) return rc;
                if (!same(ref, got)) disabled |= (unsigned)lanes;
            }
#endif
        // exact flavours, one tip frame: the team kernels of local mode (4 / 16 lanes per problem, pik_launch.hpp)
        if (exact_now && !multi)
            for (int lanes : {4, 16}) {
                if (!served(lanes)) continue;
                if (int rc = run(lanes, false, false, got)) return rc;
                if (!same(ref, got)) disabled |= (unsigned)lanes;
            }
        mask_of(s->opt) = mask_of(saved) | disabled;
        if (disabled_out) *disabled_out = mask_of(s->opt);
        return 0;
    }
    if (int rc = run(1, false, false, ref)) return rc; // the reference: one lane per elite, one launch, one per SIMD
    for (int lanes : {2, 4, 8, 16}) {
        if (!served(lanes)) continue;
        for (int passes = 0; passes < 2; ++passes) {
            if (int rc = run(lanes, passes != 0, false, got)) return rc;
            if (!same(ref, got)) disabled |= (unsigned)lanes;
        }
    }
    // the kernels specialised for the common configuration against the general ones (when this call has it)
    {
        pik::ParamsK pk;
        if (!pik::make_params_k(p, pk) && is_common(flavour_of(s, p, &pk))) {
            const bool was = s->opt.specialised;
            s->opt.specialised = false;
            Out general;
            saved.specialised = false; // (run() works on a copy of `saved`)
            const int rc = run(1, false, false, general);
            saved.specialised = was;
            s->opt.specialised = was;
            if (rc) return rc;
            if (!same(ref, general)) disabled |= 32u;
        }
    }
    // the two-per-SIMD build of the one-lane kernel, forced whatever the size of the call (one species, one tip)
    if (S == 1 && !multi) {
        if (int rc = run(1, false, true, got)) return rc;
        if (!same(ref, got)) disabled |= 1u;
    }
    if (int rc = run(1, true, false, got)) return rc;
    if (!same(ref, got)) return fail(PIKAMD_EHIP, "self test: the one-lane kernel disagrees with itself under compaction passes");
    if (disabled & 32u) s->opt.specialised = false; // (the two flavours disagree: keep to the general kernels)
    mask_of(s->opt) = mask_of(saved) | (disabled & ~32u);
    disabled = (disabled & 32u);
    if (disabled_out) *disabled_out = mask_of(s->opt) | disabled;
    return 0;
}

int32_t pikamd_self_test_cost(const pikamd_solver* s, int32_t* runs, double* total_ms) {
    if (!s) return fail(PIKAMD_EINVAL, "solver is NULL");
    if (runs) *runs = s->self_test_runs;
    if (total_ms) *total_ms = s->self_test_ms;
    return 0;
}

} // extern "C"

// Option self_test = auto: the first solve (or reserve) of a parameter set that the GENERAL or the EXACT kernels
// serve runs pikamd_self_test on 32 generated targets of the handle's own chain first -- every kernel variant
// against the one-lane kernel, bit for bit; a variant that disagrees is switched off for the handle.  Those
// kernels sit at the register cap for long chains and have come out of the compiler wrong before (DESIGN.md
// section 3); the kernels of the common configuration are fuzzed at every chain length by the test suite and
// are not re-checked here.  Costs a dozen small solves, once per parameter set and handle.
static int maybe_self_test(pikamd_solver* s, const pikamd_params* p) {
    if (!s->opt.auto_self_test || s->in_self_test || !p) return 0;
    pik::ParamsK pk;
    if (pik::make_params_k(p, pk)) return 0; // (the solve itself reports the bad parameter)
    {
        const Flavour f = flavour_of(s, p, &pk);
        if (is_common(f) && ops_at<pik::LaunchOps>(f, FAM_LAUNCH, s->chain.dof)) return 0;
    }
    // One run per KERNEL SET, not per parameter set: what selects the kernels and the paths inside them is the
    // flavour, the mode, species and elites (how a wavefront is dealt out), which joint goals and cost terms are on,
    // the line-search form and the approximate-solution return -- thresholds, weights, population and budgets do not,
    // so a plugin whose parameters change at run time does not pay again.
    unsigned long long h = 1469598103934665603ull;
    const long long key[] = {needs_literal(s, p) ? 1 : 0, p->mode, p->mode == 0 ? p->memetic_num_threads : 1,
                             p->mode == 0 ? p->memetic_elite_size : 0, pk.goal_mask, pk.line_delta, pk.approx,
                             pk.has_pos_thr, pk.has_ori_thr, pk.stop_on_valid, pk.stop_on_first,
                             p->position_scale > 0.0 ? 1 : 0, p->rotation_scale > 0.0 ? 1 : 0}; // (the pose cost's two terms)
    const unsigned char* b = reinterpret_cast<const unsigned char*>(key);
    for (size_t i = 0; i < sizeof key; ++i) h = (h ^ b[i]) * 1099511628211ull;
    for (unsigned long long k : s->self_tested)
        if (k == h) return 0;
    // ... and a SHORT run: the variants re-schedule one arithmetic, a disagreement shows in the first descent step of
    // the first generation; four generations of six steps on 32 targets cross every phase of a generation, the
    // compaction marks 1, 2 and 3 of pikamd_self_test's list (park, re-pack and resume, three times; its later marks
    // are only reached by a full-length call of pikamd_self_test) and both line-search forms (~10 ms instead of the
    // ~230 ms of full-length solves on the exact kernels).  pikamd_self_test itself runs whatever parameters it is
    // given.  The stream-ordered entry points never come here (they must not block): reserve first.
    pikamd_params q = *p;
    if (q.mode == 0) {
        q.memetic_max_generations = q.memetic_max_generations < 4 ? q.memetic_max_generations : 4;
        q.memetic_gd_max_iters = q.memetic_gd_max_iters < 6 ? q.memetic_gd_max_iters : 6;
    } else {
        q.gd_max_iters = q.gd_max_iters < 24 ? q.gd_max_iters : 24;
    }
    const auto t0 = std::chrono::steady_clock::now();
    s->in_self_test = true;
    const int rc = pikamd_self_test(s, &q, 32, nullptr);
    s->in_self_test = false;
    if (rc) return rc; // (a run that failed to run is not counted and will be tried again)
    s->self_test_runs += 1;
    s->self_test_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    s->self_tested.push_back(h);
    return 0;
}

extern "C" {

const char* pikamd_kernel_name(const pikamd_solver* s, const pikamd_params* p) {
    if (!s || !p) return "";
    pikamd_solver* m = const_cast<pikamd_solver*>(s);
    // the flavour that serves a solve call with these parameters (see solve_ops_of: a common flavour only where it
    // has kernels for the length)
    pik::ParamsK pk;
    Flavour f = flavour_of(s, p, pik::make_params_k(p, pk) ? nullptr : &pk);
    if (!ops_at<pik::LaunchOps>(f, FAM_LAUNCH, s->chain.dof)) f = unspecialised(f);
    snprintf(m->kernel_name, sizeof m->kernel_name, "%s::%s<%d>", FLAVOUR_NAMESPACE[f],
             p->mode == 1 ? "ik_gradient_kernel" : "memetic_kernel", s->chain.dof);
    return m->kernel_name;
}

} // extern "C"

// ---- what the path and search entry points share --------------------------------------------------
namespace {

// One of the three kinds of call, for its refusals: its name, the mode it wants and how it says so, the layout of its
// arrays and the name of its second required one.
struct CallKind {
    const char* name;
    int mode;
    const char* wants;      // "<name>: <wants>, got mode <m><because>"
    const char* because;
    bool paths;             // counts: P paths of W waypoints (else B problems of max_attempts attempts)
    const char* layout;
    const char* second;
};
const CallKind SOLVE_PATHS = {"pikamd_solve_paths", 1, "waypoint paths are solved in local mode (mode = 1)", "", true,
                              "[P][W][dof]", "start"};
const CallKind SEARCH = {"pikamd_search_batch", 1, "restarts are served in local mode (mode = 1)",
                         ": a restart attempt of the memetic kernels would have to start a first pass from a device-side "
                         "list of the failed problems, which their launch does not offer",
                         false, "[B][dof]", "seed"};
const CallKind SEARCH_PATHS = {"pikamd_search_paths", 1, "paths from a pose are searched in local mode (mode = 1)", "", true,
                                 "[P][W][dof]", "seed"};
const CallKind SEARCH_GLOBAL_PATHS = {"pikamd_search_global_paths", 0, "the start of a path is searched by the memetic solver (mode = 0)",
                                      ": local mode is served by pikamd_search_paths", true, "[P][W][dof]", "seed"};
const CallKind SEARCH_GLOBAL = {"pikamd_search_global_batch", 0, "restarts of the memetic solver (mode = 0)",
                                ": local mode is served by pikamd_search_batch", false, "[B][dof]", "seed"};

// What both entry points of a kind refuse, in this order (it decides which message a doubly-wrong call gets).  n, k: P
// and W, or B and max_attempts; any_null: some required array is NULL.
int check_call(const CallKind& c, const pikamd_solver* s, const pikamd_params* p, int64_t n, int32_t k, bool any_null,
               pik::ParamsK& pk) {
    if (int rc = check_solver(s)) return rc;
    if (!p) return fail(PIKAMD_EINVAL, "params is NULL");
    if (p->mode != c.mode) return fail(PIKAMD_EINVAL, "%s: %s, got mode %d%s", c.name, c.wants, (int)p->mode, c.because);
    if (c.paths) {
        if (k < 1 || n < 0)
            return fail(PIKAMD_EINVAL, "%s: %lld paths of %d waypoints: expected P >= 0 and W >= 1", c.name, (long long)n, (int)k);
    } else {
        if (k < 1 || k > PIKAMD_MAX_ATTEMPTS)
            return fail(PIKAMD_EINVAL, "%s: max_attempts %d: expected 1..%d", c.name, (int)k, PIKAMD_MAX_ATTEMPTS);
        if (n < 0) return fail(PIKAMD_EINVAL, "%s: B = %lld: expected B >= 0", c.name, (long long)n);
    }
    if (s->opt.soa) return fail(PIKAMD_EINVAL, "joint_layout soa: not with %s (its arrays are %s)", c.name, c.layout);
    if (const char* msg = pik::make_params_k(p, pk)) return fail(PIKAMD_EINVAL, "%s", msg);
    if (n > 0 && any_null)
        return fail(PIKAMD_EINVAL, "%s: goal_pos_quat, %s, solution and status must not be NULL", c.name, c.second);
    return 0;
}

// Staging of a synchronous entry point, through the synchronous entry points' job (as pikamd_solve_batch): the
// caller's arrays are registered as regions -- the inputs first --, laid out one behind the other (8-byte aligned
// pieces) in the job's pinned and device buffers, and moved with one copy in before the kernels and one copy out
// behind them, on the job's stream.
class Staging {
  public:
    static constexpr int SLOT = pik::N_DEVICE_SLOTS + PIKAMD_MAX_HOST_JOBS - 1;
    // the most regions a call registers: the arrays of the largest set (every stage_* function holds its set to this)
    static constexpr int MAX_REGIONS = 13;
    Staging(pikamd_solver* s, const char* who) : s_(s), who_(who), J_(s->jobs[PIKAMD_MAX_HOST_JOBS - 1]) {}
    hipStream_t stream() const { return J_.stream; }
    // refuses while the job is in flight; the device, and the stream at its first use
    int begin() {
        if (J_.pending)
            return fail(PIKAMD_EINVAL, "job %d is still in flight: call pikamd_wait first", PIKAMD_MAX_HOST_JOBS - 1);
        HIP_TRY(hipSetDevice(s_->device));
        if (!J_.stream) HIP_TRY(hipStreamCreateWithFlags(&J_.stream, hipStreamNonBlocking));
        return 0;
    }
    // An input (NULL: absent -- no bytes, a null device pointer) or an output (NULL: not copied out, and absent unless
    // the kernels write it anyway: `always`); returns the region's index for at().
    int in(const void* src, size_t bytes) { return add({src, nullptr, total_, src ? bytes : 0}, true); }
    int out(void* dst, size_t bytes, bool always) { return add({nullptr, dst, total_, (dst || always) ? bytes : 0}, false); }
    // the buffers, once every region is registered
    int allocate() {
        if (n_ > MAX_REGIONS) return fail(PIKAMD_EINVAL, "%s: %d arrays to stage: at most %d", who_, n_, MAX_REGIONS);
        if (int rc = J_.dev.ensure(total_)) return rc;
        return J_.host.ensure(total_);
    }
    template <class T>
    T* at(int region) const {
        return region < MAX_REGIONS && r_[region].bytes ? reinterpret_cast<T*>((char*)J_.dev.p + r_[region].off) : nullptr;
    }
    // the copy in
    int upload() {
        for (int i = 0; i < n_; ++i)
            if (r_[i].src) std::memcpy((char*)J_.host.p + r_[i].off, r_[i].src, r_[i].bytes);
        HIP_TRY(hipMemcpyAsync(J_.dev.p, J_.host.p, in_bytes_, hipMemcpyHostToDevice, J_.stream));
        return 0;
    }
    // Behind the launch (its return code): the copy out into the caller's arrays.  Work of the call may be in flight
    // once upload() has run, so the stream is drained before an error of the launch is returned.
    int finish(int launch_rc) {
        if (launch_rc) {
            (void)hipStreamSynchronize(J_.stream);
            return launch_rc;
        }
        char* hb = (char*)J_.host.p;
        hipError_t e = hipMemcpyAsync(hb + in_bytes_, (char*)J_.dev.p + in_bytes_, total_ - in_bytes_, hipMemcpyDeviceToHost, J_.stream);
        const hipError_t e2 = hipStreamSynchronize(J_.stream);
        if (e == hipSuccess) e = e2;
        if (e != hipSuccess) return fail(PIKAMD_EHIP, "%s: %s (its results are lost)", who_, hipGetErrorString(e));
        for (int i = 0; i < n_; ++i)
            if (r_[i].dst) std::memcpy(r_[i].dst, hb + r_[i].off, r_[i].bytes);
        return 0;
    }

  private:
    struct Region {
        const void* src;
        void* dst;
        size_t off, bytes;
    };
    // (a region past the last place is counted and not kept: allocate() refuses the call)
    int add(const Region& r, bool input) {
        if (n_ >= MAX_REGIONS) return n_++;
        r_[n_] = r;
        total_ += align8(r.bytes);
        if (input) in_bytes_ = total_;
        return n_++;
    }
    pikamd_solver* s_;
    const char* who_;
    pik::HostJob& J_;
    Region r_[MAX_REGIONS];
    int n_ = 0;
    size_t in_bytes_ = 0, total_ = 0;
};

const char* tips_text(const pikamd_solver* s) { return s->n_tips > 1 ? "true" : "false"; }

// the name of the kernel variant a path or search call runs: one lane, a team (exact flavours) or the cooperative
// descent.  tips: the kernels have a template argument for several tip frames (the Cartesian motions' have none: they
// are walked on one tip frame)
const char* variant_name(const pikamd_solver* s, Flavour f, const char* stem, int lanes, bool tips = true) {
    pikamd_solver* m = const_cast<pikamd_solver*>(s);
    char tail[8] = "";
    if (tips) snprintf(tail, sizeof tail, ",%s", tips_text(s));
    const char* ns = FLAVOUR_NAMESPACE[f];
    const int dof = s->chain.dof;
    if (lanes == 1)
        snprintf(m->kernel_name, sizeof m->kernel_name, "%s::ik_%s_kernel<%d%s>", ns, stem, dof, tail);
    else if (is_exact(f))
        snprintf(m->kernel_name, sizeof m->kernel_name, "%s::ik_%s_team_kernel<%d,%d>", ns, stem, dof, lanes);
    else
        snprintf(m->kernel_name, sizeof m->kernel_name, "%s::ik_%s_wide_kernel<%d,%d%s>", ns, stem, dof, lanes, tail);
    return m->kernel_name;
}
// ... of a path call of P paths in the flavour a path call runs in ("" where the name functions have nothing to name)
const char* path_variant_name(const pikamd_solver* s, const pikamd_params* p, int64_t P, const char* stem, bool tips = true) {
    if (!s || !p) return "";
    const Flavour f = flavour_of(s, p, nullptr);
    return variant_name(s, f, stem, pik::path_lanes(s, P, is_exact(f)), tips);
}

// what every stream-ordered entry point refuses of its slot
int check_slot(int32_t slot) {
    if (slot < 0 || slot >= PIKAMD_MAX_SLOTS) return fail(PIKAMD_EINVAL, "slot out of range");
    return 0;
}

} // namespace

// ---- Cartesian waypoint paths (pik_path.hpp) ----------------------------------------------------
namespace {

// the arrays of a path call: host pointers, or device pointers
struct PathArrays {
    const double *goal, *start, *max_step;
    double* solution;
    int32_t* status;
    double* cost;
    pikamd_stats* stats;
    int32_t* reached;
    bool required_null() const { return !goal || !start || !solution || !status; }
};

pik::PathArgs path_args(int64_t P, int32_t W, const PathArrays& d) {
    return {P, W, 0, d.goal, d.start, d.max_step, d.solution, d.status, d.cost, d.stats, d.reached};
}

// the arrays a set of them holds (one pointer each): what its stage_* function registers
template <class Arrays>
constexpr int n_arrays() {
    return (int)(sizeof(Arrays) / sizeof(void*));
}

// registers the arrays of a synchronous path call of P paths and W waypoints, allocates, and gives the device's
int stage_paths(Staging& st, const pikamd_solver* s, const PathArrays& h, int64_t P, int32_t W, PathArrays& dev) {
    static_assert(n_arrays<PathArrays>() <= Staging::MAX_REGIONS, "Staging::MAX_REGIONS");
    const size_t d = (size_t)s->chain.dof, g7 = 7 * (size_t)s->n_tips, paths = (size_t)P, rows = paths * (size_t)W;
    const int goal = st.in(h.goal, sizeof(double) * g7 * rows), start = st.in(h.start, sizeof(double) * d * paths);
    const int step = st.in(h.max_step, sizeof(double) * d);
    const int sol = st.out(h.solution, sizeof(double) * d * rows, true), cost = st.out(h.cost, sizeof(double) * rows, true);
    const int stats = st.out(h.stats, sizeof(pikamd_stats) * rows, true), status = st.out(h.status, sizeof(int32_t) * rows, true);
    const int reached = st.out(h.reached, sizeof(int32_t) * paths, true);
    if (int rc = st.allocate()) return rc;
    dev = {st.at<const double>(goal), st.at<const double>(start), st.at<const double>(step), st.at<double>(sol),
           st.at<int32_t>(status),    st.at<double>(cost),        st.at<pikamd_stats>(stats), st.at<int32_t>(reached)};
    return 0;
}

// The walk of a call on `st` and, where the handle applies its validity model to paths (pikamd_set_path_validity), the
// cut behind it.
int run_paths(pikamd_solver* s, const pik::PathOps* ops, const pik::ParamsK& pk, const pik::PathArgs& a, hipStream_t st,
              int slot) {
    const pik::PathValidOps* vops = nullptr;
    if (int rc = path_validity_for_call(s, SOLVE_PATHS.name, &vops)) return rc;
    if (!vops) return ops->solve(s, pk, a, st, slot);
    pik::PathArgs walk = a;
    if (int rc = path_validity_reached(s, slot, a.P, a.reached, &walk.reached)) return rc;
    if (int rc = ops->solve(s, pk, walk, st, slot)) return rc;
    return vops->paths(ext_of(s)->validity_dev.p, ext_of(s)->validity_model.n_spheres, a, walk.reached, st);
}

} // namespace

extern "C" {

int32_t pikamd_solve_paths_device(pikamd_solver* s, const pikamd_params* p, int64_t P, int32_t W,
                                  const double* d_goal_pos_quat, const double* d_start, const double* d_max_joint_step,
                                  double* d_solution, int32_t* d_status, double* d_final_cost, pikamd_stats* d_stats,
                                  int32_t* d_reached, void* stream, int32_t slot) {
    const PathArrays d = {d_goal_pos_quat, d_start, d_max_joint_step, d_solution, d_status, d_final_cost, d_stats, d_reached};
    pik::ParamsK pk;
    if (int rc = check_call(SOLVE_PATHS, s, p, P, W, d.required_null(), pk)) return rc;
    if (int rc = check_slot(slot)) return rc;
    if (P == 0) return 0;
    // (no automatic self test here: stream-ordered, see pikamd_solve_batches_device)
    const pik::PathOps* ops = path_ops_of(s, p);
    if (!ops) return no_kernels(s->chain.dof);
    HIP_TRY(hipSetDevice(s->device));
    return run_paths(s, ops, pk, path_args(P, W, d), (hipStream_t)stream, slot);
}

int32_t pikamd_solve_paths(pikamd_solver* s, const pikamd_params* p, int64_t P, int32_t W, const double* goal_pos_quat,
                           const double* start, const double* max_joint_step, double* solution, int32_t* status,
                           double* final_cost, pikamd_stats* stats, int32_t* reached) {
    const PathArrays h = {goal_pos_quat, start, max_joint_step, solution, status, final_cost, stats, reached};
    pik::ParamsK pk;
    if (int rc = check_call(SOLVE_PATHS, s, p, P, W, h.required_null(), pk)) return rc;
    if (P == 0) return 0;
    if (int rc = maybe_self_test(s, p)) return rc; // (the local-mode kernel set, as pikamd_solve_batch)
    const pik::PathOps* ops = path_ops_of(s, p);
    if (!ops) return no_kernels(s->chain.dof);
    Staging st(s, SOLVE_PATHS.name);
    if (int rc = st.begin()) return rc;
    PathArrays dev;
    if (int rc = stage_paths(st, s, h, P, W, dev)) return rc;
    if (int rc = st.upload()) return rc;
    return st.finish(run_paths(s, ops, pk, path_args(P, W, dev), st.stream(), Staging::SLOT));
}

const char* pikamd_path_kernel_name(const pikamd_solver* s, const pikamd_params* p, int64_t P) {
    return path_variant_name(s, p, P, "path");
}

} // extern "C"

// ---- Cartesian paths from a pose (pik_startpath.hpp) ------------------------------------------------
namespace {

// the arrays of a pikamd_search_paths call: host pointers, or device pointers
struct StartPathArrays {
    const double *goal, *seed, *guess, *max_step; // guess: null = the seed
    double* solution;
    int32_t* status;
    double* cost;
    pikamd_stats* stats;
    int32_t *reached, *attempts;
    pikamd_stats* totals;
    bool required_null() const { return !goal || !seed || !solution || !status; }
};

// what the entry points of both kinds (SEARCH_PATHS, SEARCH_GLOBAL_PATHS) refuse: check_call's list for a path call of
// the kind, then the attempts
int check_search_paths(const CallKind& kind, const pikamd_solver* s, const pikamd_params* p, int64_t P, int32_t W, int32_t K,
                       const StartPathArrays& d, pik::ParamsK& pk) {
    if (int rc = check_call(kind, s, p, P, W, d.required_null(), pk)) return rc;
    if (K < 1 || K > PIKAMD_MAX_ATTEMPTS)
        return fail(PIKAMD_EINVAL, "%s: max_attempts %d: expected 1..%d", kind.name, (int)K, PIKAMD_MAX_ATTEMPTS);
    return 0;
}

// registers the arrays of a synchronous call of P paths and W waypoints, allocates, and gives the device's
int stage_startpath(Staging& st, const pikamd_solver* s, const StartPathArrays& h, int64_t P, int32_t W, StartPathArrays& dev) {
    static_assert(n_arrays<StartPathArrays>() <= Staging::MAX_REGIONS, "Staging::MAX_REGIONS");
    const size_t d = (size_t)s->chain.dof, g7 = 7 * (size_t)s->n_tips, paths = (size_t)P, rows = paths * (size_t)W;
    const int goal = st.in(h.goal, sizeof(double) * g7 * rows), seed = st.in(h.seed, sizeof(double) * d * paths);
    const int guess = st.in(h.guess, sizeof(double) * d * paths), step = st.in(h.max_step, sizeof(double) * d);
    // (the outputs a caller left out are not written by the kernels either: no bytes)
    const int sol = st.out(h.solution, sizeof(double) * d * rows, true), cost = st.out(h.cost, sizeof(double) * rows, false);
    const int stats = st.out(h.stats, sizeof(pikamd_stats) * rows, false), status = st.out(h.status, sizeof(int32_t) * rows, true);
    const int reached = st.out(h.reached, sizeof(int32_t) * paths, false), attempts = st.out(h.attempts, sizeof(int32_t) * paths, false);
    const int totals = st.out(h.totals, sizeof(pikamd_stats) * paths, false);
    if (int rc = st.allocate()) return rc;
    dev = {st.at<const double>(goal), st.at<const double>(seed), st.at<const double>(guess),  st.at<const double>(step),
           st.at<double>(sol),        st.at<int32_t>(status),    st.at<double>(cost),         st.at<pikamd_stats>(stats),
           st.at<int32_t>(reached),   st.at<int32_t>(attempts),  st.at<pikamd_stats>(totals)};
    return 0;
}

// The arguments of a call on device pointers; the rows of the attempts behind the first in the slot's scratch, which
// grows only when a call needs more than any earlier one on the slot.
int startpath_args(pikamd_solver* s, int slot, int64_t P, int32_t W, int32_t K, const StartPathArrays& d,
                   uint64_t rng_seed, int64_t problem_offset, pik::StartPathArgs& a) {
    a = {};
    a.P = P;
    a.W = W;
    a.K = K;
    a.goal = d.goal;
    a.seed = d.seed;
    a.guess = d.guess ? d.guess : d.seed;
    a.max_step = d.max_step;
    a.rng_seed = rng_seed;
    a.problem_offset = problem_offset;
    a.solution = d.solution;
    a.status = d.status;
    a.cost = d.cost;
    a.stats = d.stats;
    a.reached = d.reached;
    a.attempts = d.attempts;
    a.totals = d.totals;
    const pik::StartPathScratch l = pik::startpath_scratch(P, W, K, s->chain.dof, d.cost != nullptr, d.stats != nullptr);
    if (l.total == 0) return 0;
    pik::DevBuf& buf = ext_of(s)->startpath_rows[slot];
    if (int rc = buf.ensure(l.total)) return rc;
    char* w = (char*)buf.p;
    if (d.stats) a.row_stats = w + l.off_stats;
    if (d.cost) a.row_cost = (double*)(w + l.off_cost);
    a.row_solution = (double*)(w + l.off_solution);
    a.row_status = (int*)(w + l.off_status);
    return 0;
}

} // namespace

extern "C" {

int32_t pikamd_search_paths_device(pikamd_solver* s, const pikamd_params* p, int64_t P, int32_t W,
                                   const double* d_goal_pos_quat, const double* d_seed, const double* d_initial_guess,
                                   const double* d_max_joint_step, uint64_t rng_seed, int64_t problem_offset,
                                   int32_t max_attempts, double* d_solution, int32_t* d_status, double* d_final_cost,
                                   pikamd_stats* d_stats, int32_t* d_reached, int32_t* d_attempts,
                                   pikamd_stats* d_totals, void* stream, int32_t slot) {
    const StartPathArrays d = {d_goal_pos_quat, d_seed,  d_initial_guess, d_max_joint_step, d_solution, d_status,
                               d_final_cost,    d_stats, d_reached,       d_attempts,       d_totals};
    pik::ParamsK pk;
    if (int rc = check_search_paths(SEARCH_PATHS, s, p, P, W, max_attempts, d, pk)) return rc;
    if (int rc = check_slot(slot)) return rc;
    if (P == 0) return 0;
    // (no automatic self test here: stream-ordered, see pikamd_solve_batches_device)
    const pik::StartPathOps* ops = startpath_ops_of(s, p);
    if (!ops) return no_kernels(s->chain.dof);
    HIP_TRY(hipSetDevice(s->device));
    pik::StartPathArgs a;
    if (int rc = startpath_args(s, slot, P, W, max_attempts, d, rng_seed, problem_offset, a)) return rc;
    return ops->solve(s, pk, a, (hipStream_t)stream, slot);
}

int32_t pikamd_search_paths(pikamd_solver* s, const pikamd_params* p, int64_t P, int32_t W, const double* goal_pos_quat,
                            const double* seed, const double* initial_guess, const double* max_joint_step,
                            uint64_t rng_seed, int64_t problem_offset, int32_t max_attempts, double* solution,
                            int32_t* status, double* final_cost, pikamd_stats* stats, int32_t* reached,
                            int32_t* attempts, pikamd_stats* totals) {
    const StartPathArrays h = {goal_pos_quat, seed,  initial_guess, max_joint_step, solution, status,
                               final_cost,    stats, reached,       attempts,       totals};
    pik::ParamsK pk;
    if (int rc = check_search_paths(SEARCH_PATHS, s, p, P, W, max_attempts, h, pk)) return rc;
    if (P == 0) return 0;
    if (int rc = maybe_self_test(s, p)) return rc; // (the local-mode kernel set, as pikamd_solve_batch)
    const pik::StartPathOps* ops = startpath_ops_of(s, p);
    if (!ops) return no_kernels(s->chain.dof);
    Staging st(s, SEARCH_PATHS.name);
    if (int rc = st.begin()) return rc;
    StartPathArrays dev;
    if (int rc = stage_startpath(st, s, h, P, W, dev)) return rc;
    pik::StartPathArgs a;
    if (int rc = startpath_args(s, Staging::SLOT, P, W, max_attempts, dev, rng_seed, problem_offset, a)) return rc;
    if (int rc = st.upload()) return rc;
    return st.finish(ops->solve(s, pk, a, st.stream(), Staging::SLOT));
}

const char* pikamd_search_paths_kernel_name(const pikamd_solver* s, const pikamd_params* p, int64_t P) {
    return path_variant_name(s, p, P, "startpath");
}

} // extern "C"

// ---- local IK with random restarts (pik_search.hpp), memetic IK with random restarts (pik_restart.hpp) ----
namespace {

// the arrays of a search call of either mode: host pointers, or device pointers
struct SearchArrays {
    const double *goal, *seed, *guess; // guess: null = the seed
    double* solution;
    int32_t* status;
    double* cost;
    pikamd_stats* stats;
    int32_t* attempts;
    double* all_solution;
    int32_t* all_status;
    bool required_null() const { return !goal || !seed || !solution || !status; }
};

// registers the arrays of a synchronous search call of B problems and K attempts, allocates, and gives the device's
int stage_search(Staging& st, const pikamd_solver* s, const SearchArrays& h, int64_t B, int32_t K, SearchArrays& dev) {
    static_assert(n_arrays<SearchArrays>() <= Staging::MAX_REGIONS, "Staging::MAX_REGIONS");
    const size_t d = (size_t)s->chain.dof, g7 = 7 * (size_t)s->n_tips, n = (size_t)B, rows = n * (size_t)K;
    const int goal = st.in(h.goal, sizeof(double) * g7 * n), seed = st.in(h.seed, sizeof(double) * d * n);
    const int guess = st.in(h.guess, sizeof(double) * d * n);
    const int sol = st.out(h.solution, sizeof(double) * d * n, true), cost = st.out(h.cost, sizeof(double) * n, true);
    const int stats = st.out(h.stats, sizeof(pikamd_stats) * n, true), status = st.out(h.status, sizeof(int32_t) * n, true);
    const int attempts = st.out(h.attempts, sizeof(int32_t) * n, true);
    const int all_sol = st.out(h.all_solution, sizeof(double) * d * rows, false);
    const int all_status = st.out(h.all_status, sizeof(int32_t) * rows, false);
    if (int rc = st.allocate()) return rc;
    dev = {st.at<const double>(goal), st.at<const double>(seed), st.at<const double>(guess), st.at<double>(sol),
           st.at<int32_t>(status),    st.at<double>(cost),       st.at<pikamd_stats>(stats), st.at<int32_t>(attempts),
           st.at<double>(all_sol),    st.at<int32_t>(all_status)};
    return 0;
}

pik::SearchPlan search_plan_of(const pikamd_solver* s, const pikamd_params* p, int64_t B, int32_t K) {
    return pik::search_plan(s, ext_of(s)->search_schedule, B, K, is_exact(flavour_of(s, p, nullptr)));
}

// Schedule, width and -- parallel schedule -- the per-attempt rows of a call: the caller's all_* arrays where given,
// the slot's scratch for the rest.  The scratch grows only when a call needs more than any earlier one on the slot.
int plan_search(pikamd_solver* s, const pikamd_params* p, int slot, pik::SearchArgs& a, double* all_solution,
                int32_t* all_status) {
    const pik::SearchPlan plan = search_plan_of(s, p, a.B, a.K);
    a.parallel = plan.parallel ? 1 : 0;
    a.lanes = plan.lanes;
    a.every = (all_solution || all_status) ? 1 : 0;
    a.row_solution = all_solution;
    a.row_status = all_status;
    a.row_cost = nullptr;
    a.row_stats = nullptr;
    if (!plan.parallel) return 0;
    const size_t rows = (size_t)a.B * (size_t)a.K, d = (size_t)s->chain.dof;
    const size_t off_stats = 0, off_cost = off_stats + sizeof(pikamd_stats) * rows;
    const size_t off_solution = off_cost + sizeof(double) * rows;
    const size_t off_status = off_solution + (all_solution ? 0 : sizeof(double) * d * rows);
    const size_t total = off_status + (all_status ? 0 : align8(sizeof(int32_t) * rows));
    pik::DevBuf& buf = ext_of(s)->search_rows[slot];
    if (int rc = buf.ensure(total)) return rc;
    char* w = (char*)buf.p;
    a.row_stats = w + off_stats;
    a.row_cost = (double*)(w + off_cost);
    if (!all_solution) a.row_solution = (double*)(w + off_solution);
    if (!all_status) a.row_status = (int*)(w + off_status);
    return 0;
}

// the arguments of a local-mode search on device pointers, planned (plan_search: may grow the slot's scratch)
int search_args(pikamd_solver* s, const pikamd_params* p, int slot, int64_t B, int32_t K, const SearchArrays& d,
                uint64_t rng_seed, int64_t problem_offset, pik::SearchArgs& a) {
    a = {};
    a.B = B;
    a.K = K;
    a.goal = d.goal;
    a.seed = d.seed;
    a.guess = d.guess ? d.guess : d.seed;
    a.rng_seed = rng_seed;
    a.problem_offset = problem_offset;
    a.solution = d.solution;
    a.status = d.status;
    a.cost = d.cost;
    a.stats = d.stats;
    a.attempts = d.attempts;
    return plan_search(s, p, slot, a, d.all_solution, d.all_status);
}

// the handle's gate into the arguments of a local-mode call (gate_for_call)
int search_gate(pikamd_solver* s, const pik::ParamsK& pk, int slot, hipStream_t st, pik::SearchArgs& a) {
    return gate_for_call(s, pk, slot, st, &a.gate, &a.gate_joint, &a.gate_params);
}

// The handle's sphere model into the arguments of a local-mode call: the test runs inside the exact flavours' search
// kernels (pik_search.hpp search_attempt), whose chain constants are the ones the model's image was packed with.  A
// call the fast kernels serve has no such step: refused while a model is set.
int search_validity(pikamd_solver* s, const pikamd_params* p, pik::SearchArgs* a) {
    if (!ext_of(s)->validity_set) return 0;
    if (!is_exact(flavour_of(s, p, nullptr)))
        return fail(PIKAMD_EUNSUPPORTED,
                    "pikamd_search_batch: a validity model is set and the option arithmetic = fast has the fast kernels "
                    "serve this call; they have no validity step (arithmetic = exact, or pikamd_set_validity_model(s, NULL))");
    if (int rc = validity_chain_ok(s, "pikamd_search_batch")) return rc;
    if (a) a->validity = ext_of(s)->validity_dev.p;
    return 0;
}

// ... and of a global-mode one (goal and seed apart: they go to the solver)
pik::RestartArgs restart_args(int64_t B, int32_t K, const SearchArrays& d, uint64_t rng_seed, int64_t problem_offset) {
    pik::RestartArgs r = {};
    r.B = B;
    r.K = K;
    r.user_guess = d.guess ? d.guess : d.seed;
    r.rng_seed = rng_seed;
    r.problem_offset = problem_offset;
    r.solution = d.solution;
    r.status = d.status;
    r.cost = d.cost;
    r.stats = d.stats;
    r.attempts = d.attempts;
    r.all_solution = d.all_solution;
    r.all_status = d.all_status;
    return r;
}

} // namespace

extern "C" {

int32_t pikamd_search_batch_device(pikamd_solver* s, const pikamd_params* p, int64_t B, const double* d_goal_pos_quat,
                                   const double* d_seed, const double* d_initial_guess, uint64_t rng_seed,
                                   int64_t problem_offset, int32_t max_attempts, double* d_solution, int32_t* d_status,
                                   double* d_final_cost, pikamd_stats* d_stats, int32_t* d_attempts,
                                   double* d_all_solution, int32_t* d_all_status, void* stream, int32_t slot) {
    const SearchArrays d = {d_goal_pos_quat, d_seed,  d_initial_guess, d_solution,     d_status,
                            d_final_cost,    d_stats, d_attempts,      d_all_solution, d_all_status};
    pik::ParamsK pk;
    if (int rc = check_call(SEARCH, s, p, B, max_attempts, d.required_null(), pk)) return rc;
    if (int rc = check_slot(slot)) return rc;
    if (B == 0) return 0;
    // (no automatic self test here: stream-ordered, see pikamd_solve_batches_device)
    const pik::SearchOps* ops = search_ops_of(s, p);
    if (!ops) return no_kernels(s->chain.dof);
    if (int rc = search_validity(s, p, nullptr)) return rc;
    HIP_TRY(hipSetDevice(s->device));
    pik::SearchArgs a;
    if (int rc = search_args(s, p, slot, B, max_attempts, d, rng_seed, problem_offset, a)) return rc;
    if (int rc = search_gate(s, pk, slot, (hipStream_t)stream, a)) return rc;
    if (int rc = search_validity(s, p, &a)) return rc;
    return ops->solve(s, pk, a, (hipStream_t)stream, slot);
}

int32_t pikamd_search_batch(pikamd_solver* s, const pikamd_params* p, int64_t B, const double* goal_pos_quat,
                            const double* seed, const double* initial_guess, uint64_t rng_seed, int64_t problem_offset,
                            int32_t max_attempts, double* solution, int32_t* status, double* final_cost,
                            pikamd_stats* stats, int32_t* attempts, double* all_solution, int32_t* all_status) {
    const SearchArrays h = {goal_pos_quat, seed, initial_guess, solution, status, final_cost, stats, attempts, all_solution, all_status};
    pik::ParamsK pk;
    if (int rc = check_call(SEARCH, s, p, B, max_attempts, h.required_null(), pk)) return rc;
    if (B == 0) return 0;
    if (int rc = maybe_self_test(s, p)) return rc; // (the local-mode kernel set, as pikamd_solve_batch)
    const pik::SearchOps* ops = search_ops_of(s, p);
    if (!ops) return no_kernels(s->chain.dof);
    if (int rc = search_validity(s, p, nullptr)) return rc;
    Staging st(s, SEARCH.name);
    if (int rc = st.begin()) return rc;
    SearchArrays d;
    if (int rc = stage_search(st, s, h, B, max_attempts, d)) return rc;
    pik::SearchArgs a;
    if (int rc = search_args(s, p, Staging::SLOT, B, max_attempts, d, rng_seed, problem_offset, a)) return rc;
    if (int rc = search_gate(s, pk, Staging::SLOT, st.stream(), a)) return rc;
    if (int rc = search_validity(s, p, &a)) return rc;
    if (int rc = st.upload()) return rc;
    return st.finish(ops->solve(s, pk, a, st.stream(), Staging::SLOT));
}

const char* pikamd_search_kernel_name(const pikamd_solver* s, const pikamd_params* p, int64_t B, int32_t max_attempts,
                                      int32_t* attempts_in_flight) {
    if (attempts_in_flight) *attempts_in_flight = 0;
    if (!s || !p || B < 0 || max_attempts < 1 || max_attempts > PIKAMD_MAX_ATTEMPTS) return "";
    const pik::SearchPlan plan = search_plan_of(s, p, B, max_attempts);
    if (attempts_in_flight) *attempts_in_flight = plan.parallel ? max_attempts : 1;
    return variant_name(s, flavour_of(s, p, nullptr), "search", plan.lanes);
}

} // extern "C"

namespace {

// The record of the memetic solves of a global-mode call of B problems: every attempt writes its rows, read by the
// step behind it.
pik::BatchRecord restart_record(int64_t B, const double* goal, const double* seed, const double* guess,
                                int64_t problem_offset, double* solution, int* status, double* cost, void* stats) {
    pik::BatchRecord rec;
    std::memset(&rec, 0, sizeof rec);
    rec.B = B;
    rec.goal = goal;
    rec.seed = seed;
    rec.guess = guess;
    rec.problem_offset = problem_offset;
    rec.solution = solution;
    rec.status = status;
    rec.cost = cost;
    rec.stats = stats;
    return rec;
}

// the open count of the slot's restart list, in its counter block
unsigned* restart_open_count(const pikamd_solver* s, int slot) {
    return (unsigned*)(s->counters + pik::COUNTER_BLOCK * (size_t)slot + 128);
}

// THE restart loop of a global-mode call on `stream`: up to K attempts of the memetic solver on `rec` -- attempt 0 by
// run_solve on every problem, an attempt behind it by the restart launcher on the open problems of `list` -- and behind
// every attempt the caller's step, behind(attempt, last), which folds the attempt's rows and writes the next list and
// its count (n_list).  The call is keyed by rng_seed (restart_attempt_seed); `who` names it in a PIKAMD_EHIP text.
// sync_between: the host-pointer entry point -- the open count is read back behind every step but the last, and no
// attempt is enqueued once it is zero; the stream-ordered entry point never synchronises here.  Every failure in here
// marks the slot's counters dirty (a launch that failed half-way leaves counters behind: the next call on the slot
// clears them, in here -- behind the caller's prepare kernel, which reads and writes no counter); what a caller does in
// front -- scratch, reserve, prepare, its lookups -- does not.
template <class Behind>
int run_restart_attempts(pikamd_solver* s, const pikamd_params* p, const pik::ParamsK& pk, const pik::RestartOps* ops,
                         pik::BatchRecord rec, const int* list, const unsigned* n_list, int K, uint64_t rng_seed,
                         const char* who, hipStream_t stream, int slot, bool sync_between, Behind behind) {
    auto give_up = [&](int rc) {
        s->counters_dirty[slot] = true;
        return rc;
    };
    if (s->counters_dirty[slot]) {
        HIP_TRY(hipMemsetAsync(s->counters + pik::COUNTER_BLOCK * (size_t)slot, 0, pik::COUNTER_BLOCK, stream));
        s->counters_dirty[slot] = false;
    }
    long long open = rec.B;
    for (int a = 0; a < K; ++a) {
        const bool last = a == K - 1;
        const unsigned long long seed_a = pik::restart_attempt_seed(rng_seed, a);
        if (a == 0) {
            if (int rc = run_solve(s, p, pk, &rec, 1, seed_a, stream, slot)) return give_up(rc);
        } else {
            pik::BatchRecord copy = rec; // (the launch fills in `start`)
            if (int rc = ops->attempt(s, p, pk, &copy, seed_a, list, sync_between ? open : -1, stream, slot))
                return give_up(rc);
        }
        if (int rc = behind(a, last)) return give_up(rc);
        if (sync_between && !last) {
            unsigned cnt = 0;
            hipError_t e = hipMemcpyAsync(&cnt, n_list, sizeof cnt, hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return give_up(fail(PIKAMD_EHIP, "%s: %s", who, hipGetErrorString(e)));
            open = (long long)cnt;
            if (open == 0) break;
        }
    }
    return 0;
}

// One pikamd_search_global_batch call on `stream` (device pointers in `r`: B, K, user_guess, the key, the primary
// outputs and all_*; goal / seed apart): the rows and lists in the slot's scratch, and behind an attempt the gate, the
// validity rows and the fold.
int run_search_global(pikamd_solver* s, const pikamd_params* p, const pik::ParamsK& pk, const pik::RestartOps* ops,
                      pik::RestartArgs r, const double* d_goal, const double* d_seed, hipStream_t stream, int slot,
                      bool sync_between) {
    const size_t n = (size_t)r.B, d = (size_t)s->chain.dof;
    // the slot's scratch: guess | row solution | row cost | row stats | row status | open | list
    const size_t off_guess = 0, off_sol = off_guess + sizeof(double) * d * n, off_cost = off_sol + sizeof(double) * d * n;
    const size_t off_stats = off_cost + sizeof(double) * n, off_status = off_stats + sizeof(pikamd_stats) * n;
    const size_t off_open = off_status + align8(sizeof(int32_t) * n), off_list = off_open + align8(sizeof(int32_t) * n);
    const size_t total = off_list + align8(sizeof(int32_t) * n);
    pik::DevBuf& buf = ext_of(s)->restart_rows[slot];
    if (int rc = buf.ensure(total)) return rc;
    if (int rc = ops->reserve(s, p, pk, r.B, slot)) return rc;
    char* w = (char*)buf.p;
    r.guess = (double*)(w + off_guess);
    r.row_solution = (double*)(w + off_sol);
    r.row_cost = (const double*)(w + off_cost);
    r.row_stats = w + off_stats;
    r.row_status = (int*)(w + off_status);
    r.open = (int*)(w + off_open);
    r.list = (int*)(w + off_list);
    r.n_list = restart_open_count(s, slot);
    r.every = (r.all_solution || r.all_status) ? 1 : 0;
    r.goal = d_goal;
    r.seed = d_seed;
    if (int rc = gate_for_call(s, pk, slot, stream, &r.gate, &r.gate_joint, &r.gate_params)) return rc;
    // the validity step behind the gate: the rows kernel of the sphere model, where the handle has one
    const pik::ValidityOps* vops = nullptr;
    if (int rc = validity_for_call(s, SEARCH_GLOBAL.name, &vops)) return rc;
    const pik::ValidityRows vr = {r.B, r.every, 0, r.open, r.row_solution, r.row_status, d_seed};
    if (int rc = ops->prepare(s, pk, r, stream, slot)) return rc;
    const pik::BatchRecord rec = restart_record(r.B, d_goal, d_seed, r.guess, r.problem_offset, r.row_solution, r.row_status,
                                                (double*)(w + off_cost), w + off_stats);
    return run_restart_attempts(s, p, pk, ops, rec, r.list, r.n_list, r.K, r.rng_seed, SEARCH_GLOBAL.name, stream, slot,
                                sync_between, [&](int attempt, bool last) {
        r.attempt = attempt;
        r.last = last ? 1 : 0;
        if (r.gate)
            if (int rc = ops->gate(s, pk, r, stream, slot)) return rc;
        if (vops)
            if (int rc = vops->rows(ext_of(s)->validity_dev.p, ext_of(s)->validity_model.n_spheres, vr, stream)) return rc;
        return ops->fold(s, pk, r, stream, slot);
    });
}

} // namespace

extern "C" {

int32_t pikamd_search_global_batch_device(pikamd_solver* s, const pikamd_params* p, int64_t B,
                                          const double* d_goal_pos_quat, const double* d_seed,
                                          const double* d_initial_guess, uint64_t rng_seed, int64_t problem_offset,
                                          int32_t max_attempts, double* d_solution, int32_t* d_status,
                                          double* d_final_cost, pikamd_stats* d_stats, int32_t* d_attempts,
                                          double* d_all_solution, int32_t* d_all_status, void* stream, int32_t slot) {
    const SearchArrays d = {d_goal_pos_quat, d_seed,  d_initial_guess, d_solution,     d_status,
                            d_final_cost,    d_stats, d_attempts,      d_all_solution, d_all_status};
    pik::ParamsK pk;
    if (int rc = check_call(SEARCH_GLOBAL, s, p, B, max_attempts, d.required_null(), pk)) return rc;
    if (int rc = check_slot(slot)) return rc;
    if (B == 0) return 0;
    // (no automatic self test here: stream-ordered, see pikamd_solve_batches_device)
    const pik::RestartOps* ops = restart_ops_of(s, p, pk);
    if (!ops) return no_kernels(s->chain.dof);
    HIP_TRY(hipSetDevice(s->device));
    return run_search_global(s, p, pk, ops, restart_args(B, max_attempts, d, rng_seed, problem_offset), d.goal, d.seed,
                             (hipStream_t)stream, slot, false);
}

int32_t pikamd_search_global_batch(pikamd_solver* s, const pikamd_params* p, int64_t B, const double* goal_pos_quat,
                                   const double* seed, const double* initial_guess, uint64_t rng_seed,
                                   int64_t problem_offset, int32_t max_attempts, double* solution, int32_t* status,
                                   double* final_cost, pikamd_stats* stats, int32_t* attempts, double* all_solution,
                                   int32_t* all_status) {
    const SearchArrays h = {goal_pos_quat, seed, initial_guess, solution, status, final_cost, stats, attempts, all_solution, all_status};
    pik::ParamsK pk;
    if (int rc = check_call(SEARCH_GLOBAL, s, p, B, max_attempts, h.required_null(), pk)) return rc;
    if (B == 0) return 0;
    if (int rc = maybe_self_test(s, p)) return rc; // (the GLOBAL-mode kernel set, as pikamd_solve_batch)
    const pik::RestartOps* ops = restart_ops_of(s, p, pk);
    if (!ops) return no_kernels(s->chain.dof);
    Staging st(s, SEARCH_GLOBAL.name);
    if (int rc = st.begin()) return rc;
    SearchArrays d;
    if (int rc = stage_search(st, s, h, B, max_attempts, d)) return rc;
    if (int rc = st.upload()) return rc;
    return st.finish(run_search_global(s, p, pk, ops, restart_args(B, max_attempts, d, rng_seed, problem_offset), d.goal,
                                       d.seed, st.stream(), Staging::SLOT, true));
}

} // extern "C"

// ---- Cartesian paths from a pose, memetic start (pik_globalpath.hpp) ---------------------------------
namespace {

// One call on `stream` (device pointers in `d`): the rows and lists in the slot's scratch, and the restart loop
// (run_restart_attempts) over the memetic solves of waypoint 0 with the tail kernel behind every attempt.
int run_search_global_paths(pikamd_solver* s, const pikamd_params* p, const pik::ParamsK& pk, const pik::RestartOps* rops,
                            const pik::GlobalPathOps* gops, int64_t P, int32_t W, int32_t K, const StartPathArrays& d,
                            uint64_t rng_seed, int64_t problem_offset, hipStream_t stream, int slot, bool sync_between) {
    const int g7 = 7 * s->n_tips;
    const pik::GlobalPathScratch l =
        pik::globalpath_scratch(P, W, K, s->chain.dof, g7, d.cost != nullptr, d.stats != nullptr);
    pik::DevBuf& buf = ext_of(s)->globalpath_rows[slot];
    if (int rc = buf.ensure(l.total)) return rc;
    if (int rc = rops->reserve(s, p, pk, P, slot)) return rc;
    char* w = (char*)buf.p;
    pik::GlobalPathArgs a = {};
    a.P = P;
    a.W = W;
    a.K = K;
    a.g7 = g7;
    a.goal = d.goal;
    a.seed = d.seed;
    a.user_guess = d.guess ? d.guess : d.seed;
    a.max_step = d.max_step;
    a.rng_seed = rng_seed;
    a.problem_offset = problem_offset;
    a.solution = d.solution;
    a.status = d.status;
    a.cost = d.cost;
    a.stats = d.stats;
    a.reached = d.reached;
    a.attempts = d.attempts;
    a.totals = d.totals;
    if (K > 1) {
        if (d.stats) a.row_stats = w + l.off_row_stats;
        if (d.cost) a.row_cost = (double*)(w + l.off_row_cost);
        a.row_solution = (double*)(w + l.off_row_solution);
        a.row_status = (int*)(w + l.off_row_status);
    }
    a.goal0 = (double*)(w + l.off_goal0);
    a.guess = (double*)(w + l.off_guess);
    a.m_solution = (const double*)(w + l.off_m_solution);
    a.m_cost = (const double*)(w + l.off_m_cost);
    a.m_stats = w + l.off_m_stats;
    a.m_status = (const int*)(w + l.off_m_status);
    a.best = (int*)(w + l.off_best);
    a.open = (int*)(w + l.off_open);
    a.list = (int*)(w + l.off_list);
    a.n_list = restart_open_count(s, slot);
    if (int rc = gops->prepare(s, pk, a, stream, slot)) return rc;
    const pik::BatchRecord rec = restart_record(P, a.goal0, d.seed, a.guess, problem_offset, (double*)(w + l.off_m_solution),
                                                (int*)(w + l.off_m_status), (double*)(w + l.off_m_cost), w + l.off_m_stats);
    return run_restart_attempts(s, p, pk, rops, rec, a.list, a.n_list, K, rng_seed, SEARCH_GLOBAL_PATHS.name, stream, slot,
                                sync_between, [&](int attempt, bool last) {
        a.attempt = attempt;
        a.last = last ? 1 : 0;
        return gops->tail(s, pk, a, stream, slot);
    });
}

} // namespace

extern "C" {

int32_t pikamd_search_global_paths_device(pikamd_solver* s, const pikamd_params* p, int64_t P, int32_t W,
                                          const double* d_goal_pos_quat, const double* d_seed,
                                          const double* d_initial_guess, const double* d_max_joint_step,
                                          uint64_t rng_seed, int64_t problem_offset, int32_t max_attempts,
                                          double* d_solution, int32_t* d_status, double* d_final_cost,
                                          pikamd_stats* d_stats, int32_t* d_reached, int32_t* d_attempts,
                                          pikamd_stats* d_totals, void* stream, int32_t slot) {
    const StartPathArrays d = {d_goal_pos_quat, d_seed,  d_initial_guess, d_max_joint_step, d_solution, d_status,
                               d_final_cost,    d_stats, d_reached,       d_attempts,       d_totals};
    pik::ParamsK pk;
    if (int rc = check_search_paths(SEARCH_GLOBAL_PATHS, s, p, P, W, max_attempts, d, pk)) return rc;
    if (int rc = check_slot(slot)) return rc;
    if (P == 0) return 0;
    // (no automatic self test here: stream-ordered, see pikamd_solve_batches_device)
    const pik::RestartOps* rops = restart_ops_of(s, p, pk);
    const pik::GlobalPathOps* gops = globalpath_ops_of(s, p);
    if (!rops || !gops) return no_kernels(s->chain.dof);
    HIP_TRY(hipSetDevice(s->device));
    return run_search_global_paths(s, p, pk, rops, gops, P, W, max_attempts, d, rng_seed, problem_offset,
                                   (hipStream_t)stream, slot, false);
}

int32_t pikamd_search_global_paths(pikamd_solver* s, const pikamd_params* p, int64_t P, int32_t W,
                                   const double* goal_pos_quat, const double* seed, const double* initial_guess,
                                   const double* max_joint_step, uint64_t rng_seed, int64_t problem_offset,
                                   int32_t max_attempts, double* solution, int32_t* status, double* final_cost,
                                   pikamd_stats* stats, int32_t* reached, int32_t* attempts, pikamd_stats* totals) {
    const StartPathArrays h = {goal_pos_quat, seed,  initial_guess, max_joint_step, solution, status,
                               final_cost,    stats, reached,       attempts,       totals};
    pik::ParamsK pk;
    if (int rc = check_search_paths(SEARCH_GLOBAL_PATHS, s, p, P, W, max_attempts, h, pk)) return rc;
    if (P == 0) return 0;
    // (both kernel sets: the GLOBAL-mode one of waypoint 0 and the local-mode one of the waypoints behind it)
    if (int rc = maybe_self_test(s, p)) return rc;
    pikamd_params p_local = *p;
    p_local.mode = 1;
    if (int rc = maybe_self_test(s, &p_local)) return rc;
    const pik::RestartOps* rops = restart_ops_of(s, p, pk);
    const pik::GlobalPathOps* gops = globalpath_ops_of(s, p);
    if (!rops || !gops) return no_kernels(s->chain.dof);
    Staging st(s, SEARCH_GLOBAL_PATHS.name);
    if (int rc = st.begin()) return rc;
    StartPathArrays dev;
    if (int rc = stage_startpath(st, s, h, P, W, dev)) return rc;
    if (int rc = st.upload()) return rc;
    return st.finish(run_search_global_paths(s, p, pk, rops, gops, P, W, max_attempts, dev, rng_seed, problem_offset,
                                             st.stream(), Staging::SLOT, true));
}

const char* pikamd_search_global_paths_kernel_name(const pikamd_solver* s, const pikamd_params* p, int64_t P) {
    return path_variant_name(s, p, P, "globalpath");
}

} // extern "C"

// ---- computeCartesianPath in one call (pik_cartesian.hpp, pik_interp.hpp) ---------------------------
namespace {

const CallKind CARTESIAN = {"pikamd_cartesian_paths", 1, "Cartesian motions are walked in local mode (mode = 1)", "", true,
                            "[P][W][dof]", "start"};

// what pikamd_interpolate_poses refuses of its parameter object (W apart)
int check_cartesian(const char* who, const pikamd_cartesian* c) {
    if (!c) return fail(PIKAMD_EINVAL, "%s: the pikamd_cartesian is NULL", who);
    if (c->frame < PIKAMD_CARTESIAN_GLOBAL || c->frame > PIKAMD_CARTESIAN_OFFSET)
        return fail(PIKAMD_EINVAL, "%s: frame %d: expected 0 (global), 1 (tip) or 2 (offset)", who, (int)c->frame);
    if (c->min_steps < 0) return fail(PIKAMD_EINVAL, "%s: min_steps %d: expected >= 0", who, (int)c->min_steps);
    if (!(c->max_translation > 0.0) && !(c->max_rotation > 0.0))
        return fail(PIKAMD_EINVAL, "%s: neither max_translation nor max_rotation is > 0: no step size", who);
    return 0;
}

pik_interp::Motion motion_of(const pikamd_cartesian* c) {
    return {(int)c->frame, pik::cartesian_min_steps(c->min_steps, c->jump_factor), c->max_translation, c->max_rotation};
}

// the arrays of a pikamd_cartesian_paths call: host pointers, or device pointers
struct CartesianArrays {
    const double *start, *target, *max_step;
    double* solution;
    int32_t* status;
    double* cost;
    pikamd_stats* stats;
    int32_t *reached, *steps;
    double *fraction, *goals;
};

// what the entry points of both Cartesian kinds (CARTESIAN, WAYPOINTS) refuse first: check_call's list for a path call
// of the kind (its arrays apart), the parameter object, several tip frames
int check_cartesian_call(const CallKind& kind, const pikamd_solver* s, const pikamd_params* p, const pikamd_cartesian* c,
                         int64_t P, int32_t W, pik::ParamsK& pk) {
    if (int rc = check_call(kind, s, p, P, W, false, pk)) return rc;
    if (int rc = check_cartesian(kind.name, c)) return rc;
    if (s->n_tips > 1)
        return fail(PIKAMD_EUNSUPPORTED, "%s: %d tip frames: a Cartesian motion is that of one tip frame", kind.name, s->n_tips);
    return 0;
}

// what both entry points refuse: check_cartesian_call's list, then the arrays
int check_cartesian_paths(const pikamd_solver* s, const pikamd_params* p, const pikamd_cartesian* c, int64_t P, int32_t W,
                          const CartesianArrays& d, pik::ParamsK& pk) {
    if (int rc = check_cartesian_call(CARTESIAN, s, p, c, P, W, pk)) return rc;
    if (!d.steps) return fail(PIKAMD_EINVAL, "%s: steps must not be NULL (a path with steps[p] > W was not walked)", CARTESIAN.name);
    if (P > 0 && (!d.start || !d.target || !d.solution || !d.status))
        return fail(PIKAMD_EINVAL, "%s: start, target, solution and status must not be NULL", CARTESIAN.name);
    return 0;
}

// registers the arrays of a synchronous call of P paths and W rows, allocates, and gives the device's
int stage_cartesian(Staging& st, const pikamd_solver* s, const CartesianArrays& h, int64_t P, int32_t W, CartesianArrays& dev) {
    static_assert(n_arrays<CartesianArrays>() <= Staging::MAX_REGIONS, "Staging::MAX_REGIONS");
    const size_t d = (size_t)s->chain.dof, paths = (size_t)P, rows = paths * (size_t)W;
    const int start = st.in(h.start, sizeof(double) * d * paths), target = st.in(h.target, sizeof(double) * 7 * paths);
    const int step = st.in(h.max_step, sizeof(double) * d);
    // (the outputs a caller left out are not written by the kernels either: no bytes -- the poses apart, which the
    // walk reads)
    const int sol = st.out(h.solution, sizeof(double) * d * rows, true), cost = st.out(h.cost, sizeof(double) * rows, false);
    const int stats = st.out(h.stats, sizeof(pikamd_stats) * rows, false), status = st.out(h.status, sizeof(int32_t) * rows, true);
    const int reached = st.out(h.reached, sizeof(int32_t) * paths, false), steps = st.out(h.steps, sizeof(int32_t) * paths, true);
    const int fraction = st.out(h.fraction, sizeof(double) * paths, false), goals = st.out(h.goals, sizeof(double) * 7 * rows, true);
    if (int rc = st.allocate()) return rc;
    dev = {st.at<const double>(start), st.at<const double>(target), st.at<const double>(step),  st.at<double>(sol),
           st.at<int32_t>(status),     st.at<double>(cost),         st.at<pikamd_stats>(stats), st.at<int32_t>(reached),
           st.at<int32_t>(steps),      st.at<double>(fraction),     st.at<double>(goals)};
    return 0;
}

pik::CartesianArgs cartesian_args(const pikamd_cartesian* c, int64_t P, int32_t W, const CartesianArrays& d) {
    pik::CartesianArgs a = {};
    a.path = path_args(P, W, {d.goals, d.start, d.max_step, d.solution, d.status, d.cost, d.stats, d.reached});
    a.target = d.target;
    a.goals = d.goals;
    a.steps = d.steps;
    a.fraction = d.fraction;
    a.frame = c->frame;
    a.min_steps = pik::cartesian_min_steps(c->min_steps, c->jump_factor);
    a.max_translation = c->max_translation;
    a.max_rotation = c->max_rotation;
    a.jump_factor = c->jump_factor;
    return a;
}

// The two steps of a call on `st`: the prepare kernel of the flavour pikamd_fk_batch runs in (the handle's), the walk
// of the flavour a path call with these parameters runs in.
int run_cartesian(pikamd_solver* s, const pikamd_params* p, const pik::ParamsK& pk, const pik::CartesianArgs& a,
                  hipStream_t st, int slot) {
    const int dof = s->chain.dof;
    const pik::CartesianOps* fk_ops = ops_at<pik::CartesianOps>(flavour_of(s, nullptr, nullptr), FAM_CARTESIAN, dof);
    const pik::CartesianOps* walk_ops = ops_at<pik::CartesianOps>(flavour_of(s, p, nullptr), FAM_CARTESIAN, dof);
    if (!fk_ops || !walk_ops) return no_kernels(dof);
    const pik::PathValidOps* vops = nullptr;
    if (int rc = path_validity_for_call(s, CARTESIAN.name, &vops)) return rc;
    if (int rc = fk_ops->prepare(s, pk, a, st, slot)) return rc;
    if (!vops) return walk_ops->walk(s, pk, a, st, slot);
    // with the validity step: the walk without the relative test (the prepare step above kept the caller's
    // jump_factor: the minimum step count depends on it), then the cut and cartesian_tail with the caller's
    pik::CartesianArgs walk = a;
    walk.jump_factor = 0.0;
    if (int rc = path_validity_reached(s, slot, a.path.P, a.path.reached, &walk.path.reached)) return rc;
    if (int rc = walk_ops->walk(s, pk, walk, st, slot)) return rc;
    return vops->cartesian(ext_of(s)->validity_dev.p, ext_of(s)->validity_model.n_spheres, a, walk.path.reached, st);
}

} // namespace

extern "C" {

int32_t pikamd_interpolate_poses(const pikamd_cartesian* c, int64_t P, int32_t W, const double* start_pose,
                                 const double* target, double* goals, int32_t* steps) {
    const char* const who = "pikamd_interpolate_poses";
    if (int rc = check_cartesian(who, c)) return rc;
    if (W < 1 || P < 0) return fail(PIKAMD_EINVAL, "%s: %lld paths of %d waypoints: expected P >= 0 and W >= 1", who, (long long)P, (int)W);
    if (!start_pose || !target || !goals || !steps)
        return fail(PIKAMD_EINVAL, "%s: start_pose, target, goals and steps must not be NULL", who);
    const pik_interp::Motion m = motion_of(c);
    for (int64_t i = 0; i < P; ++i) {
        double a[7], t[7];
        for (int e = 0; e < 7; ++e) {
            a[e] = start_pose[7 * i + e];
            t[e] = target[7 * i + e];
        }
        steps[i] = pik_interp::interpolate_path(m, W, a, t, goals + 7 * i * (int64_t)W);
    }
    return 0;
}

int32_t pikamd_cartesian_paths_device(pikamd_solver* s, const pikamd_params* p, const pikamd_cartesian* c, int64_t P,
                                      int32_t W, const double* d_start, const double* d_target,
                                      const double* d_max_joint_step, double* d_solution, int32_t* d_status,
                                      double* d_final_cost, pikamd_stats* d_stats, int32_t* d_reached,
                                      int32_t* d_steps, double* d_fraction, double* d_goals, void* stream,
                                      int32_t slot) {
    CartesianArrays d = {d_start, d_target, d_max_joint_step, d_solution, d_status, d_final_cost,
                         d_stats, d_reached, d_steps,         d_fraction, d_goals};
    pik::ParamsK pk;
    if (int rc = check_cartesian_paths(s, p, c, P, W, d, pk)) return rc;
    if (int rc = check_slot(slot)) return rc;
    if (P == 0) return 0;
    // (no automatic self test here: stream-ordered, see pikamd_solve_batches_device)
    HIP_TRY(hipSetDevice(s->device));
    if (!d.goals) {
        // the poses in the slot's scratch, which grows only past the largest earlier call on the slot
        pik::DevBuf& buf = ext_of(s)->cartesian_goals[slot];
        if (int rc = buf.ensure(sizeof(double) * 7 * (size_t)P * (size_t)W)) return rc;
        d.goals = (double*)buf.p;
    }
    return run_cartesian(s, p, pk, cartesian_args(c, P, W, d), (hipStream_t)stream, slot);
}

int32_t pikamd_cartesian_paths(pikamd_solver* s, const pikamd_params* p, const pikamd_cartesian* c, int64_t P,
                               int32_t W, const double* start, const double* target, const double* max_joint_step,
                               double* solution, int32_t* status, double* final_cost, pikamd_stats* stats,
                               int32_t* reached, int32_t* steps, double* fraction, double* goals) {
    const CartesianArrays h = {start, target, max_joint_step, solution, status, final_cost,
                               stats, reached, steps,          fraction, goals};
    pik::ParamsK pk;
    if (int rc = check_cartesian_paths(s, p, c, P, W, h, pk)) return rc;
    if (P == 0) return 0;
    if (int rc = maybe_self_test(s, p)) return rc; // (the local-mode kernel set, as pikamd_solve_batch)
    Staging st(s, CARTESIAN.name);
    if (int rc = st.begin()) return rc;
    CartesianArrays dev;
    if (int rc = stage_cartesian(st, s, h, P, W, dev)) return rc;
    if (int rc = st.upload()) return rc;
    return st.finish(run_cartesian(s, p, pk, cartesian_args(c, P, W, dev), st.stream(), Staging::SLOT));
}

const char* pikamd_cartesian_kernel_name(const pikamd_solver* s, const pikamd_params* p, int64_t P) {
    return path_variant_name(s, p, P, "cartesian", false);
}

} // extern "C"

// ---- computeCartesianPath through waypoints (pik_polyline.hpp) ---------------------------------------
namespace {

const CallKind WAYPOINTS = {"pikamd_cartesian_waypoints", 1, "Cartesian motions are walked in local mode (mode = 1)", "", true,
                            "[P][W][dof]", "start"};

// the arrays of a pikamd_cartesian_waypoints call: host pointers, or device pointers
struct WaypointArrays {
    const double *start, *targets;
    const int32_t* n_targets;
    const double* max_step;
    double* solution;
    int32_t* status;
    double* cost;
    pikamd_stats* stats;
    int32_t *reached, *steps, *segment_steps;
    double *fraction, *goals;
};

// what both entry points refuse: check_cartesian_call's list, then the target list's own and the arrays
int check_cartesian_waypoints(const pikamd_solver* s, const pikamd_params* p, const pikamd_cartesian* c, int64_t P, int32_t S,
                              int32_t W, const WaypointArrays& d, pik::ParamsK& pk) {
    const char* const who = WAYPOINTS.name;
    if (int rc = check_cartesian_call(WAYPOINTS, s, p, c, P, W, pk)) return rc;
    if (!d.steps) return fail(PIKAMD_EINVAL, "%s: steps must not be NULL (a path with steps[p] > W has a segment that did not fit)", who);
    if (S < 1) return fail(PIKAMD_EINVAL, "%s: %d targets per path: expected S >= 1", who, (int)S);
    if (S > W) return fail(PIKAMD_EINVAL, "%s: %d targets in %d rows: expected S <= W (every segment needs a row)", who, (int)S, (int)W);
    if (P > 0 && (!d.start || !d.targets || !d.solution || !d.status))
        return fail(PIKAMD_EINVAL, "%s: start, targets, solution and status must not be NULL", who);
    return 0;
}

// registers the arrays of a synchronous call of P paths, S targets and W rows, allocates, and gives the device's
int stage_waypoints(Staging& st, const pikamd_solver* s, const WaypointArrays& h, int64_t P, int32_t S, int32_t W,
                    WaypointArrays& dev) {
    static_assert(n_arrays<WaypointArrays>() <= Staging::MAX_REGIONS, "Staging::MAX_REGIONS");
    const size_t d = (size_t)s->chain.dof, paths = (size_t)P, rows = paths * (size_t)W, segs = paths * (size_t)S;
    const int start = st.in(h.start, sizeof(double) * d * paths), targets = st.in(h.targets, sizeof(double) * 7 * segs);
    const int count = st.in(h.n_targets, sizeof(int32_t) * paths), step = st.in(h.max_step, sizeof(double) * d);
    // (the outputs a caller left out are not written by the kernels either: no bytes -- the poses apart, which the
    // walk reads)
    const int sol = st.out(h.solution, sizeof(double) * d * rows, true), cost = st.out(h.cost, sizeof(double) * rows, false);
    const int stats = st.out(h.stats, sizeof(pikamd_stats) * rows, false), status = st.out(h.status, sizeof(int32_t) * rows, true);
    const int reached = st.out(h.reached, sizeof(int32_t) * paths, false), steps = st.out(h.steps, sizeof(int32_t) * paths, true);
    const int segsteps = st.out(h.segment_steps, sizeof(int32_t) * segs, false);
    const int fraction = st.out(h.fraction, sizeof(double) * paths, false), goals = st.out(h.goals, sizeof(double) * 7 * rows, true);
    if (int rc = st.allocate()) return rc;
    dev = {st.at<const double>(start), st.at<const double>(targets), st.at<const int32_t>(count), st.at<const double>(step),
           st.at<double>(sol),         st.at<int32_t>(status),       st.at<double>(cost),         st.at<pikamd_stats>(stats),
           st.at<int32_t>(reached),    st.at<int32_t>(steps),        st.at<int32_t>(segsteps),    st.at<double>(fraction),
           st.at<double>(goals)};
    return 0;
}

// The passes of a call on `st`: per segment the segment kernel of the flavour pikamd_fk_batch runs in (the handle's)
// and the walk of the flavour a path call with these parameters runs in; the finish behind them.  `state`: the
// per-path state (polyline_state_bytes) in the slot's scratch.
int run_polyline(pikamd_solver* s, const pikamd_params* p, const pik::ParamsK& pk, const pikamd_cartesian* c, int64_t P,
                 int32_t S, int32_t W, const WaypointArrays& d, void* state, hipStream_t st, int slot) {
    const int dof = s->chain.dof;
    const pik::PolylineOps* fk_ops = ops_at<pik::PolylineOps>(flavour_of(s, nullptr, nullptr), FAM_POLYLINE, dof);
    const pik::PolylineOps* walk_ops = ops_at<pik::PolylineOps>(flavour_of(s, p, nullptr), FAM_POLYLINE, dof);
    if (!fk_ops || !walk_ops) return no_kernels(dof);
    const pik::PathValidOps* vops = nullptr;
    if (int rc = path_validity_for_call(s, WAYPOINTS.name, &vops)) return rc;
    pik::PolylineArgs a = {};
    a.path = path_args(P, W, {d.goals, d.start, d.max_step, d.solution, d.status, d.cost, d.stats, d.reached});
    a.targets = d.targets;
    a.n_targets = d.n_targets;
    a.goals = d.goals;
    a.steps = d.steps;
    a.segment_steps = d.segment_steps;
    a.fraction = d.fraction;
    a.st = pik::polyline_state_at(state, P);
    a.S = S;
    a.frame = c->frame;
    a.min_steps = pik::cartesian_min_steps(c->min_steps, 0.0); // (no jump test per segment: MoveIt's minimum is 1)
    a.max_translation = c->max_translation;
    a.max_rotation = c->max_rotation;
    a.jump_factor = c->jump_factor;
    for (int i = 0; i < S; ++i) {
        a.seg = i;
        if (int rc = fk_ops->segment(s, pk, a, st, slot)) return rc;
        if (int rc = walk_ops->walk(s, pk, a, st, slot)) return rc;
        // (pikamd_set_path_validity: the cut of this segment, in front of the next segment kernel)
        if (vops)
            if (int rc = vops->segment(ext_of(s)->validity_dev.p, ext_of(s)->validity_model.n_spheres, a, st)) return rc;
    }
    return walk_ops->finish(s, pk, a, st, slot);
}

} // namespace

extern "C" {

int32_t pikamd_cartesian_waypoints_device(pikamd_solver* s, const pikamd_params* p, const pikamd_cartesian* c, int64_t P,
                                          int32_t S, int32_t W, const double* d_start, const double* d_targets,
                                          const int32_t* d_n_targets, const double* d_max_joint_step, double* d_solution,
                                          int32_t* d_status, double* d_final_cost, pikamd_stats* d_stats,
                                          int32_t* d_reached, int32_t* d_steps, int32_t* d_segment_steps,
                                          double* d_fraction, double* d_goals, void* stream, int32_t slot) {
    WaypointArrays d = {d_start,  d_targets, d_n_targets, d_max_joint_step, d_solution,  d_status,  d_final_cost,
                        d_stats,  d_reached, d_steps,     d_segment_steps,  d_fraction,  d_goals};
    pik::ParamsK pk;
    if (int rc = check_cartesian_waypoints(s, p, c, P, S, W, d, pk)) return rc;
    if (int rc = check_slot(slot)) return rc;
    if (P == 0) return 0;
    // (no automatic self test here: stream-ordered, see pikamd_solve_batches_device)
    HIP_TRY(hipSetDevice(s->device));
    // the per-path state and, without d_goals, the poses in the slot's scratch, which grows only past the largest
    // earlier call on the slot
    const size_t state = align8(pik::polyline_state_bytes(P));
    pik::DevBuf& buf = ext_of(s)->polyline_rows[slot];
    if (int rc = buf.ensure(state + (d.goals ? 0 : sizeof(double) * 7 * (size_t)P * (size_t)W))) return rc;
    if (!d.goals) d.goals = reinterpret_cast<double*>((char*)buf.p + state);
    return run_polyline(s, p, pk, c, P, S, W, d, buf.p, (hipStream_t)stream, slot);
}

int32_t pikamd_cartesian_waypoints(pikamd_solver* s, const pikamd_params* p, const pikamd_cartesian* c, int64_t P,
                                   int32_t S, int32_t W, const double* start, const double* targets,
                                   const int32_t* n_targets, const double* max_joint_step, double* solution,
                                   int32_t* status, double* final_cost, pikamd_stats* stats, int32_t* reached,
                                   int32_t* steps, int32_t* segment_steps, double* fraction, double* goals) {
    const WaypointArrays h = {start, targets, n_targets, max_joint_step, solution, status, final_cost,
                              stats, reached, steps,     segment_steps,  fraction, goals};
    pik::ParamsK pk;
    if (int rc = check_cartesian_waypoints(s, p, c, P, S, W, h, pk)) return rc;
    if (P == 0) return 0;
    if (int rc = maybe_self_test(s, p)) return rc; // (the local-mode kernel set, as pikamd_solve_batch)
    Staging st(s, WAYPOINTS.name);
    if (int rc = st.begin()) return rc;
    WaypointArrays dev;
    if (int rc = stage_waypoints(st, s, h, P, S, W, dev)) return rc;
    // (the per-path state: a buffer of its own, in the slot's scratch)
    pik::DevBuf& state = ext_of(s)->polyline_rows[Staging::SLOT];
    if (int rc = state.ensure(pik::polyline_state_bytes(P))) return rc;
    if (int rc = st.upload()) return rc;
    return st.finish(run_polyline(s, p, pk, c, P, S, W, dev, state.p, st.stream(), Staging::SLOT));
}

const char* pikamd_cartesian_waypoints_kernel_name(const pikamd_solver* s, const pikamd_params* p, int64_t P) {
    return path_variant_name(s, p, P, "polyline", false);
}

} // extern "C"

extern "C" {

// ---- the approximate-solution gate (src/pick_ik_plugin.cpp:219-267) --------------------------------

int32_t pikamd_set_approximate_gate(pikamd_solver* s, const pikamd_gate* gate) {
    if (int rc = check_solver(s)) return rc;
    SolverExt* x = ext_of(s);
    x->gate_set = gate != nullptr;
    if (gate) x->gate = *gate;
    return 0;
}

// ---- the validity model inside the path entry points that start from a joint state (pik_pathvalid.hpp) ----
int32_t pikamd_set_path_validity(pikamd_solver* s, int32_t on) {
    if (on != 0 && on != 1) return fail(PIKAMD_EINVAL, "pikamd_set_path_validity: on = %d: expected 0 or 1", (int)on);
    if (int rc = check_solver(s)) return rc;
    ext_of(s)->path_validity = on;
    return 0;
}

// ---- the sphere validity model (the solution callback's place, src/pick_ik_plugin.cpp:269-274) -------
int32_t pikamd_set_validity_model(pikamd_solver* s, const pikamd_validity_model* m) {
    if (int rc = check_solver(s)) return rc;
    SolverExt* x = ext_of(s);
    if (!m) {
        x->validity_set = false;
        return 0;
    }
    const char* who = "pikamd_set_validity_model";
    if (m->n_spheres < 0 || m->n_spheres > PIKAMD_MAX_SPHERES)
        return fail(PIKAMD_EINVAL, "%s: n_spheres %d: expected 0..%d", who, (int)m->n_spheres, PIKAMD_MAX_SPHERES);
    if (m->n_pairs < 0 || m->n_pairs > PIKAMD_MAX_SPHERE_PAIRS)
        return fail(PIKAMD_EINVAL, "%s: n_pairs %d: expected 0..%d", who, (int)m->n_pairs, PIKAMD_MAX_SPHERE_PAIRS);
    if ((m->n_spheres > 0 && !m->spheres) || (m->n_pairs > 0 && !m->pairs))
        return fail(PIKAMD_EINVAL, "%s: spheres / pairs must not be NULL", who);
    if (int rc = validity_chain_ok(s, who)) return rc;
    const int dof = s->chain.dof;
    for (int k = 0; k < m->n_spheres; ++k) {
        const pikamd_sphere& sp = m->spheres[k];
        if (!(std::isfinite(sp.radius) && sp.radius >= 0.0 && std::isfinite(sp.centre[0]) && std::isfinite(sp.centre[1]) &&
              std::isfinite(sp.centre[2])))
            return fail(PIKAMD_EINVAL, "%s: sphere %d: centre and radius must be finite, the radius not below 0", who, k);
        if (sp.after_variable < -1 || sp.after_variable >= dof)
            return fail(PIKAMD_EINVAL, "%s: sphere %d: after_variable %d: expected -1..%d", who, k, (int)sp.after_variable, dof - 1);
        if (sp.after_variable >= 0 && ((x->planar_xy_mask >> sp.after_variable) & 1u))
            return fail(PIKAMD_EINVAL, "%s: sphere %d: after_variable %d is the x or y slot of a planar joint (name its theta)",
                        who, k, (int)sp.after_variable);
    }
    for (int p = 0; p < m->n_pairs; ++p) {
        const int a = m->pairs[2 * p], b = m->pairs[2 * p + 1];
        if (a < 0 || a >= m->n_spheres || b < 0 || b >= m->n_spheres || a == b)
            return fail(PIKAMD_EINVAL, "%s: pair %d = (%d, %d): two different spheres of 0..%d expected", who, p, a, b,
                        (int)m->n_spheres - 1);
    }
    const pik::ValidityOps* ops = validity_ops_of(s);
    if (!ops) return no_kernels(dof);
    // the kernels' copy: the spheres in chain order (stable), the caller's numbering kept beside them
    pik::ValidityModelK k;
    std::memset(&k, 0, sizeof k);
    k.n_spheres = m->n_spheres;
    k.n_pairs = m->n_pairs;
    int n = 0;
    for (int v = -1; v < dof; ++v)
        for (int i = 0; i < m->n_spheres; ++i) {
            const pikamd_sphere& sp = m->spheres[i];
            if (sp.after_variable != v) continue;
            k.after[n] = v;
            k.index[n] = i;
            for (int c = 0; c < 3; ++c) k.centre[n][c] = sp.centre[c];
            if (sp.centre[0] == 0.0 && sp.centre[1] == 0.0 && sp.centre[2] == 0.0) k.zero_mask |= 1u << n;
            ++n;
        }
    for (int i = 0; i < m->n_spheres; ++i) k.radius[i] = m->spheres[i].radius;
    for (int p = 0; p < 2 * m->n_pairs; ++p) k.pairs[p / 2][p % 2] = m->pairs[p];
    std::vector<char> image(ops->image_bytes);
    ops->pack(s, k, image.data());
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize()); // (no kernel in flight reads the image that is rewritten)
    x->validity_set = false;
    if (int rc = x->validity_dev.ensure(image.size())) return rc;
    HIP_TRY(hipMemcpy(x->validity_dev.p, image.data(), image.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    x->validity_model = k;
    x->validity_set = true;
    return 0;
}

// what both validity entry points refuse
static int check_validity_call(pikamd_solver* s, int64_t n, const void* q, const void* valid, const pik::ValidityOps** ops) {
    if (int rc = check_solver(s)) return rc;
    const char* who = "pikamd_validity_batch";
    if (!ext_of(s)->validity_set) return fail(PIKAMD_EINVAL, "%s: the handle has no validity model (pikamd_set_validity_model)", who);
    if (n < 0) return fail(PIKAMD_EINVAL, "%s: n = %lld: expected n >= 0", who, (long long)n);
    if (n > 0 && (!q || !valid)) return fail(PIKAMD_EINVAL, "%s: q and valid must not be NULL", who);
    if (s->opt.soa) return fail(PIKAMD_EINVAL, "joint_layout soa: not with %s (its arrays are [n][dof])", who);
    if (int rc = validity_chain_ok(s, who)) return rc;
    *ops = validity_ops_of(s);
    return *ops ? 0 : no_kernels(s->chain.dof);
}

int32_t pikamd_validity_batch_device(pikamd_solver* s, int64_t n, const double* d_q, int32_t* d_valid,
                                     double* d_clearance, double* d_centres, void* stream) {
    const pik::ValidityOps* ops = nullptr;
    if (int rc = check_validity_call(s, n, d_q, d_valid, &ops)) return rc;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(s->device));
    return ops->check(ext_of(s)->validity_dev.p, ext_of(s)->validity_model.n_spheres, n, d_q, d_valid, d_clearance,
                      d_centres, (hipStream_t)stream);
}

int32_t pikamd_validity_batch(pikamd_solver* s, int64_t n, const double* q, int32_t* valid, double* clearance,
                              double* centres) {
    const pik::ValidityOps* ops = nullptr;
    if (int rc = check_validity_call(s, n, q, valid, &ops)) return rc;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(s->device));
    const size_t d = (size_t)s->chain.dof, N = (size_t)n, n3 = 3 * (size_t)ext_of(s)->validity_model.n_spheres;
    const size_t sz[4] = {sizeof(double) * d * N, sizeof(int32_t) * N, sizeof(double) * N, sizeof(double) * n3 * N};
    for (int i = 0; i < 4; ++i)
        if (int rc = s->stage[i].ensure(sz[i])) return rc;
    HIP_TRY(hipMemcpy(s->stage[0].p, q, sz[0], hipMemcpyHostToDevice));
    if (int rc = pikamd_validity_batch_device(s, n, (const double*)s->stage[0].p, (int32_t*)s->stage[1].p,
                                              clearance ? (double*)s->stage[2].p : nullptr,
                                              (centres && n3) ? (double*)s->stage[3].p : nullptr, nullptr))
        return rc;
    HIP_TRY(hipMemcpy(valid, s->stage[1].p, sz[1], hipMemcpyDeviceToHost));
    if (clearance) HIP_TRY(hipMemcpy(clearance, s->stage[2].p, sz[2], hipMemcpyDeviceToHost));
    if (centres && n3) HIP_TRY(hipMemcpy(centres, s->stage[3].p, sz[3], hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

// the definition of the header, literally: pikamd_cost_batch under p', then the joint test
int32_t pikamd_gate_batch(pikamd_solver* s, const pikamd_params* p, const pikamd_gate* gate, int64_t n,
                          const double* goal_pos_quat, const double* seed, const double* q, int32_t* pass) {
    if (int rc = check_solver(s)) return rc;
    if (!p) return fail(PIKAMD_EINVAL, "params is NULL");
    if (!gate || !goal_pos_quat || !seed || !q || !pass)
        return fail(PIKAMD_EINVAL, "pikamd_gate_batch: gate, goal_pos_quat, seed, q and pass must not be NULL");
    if (n < 0) return fail(PIKAMD_EINVAL, "pikamd_gate_batch: n = %lld: expected n >= 0", (long long)n);
    if (s->opt.soa) return fail(PIKAMD_EINVAL, "joint_layout soa: not with pikamd_gate_batch (its arrays are [n][dof])");
    if (n == 0) return 0;
    pikamd_params pg = *p;
    if (gate->cost_threshold > 0.0) {
        pg.cost_threshold = gate->cost_threshold;
    } else {
        pg.center_joints_weight = pg.avoid_joint_limits_weight = pg.minimal_displacement_weight = 0.0;
    }
    if (int rc = pikamd_cost_batch(s, &pg, n, goal_pos_quat, seed, q, nullptr, pass)) return rc;
    if (gate->joint_threshold > 0.0) {
        const size_t d = (size_t)s->chain.dof;
        for (size_t i = 0; i < (size_t)n; ++i)
            for (size_t j = 0; j < d; ++j)
                if (std::fabs(q[i * d + j] - seed[i * d + j]) > gate->joint_threshold) pass[i] = 0;
    }
    return 0;
}

} // extern "C"

extern "C" {

// ---- the routed launcher's record (tests, profile scripts) ----------------------------------------

int32_t pikamd_debug_regime(pikamd_solver* s, int32_t slot, int64_t publish_load, int32_t max_passes,
                            int32_t* n_passes, uint32_t* survivors, uint32_t* others_load, int32_t* variant) {
    if (int rc = check_solver(s)) return rc;
    if (slot < 0 || slot >= pik::N_SLOTS) return fail(PIKAMD_EINVAL, "slot out of range");
    if (max_passes < 0 || (max_passes > 0 && (!survivors || !others_load || !variant)))
        return fail(PIKAMD_EINVAL, "bad arguments");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize()); // (the routers of the calls in flight write what is read and overwritten here)
    if (publish_load >= 0) {
        const uint32_t v = publish_load > 0xffffffffll ? 0xffffffffu : (uint32_t)publish_load;
        HIP_TRY(hipMemcpy(pik::route_loads(s) + slot, &v, sizeof v, hipMemcpyHostToDevice));
    }
    const int routed = ext_of(s)->routed_passes[slot];
    if (n_passes) *n_passes = routed;
    if (routed > 0 && max_passes > 0) {
        uint32_t rec[pik::ROUTE_MAX_PASSES * 4];
        HIP_TRY(hipMemcpy(rec, pik::route_record(s, slot), sizeof rec, hipMemcpyDeviceToHost));
        for (int k = 0; k < routed && k < max_passes; ++k) {
            survivors[k] = rec[4 * k + 0];
            others_load[k] = rec[4 * k + 1];
            variant[k] = (int32_t)rec[4 * k + 2];
        }
    }
    return 0;
}

} // extern "C"
