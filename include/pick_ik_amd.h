/*
 * pick_ik_amd.h -- C ABI of the MI355X-native batched IK solver (libpick_ik_amd.so).
 *
 * This is the boundary a MoveIt-side maintainer binds: pick_ik's plugin
 * (reference src/pick_ik_plugin.cpp:73-294) builds cost_fn/solution_fn closures and calls
 * ik_memetic()/ik_gradient() once per pose; this library takes the same inputs as plain arrays
 * (B = 1 from the plugin shim, B = thousands..millions from batch callers) and runs the whole
 * solve on the GPU.  No torch / Eigen / MoveIt types appear in any signature.
 *
 * Conventions
 *   - every function returns 0 on success or a negative PIKAMD_E* code and never throws;
 *     pikamd_last_error() returns a thread-local message for the last failure on this thread.
 *   - *_batch entry points take HOST pointers and do their own H2D/D2H;
 *     *_device entry points take DEVICE pointers (HBM-resident inputs/outputs) plus a hipStream_t
 *     passed as void* and only enqueue work -- nothing is synchronised.
 *   - all floating point is IEEE-754 binary64, exactly like the reference (double / Eigen::Isometry3d).
 *   - a solver handle is bound to one GPU and is not thread-safe (one handle per host thread/GPU).
 *   - there is NO CPU fallback: every entry point fails with PIKAMD_ENODEVICE when no gfx950
 *     device is available.
 */
#ifndef PICK_IK_AMD_H
#define PICK_IK_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIKAMD_MAX_DOF 16 /* variables of a chain; the kernels are instantiated for 1..16 */

/* status[] values: moveit_msgs::msg::MoveItErrorCodes as used in src/pick_ik_plugin.cpp:209-217 */
#define PIKAMD_SUCCESS 1
#define PIKAMD_APPROXIMATE 2 /* best-so-far returned because return_approximate_solution was set
                                (src/ik_memetic.cpp:277-280, src/ik_gradient.cpp:135-137) */
#define PIKAMD_NO_IK_SOLUTION (-31)

/* error codes */
#define PIKAMD_EINVAL (-1)
#define PIKAMD_ENODEVICE (-2)
#define PIKAMD_EHIP (-3)
#define PIKAMD_EUNSUPPORTED (-4)

#define PIKAMD_JOINT_REVOLUTE 0
#define PIKAMD_JOINT_PRISMATIC 1
/* A PLANAR joint (moveit::core::PlanarJointModel, the usual virtual joint of a mobile base; the
 * reference reaches it through RobotState, src/forward_kinematics.cpp:72-79 / src/fk_moveit.cpp): three
 * variables x, y, theta with computeTransform = Translation(x, y, 0) * AngleAxis(theta, UnitZ) in the
 * joint frame, i.e. exactly a prismatic joint along x, one along y and a revolute one about z with
 * identity origins in between.  Its variables occupy three consecutive slots of the chain arrays:
 * _X carries the joint's origin, _Y and _THETA follow immediately (their origin / axis entries are
 * ignored); qmin / qmax / vmax / bounded are per variable as for every joint (pick_ik treats the
 * variables of a multi-variable joint independently, src/robot.cpp:144-150). */
#define PIKAMD_JOINT_PLANAR_X 2
#define PIKAMD_JOINT_PLANAR_Y 3
#define PIKAMD_JOINT_PLANAR_THETA 4
/* A FLOATING joint (moveit::core::FloatingJointModel, the virtual joint of a free-flying base; the
 * reference states its frame in src/forward_kinematics.cpp:64-70 and reaches it live through
 * RobotState, src/fk_moveit.cpp:22-31): seven variables trans_x trans_y trans_z rot_x rot_y rot_z rot_w
 * in seven consecutive slots and ONE transform,
 *     Translation3d(v[0], v[1], v[2]) * Quaterniond(w = v[6], x = v[3], y = v[4], z = v[5]),
 * the quaternion taken as it is (Eigen toRotationMatrix of the unnormalised value -- what MoveIt
 * multiplies in; pick_ik treats the seven variables independently, src/robot.cpp:144-150, so the
 * search moves them one by one between their bounds).  _TX carries the joint's origin; axis entries
 * are ignored.  These variables are not single-axis motions: a chain with a floating joint runs the
 * literal kernels (MoveIt's chain product and 2 dof + 3 evaluations per gradient step, the arithmetic
 * the verification build checks bit for bit against the oracle), not the Denavit-Hartenberg ones. */
#define PIKAMD_JOINT_FLOATING_TX 5
#define PIKAMD_JOINT_FLOATING_TY 6
#define PIKAMD_JOINT_FLOATING_TZ 7
#define PIKAMD_JOINT_FLOATING_RX 8
#define PIKAMD_JOINT_FLOATING_RY 9
#define PIKAMD_JOINT_FLOATING_RZ 10
#define PIKAMD_JOINT_FLOATING_RW 11

/* Serial chain base -> tip; replaces what Robot::from / make_fk_fn pull out of the MoveIt
 * RobotModel (src/robot.cpp:44-85, src/fk_moveit.cpp:11-35).  Fixed joints are collapsed into the
 * next joint's origin; the fixed links after the last actuated joint are collapsed into tip. */
typedef struct pikamd_chain {
    int32_t dof;
    const double* origin_xyz_rpy; /* [dof][6] URDF <origin xyz rpy> of each joint           */
    const double* axis;           /* [dof][3] joint axis (normalised internally)            */
    const int32_t* joint_type;    /* [dof] PIKAMD_JOINT_*; NULL = all revolute              */
    const double* tip_xyz_rpy;    /* [6]  fixed transform after the last joint              */
    const double* qmin;           /* [dof] position bounds                                  */
    const double* qmax;           /* [dof]                                                  */
    const double* vmax;           /* [dof] max velocity (minimal-displacement weights); NULL = 0 */
    const uint8_t* bounded;       /* [dof] position_bounded_; NULL = all bounded            */
} pikamd_chain;

/* Several tip links -- the plugin's tip_frames (src/pick_ik_plugin.cpp:57-69; one pose cost and one
 * frame test per tip, src/goal.cpp:27-49, 80-89; the active variables are the union of the joints on
 * the way to any tip, src/robot.cpp:130-160).  Each tip is described by the joints on ITS path from
 * the base, like a chain of its own; a joint shared by several tips (a torso) appears in every such
 * path with the same variable index.  With a multi-tip solver every goal / pose array of this API
 * holds n_tips consecutive poses per problem: goal_pos_quat [B][n_tips][7], fk -> [n][n_tips][7]. */
#define PIKAMD_MAX_TIPS 8
typedef struct pikamd_tip {
    int32_t n_joints;
    const int32_t* variable;      /* [n_joints] index of each joint's variable, strictly increasing */
    const double* origin_xyz_rpy; /* [n_joints][6] */
    const double* axis;           /* [n_joints][3] */
    const int32_t* joint_type;    /* [n_joints]; NULL = all revolute */
    const double* tip_xyz_rpy;    /* [6] */
} pikamd_tip;
typedef struct pikamd_multi_chain {
    int32_t dof;    /* number of active variables */
    int32_t n_tips; /* 1 .. PIKAMD_MAX_TIPS */
    const pikamd_tip* tips;
    const double* qmin; /* [dof] */
    const double* qmax;
    const double* vmax;     /* NULL = 0 */
    const uint8_t* bounded; /* NULL = all bounded */
} pikamd_multi_chain;

/* Mirrors src/pick_ik_parameters.yaml (same names, same defaults) minus the wall-clock limits
 * (memetic_gd_max_time, the plugin timeout): iteration budgets bind instead. */
typedef struct pikamd_params {
    int32_t mode; /* 0 = "global" (memetic, src/ik_memetic.cpp), 1 = "local" (src/ik_gradient.cpp) */
    double gd_step_size;
    int32_t gd_max_iters;
    double gd_min_cost_delta;
    double position_threshold;
    double orientation_threshold;
    double cost_threshold;
    double position_scale;
    double rotation_scale;
    double center_joints_weight;
    double avoid_joint_limits_weight;
    double minimal_displacement_weight;
    int32_t stop_optimization_on_valid_solution;
    int32_t memetic_num_threads; /* species (lock-step on the GPU); pow2ceil(it) * pow2ceil(elite_size) <= 64 */
    int32_t memetic_stop_on_first_solution;
    int32_t memetic_population_size;
    int32_t memetic_elite_size;
    double memetic_wipeout_fitness_tol;
    int32_t memetic_max_generations;
    int32_t memetic_gd_max_iters;
    int32_t return_approximate_solution; /* KinematicsQueryOptions::return_approximate_solution */
} pikamd_params;

/* per-problem counters (optional output) */
typedef struct pikamd_stats {
    int64_t cost_evals;  /* cost_fn invocations the reference algorithm makes for this solve */
    int32_t generations; /* memetic generations run / gd iterations in local mode */
    int32_t wipeouts;
    int32_t pool_erasures;
    int32_t reserved;
} pikamd_stats;

typedef struct pikamd_solver pikamd_solver;

/* yaml defaults */
void pikamd_default_params(pikamd_params* p);

/* Replaces PickIKPlugin::initialize's model extraction (src/pick_ik_plugin.cpp:22-71).
 * device_ordinal: HIP device index (>= 0). */
int32_t pikamd_create(const pikamd_chain* chain, int32_t device_ordinal, pikamd_solver** out);
int32_t pikamd_create_multi(const pikamd_multi_chain* chain, int32_t device_ordinal,
                            pikamd_solver** out);
int32_t pikamd_n_tips(const pikamd_solver* s); /* 1 for a solver made by pikamd_create */

/* Mimic joints on a tip path.  A mimic joint is no variable (src/robot.cpp:144-150 keeps it out of the active
 * variables), but the reference's forward kinematics moves it with its master: RobotState::setJointGroupPositions
 * (src/fk_moveit.cpp:22) ends in updateMimicJoints, i.e. the joint sits at multiplier * q[master] + offset.  Such a
 * joint is one more step of the chain product whose value follows a variable; it is declared here, behind the
 * variable whose joint it follows on the path.  The origins of the chain description are split accordingly: the
 * mimic joint's origin is the fixed transform from the previous moving joint of the path to it, and the next
 * joint's origin starts behind it.  (A mimic joint with multiplier 0 is a constant joint: fold it into the next
 * origin instead.)  Chains with mimic joints are solved by the exact kernels (like chains with a floating joint:
 * the Denavit-Hartenberg form has one variable per step).  Call before the first solve; n = 0 removes them. */
#define PIKAMD_MAX_MIMIC 4 /* per tip path */
typedef struct pikamd_mimic_joint {
    int32_t tip;             /* the tip path it lies on (0 for a solver made by pikamd_create) */
    int32_t after_variable;  /* it follows the joint of this variable on that path; -1 = in front of the first */
    int32_t master_variable; /* value = multiplier * q[master_variable] + offset */
    int32_t joint_type;      /* PIKAMD_JOINT_REVOLUTE or PIKAMD_JOINT_PRISMATIC */
    double origin_xyz_rpy[6];
    double axis[3];
    double multiplier, offset;
} pikamd_mimic_joint;
int32_t pikamd_set_mimic_joints(pikamd_solver* s, int32_t n, const pikamd_mimic_joint* joints);
void pikamd_destroy(pikamd_solver* s);
/* out [dof][7]: min max mid half_span max_velocity_rcp minimal_displacement_factor bounded
 * (Robot::Variable table, include/pick_ik/robot.hpp:15-37) */
int32_t pikamd_variables(const pikamd_solver* s, double* out);

/* make_fk_fn (src/fk_moveit.cpp:11-35): tip pose for n joint vectors.
 * q [n][dof] -> pos_quat [n][7] = x y z qw qx qy qz. */
int32_t pikamd_fk_batch(pikamd_solver* s, int64_t n, const double* q, double* pos_quat);

/* make_cost_fn / make_is_solution_test_fn (src/goal.cpp:188-203, 163-186) for n candidates.
 * goal [n][7], seed [n][dof] (minimal-displacement reference), q [n][dof] ->
 * cost [n] (may be NULL), is_solution [n] (may be NULL). */
int32_t pikamd_cost_batch(pikamd_solver* s, const pikamd_params* p, int64_t n,
                          const double* goal_pos_quat, const double* seed, const double* q,
                          double* cost, int32_t* is_solution);

/* One step() (src/ik_gradient.cpp:24-94) on n independent GradientIk states.
 * in/out: local [n][dof], best [n][dof], local_cost [n], best_cost [n];
 * out: gradient [n][dof], improved [n] (may be NULL). */
int32_t pikamd_gd_step_batch(pikamd_solver* s, const pikamd_params* p, int64_t n,
                             const double* goal_pos_quat, const double* seed, double* local,
                             double* best, double* local_cost, double* best_cost,
                             double* gradient, int32_t* improved);

/* ik_memetic (src/ik_memetic.cpp:285-373) or ik_gradient (src/ik_gradient.cpp:96-139), selected by
 * p->mode, for B independent problems.
 *   goal_pos_quat [B][7]  goal pose in the chain's base frame (x y z qw qx qy qz)
 *   seed          [B][dof] ik_seed_state
 *   rng_seed, problem_offset: random streams are keyed by (rng_seed, problem_offset + b), so a
 *                 batch sharded over several GPUs/calls gives the same answers as one call.
 *   solution [B][dof] (seed on failure, src/pick_ik_plugin.cpp:213-217), status [B],
 *   final_cost [B] (may be NULL), stats [B] (may be NULL).
 * Synchronous; staged through the library's own pinned buffers and stream (it never touches the
 * caller's slots of the device entry points). */
int32_t pikamd_solve_batch(pikamd_solver* s, const pikamd_params* p, int64_t B,
                           const double* goal_pos_quat, const double* seed, uint64_t rng_seed,
                           int64_t problem_offset, double* solution, int32_t* status,
                           double* final_cost, pikamd_stats* stats);

/* Same, on HBM-resident buffers; enqueues on `stream` (a hipStream_t, NULL = default stream) and
 * returns without synchronising.  Scratch memory is owned by the handle and reused across calls on
 * the same `slot` (0 <= slot < PIKAMD_MAX_SLOTS); calls on different slots may be in flight
 * concurrently on different streams. */
#define PIKAMD_MAX_SLOTS 128
int32_t pikamd_solve_batch_device(pikamd_solver* s, const pikamd_params* p, int64_t B,
                                  const double* d_goal_pos_quat, const double* d_seed,
                                  uint64_t rng_seed, int64_t problem_offset, double* d_solution,
                                  int32_t* d_status, double* d_final_cost, pikamd_stats* d_stats,
                                  void* stream, int32_t slot);
int32_t pikamd_fk_batch_device(pikamd_solver* s, int64_t n, const double* d_q, double* d_pos_quat,
                               void* stream);
/* Optional: allocate slot `slot`'s scratch for calls of up to B problems (all batches together) with
 * these parameters and upload the chain constants now, so that the first solve on the slot does not
 * allocate (hipMalloc synchronises the device). */
int32_t pikamd_reserve(pikamd_solver* s, const pikamd_params* p, int64_t B, int32_t slot,
                       void* stream);

/* ---- several batches per call -------------------------------------------------------------
 * The plugin solves one pose per call (src/pick_ik_plugin.cpp:73-294); a batch caller (a planner
 * sampling goal poses, a server collecting requests) has MANY independent batches.  One call here
 * takes up to PIKAMD_MAX_BATCHES of them and solves their problems as ONE pool: the persistent
 * wavefronts pull problems of all batches from one queue, so that the long tail of one batch (the
 * ~1 % of targets that run all memetic_max_generations) overlaps with the bulk of the others instead
 * of idling the chip.  Every batch gets exactly the answers a call of its own would give (random
 * streams are keyed by (rng_seed, problem_offset + b) per batch; asserted bit for bit by the tests).
 *
 * A batch also separates the two joint vectors the plugin keeps per call
 * (src/pick_ik_plugin.cpp:199-245): `seed` = ik_seed_state, which the minimal-displacement cost
 * (src/goal.cpp:131-144) measures against and which is returned on failure, and `initial_guess` =
 * init_state, where the search starts -- ik_seed_state on the first attempt, a random valid
 * configuration on restarts (:241-245).  NULL = seed.  On failure final_cost holds the cost of the
 * initial guess. */
#define PIKAMD_MAX_BATCHES 64
typedef struct pikamd_batch {
    int64_t B;
    const double* goal_pos_quat; /* [B][n_tips][7] */
    const double* seed;          /* [B][dof] ik_seed_state */
    const double* initial_guess; /* [B][dof] or NULL (= seed) */
    int64_t problem_offset;      /* random streams of problem b: (rng_seed, problem_offset + b) */
    double* solution;            /* [B][dof] */
    int32_t* status;             /* [B] */
    double* final_cost;          /* [B] or NULL */
    pikamd_stats* stats;         /* [B] or NULL */
    uint32_t* completed;         /* device entry point only, or NULL: a counter in device / pinned host
                                    memory that is incremented (release, system scope) once per
                                    finished problem of this batch, AFTER its results are in memory:
                                    completed == B  <=>  the batch is done, before the call is */
} pikamd_batch;

/* device pointers in every record; enqueues on `stream` and returns (see pikamd_solve_batch_device) */
int32_t pikamd_solve_batches_device(pikamd_solver* s, const pikamd_params* p, int32_t n_batches,
                                    const pikamd_batch* batches, uint64_t rng_seed, void* stream,
                                    int32_t slot);

/* Host pointers, asynchronous: inputs are copied into pinned staging memory, H2D copies, kernels and
 * D2H copies are enqueued on job `job`'s own stream (0 <= job < PIKAMD_MAX_HOST_JOBS), and the call
 * returns.  pikamd_wait(job) blocks until the job is done and copies the results into the batches'
 * output arrays (which must stay valid until then).  Jobs overlap each other's PCIe transfers and
 * kernels.  The input arrays may be reused as soon as the call returns. */
#define PIKAMD_MAX_HOST_JOBS 16
int32_t pikamd_solve_batches_async(pikamd_solver* s, const pikamd_params* p, int32_t n_batches,
                                   const pikamd_batch* batches, uint64_t rng_seed, int32_t job);
int32_t pikamd_wait(pikamd_solver* s, int32_t job);
/* = pikamd_solve_batches_async + pikamd_wait on an internal job */
int32_t pikamd_solve_batches(pikamd_solver* s, const pikamd_params* p, int32_t n_batches,
                             const pikamd_batch* batches, uint64_t rng_seed);

/* ---- several GPUs of one node ----------------------------------------------------------------
 * Every target pose is an independent problem (the reference solves one per call,
 * src/pick_ik_plugin.cpp:73-294; its only parallelism are the species threads of one solve,
 * src/ik_memetic.cpp:312-353), so a batch shards trivially: device r of n solves the contiguous range
 * pikamd_shard_bounds(B, r, n) with problem_offset + its first index as the random-stream key -- the
 * sharded call returns exactly what one call over the whole batch on one device returns, whatever n is.
 * solvers[r] is a handle created on device r's ordinal for the same chain (one handle per device; a
 * handle may not appear twice).  Host pointers: every device gets its own host thread, which stages
 * its shard in up to two chunks (option "shard_chunks"; asynchronous jobs 0, 1 of that handle: the second
 * one's PCIe transfers overlap the first one's kernels) and writes the results straight into the caller's arrays -- the "gather" is the
 * shards' device-to-host copies; no collective is needed for host-resident results (a caller who wants
 * the results resident on every GPU all-gathers them with RCCL, as bench.py does).  Synchronous. */
void pikamd_shard_bounds(int64_t total, int32_t rank, int32_t world, int64_t* lo, int64_t* hi);
int32_t pikamd_solve_batch_sharded(pikamd_solver* const* solvers, int32_t n_devices, const pikamd_params* p,
                                   int64_t B, const double* goal_pos_quat, const double* seed,
                                   const double* initial_guess /* NULL = seed */, uint64_t rng_seed,
                                   int64_t problem_offset, double* solution, int32_t* status,
                                   double* final_cost /* may be NULL */, pikamd_stats* stats /* may be NULL */);

/* ---- robot description -> solver ----------------------------------------------------------
 * Robot::from / get_link_indices / get_active_variable_indices (src/robot.cpp:44-160) over a URDF
 * document instead of a live MoveIt RobotModel: the actuated single-variable joints on the way from
 * base_link to the tip link(s), fixed joints folded into the next origin, mimic joints excluded
 * (src/robot.cpp:144-150; held at zero), continuous joints unbounded.  With several tips the variables
 * are numbered in the order they are first met walking the tips' paths in the order given (list the
 * tips so that shared joints come first).  pikamd_urdf_extract needs no device and returns the
 * description it found (the joint vector's order is variable_names); pikamd_create_from_urdf =
 * extract + pikamd_create / pikamd_create_multi. */
#define PIKAMD_MAX_NAME 64
typedef struct pikamd_urdf_model {
    int32_t dof, n_tips;
    char variable_names[PIKAMD_MAX_DOF][PIKAMD_MAX_NAME];
    double qmin[PIKAMD_MAX_DOF], qmax[PIKAMD_MAX_DOF], vmax[PIKAMD_MAX_DOF];
    uint8_t bounded[PIKAMD_MAX_DOF];
    struct {
        int32_t n_joints;
        int32_t variable[PIKAMD_MAX_DOF];
        double origin_xyz_rpy[PIKAMD_MAX_DOF][6];
        double axis[PIKAMD_MAX_DOF][3];
        int32_t joint_type[PIKAMD_MAX_DOF];
        double tip_xyz_rpy[6];
    } tips[PIKAMD_MAX_TIPS];
    int32_t n_mimic; /* mimic joints that follow a variable of their path (pikamd_set_mimic_joints) */
    pikamd_mimic_joint mimic[PIKAMD_MAX_TIPS * PIKAMD_MAX_MIMIC];
} pikamd_urdf_model;
int32_t pikamd_urdf_extract(const char* urdf_xml, const char* base_link, const char* const* tip_links,
                            int32_t n_tips, pikamd_urdf_model* out);
int32_t pikamd_create_from_urdf(const char* urdf_xml, const char* base_link, const char* const* tip_links,
                                int32_t n_tips, int32_t device_ordinal, pikamd_solver** out);

/* ---- a host cost function that takes part in the search ----------------------------------------------
 * Reference: kinematics::KinematicsBase::IKCostFn -- src/pick_ik_plugin.cpp:130-135 pushes one Goal of weight 1
 * per tip pose (make_ik_cost_fn, src/goal.cpp:146-161); the goal is summed into cost_fn (src/goal.cpp:188-203)
 * and must stay below cost_threshold^2 in solution_fn (src/goal.cpp:175-182).  It is an opaque host closure
 * evaluated at EVERY cost evaluation of the search, which no GPU kernel can call and no host round trip per
 * evaluation can afford (96 us each, 13 000 per solve).  pikamd_solve_batch_host therefore runs such queries ON
 * THE HOST: the reference's algorithm, one problem after the other on the calling thread, with the arithmetic of
 * the library's exact kernels compiled for the host and the library's random streams -- bit-identical to the CPU
 * oracle given the same callback (its math mode "fma"; "portable" for the verification library), and bit-identical
 * to the exact kernels' answer when the callback returns 0.  About 7 ms per default-parameter solve per core.
 *   cost_fn(q, dof, pose_index, user) -> the cost of joint vector q for tip pose `pose_index` (0 .. n_tips-1); it
 *   must be a pure function of its arguments.  cost_fn == NULL is refused: queries without a host cost function
 *   belong on the GPU (pikamd_solve_batch).  All arrays are host memory, [B][dof] / [B][n_tips][7] (a handle
 *   with joint_layout = soa is refused); initial_guess may be NULL (= seed).  A callback value that is not below
 *   cost_threshold^2 rejects a candidate exactly as the reference's `cost >= threshold` does (a NaN passes, as
 *   there).  Wall-clock limits: options host_max_time / host_gd_max_time below -- on THIS path the reference's
 *   clocks exist (a problem cut short returns what the reference returns at a timeout: its best individual if
 *   that is acceptable, else failure). */
typedef double (*pikamd_cost_fn)(const double* q, int32_t dof, int32_t pose_index, void* user);
int32_t pikamd_solve_batch_host(pikamd_solver* s, const pikamd_params* p, int64_t B, const double* goal_pos_quat,
                                const double* seed, const double* initial_guess, uint64_t rng_seed,
                                int64_t problem_offset, pikamd_cost_fn cost_fn, void* user, double* solution,
                                int32_t* status, double* final_cost, pikamd_stats* stats);

/* ---- scheduling options of a handle -------------------------------------------------------
 * How a call is cut into launches is chosen by the library (lanes per elite and
 * compaction passes from the number of problems still running, two wavefronts per SIMD from a size
 * threshold, latency- or throughput-greedy from the number of other calls in flight).  None of it
 * changes a result; a caller who knows better can pin each choice per handle.  Options are read when
 * a call is made.  THE LIBRARY never reads the environment; the Python test binding
 * (pick_ik_amd/solver.py ENV_OPTIONS) is what turns the PIK_* variables of the test suite and the tools
 * into pikamd_set_option calls -- a C or C++ caller sets options explicitly.  value NULL or "" restores
 * the default.
 *   "host_max_time", "host_gd_max_time"  wall-clock limits of pikamd_solve_batch_host in seconds ("0": none) --
 *                               the reference's max_time of a query / of one elite's descent, read in front
 *                               of every generation / descent step (src/ik_memetic.cpp:75-78, 226-228,
 *                               src/ik_gradient.cpp:112-115); the device paths have iteration budgets only
 *   "lanes_per_elite"           "0" adaptive | "1" "2" "4" "8" "16" (several tip frames: no "4"; a value a
 *                               call cannot have falls back to adaptive)
 *   "lanes_per_elite_schedule"  "g0:l0,g1:l1,..."  passes starting at generation >= g_i use l_i lanes (g0 = 0)
 *   "passes"                    "2,4,8,..." generation marks of the compaction passes | "none"
 *   "two_per_simd"              "0" never | "1" default threshold | "<n>" from n first-pass wavefronts on
 *   "regime"                    "adaptive" | "latency" | "throughput"
 *   "specialised"               "1" the kernels compiled for the common configuration (bounded revolute
 *                               variables, no joint goals, four elites, one species ...) serve the calls that
 *                               have it -- same bits, 15-19 % faster | "0" the general kernels always
 *   "shard_chunks"              "1".."8" host jobs per device of pikamd_solve_batch_sharded (default 2)
 *   "joint_layout"              "aos" (default): the joint-vector arrays of the solve entry points (seed,
 *                               initial_guess, solution) are [B][dof], one problem's vector contiguous -- what
 *                               a MoveIt caller holds | "soa": they are [dof][B] per batch (structure of
 *                               arrays); poses stay [B][n_tips][7].  The library transposes on the device in
 *                               front of and behind the kernels (180 bytes per problem); not with completion
 *                               counters, not with pikamd_solve_batch_sharded.  Unlike the options above this
 *                               one changes what the caller's arrays MEAN, not a result.
 *   "arithmetic"                "exact" (default): the exact kernels -- the reference's literal algorithm (MoveIt's
 *                               chain product, 2 dof + 3 cost evaluations per gradient step, IEEE square roots and
 *                               divisions) with fused multiply-adds at stated places; BIT-IDENTICAL to the CPU
 *                               oracle's math mode "fma" on every entry point: the joint vector a caller gets is
 *                               the one src/ik_memetic.cpp:356-370 returns | "fast" (opt-in): the
 *                               Denavit-Hartenberg kernels (frame-based gradient probes, in-house square roots;
 *                               whole solves agree with the reference statistically), about
 *                               twice the throughput.  (Chains with a floating or a mimic joint always run the
 *                               exact kernels.)
 *   "self_test"                 "auto" (default): the first pikamd_reserve or host-pointer solve of a KERNEL SET
 *                               (flavour, mode, species, elites, enabled cost terms -- not thresholds, weights or
 *                               budgets) that the general or the exact kernels serve runs a short pikamd_self_test
 *                               first (a dozen solves of 32 targets, four generations: ~10 ms, once per kernel set
 *                               and handle; pikamd_self_test_cost reports it).  The stream-ordered entry points
 *                               (pikamd_solve_batch[es]_device) never run it: they do not block -- reserve first.
 *                               | "off": only when pikamd_self_test is called
 * pikamd_set_option and pikamd_self_test change the handle's options: like every call on a handle they must not
 * run concurrently with another call on the same handle (a handle is used from one thread at a time).
 * The reference has no counterpart (its only scheduling parameter is memetic_num_threads,
 * src/ik_memetic.cpp:299-335, which pikamd_params carries). */
int32_t pikamd_set_option(pikamd_solver* s, const char* name, const char* value);

/* ---- self test ------------------------------------------------------------------------------
 * Every kernel variant re-schedules the same arithmetic, so on ANY input all of them must return the
 * same bits as the one-lane kernel -- a property that can be checked on the device, without the oracle.
 * pikamd_self_test solves n (1..4096) generated reachable targets of THIS chain with THESE parameters by
 * every variant the handle may choose (2 / 4 / 8 / 16 lanes per elite, with and without compaction passes,
 * the two-wavefronts-per-SIMD build) and compares solutions, status words, costs and counters bit for bit
 * with the one-lane kernel's.  A variant that disagrees is switched off for the handle (the adaptive
 * schedule then never picks it) and reported: *disabled_mask bit v = v lanes per elite (2, 4, 8, 16), bit 1
 * = the two-per-SIMD build, bit 32 = the common-configuration kernels against the general ones.  Why it exists: the multi-lane kernels of long chains compile at the register
 * cap, and twice during development such a kernel came out wrong after a change elsewhere in the source
 * (DESIGN.md section 3); the shipped kernels pass this test on every chain the tests generate -- a
 * deployment on its own robot can make sure in ~20 ms at start-up (the plugin shim does, once per group).
 * The reference has no counterpart. */
int32_t pikamd_self_test(pikamd_solver* s, const pikamd_params* p, int32_t n, uint32_t* disabled_mask);
/* what the AUTOMATIC self tests of this handle (option self_test = auto) have cost so far: how many ran, and their
 * wall-clock time in milliseconds (either pointer may be NULL) */
int32_t pikamd_self_test_cost(const pikamd_solver* s, int32_t* runs, double* total_ms);

/* library / kernel introspection for benches and tests */
const char* pikamd_last_error(void);
const char* pikamd_version(void);
/* name of the kernel pikamd_solve_batch* launches for this handle and these parameters, with the namespace
 * of the flavour that serves the call: `pik_common::memetic_kernel<7>` (kernels compiled for the common
 * configuration), `pik::...` (general), `pik_strict::...` (literal: floating-joint chains, and everything
 * in libpick_ik_amd_strict.so) -- for matching rocprof rows, and for tests that must know which ran */
const char* pikamd_kernel_name(const pikamd_solver* s, const pikamd_params* p);

/* ---- Cartesian waypoint paths: chained local IK ---------------------------------------------
 * What MoveIt's computeCartesianPath, servoing and straight-line approach sampling do with local mode
 * (p->mode must be 1): P paths of W waypoints each, every waypoint solved from the previous waypoint's
 * answer, a path stopping at its first failure.  One kernel launch walks all waypoints of all paths on the
 * device; the previous answer becomes the next seed in registers.  The result is DEFINED as what this loop of
 * pikamd_solve_batch calls returns, bit for bit:
 *
 *   seed[p] = start[p]; held[p] = true; reached[p] = 0
 *   for k in 0 .. W-1:
 *     for every p with held[p]:
 *       (sol, st, cost, stats) = pikamd_solve_batch(local mode, goal[p][k], seed = initial guess = seed[p])
 *       jump = st > 0 and max_joint_step given and any j: |sol[j] - seed[p][j]| > max_joint_step[j]
 *              (an entry of max_joint_step that is 0 or less, or not a number, sets no limit for its variable)
 *       if st > 0 and not jump: solution[p][k] = sol; status[p][k] = st; seed[p] = sol; reached[p] += 1
 *       else: solution[p][k] = seed[p]; status[p][k] = jump ? PIKAMD_PATH_JUMP : st; held[p] = false
 *       final_cost[p][k] = cost; stats[p][k] = stats      (what the call returned, also for a refused jump)
 *     for every p not held before this k:
 *       solution[p][k] = seed[p]; status[p][k] = PIKAMD_NOT_ATTEMPTED; final_cost[p][k] = 0; stats[p][k] = zero
 *
 * st > 0 covers PIKAMD_SUCCESS and PIKAMD_APPROXIMATE: with return_approximate_solution set (servoing) a path
 * never stops on a solver failure.  seed[p] is both the start of the search and the minimal-displacement
 * reference.  Local mode draws no random numbers: there is no rng_seed.  reached[p] / W is
 * computeCartesianPath's fraction.
 *   goal_pos_quat [P][W][n_tips][7], start [P][dof], max_joint_step [dof] (may be NULL),
 *   solution [P][W][dof], status [P][W], final_cost [P][W] (may be NULL), stats [P][W] (may be NULL),
 *   reached [P] (may be NULL).
 * Not with the option joint_layout = soa. */
#define PIKAMD_NOT_ATTEMPTED 0   /* status of a waypoint behind the one its path stopped at */
#define PIKAMD_PATH_JUMP (-1001) /* the waypoint was solved, but a variable moved further than max_joint_step
                                    allows (outside the values of MoveItErrorCodes) */
/* [host-api-begin] Entry points added after the committed kernel profiles were taken.  They are host functions: the
 * hash of a kernel flavour's DEVICE source (pick_ik_amd/build.py flavour_sha) leaves the declarations between this
 * comment and the matching end comment out, so that adding host API does not mark the profiles of untouched kernels stale. */
/* host pointers; synchronous, staged through the library's own pinned buffers and stream like
 * pikamd_solve_batch, behind the same automatic self test of the local-mode kernels */
int32_t pikamd_solve_paths(pikamd_solver* s, const pikamd_params* p, int64_t P, int32_t W,
                           const double* goal_pos_quat, const double* start, const double* max_joint_step,
                           double* solution, int32_t* status, double* final_cost, pikamd_stats* stats,
                           int32_t* reached);
/* device pointers (max_joint_step too); enqueues on `stream` and returns without synchronising, no self test
 * (see pikamd_solve_batch_device for `slot`) */
int32_t pikamd_solve_paths_device(pikamd_solver* s, const pikamd_params* p, int64_t P, int32_t W,
                                  const double* d_goal_pos_quat, const double* d_start,
                                  const double* d_max_joint_step, double* d_solution, int32_t* d_status,
                                  double* d_final_cost, pikamd_stats* d_stats, int32_t* d_reached,
                                  void* stream, int32_t slot);
/* name of the kernel pikamd_solve_paths* launches for P paths (see pikamd_kernel_name), e.g.
 * `pik_exact::ik_path_team_kernel<7,16>` */
const char* pikamd_path_kernel_name(const pikamd_solver* s, const pikamd_params* p, int64_t P);

/* ---- Local IK with random restarts ---------------------------------------------------------------
 * The loop searchPositionIK runs around the solver (src/pick_ik_plugin.cpp:145-291): solve; when no solution came
 * back, draw a random valid configuration (Robot::set_random_valid_configuration, src/robot.cpp:23-30, 87-95) and
 * solve again from there -- for B problems and up to max_attempts attempts each in ONE launch.  p->mode must be 1
 * (local mode).  The result is DEFINED as what this loop of pikamd_solve_batch calls returns, bit for bit:
 *
 *   init[b] = initial_guess ? initial_guess[b] : seed[b]
 *   if some bounded variable j has !(init[b][j] <= qmax[j] && init[b][j] >= qmin[j]):   (src/pick_ik_plugin.cpp:152-159;
 *       init[b] = draw(b, 0, init[b])                                                     a NaN is invalid)
 *   for a in 0 .. max_attempts-1, for every b still open:
 *     (sol, st, cost, stats) = pikamd_solve_batch(local mode, goal[b], seed = seed[b], initial_guess = init[b])
 *     if p->return_approximate_solution and a gate is set and st > 0 and not pass(sol, seed[b]):
 *       st = PIKAMD_GATE_REFUSED; sol = seed[b]     (the approximate-solution gate below, :263-266; cost and stats stay
 *                                                    what the solve returned, as for a refused path jump)
 *     if a model is set and st > 0 and not valid(sol):  st = PIKAMD_VALIDITY_REFUSED; sol = seed[b]
 *                                                   (the validity model below, in the solution callback's place, :269-274;
 *                                                    cost and stats stay what the solve returned; no cost_fn invocation
 *                                                    is counted)
 *     solution[b] = sol; status[b] = st; final_cost[b] = cost; stats[b] += stats (field by field); attempts[b] = a + 1
 *     if st > 0: b is closed        (PIKAMD_SUCCESS or PIKAMD_APPROXIMATE: error_code SUCCESS ends the reference's loop)
 *     else: init[b] = draw(b, a + 1, init[b])
 *
 *   draw(b, e, prev)[j] = bounded[j] ? (qmax[j] - qmin[j]) * u + qmin[j]
 *                                    : ((prev[j] + pi) - (prev[j] - pi)) * u + (prev[j] - pi)
 *     u = the [0,1) double of Philox stream RESTART (= 3), key (rng_seed, problem_offset + b), epoch e, individual 0,
 *         slot j -- the counter / key layout of every other draw of this library (streams 1 and 2 are as they were).
 *     Every product, sum and difference of draw is rounded on its own, in every kernel flavour: the restart states
 *     are the same doubles whatever serves the call.  An unbounded variable's draw is centred on the PREVIOUS
 *     attempt's start, as in the reference.
 *
 * Consequences: max_attempts = 1 with a valid initial guess is exactly pikamd_solve_batch (with a gate:
 * pikamd_solve_batch + pikamd_gate_batch; with a model: + pikamd_validity_batch).  With return_approximate_solution set
 * and neither a gate nor a model on the handle, attempt 0 always closes a problem (attempts == 1 everywhere); with a
 * gate or a model the restarts run for every refused answer.  A batch cut into
 * calls or shards with matching problem_offset gives the answers of one call.  The attempts of one problem are
 * independent computations, so the library may run them one after the other or side by side (option
 * search_schedule = adaptive | sequential | parallel: like the other scheduling options it changes no result).
 * all_solution / all_status: when either is given EVERY attempt of every problem is run and recorded, without an
 * early exit -- the rows behind a problem's winner are real results (several distinct IK solutions per target, for
 * a caller who collision-checks them); row a is what one pikamd_solve_batch from start a returns, gated and tested
 * like the loop's.  The primary outputs are the loop's whether or not all_* is given.
 * The approximate-solution gate (src/pick_ik_plugin.cpp:219-267) is the handle's (pikamd_set_approximate_gate below;
 * none by default).  The solution callback (:269-274) is host code and stays with the caller; the validity model of the
 * handle (pikamd_set_validity_model below; none by default) stands in its place, applied whenever the handle has one,
 * independent of return_approximate_solution.  A call that the fast kernels serve (option arithmetic = fast) is refused
 * with PIKAMD_EUNSUPPORTED while a model is set: the test's arithmetic is the exact flavour's.
 * GLOBAL mode (mode 0) is refused here: pikamd_search_global_batch serves it.
 *   goal_pos_quat [B][n_tips][7], seed [B][dof], initial_guess [B][dof] (NULL = seed), solution [B][dof], status [B],
 *   final_cost [B] (may be NULL), stats [B] (may be NULL), attempts [B] (may be NULL),
 *   all_solution [B][max_attempts][dof] (may be NULL), all_status [B][max_attempts] (may be NULL).
 * Not with the option joint_layout = soa.  B = 0 returns 0. */
#define PIKAMD_MAX_ATTEMPTS 64
/* host pointers; synchronous, staged through the library's own pinned buffers and stream like pikamd_solve_batch,
 * behind the same automatic self test of the local-mode kernels */
int32_t pikamd_search_batch(pikamd_solver* s, const pikamd_params* p, int64_t B, const double* goal_pos_quat,
                            const double* seed, const double* initial_guess, uint64_t rng_seed,
                            int64_t problem_offset, int32_t max_attempts, double* solution, int32_t* status,
                            double* final_cost, pikamd_stats* stats, int32_t* attempts, double* all_solution,
                            int32_t* all_status);
/* device pointers; enqueues on `stream` and returns without synchronising, no self test (see
 * pikamd_solve_batch_device for `slot`).  The per-attempt scratch of the parallel schedule belongs to the
 * handle's slot; it grows only when a call needs more than any earlier call on that slot did (a grow frees, and a
 * free synchronises the device: run the largest call first where that matters). */
int32_t pikamd_search_batch_device(pikamd_solver* s, const pikamd_params* p, int64_t B,
                                   const double* d_goal_pos_quat, const double* d_seed,
                                   const double* d_initial_guess, uint64_t rng_seed, int64_t problem_offset,
                                   int32_t max_attempts, double* d_solution, int32_t* d_status,
                                   double* d_final_cost, pikamd_stats* d_stats, int32_t* d_attempts,
                                   double* d_all_solution, int32_t* d_all_status, void* stream, int32_t slot);
/* name of the kernel pikamd_search_batch* launches for B problems of max_attempts attempts (see
 * pikamd_kernel_name), e.g. `pik_exact::ik_search_team_kernel<7,16>`; *attempts_in_flight (may be NULL): 1 = the
 * sequential schedule (a lane or team walks a problem's attempts), max_attempts = the parallel one (every attempt
 * of every problem on the chip at once, a small finalize kernel behind them) */
const char* pikamd_search_kernel_name(const pikamd_solver* s, const pikamd_params* p, int64_t B,
                                      int32_t max_attempts, int32_t* attempts_in_flight);
/* ---- Memetic IK with random restarts (global mode) -------------------------------------------------
 * The same loop around the memetic solver, for B problems and up to max_attempts attempts each in ONE call.
 * p->mode must be 0 (global mode; mode 1 is pikamd_search_batch's).  The result is DEFINED as this loop, bit for bit:
 *
 *   init[b] = initial_guess ? initial_guess[b] : seed[b]
 *   if init[b] is invalid (a bounded variable outside its limits, or a NaN): init[b] = draw(b, 0, init[b])
 *   for a in 0 .. max_attempts-1, for every b still open:
 *     (sol, st, cost, stats) = one pikamd_batch record {B = 1, goal[b], seed[b], initial_guess = init[b],
 *                                problem_offset = problem_offset + b} solved by pikamd_solve_batches in global mode
 *                                with rng_seed_a = rng_seed + ((uint64_t)a << 32)      (mod 2^64)
 *     if p->return_approximate_solution and a gate is set and st > 0 and not pass(sol, seed[b]):
 *       st = PIKAMD_GATE_REFUSED; sol = seed[b]                  (as in pikamd_search_batch; cost and stats stay)
 *     if a model is set and st > 0 and not valid(sol):  st = PIKAMD_VALIDITY_REFUSED; sol = seed[b]          (likewise)
 *     solution[b] = sol; status[b] = st; final_cost[b] = cost; stats[b] += stats (field by field); attempts[b] = a + 1
 *     if st > 0: b is closed     else: init[b] = draw(b, a + 1, init[b])
 *
 * draw is exactly the draw of pikamd_search_batch above: Philox stream RESTART (= 3), keyed by the CALLER's rng_seed
 * (not rng_seed_a), every operation rounded on its own.
 * Why a << 32: a draw's key is ((uint32)seed ^ stream, (seed >> 32) + (problem >> 32)).  Adding a to the LOW word
 * would make attempt 1's REPRODUCE key (stream 2) equal attempt 0's RESTART key -- (0 + 1) ^ 2 == 0 ^ 3.  The high
 * word gives every attempt INIT / REPRODUCE streams of its own for all problem indices below 2^32; a = 0 is the
 * caller's seed unchanged.
 *
 * Consequences: max_attempts = 1 with a valid initial guess is exactly pikamd_solve_batch (with a gate: +
 * pikamd_gate_batch; with a model: + pikamd_validity_batch).  With return_approximate_solution set and neither a gate
 * nor a model on the handle, every problem closes at attempt 0.  A batch cut into calls or shards with matching
 * problem_offset gives the answers of one call.  A restart starts from the re-drawn state, as the plugin shim's loop
 * does (the reference re-randomises init_state but keeps passing ik_seed_state; seed[b] stays the displacement
 * reference and what a failure returns).  The approximate-solution gate is the handle's
 * (pikamd_set_approximate_gate); the solution callback stays with the caller, and the handle's validity model
 * (pikamd_set_validity_model) stands in its place -- for every kernel flavour: the test is a kernel of its own between
 * an attempt and its fold.
 * all_solution [B][max_attempts][dof] / all_status [B][max_attempts]: when either is given EVERY attempt of every
 * problem runs, without an early exit; row a is what the one-record solve above returns from the start the loop's
 * draws give attempt a (every attempt counted as failed) with rng_seed_a, gated and tested like the loop's.  The primary outputs
 * are the loop's either way.
 * Accepts what pikamd_solve_batch accepts in global mode: every kernel flavour, species, several tip frames,
 * floating and mimic chains, unbounded variables.  max_attempts is 1..PIKAMD_MAX_ATTEMPTS; B = 0 returns 0; NULL is
 * checked as in pikamd_search_batch (final_cost, stats, attempts, all_* may be NULL).  Not with the option
 * joint_layout = soa.  No completion counters. */
/* host pointers; synchronous, staged through the library's own pinned buffers and stream, behind the automatic
 * self test of the GLOBAL-mode kernels.  Stops enqueuing attempts once no problem is open. */
int32_t pikamd_search_global_batch(pikamd_solver* s, const pikamd_params* p, int64_t B, const double* goal_pos_quat,
                                   const double* seed, const double* initial_guess, uint64_t rng_seed,
                                   int64_t problem_offset, int32_t max_attempts, double* solution, int32_t* status,
                                   double* final_cost, pikamd_stats* stats, int32_t* attempts, double* all_solution,
                                   int32_t* all_status);
/* device pointers; enqueues ALL max_attempts attempts on `stream` and returns without synchronising, no self test
 * (see pikamd_solve_batch_device for `slot`): the passes of an attempt nobody is open for find a count of 0 and
 * return.  The scratch of the call (the starts, one attempt's rows, the open list) belongs to the handle's slot; it
 * grows only when a call needs more than any earlier call on that slot did (a grow frees, and a free synchronises
 * the device: run the largest call first where that matters). */
int32_t pikamd_search_global_batch_device(pikamd_solver* s, const pikamd_params* p, int64_t B,
                                          const double* d_goal_pos_quat, const double* d_seed,
                                          const double* d_initial_guess, uint64_t rng_seed, int64_t problem_offset,
                                          int32_t max_attempts, double* d_solution, int32_t* d_status,
                                          double* d_final_cost, pikamd_stats* d_stats, int32_t* d_attempts,
                                          double* d_all_solution, int32_t* d_all_status, void* stream, int32_t slot);
/* ---- The approximate-solution gate ------------------------------------------------------------------
 * With return_approximate_solution set the reference passes every answer of the solver through a gate
 * (src/pick_ik_plugin.cpp:219-267): an answer it refuses becomes NO_IK_SOLUTION and the loop restarts from a random
 * state.  The reference builds frame tests from its two approximate POSE thresholds and never uses them (:234-248); what
 * it applies is make_is_solution_test_fn(frame_tests, goals, approximate_solution_cost_threshold) and then the
 * joint-jump test.  That is the gate here; the two dead thresholds are not carried.
 *
 * pikamd_gate_batch: pass[i] = the reference's approx_solution_valid for candidate q[i], DEFINED by entry points above:
 *   - is_solution[i] of pikamd_cost_batch(s, p', n, goal, seed, q, ...), p' = p with cost_threshold =
 *     gate->cost_threshold when that is > 0, else p with the three joint-goal weights set to 0, AND
 *   - for no j: fabs(q[i][j] - seed[i][j]) > gate->joint_threshold (tested only when gate->joint_threshold > 0).
 * The comparisons are written exactly so: a NaN threshold limits nothing, a NaN difference does not trip the limit.
 * Host pointers, arrays shaped as pikamd_cost_batch's, needs a device; n = 0 returns 0; a NULL gate or array and a
 * handle with joint_layout = soa are refused (PIKAMD_EINVAL).  The evaluation is no cost_fn invocation of the solver:
 * stats.cost_evals does not count it.
 *
 * pikamd_set_approximate_gate: the gate of pikamd_search_batch* and pikamd_search_global_batch* on this handle (the
 * step in their loops above), applied only when p->return_approximate_solution is set (:222), to PIKAMD_SUCCESS as
 * well as PIKAMD_APPROXIMATE -- a SUCCESS further than joint_threshold from the seed is refused, as in the reference.
 * A failed attempt is not evaluated.  NULL = no gate, the default: every result is what it was.  Like
 * pikamd_set_option: not concurrent with another call on the handle, read when a call is made.
 * pikamd_solve_batch*, pikamd_solve_paths* and pikamd_solve_batch_host IGNORE the gate: they are the solver, the gate
 * belongs to the loop around it.  They ignore a validity model (pikamd_set_validity_model) in the same way, and so does
 * every path entry point. */
typedef struct pikamd_gate {
    double cost_threshold;  /* approximate_solution_cost_threshold; <= 0: no goal is tested (:240-242) */
    double joint_threshold; /* approximate_solution_joint_threshold; not > 0: no limit (:253) */
} pikamd_gate;
#define PIKAMD_GATE_REFUSED (-1002) /* outside MoveItErrorCodes, like PIKAMD_PATH_JUMP; a MoveIt caller reports NO_IK_SOLUTION */
int32_t pikamd_gate_batch(pikamd_solver* s, const pikamd_params* p, const pikamd_gate* gate, int64_t n,
                          const double* goal_pos_quat, const double* seed, const double* q, int32_t* pass);
int32_t pikamd_set_approximate_gate(pikamd_solver* s, const pikamd_gate* gate);
/* ---- Cartesian paths from a pose: restart the start state until the path holds ----------------------
 * A planner has a Cartesian motion (approach, retreat, straight-line segment) and a pose to start it from, but no
 * joint state: it needs a start configuration from which the whole motion is feasible.  With the entry points above
 * that is a host loop -- waypoint 0 with restarts, the path from its answer, a look at `reached`, another start when
 * the path broke -- of up to 2 * max_attempts dependent launches, and the restart states are not the caller's to
 * reproduce.  Here P paths of W waypoints and up to max_attempts attempts each run in ONE launch.  p->mode must be 1
 * (local mode).  The result is DEFINED by the entry points above, bit for bit:
 *
 *   init[p] = initial_guess ? initial_guess[p] : seed[p]
 *   if init[p] is invalid (a bounded variable outside its limits, or a NaN): init[p] = draw(p, 0, init[p])
 *   best[p] = -1
 *   for a in 0 .. max_attempts-1, for every p still open:
 *     (sol0, st0, c0, stats0) = pikamd_solve_batch(local mode, goal[p][0], seed = seed[p], initial_guess = init[p])
 *     rows_a = W rows:
 *       row 0 = (st0 > 0 ? sol0 : seed[p], st0, c0, stats0)      (what the call returned; NO joint-step test here)
 *       if st0 > 0 and W > 1: rows 1.. = pikamd_solve_paths(local mode, P = 1, W - 1, goal[p][1..], start = sol0,
 *                                                           max_joint_step)
 *       else:                 rows 1.. = (seed[p], PIKAMD_NOT_ATTEMPTED, 0, zero)
 *     reached_a = st0 > 0 ? 1 + reached of that path call : 0
 *     totals[p] += every stats row of rows_a, field by field;  attempts[p] = a + 1
 *     if reached_a > best[p]: the outputs of p become rows_a; best[p] = reached_a      (first among equals wins)
 *     if reached_a == W: p is closed     else: init[p] = draw(p, a + 1, init[p])
 *   reached[p] = best[p]
 *
 * draw is exactly the draw of pikamd_search_batch above: Philox stream RESTART (= 3), key (rng_seed,
 * problem_offset + p), every operation rounded on its own.  seed[p] stays the minimal-displacement reference of
 * waypoint 0 and is what a failed waypoint 0 returns; from waypoint 1 on the previous answer is both the reference and
 * the start, as in pikamd_solve_paths.  The handle's approximate-solution gate is NOT applied, as in
 * pikamd_solve_paths.
 *
 * Consequences: W = 1 is pikamd_search_batch with no gate (stats[p][0] is the kept attempt's, totals[p] the sum
 * pikamd_search_batch reports; a problem that no attempt solved keeps the row of its FIRST attempt, so its final_cost
 * is the first attempt's where pikamd_search_batch reports the last one's).  max_attempts = 1 with a valid initial guess is one pikamd_solve_batch followed by one
 * pikamd_solve_paths.  With return_approximate_solution set every waypoint is solved (st > 0), so only a refused jump
 * reopens a path.  A batch cut into calls or shards with matching problem_offset gives the answers of one call.
 *   goal_pos_quat [P][W][n_tips][7], seed [P][dof], initial_guess [P][dof] (NULL = seed), max_joint_step [dof] (may be
 *   NULL), solution [P][W][dof], status [P][W], final_cost [P][W] (may be NULL), stats [P][W] (may be NULL),
 *   reached [P] (may be NULL), attempts [P] (may be NULL), totals [P] (may be NULL).
 * max_attempts is 1..PIKAMD_MAX_ATTEMPTS, W >= 1; P = 0 returns 0.  Not with the option joint_layout = soa.
 * Not served (out of scope): global mode for waypoint 0 (pikamd_search_global_paths below); a parallel schedule over
 * the attempts (attempt a + 1 depends on how far attempt a got); a relative (mean-step) jump threshold; all_* rows per
 * attempt. */
/* host pointers; synchronous, staged through the library's own pinned buffers and stream like pikamd_solve_batch,
 * behind the same automatic self test of the local-mode kernels */
int32_t pikamd_search_paths(pikamd_solver* s, const pikamd_params* p, int64_t P, int32_t W,
                            const double* goal_pos_quat, const double* seed, const double* initial_guess,
                            const double* max_joint_step, uint64_t rng_seed, int64_t problem_offset,
                            int32_t max_attempts, double* solution, int32_t* status, double* final_cost,
                            pikamd_stats* stats, int32_t* reached, int32_t* attempts, pikamd_stats* totals);
/* device pointers (max_joint_step too); enqueues on `stream` and returns without synchronising, no self test (see
 * pikamd_solve_batch_device for `slot`).  The rows of the attempts behind the first are kept in scratch that belongs
 * to the handle's slot; it grows only when a call needs more than any earlier call on that slot did (a grow frees,
 * and a free synchronises the device: run the largest call first where that matters). */
int32_t pikamd_search_paths_device(pikamd_solver* s, const pikamd_params* p, int64_t P, int32_t W,
                                   const double* d_goal_pos_quat, const double* d_seed,
                                   const double* d_initial_guess, const double* d_max_joint_step, uint64_t rng_seed,
                                   int64_t problem_offset, int32_t max_attempts, double* d_solution,
                                   int32_t* d_status, double* d_final_cost, pikamd_stats* d_stats, int32_t* d_reached,
                                   int32_t* d_attempts, pikamd_stats* d_totals, void* stream, int32_t slot);
/* name of the kernel pikamd_search_paths* launches for P paths (see pikamd_kernel_name), e.g.
 * `pik_exact::ik_startpath_team_kernel<7,16>` */
const char* pikamd_search_paths_kernel_name(const pikamd_solver* s, const pikamd_params* p, int64_t P);
/* ---- Cartesian paths from a pose: memetic start, Cartesian path behind -------------------------------
 * pikamd_search_paths above restarts a LOCAL descent for waypoint 0.  Waypoint 0 is the one waypoint with no
 * neighbouring joint state -- a cold query from a pose alone, the kind the memetic solver (global mode, the default
 * mode) exists for.  Here waypoint 0 of every attempt is solved in GLOBAL mode and the waypoints behind it in local
 * mode, for P paths of W waypoints and up to max_attempts attempts each, in ONE call.  p->mode must be 0 (mode 1 is
 * refused: pikamd_search_paths serves it).  With p_local = p with mode = 1 the result is DEFINED by the entry points
 * above, bit for bit:
 *
 *   init[p] = initial_guess ? initial_guess[p] : seed[p]
 *   if init[p] is invalid (a bounded variable outside its limits, or a NaN): init[p] = draw(p, 0, init[p])
 *   best[p] = -1
 *   for a in 0 .. max_attempts-1, for every p still open:
 *     (sol0, st0, c0, stats0) = one pikamd_batch record {B = 1, goal[p][0], seed[p], initial_guess = init[p],
 *                                problem_offset = problem_offset + p} solved by pikamd_solve_batches with p (global
 *                                mode) and rng_seed_a = rng_seed + ((uint64_t)a << 32)      (mod 2^64)
 *     rows_a = W rows:
 *       row 0 = (sol0, st0, c0, stats0)      (what the call returned: the seed and the guess's cost on failure; NO
 *                                             joint-step test here)
 *       if st0 > 0 and W > 1: rows 1.. = pikamd_solve_paths(p_local, P = 1, W - 1, goal[p][1..], start = sol0,
 *                                                           max_joint_step)
 *       else:                 rows 1.. = (seed[p], PIKAMD_NOT_ATTEMPTED, 0, zero)
 *     reached_a = st0 > 0 ? 1 + reached of that path call : 0
 *     totals[p] += every stats row of rows_a, field by field (wipeouts, pool_erasures and reserved included)
 *     attempts[p] = a + 1
 *     if reached_a > best[p]: the outputs of p become rows_a; best[p] = reached_a      (the first among equals wins)
 *     if reached_a == W: p is closed     else: init[p] = draw(p, a + 1, init[p])
 *   reached[p] = best[p]
 *
 * draw is exactly the draw of pikamd_search_batch: Philox stream RESTART (= 3), keyed by the CALLER's rng_seed (not
 * rng_seed_a) and problem_offset + p; the attempt seeds rng_seed_a are those of pikamd_search_global_batch.  The
 * handle's approximate-solution gate is NOT applied, as in pikamd_search_paths.
 *
 * Consequences: max_attempts = 1 with a valid initial guess is one global-mode pikamd_solve_batch followed by one
 * pikamd_solve_paths with p_local.  W = 1 is pikamd_search_global_batch without a gate, with one difference: a problem
 * that no attempt solved keeps the row of its FIRST attempt (stats[p][0] is the kept attempt's, totals[p] the sum
 * pikamd_search_global_batch reports).  A call cut into calls or shards with matching problem_offset gives the answers
 * of one call.  With return_approximate_solution set every waypoint is solved (st > 0), so only a refused jump reopens
 * a path.
 *   Arrays and the NULLs allowed: as pikamd_search_paths.
 * max_attempts is 1..PIKAMD_MAX_ATTEMPTS, W >= 1; P = 0 returns 0.  Not with the option joint_layout = soa.  No
 * completion counters.  Accepts what pikamd_solve_batch accepts in global mode.
 * Not served (out of scope): the approximate-solution gate; all_* rows per attempt; a relative (mean-step) jump
 * threshold; a parallel schedule over the attempts. */
/* host pointers; synchronous, staged through the library's own pinned buffers and stream, behind the automatic self
 * tests of BOTH kernel sets (the global-mode one of p, the local-mode one of p_local).  Reads the number of open paths
 * back behind every attempt and stops enqueuing attempts once it is zero. */
int32_t pikamd_search_global_paths(pikamd_solver* s, const pikamd_params* p, int64_t P, int32_t W,
                                   const double* goal_pos_quat, const double* seed, const double* initial_guess,
                                   const double* max_joint_step, uint64_t rng_seed, int64_t problem_offset,
                                   int32_t max_attempts, double* solution, int32_t* status, double* final_cost,
                                   pikamd_stats* stats, int32_t* reached, int32_t* attempts, pikamd_stats* totals);
/* device pointers (max_joint_step too); enqueues ALL max_attempts attempts on `stream` and returns without
 * synchronising, no self test (see pikamd_solve_batch_device for `slot`): the kernels of an attempt no path is open
 * for find nothing to do and return.  The scratch of the call (the waypoint-0 goals, the starts, the memetic rows, the
 * rows of an attempt behind the first, the open list) belongs to the handle's slot; it grows only when a call needs
 * more than any earlier call on that slot did (a grow frees, and a free synchronises the device: run the largest call
 * first where that matters). */
int32_t pikamd_search_global_paths_device(pikamd_solver* s, const pikamd_params* p, int64_t P, int32_t W,
                                          const double* d_goal_pos_quat, const double* d_seed,
                                          const double* d_initial_guess, const double* d_max_joint_step,
                                          uint64_t rng_seed, int64_t problem_offset, int32_t max_attempts,
                                          double* d_solution, int32_t* d_status, double* d_final_cost,
                                          pikamd_stats* d_stats, int32_t* d_reached, int32_t* d_attempts,
                                          pikamd_stats* d_totals, void* stream, int32_t slot);
/* name of the kernel that walks the waypoints behind the first for P paths (see pikamd_kernel_name), e.g.
 * `pik_exact::ik_globalpath_team_kernel<7,16>`; the memetic kernels in front of it are pikamd_kernel_name's */
const char* pikamd_search_global_paths_kernel_name(const pikamd_solver* s, const pikamd_params* p, int64_t P);
/* ---- computeCartesianPath in one call -----------------------------------------------------------------
 * pikamd_solve_paths walks waypoints the caller made.  What computeCartesianPath is GIVEN is a start joint state, a
 * target pose or offset, a maximum end-effector step and jump thresholds; here P such motions go in, the poses are
 * generated on the device, every path is walked for its OWN number of steps, the absolute and the relative jump test
 * are applied and MoveIt's fraction comes out.
 *
 * pikamd_interpolate_poses (a host function: no handle, no device, like pikamd_shard_bounds).  Quaternions are w x y z.
 * Per path, a = the start pose (ta, qa) and b the resolved target:
 *   GLOBAL: (tt, qt)        TIP: (ta + R(qa) tt, qa (x) qt)        OFFSET: (ta + tt, qa)
 * (R(q): Eigen's toRotationMatrix, no normalisation; (x): the Hamilton product).
 *   trans = |tb - ta|;  rot = 2 atan2(|d.xyz|, |d.w|), d = qa (x) conj(qb)           (Eigen's angularDistance)
 *   t_steps = max_translation > 0 ? floor(trans / max_translation) : 0;  r_steps likewise from rot and max_rotation
 *   n = max(t_steps, r_steps) + 1, raised to the minimum min_steps gives (0: 10 when jump_factor > 0, else 1);
 *   a quotient that is not finite or not below 2^31 gives n = INT32_MAX;  steps[p] = n
 *   waypoint k (0 <= k < n): pct = (double)(k + 1) / (double)n; position pct tb + (1 - pct) ta; orientation Eigen's
 *   slerp(pct, qa, qb): d = qa . qb; |d| >= 1 - 2^-52: the scales are 1 - pct and pct, else theta = acos|d| and they
 *   are sin((1 - pct) theta) / sin theta and sin(pct theta) / sin theta; the second is negated when d < 0; the result
 *   is not normalised.
 * Rows k >= n, and EVERY row of a path with n > W, hold b.  start_pose [P][7], target [P][7], goals [P][W][7],
 * steps [P].  Refused (PIKAMD_EINVAL): a NULL pointer, frame outside 0..2, W < 1, min_steps < 0, neither
 * max_translation nor max_rotation > 0.  P = 0 returns 0.
 * The arithmetic is one header (pik_interp.hpp: IEEE operations rounded one by one, IEEE square roots and quotients,
 * sine and arctangent of one fixed form) compiled for the host and for the device: within one library the host
 * function and the kernels return the SAME BITS in every flavour.
 *
 * pikamd_cartesian_paths.  p->mode must be 1.  The result is DEFINED by the entry points above, bit for bit:
 *
 *   pose0 = pikamd_fk_batch(s, P, start)
 *   (goals, steps) = pikamd_interpolate_poses(c, P, W, pose0, target)
 *   for every p, n = steps[p]:
 *     if n > W:  every row = (start[p], PIKAMD_NOT_ATTEMPTED, 0, zero); reached[p] = 0; fraction[p] = 0
 *     else:
 *       rows 0..n-1 = pikamd_solve_paths(p, P = 1, W = n, goals[p][0..n-1], start[p], max_joint_step); r = its reached
 *       rows n..W-1 = (solution row n-1, PIKAMD_NOT_ATTEMPTED, 0, zero)
 *       fraction[p] = (double)r / (double)n
 *       if c->jump_factor > 0 and r >= 1:
 *         traj[0] = start[p]; traj[i] = solution[p][i-1] for i = 1..r
 *         dist[i] = sum over j ascending of fabs(traj[i+1][j] - traj[i][j]), i = 0..r-1   (from 0.0, every operation
 *                   rounded on its own)
 *         total = sum of dist[i], i ascending;  thres = c->jump_factor * (total / (double)r)
 *         for the first i with dist[i] > thres:
 *           fraction[p] *= (double)(i+1) / (double)(r+1)                          (MoveIt: (i+1) / traj.size())
 *           solution rows i..W-1 = traj[i]; status[p][i] = PIKAMD_PATH_RELATIVE_JUMP (its cost and stats stay what the
 *           solve returned); rows i+1..W-1 = (traj[i], PIKAMD_NOT_ATTEMPTED, 0, zero);  r = i
 *       reached[p] = r
 *
 * Consequences: when jump_factor is not > 0 and every steps[p] equals W, the call is pikamd_fk_batch +
 * pikamd_interpolate_poses + pikamd_solve_paths.  A path with steps[p] > W was not walked: call again with W >= the
 * largest steps[p].  dist is MoveIt's group distance for bounded revolute and prismatic variables; continuous, planar
 * and floating variables are compared unwrapped, variable by variable -- the departure max_joint_step already has.
 * The absolute thresholds (JumpThreshold::revolute and prismatic) are the caller's max_joint_step.  The handle's
 * approximate-solution gate is NOT applied, as in pikamd_solve_paths.
 *   start [P][dof], target [P][7], max_joint_step [dof] (may be NULL), solution [P][W][dof], status [P][W],
 *   final_cost [P][W] (may be NULL), stats [P][W] (may be NULL), reached [P] (may be NULL), steps [P] (REQUIRED),
 *   fraction [P] (may be NULL), goals [P][W][7] (may be NULL): the poses that were walked.
 * Refused: several tip frames (PIKAMD_EUNSUPPORTED); mode 0, joint_layout = soa, steps == NULL and everything
 * pikamd_interpolate_poses refuses (PIKAMD_EINVAL).  P = 0 returns 0.
 * Not served (out of scope): the relative test inside pikamd_search_paths and pikamd_search_global_paths, a validity
 * callback, sharding, a plugin-shim entry (KinematicsBase has none).
 * pikamd_cartesian_paths: host pointers; synchronous, staged through the library's own pinned buffers and stream like
 * pikamd_solve_paths, behind the same automatic self test of the local-mode kernels; honours lanes_per_elite as
 * pikamd_solve_paths does.  pikamd_cartesian_paths_device: device pointers (max_joint_step too); enqueues a prepare
 * kernel (forward kinematics, poses, steps) and the walk on `stream` and returns without synchronising, no self test
 * (see pikamd_solve_batch_device for `slot`).  Without d_goals the poses are kept in scratch that belongs to the
 * handle's slot; it grows only when a call needs more than any earlier call on that slot did (a grow frees, and a free
 * synchronises the device: run the largest call first where that matters).  pikamd_cartesian_kernel_name: the kernel
 * that walks P paths (see pikamd_kernel_name), e.g. `pik_exact::ik_cartesian_team_kernel<7,16>`. */
#define PIKAMD_PATH_RELATIVE_JUMP (-1003) /* outside MoveItErrorCodes, like PIKAMD_PATH_JUMP */
#define PIKAMD_CARTESIAN_GLOBAL 0 /* target is a pose in the base frame */
#define PIKAMD_CARTESIAN_TIP 1    /* target is relative to the start tip frame: b = a * target */
#define PIKAMD_CARTESIAN_OFFSET 2 /* target's translation is added to the start's in the base frame, orientation kept
                                     (target's quaternion ignored) */
typedef struct pikamd_cartesian {
    int32_t frame;          /* PIKAMD_CARTESIAN_* */
    int32_t min_steps;      /* 0 = MoveIt's rule: 10 when jump_factor > 0, else 1; > 0: that many */
    double max_translation; /* MaxEEFStep::translation; not > 0: not limiting */
    double max_rotation;    /* MaxEEFStep::rotation (rad); not > 0: not limiting */
    double jump_factor;     /* relative jump threshold factor; not > 0: no relative test */
} pikamd_cartesian;
int32_t pikamd_interpolate_poses(const pikamd_cartesian* c, int64_t P, int32_t W, const double* start_pose,
                                 const double* target, double* goals, int32_t* steps);
int32_t pikamd_cartesian_paths(pikamd_solver* s, const pikamd_params* p, const pikamd_cartesian* c, int64_t P,
                               int32_t W, const double* start, const double* target, const double* max_joint_step,
                               double* solution, int32_t* status, double* final_cost, pikamd_stats* stats,
                               int32_t* reached, int32_t* steps, double* fraction, double* goals);
int32_t pikamd_cartesian_paths_device(pikamd_solver* s, const pikamd_params* p, const pikamd_cartesian* c, int64_t P,
                                      int32_t W, const double* d_start, const double* d_target,
                                      const double* d_max_joint_step, double* d_solution, int32_t* d_status,
                                      double* d_final_cost, pikamd_stats* d_stats, int32_t* d_reached,
                                      int32_t* d_steps, double* d_fraction, double* d_goals, void* stream,
                                      int32_t slot);
const char* pikamd_cartesian_kernel_name(const pikamd_solver* s, const pikamd_params* p, int64_t P);
/* ---- computeCartesianPath through waypoints ---------------------------------------------------------------
 * MoveIt's computeCartesianPath has a second overload: a LIST of waypoints per motion (approach - grasp - retreat,
 * corners, anything that is not one straight line).  Segment i starts at the tip pose of the joint state segment i-1
 * ended in -- that is not waypoint i-1 itself --, so its poses and its step count exist only once segment i-1 has been
 * solved.  With pikamd_cartesian_paths that is S dependent calls, each staged and synchronised, the complete paths
 * picked and repacked on the host between them, and the relative jump test -- which MoveIt applies ONCE, to the
 * stitched trajectory -- redone by hand.  Here P motions of up to S targets each go in and one call does it, with no
 * host round trip between the segments.
 *
 * pikamd_cartesian_waypoints.  p->mode must be 1.  pikamd_cartesian is reused unchanged.  The result is DEFINED by the
 * entry points above, bit for bit:
 *
 *   c1 = *c with jump_factor = 0     (MoveIt walks every segment of a waypoint list with NO jump test, so min_steps = 0
 *                                     resolves to 1 here, never to 10; a min_steps > 0 holds for every segment)
 *   for every p:  S_p = n_targets ? clamp(n_targets[p], 0, S) : S
 *     every row = (start[p], PIKAMD_NOT_ATTEMPTED, 0, zero); every goals row = seven zeros; segment_steps[p][*] = 0
 *     cur = start[p]; off = 0; held = 0; frac = 0.0; need = 0
 *     for i in 0 .. S_p-1:
 *       room = W - off
 *       if room == 0: n_i = the steps of pikamd_interpolate_poses(c1, 1, 1, pikamd_fk_batch(cur), targets[p][i])
 *       else:         (rows, n_i, r_i, g) = pikamd_cartesian_paths(p, c1, P = 1, W = room, start = cur, targets[p][i],
 *                                                                  max_joint_step)
 *       segment_steps[p][i] = n_i;  need = off + n_i, saturating at INT32_MAX
 *       if room > 0: goals rows off..W-1 = g                  (a segment that does not fit: every one of them its target)
 *       if n_i > room:                 rows off..W-1 = (cur, NOT_ATTEMPTED, 0, zero); stop       (did not fit; frac stays)
 *       rows off..W-1 = rows                                   (the next segment overwrites what lies behind n_i)
 *       held = off + r_i
 *       if r_i == n_i: frac = (double)(i+1) / (double)S_p; cur = solution row off+n_i-1; off += n_i
 *       else:          frac = (double)i / (double)S_p + ((double)r_i / (double)n_i) / (double)S_p; stop
 *     steps[p] = need;  r = held
 *     if c->jump_factor > 0 and r >= 1: the relative test of pikamd_cartesian_paths, statement for statement, over
 *        traj[0] = start[p], traj[j] = solution[p][j-1], j = 1..r   (fraction = frac * (i+1)/(r+1), row i =
 *        PIKAMD_PATH_RELATIVE_JUMP, rows behind it blank with traj[i], r = i)
 *     reached[p] = r;  fraction[p] = the result
 *
 * Every floating-point operation is rounded on its own.  Consequences:
 *   - S = 1 with jump_factor not > 0 is pikamd_cartesian_paths, array for array (segment_steps[p][0] = steps[p]).
 *   - S = 1 with jump_factor > 0 is pikamd_cartesian_paths when min_steps > 0 is given explicitly.  With min_steps = 0
 *     the two differ in MoveIt's minimum: 1 here, 10 there.  That is MoveIt's own behaviour for a waypoint list.
 *   - In the TIP and OFFSET frames target i is relative to the tip pose of the state segment i-1 ended in.
 *   - The absolute thresholds are the caller's max_joint_step, applied while walking: the departure
 *     pikamd_cartesian_paths already has.
 *   - S_p = 0 gives reached 0, steps 0, fraction 0.
 *   - steps[p] > W means: call again with W >= steps[p] (when the segment that did not fit was not the last, again
 *     until it holds).  The rows in front of the segment that did not fit are valid.
 *   - The handle's approximate-solution gate is NOT applied.
 *   start [P][dof], targets [P][S][7] (meaning per c->frame), n_targets [P] (may be NULL: S for every path; values are
 *   clamped to 0..S), max_joint_step [dof] (may be NULL), solution [P][W][dof], status [P][W], final_cost [P][W] (may be
 *   NULL), stats [P][W] (may be NULL), reached [P] (may be NULL), steps [P] (REQUIRED: the rows the path needs in all),
 *   segment_steps [P][S] (may be NULL: the step count of every segment started, 0 for the others), fraction [P] (may be
 *   NULL), goals [P][W][7] (may be NULL): the poses that were walked.
 * Refused: several tip frames (PIKAMD_EUNSUPPORTED); everything pikamd_cartesian_paths refuses, S < 1, S > W (every
 * segment needs at least one row) and a NULL targets (PIKAMD_EINVAL).  P = 0 returns 0.  No plugin-shim entry
 * (KinematicsBase has none).
 * pikamd_cartesian_waypoints: host pointers; synchronous, staged through the library's own pinned buffers and stream
 * like pikamd_cartesian_paths, behind the same automatic self test of the local-mode kernels; honours lanes_per_elite
 * as pikamd_solve_paths does.  pikamd_cartesian_waypoints_device: device pointers (n_targets and max_joint_step too);
 * enqueues S passes -- a segment kernel (forward kinematics of the current state, poses, steps) and the walk of the
 * segment -- and a finish kernel (blank rows, relative test, reached, steps, fraction) on `stream` and returns without
 * synchronising, no self test (see pikamd_solve_batch_device for `slot`).  A pass in which no path is open finds
 * nothing to walk.  The per-path state of the passes and, without d_goals, the poses are kept in scratch that belongs
 * to the handle's slot; it grows only when a call needs more than any earlier call on that slot did (a grow frees,
 * and a free synchronises the device: run the largest call first where that matters).
 * pikamd_cartesian_waypoints_kernel_name: the kernel that walks the segments of P paths (see pikamd_kernel_name), e.g.
 * `pik_exact::ik_polyline_team_kernel<7,16>`. */
int32_t pikamd_cartesian_waypoints(pikamd_solver* s, const pikamd_params* p, const pikamd_cartesian* c, int64_t P,
                                   int32_t S, int32_t W, const double* start, const double* targets,
                                   const int32_t* n_targets, const double* max_joint_step, double* solution,
                                   int32_t* status, double* final_cost, pikamd_stats* stats, int32_t* reached,
                                   int32_t* steps, int32_t* segment_steps, double* fraction, double* goals);
int32_t pikamd_cartesian_waypoints_device(pikamd_solver* s, const pikamd_params* p, const pikamd_cartesian* c, int64_t P,
                                          int32_t S, int32_t W, const double* d_start, const double* d_targets,
                                          const int32_t* d_n_targets, const double* d_max_joint_step, double* d_solution,
                                          int32_t* d_status, double* d_final_cost, pikamd_stats* d_stats,
                                          int32_t* d_reached, int32_t* d_steps, int32_t* d_segment_steps,
                                          double* d_fraction, double* d_goals, void* stream, int32_t slot);
const char* pikamd_cartesian_waypoints_kernel_name(const pikamd_solver* s, const pikamd_params* p, int64_t P);
/* ---- Sphere collision model: the validity test of a handle -------------------------------------------
 * Behind every solve searchPositionIK calls the solution callback (src/pick_ik_plugin.cpp:269-274), in MoveIt the
 * state-validity check: an answer it refuses becomes a failure and the search restarts from a random state.  A host
 * callback cannot run inside a device search; what can is the test GPU planners use: the robot as spheres fixed to
 * its links, obstacles as spheres fixed in the base frame, and a list of sphere pairs that must not overlap.
 *
 * pikamd_validity_batch: valid[i] / clearance[i] / centres[i] of candidate q[i], DEFINED by entry points above:
 *   centre_k(q):  after_variable = -1: centres[k] as given (copied, no arithmetic)
 *                 after_variable = v:  the position (first three numbers) of pikamd_fk_batch of a handle made by
 *                                      pikamd_create IN THE SAME LIBRARY, arithmetic = exact, for the chain cut behind
 *                                      variable v: dof = v + 1, the first v + 1 entries of every per-variable array,
 *                                      tip_xyz_rpy = (centre, 0, 0, 0), evaluated at q[0..v]
 *   for pair m = (i, j), ascending m:  dx, dy, dz = centre_i - centre_j by component
 *                                      d2 = (dx*dx + dy*dy) + dz*dz;  clear_m = sqrt(d2) - (r_i + r_j)
 *                                      (every operation rounded on its own, IEEE square root, in every flavour)
 *   clearance = +infinity;  for m ascending: if clear_m < clearance: clearance = clear_m      (a NaN never replaces)
 *   valid = 0 if clear_m < 0.0 for some m, else 1                                        (a NaN does not trip the test)
 * Touching spheres (clear_m = 0.0) are valid.  n_pairs = 0 gives valid = 1 and clearance = +infinity everywhere.  The
 * same arithmetic serves every handle, whatever its option `arithmetic` (as the restart draws do).
 *   q [n][dof], valid [n], clearance [n] (may be NULL), centres [n][n_spheres][3] (may be NULL; caller's sphere order).
 * Without a model on the handle: PIKAMD_EINVAL.  n = 0 returns 0.  Not with the option joint_layout = soa.
 *
 * pikamd_set_validity_model: the model of this handle (NULL: none, the default); like pikamd_set_option not concurrent
 * with another call on the handle, read when a call is made.  It copies the model, uploads it and synchronises.
 * PIKAMD_EINVAL: a NULL array that is needed, counts outside 0..PIKAMD_MAX_SPHERES / 0..PIKAMD_MAX_SPHERE_PAIRS, a
 * radius or centre that is not finite, a radius below 0, a pair index out of range or i == j, after_variable outside
 * -1..dof-1 or naming the _X / _Y slot of a planar joint (the chain cannot be cut there).  PIKAMD_EUNSUPPORTED: a
 * handle with several tip frames, with a floating joint, or with mimic joints.
 *
 * The model is the validity step of pikamd_search_batch* and pikamd_search_global_batch* (their loops above), applied
 * to PIKAMD_SUCCESS as well as PIKAMD_APPROXIMATE, behind the gate; a failed or gate-refused attempt is not tested.
 * pikamd_solve_batch*, pikamd_solve_batch_host and every path entry point (pikamd_solve_paths*, pikamd_search_paths*,
 * pikamd_search_global_paths*, pikamd_cartesian_paths*, pikamd_cartesian_waypoints*) IGNORE it. */
#define PIKAMD_MAX_SPHERES 32
#define PIKAMD_MAX_SPHERE_PAIRS 256
#define PIKAMD_VALIDITY_REFUSED (-1004) /* outside MoveItErrorCodes, like PIKAMD_GATE_REFUSED */
typedef struct pikamd_sphere {
    int32_t after_variable; /* the sphere is fixed to the link behind the joint of this variable; -1: fixed in the base frame (an obstacle, the base link) */
    int32_t reserved;       /* 0 */
    double centre[3];       /* in that link's frame (after_variable = -1: in the base frame) */
    double radius;
} pikamd_sphere;
typedef struct pikamd_validity_model {
    int32_t n_spheres;
    const pikamd_sphere* spheres;
    int32_t n_pairs;
    const int32_t* pairs; /* [n_pairs][2] sphere indices that must not overlap */
} pikamd_validity_model;
int32_t pikamd_set_validity_model(pikamd_solver* s, const pikamd_validity_model* m);
/* host pointers; synchronous */
int32_t pikamd_validity_batch(pikamd_solver* s, int64_t n, const double* q, int32_t* valid, double* clearance,
                              double* centres);
/* device pointers; enqueues on `stream` and returns without synchronising */
int32_t pikamd_validity_batch_device(pikamd_solver* s, int64_t n, const double* d_q, int32_t* d_valid,
                                     double* d_clearance, double* d_centres, void* stream);
/* ---- The validity model inside the path entry points that start from a joint state --------------------
 * computeCartesianPath always receives a validity callback: it hands it to setFromIK for every waypoint, the first
 * waypoint whose answer is in collision ends the path, the fraction counts the waypoints in front of it, and the
 * relative jump test then runs over what is left.  pikamd_set_path_validity is the opt-in that puts the handle's
 * sphere model (pikamd_set_validity_model above) in that place.
 *
 * With applies = (the switch is on and the handle has a model), the loop that defines pikamd_solve_paths (above)
 * reads, for path p and waypoint k while held[p]:
 *     (sol, st, cost, stats) = pikamd_solve_batch(local mode, goal[p][k], seed = initial guess = seed[p])
 *     jump    = st > 0 and (the joint-step test, unchanged)
 *     refused = applies and st > 0 and not jump and valid(sol) == 0
 *                   (valid: pikamd_validity_batch's, bit for bit; a jumped answer is not tested; no cost_fn invocation
 *                    is counted)
 *     if st > 0 and not jump and not refused: hold, as before
 *     else: solution[p][k] = seed[p]; status[p][k] = jump ? PIKAMD_PATH_JUMP : refused ? PIKAMD_VALIDITY_REFUSED : st;
 *           held[p] = false
 *     final_cost[p][k] = cost; stats[p][k] = stats      (what the call returned, also for a refused answer)
 * With applies false this is the loop as it stands above: nothing changes.  The rows behind the refused one are blank
 * as behind any other stop, and reached[p] counts the waypoints in front of it.
 *
 * pikamd_cartesian_paths is defined by pikamd_solve_paths per path and pikamd_cartesian_waypoints by
 * pikamd_cartesian_paths per segment, so both inherit the step:
 *   - pikamd_cartesian_paths: r counts the waypoints in front of the refused one, fraction = r / n, and the relative
 *     test runs afterwards, over traj[0..r] of the cut path (MoveIt's order).  A cut changes the mean step, so the
 *     relative stop can move, appear or vanish.
 *   - pikamd_cartesian_waypoints: a refused row gives r_i < n_i; the path stops in that segment with
 *     frac = i / S_p + (r_i / n_i) / S_p, and no later segment is started.  The relative test runs once, over the
 *     stitched rows.
 *   - The start state is not tested (MoveIt does not test it either).
 * The test's arithmetic is the exact flavour's for every handle, as in pikamd_search_global_batch: a handle with
 * arithmetic = fast is served (unlike pikamd_search_batch).  On the device the step is a pass of its own behind the
 * walk (no walk kernel changes, no host round trip): the descents behind a collision are run and thrown away.
 *
 * pikamd_search_paths* and pikamd_search_global_paths* keep ignoring the model whatever the switch says: their
 * attempt loops are fused with the walk.  pikamd_solve_batch* ignores it as before.
 *
 * pikamd_set_path_validity: 0 (the default) or 1; any other value is PIKAMD_EINVAL.  Like pikamd_set_approximate_gate
 * not concurrent with another call on the handle, read when a call is made.  It needs no model: with the switch on and
 * no model nothing changes, and pikamd_set_validity_model(s, NULL) leaves the switch as it is.  A handle the model
 * cannot walk (several tip frames, a floating joint, mimic joints set after the model) is PIKAMD_EUNSUPPORTED at the
 * path call.  A path call with reached = NULL keeps the count the step reads in the slot's scratch, which grows only
 * when a call needs more. */
/* 0 (default): the path entry points ignore the handle's validity model, as before.
 * 1: pikamd_solve_paths*, pikamd_cartesian_paths*, pikamd_cartesian_waypoints* apply it (above). */
int32_t pikamd_set_path_validity(pikamd_solver* s, int32_t on);
/* ---- Device-side choice of the regime (option device_regime) -------------------------------------
 * A memetic call on one tip frame with one species and nothing forced (lanes_per_elite, its schedule, regime) is cut
 * into passes whose kernel variant is chosen when the pass starts: a one-wavefront router in front of the pass takes
 * the latency schedule (most lanes per elite that fit the chip) unless the calls in flight on the handle's OTHER
 * slots hold at least regime_threshold problems (default: SIMD count * 32 / pow2ceil(elites), half of what puts a
 * one-lane wavefront on every SIMD), in which case it takes the throughput schedule (one lane per elite).  Like every scheduling option
 * this changes no result.  device_regime = 0: the regime is chosen once per call on the host, from the number of
 * other calls in flight when it is enqueued.
 *
 * pikamd_debug_regime (tests, profile scripts; synchronises the device): for the LAST solve call on `slot`,
 * *n_passes = the passes the routed launcher cut it into, or -1 when the call was not routed (host rule); for pass
 * k < min(*n_passes, max_passes): survivors[k] = problems the pass started with, others_load[k] = the load the
 * router saw on the other slots, variant[k] = the kernel variant it chose (5 / 4 / 3 / 2: 16 / 8 / 4 / 2 lanes per
 * elite, 1: one lane, 7: one lane, two wavefronts per SIMD; 0: no survivor, no kernel ran).  publish_load >= 0: first
 * sets the load `slot` publishes to the other slots' routers to that many problems (a slot with no call in flight:
 * an artificial load; a routed call on the slot overwrites it); < 0: leaves it.  Any of the output pointers may be
 * NULL with max_passes = 0. */
int32_t pikamd_debug_regime(pikamd_solver* s, int32_t slot, int64_t publish_load, int32_t max_passes,
                            int32_t* n_passes, uint32_t* survivors, uint32_t* others_load, int32_t* variant);
/* [host-api-end] */

#ifdef __cplusplus
}
#endif
#endif /* PICK_IK_AMD_H */
