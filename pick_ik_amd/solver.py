"""ctypes binding of libpick_ik_amd.so (include/pick_ik_amd.h) -- the host-side mirror of pick_ik's
solver interface for batch callers.

Names follow the reference: ``ik_memetic`` / ``ik_gradient`` (include/pick_ik/ik_memetic.hpp:97-104,
include/pick_ik/ik_gradient.hpp:43-49), ``Params`` carries the fields of
src/pick_ik_parameters.yaml.  There is no CPU implementation behind this module: if the HIP
library is missing or no gfx950 device is present every call raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PIK_LIB") or os.path.join(_HERE, "libpick_ik_amd.so")  # (PIK_LIB: A/B experiments)
#: verification build (no FMA contraction, generic rotations); see pick_ik_amd/build.py
LIB_STRICT_PATH = os.environ.get("PIK_LIB_STRICT") or os.path.join(_HERE, "libpick_ik_amd_strict.so")

SUCCESS = 1
APPROXIMATE = 2
NO_IK_SOLUTION = -31
NOT_ATTEMPTED = 0  # solve_paths: a waypoint behind the one its path stopped at
PATH_JUMP = -1001  # solve_paths: solved, but a variable moved further than max_joint_step allows
MAX_ATTEMPTS = 64  # search_batch: PIKAMD_MAX_ATTEMPTS
MAX_SLOTS = 128
MAX_BATCHES = 64
MAX_HOST_JOBS = 16


class PickIkAmdError(RuntimeError):
    pass


class Params(C.Structure):
    """pikamd_params: src/pick_ik_parameters.yaml names and defaults, iteration budgets only."""

    _fields_ = [
        ("mode", C.c_int32),
        ("gd_step_size", C.c_double),
        ("gd_max_iters", C.c_int32),
        ("gd_min_cost_delta", C.c_double),
        ("position_threshold", C.c_double),
        ("orientation_threshold", C.c_double),
        ("cost_threshold", C.c_double),
        ("position_scale", C.c_double),
        ("rotation_scale", C.c_double),
        ("center_joints_weight", C.c_double),
        ("avoid_joint_limits_weight", C.c_double),
        ("minimal_displacement_weight", C.c_double),
        ("stop_optimization_on_valid_solution", C.c_int32),
        ("memetic_num_threads", C.c_int32),
        ("memetic_stop_on_first_solution", C.c_int32),
        ("memetic_population_size", C.c_int32),
        ("memetic_elite_size", C.c_int32),
        ("memetic_wipeout_fitness_tol", C.c_double),
        ("memetic_max_generations", C.c_int32),
        ("memetic_gd_max_iters", C.c_int32),
        ("return_approximate_solution", C.c_int32),
    ]


class _Chain(C.Structure):
    _fields_ = [
        ("dof", C.c_int32),
        ("origin_xyz_rpy", C.POINTER(C.c_double)),
        ("axis", C.POINTER(C.c_double)),
        ("joint_type", C.POINTER(C.c_int32)),
        ("tip_xyz_rpy", C.POINTER(C.c_double)),
        ("qmin", C.POINTER(C.c_double)),
        ("qmax", C.POINTER(C.c_double)),
        ("vmax", C.POINTER(C.c_double)),
        ("bounded", C.POINTER(C.c_uint8)),
    ]


class _Tip(C.Structure):
    _fields_ = [
        ("n_joints", C.c_int32),
        ("variable", C.POINTER(C.c_int32)),
        ("origin_xyz_rpy", C.POINTER(C.c_double)),
        ("axis", C.POINTER(C.c_double)),
        ("joint_type", C.POINTER(C.c_int32)),
        ("tip_xyz_rpy", C.POINTER(C.c_double)),
    ]


class _MultiChain(C.Structure):
    _fields_ = [
        ("dof", C.c_int32),
        ("n_tips", C.c_int32),
        ("tips", C.POINTER(_Tip)),
        ("qmin", C.POINTER(C.c_double)),
        ("qmax", C.POINTER(C.c_double)),
        ("vmax", C.POINTER(C.c_double)),
        ("bounded", C.POINTER(C.c_uint8)),
    ]


class Gate(C.Structure):
    """pikamd_gate: the approximate-solution gate (src/pick_ik_plugin.cpp:219-267)"""
    _fields_ = [("cost_threshold", C.c_double), ("joint_threshold", C.c_double)]


#: status of an answer the gate refused (PIKAMD_GATE_REFUSED)
GATE_REFUSED = -1002


class Sphere(C.Structure):
    """pikamd_sphere: a sphere fixed to the link behind the joint of variable `after_variable` (-1: fixed in the base
    frame -- an obstacle, the base link), its centre in that link's frame"""
    _fields_ = [("after_variable", C.c_int32), ("reserved", C.c_int32), ("centre", C.c_double * 3), ("radius", C.c_double)]

    def __init__(self, after_variable=-1, centre=(0.0, 0.0, 0.0), radius=0.0):
        super().__init__(int(after_variable), 0, (C.c_double * 3)(*[float(v) for v in centre]), float(radius))


class ValidityModel(C.Structure):
    """pikamd_validity_model"""
    _fields_ = [("n_spheres", C.c_int32), ("spheres", C.POINTER(Sphere)), ("n_pairs", C.c_int32), ("pairs", C.POINTER(C.c_int32))]


#: limits of a validity model (PIKAMD_MAX_SPHERES, PIKAMD_MAX_SPHERE_PAIRS) and the status of an answer the validity
#: test refused (PIKAMD_VALIDITY_REFUSED)
MAX_SPHERES, MAX_SPHERE_PAIRS = 32, 256
VALIDITY_REFUSED = -1004

#: cartesian_paths: the first waypoint whose joint-space step is further than jump_factor times the mean step
#: (PIKAMD_PATH_RELATIVE_JUMP)
PATH_RELATIVE_JUMP = -1003
#: Cartesian.frame (PIKAMD_CARTESIAN_*): the target is a pose in the base frame / relative to the start tip frame / a
#: translation added to the start's in the base frame, orientation kept
CARTESIAN_GLOBAL, CARTESIAN_TIP, CARTESIAN_OFFSET = 0, 1, 2


class Cartesian(C.Structure):
    """pikamd_cartesian: what computeCartesianPath is given beside the start state and the target -- the frame of the
    target, MaxEEFStep (max_translation, max_rotation; not > 0: not limiting), the minimum step count (0: MoveIt's rule,
    10 with a relative test and 1 without) and the relative jump threshold factor (not > 0: no relative test)"""
    _fields_ = [("frame", C.c_int32), ("min_steps", C.c_int32), ("max_translation", C.c_double),
                ("max_rotation", C.c_double), ("jump_factor", C.c_double)]

    def __init__(self, frame=CARTESIAN_GLOBAL, min_steps=0, max_translation=0.0, max_rotation=0.0, jump_factor=0.0):
        super().__init__(frame, min_steps, max_translation, max_rotation, jump_factor)


class Batch(C.Structure):
    """pikamd_batch: one batch of a multi-batch call (device or host pointers, see the header)."""

    _fields_ = [
        ("B", C.c_int64),
        ("goal_pos_quat", C.c_void_p),
        ("seed", C.c_void_p),
        ("initial_guess", C.c_void_p),
        ("problem_offset", C.c_int64),
        ("solution", C.c_void_p),
        ("status", C.c_void_p),
        ("final_cost", C.c_void_p),
        ("stats", C.c_void_p),
        ("completed", C.c_void_p),
    ]


MAX_DOF, MAX_TIPS, MAX_NAME, MAX_MIMIC = 16, 8, 64, 4  # (PIKAMD_MAX_MIMIC: per tip path)


class _UrdfTip(C.Structure):
    _fields_ = [("n_joints", C.c_int32), ("variable", C.c_int32 * MAX_DOF),
                ("origin_xyz_rpy", C.c_double * 6 * MAX_DOF), ("axis", C.c_double * 3 * MAX_DOF),
                ("joint_type", C.c_int32 * MAX_DOF), ("tip_xyz_rpy", C.c_double * 6)]


class MimicJointC(C.Structure):
    """pikamd_mimic_joint / pko_mimic_joint"""
    _fields_ = [("tip", C.c_int32), ("after_variable", C.c_int32), ("master_variable", C.c_int32), ("joint_type", C.c_int32),
                ("origin_xyz_rpy", C.c_double * 6), ("axis", C.c_double * 3), ("multiplier", C.c_double), ("offset", C.c_double)]


def mimic_array(chain):
    """the chain's MimicJoint records as a C array (None when it has none)"""
    ms = tuple(getattr(chain, "mimic", ()) or ())
    if not ms:
        return None
    arr = (MimicJointC * len(ms))()
    for i, m in enumerate(ms):
        arr[i] = MimicJointC(int(m.tip), int(m.after_variable), int(m.master_variable), int(m.joint_type),
                             (C.c_double * 6)(*[float(x) for x in m.origin_xyz_rpy]), (C.c_double * 3)(*[float(x) for x in m.axis]),
                             float(m.multiplier), float(m.offset))
    return arr


class UrdfModel(C.Structure):
    """pikamd_urdf_model: what pikamd_urdf_extract found between base_link and the tip link(s)."""

    _fields_ = [("dof", C.c_int32), ("n_tips", C.c_int32), ("variable_names", (C.c_char * MAX_NAME) * MAX_DOF),
                ("qmin", C.c_double * MAX_DOF), ("qmax", C.c_double * MAX_DOF), ("vmax", C.c_double * MAX_DOF),
                ("bounded", C.c_uint8 * MAX_DOF), ("tips", _UrdfTip * MAX_TIPS),
                ("n_mimic", C.c_int32), ("mimic", MimicJointC * (MAX_TIPS * MAX_MIMIC))]


STATS_DTYPE = np.dtype(
    [("cost_evals", "<i8"), ("generations", "<i4"), ("wipeouts", "<i4"),
     ("pool_erasures", "<i4"), ("reserved", "<i4")])

#: every symbol include/pick_ik_amd.h declares
EXPORTED_SYMBOLS = (
    "pikamd_default_params", "pikamd_create", "pikamd_destroy", "pikamd_variables",
    "pikamd_fk_batch", "pikamd_cost_batch", "pikamd_gd_step_batch", "pikamd_solve_batch",
    "pikamd_solve_batch_device", "pikamd_fk_batch_device", "pikamd_last_error", "pikamd_version",
    "pikamd_kernel_name", "pikamd_reserve", "pikamd_create_multi", "pikamd_n_tips",
    "pikamd_solve_batches_device", "pikamd_solve_batches_async", "pikamd_wait", "pikamd_solve_batches",
    "pikamd_urdf_extract", "pikamd_create_from_urdf", "pikamd_set_option", "pikamd_solve_batch_host", "pikamd_set_mimic_joints",
    "pikamd_shard_bounds", "pikamd_solve_batch_sharded", "pikamd_self_test", "pikamd_self_test_cost",
    "pikamd_solve_paths", "pikamd_solve_paths_device", "pikamd_path_kernel_name",
    "pikamd_search_batch", "pikamd_search_batch_device", "pikamd_search_kernel_name",
    "pikamd_debug_regime", "pikamd_search_global_batch", "pikamd_search_global_batch_device",
    "pikamd_gate_batch", "pikamd_set_approximate_gate",
    "pikamd_search_paths", "pikamd_search_paths_device", "pikamd_search_paths_kernel_name",
    "pikamd_search_global_paths", "pikamd_search_global_paths_device", "pikamd_search_global_paths_kernel_name",
    "pikamd_interpolate_poses", "pikamd_cartesian_paths", "pikamd_cartesian_paths_device", "pikamd_cartesian_kernel_name",
    "pikamd_cartesian_waypoints", "pikamd_cartesian_waypoints_device", "pikamd_cartesian_waypoints_kernel_name",
    "pikamd_set_validity_model", "pikamd_validity_batch", "pikamd_validity_batch_device",
    "pikamd_set_path_validity",
)

_libs = {}


# double cost_fn(const double* q, int32_t dof, int32_t pose_index, void* user) -- pikamd_cost_fn
COST_FN = C.CFUNCTYPE(C.c_double, C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_void_p)


def cost_callback(fn):
    """Python callable fn(q: ndarray[dof], pose_index) -> float as a pikamd_cost_fn"""
    def trampoline(q, dof, pose, _user):
        return float(fn(np.ctypeslib.as_array(q, shape=(dof,)).copy(), int(pose)))
    return COST_FN(trampoline)


def lib(strict: bool = False):
    """Load the HIP library; fails loudly when it has not been built (no fallback)."""
    if strict in _libs:
        return _libs[strict]
    path = LIB_STRICT_PATH if strict else LIB_PATH
    if not os.path.exists(path):
        raise PickIkAmdError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). pick_ik_amd has no CPU fallback.")
    L = C.CDLL(path)
    dp = C.POINTER(C.c_double)
    ip = C.POINTER(C.c_int32)
    vp = C.c_void_p
    L.pikamd_default_params.argtypes = [C.POINTER(Params)]
    L.pikamd_default_params.restype = None
    L.pikamd_create.argtypes = [C.POINTER(_Chain), C.c_int32, C.POINTER(vp)]
    L.pikamd_create_multi.argtypes = [C.POINTER(_MultiChain), C.c_int32, C.POINTER(vp)]
    L.pikamd_create_multi.restype = C.c_int32
    L.pikamd_n_tips.argtypes = [vp]
    L.pikamd_n_tips.restype = C.c_int32
    L.pikamd_destroy.argtypes = [vp]
    L.pikamd_destroy.restype = None
    L.pikamd_variables.argtypes = [vp, dp]
    L.pikamd_fk_batch.argtypes = [vp, C.c_int64, dp, dp]
    L.pikamd_cost_batch.argtypes = [vp, C.POINTER(Params), C.c_int64, dp, dp, dp, dp, ip]
    L.pikamd_gd_step_batch.argtypes = [vp, C.POINTER(Params), C.c_int64, dp, dp, dp, dp, dp, dp,
                                       dp, ip]
    L.pikamd_solve_batch.argtypes = [vp, C.POINTER(Params), C.c_int64, dp, dp, C.c_uint64,
                                     C.c_int64, dp, ip, dp, vp]
    L.pikamd_solve_batch_device.argtypes = [vp, C.POINTER(Params), C.c_int64, vp, vp, C.c_uint64,
                                            C.c_int64, vp, vp, vp, vp, vp, C.c_int32]
    L.pikamd_fk_batch_device.argtypes = [vp, C.c_int64, vp, vp, vp]
    L.pikamd_solve_batches_device.argtypes = [vp, C.POINTER(Params), C.c_int32, C.POINTER(Batch),
                                              C.c_uint64, vp, C.c_int32]
    L.pikamd_solve_batches_async.argtypes = [vp, C.POINTER(Params), C.c_int32, C.POINTER(Batch),
                                             C.c_uint64, C.c_int32]
    L.pikamd_wait.argtypes = [vp, C.c_int32]
    L.pikamd_solve_batches.argtypes = [vp, C.POINTER(Params), C.c_int32, C.POINTER(Batch), C.c_uint64]
    L.pikamd_reserve.argtypes = [vp, C.POINTER(Params), C.c_int64, C.c_int32, vp]
    L.pikamd_reserve.restype = C.c_int32
    L.pikamd_urdf_extract.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int32,
                                      C.POINTER(UrdfModel)]
    L.pikamd_urdf_extract.restype = C.c_int32
    L.pikamd_create_from_urdf.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int32, C.c_int32,
                                          C.POINTER(vp)]
    L.pikamd_create_from_urdf.restype = C.c_int32
    L.pikamd_shard_bounds.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.pikamd_shard_bounds.restype = None
    L.pikamd_solve_batch_sharded.argtypes = [C.POINTER(vp), C.c_int32, C.POINTER(Params), C.c_int64, dp, dp, dp,
                                             C.c_uint64, C.c_int64, dp, ip, dp, vp]
    L.pikamd_solve_batch_sharded.restype = C.c_int32
    L.pikamd_self_test.argtypes = [vp, C.POINTER(Params), C.c_int32, C.POINTER(C.c_uint32)]
    L.pikamd_self_test.restype = C.c_int32
    L.pikamd_self_test_cost.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.pikamd_self_test_cost.restype = C.c_int32
    L.pikamd_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.pikamd_set_option.restype = C.c_int32
    L.pikamd_solve_batch_host.argtypes = [vp, C.POINTER(Params), C.c_int64, dp, dp, dp, C.c_uint64, C.c_int64, COST_FN,
                                          vp, dp, ip, dp, vp]
    L.pikamd_solve_batch_host.restype = C.c_int32
    L.pikamd_set_mimic_joints.argtypes = [vp, C.c_int32, C.POINTER(MimicJointC)]
    L.pikamd_set_mimic_joints.restype = C.c_int32
    L.pikamd_last_error.restype = C.c_char_p
    L.pikamd_version.restype = C.c_char_p
    L.pikamd_kernel_name.restype = C.c_char_p
    L.pikamd_kernel_name.argtypes = [vp, C.POINTER(Params)]
    L.pikamd_solve_paths.argtypes = [vp, C.POINTER(Params), C.c_int64, C.c_int32, dp, dp, dp, dp, ip, dp, vp, ip]
    L.pikamd_solve_paths.restype = C.c_int32
    L.pikamd_solve_paths_device.argtypes = [vp, C.POINTER(Params), C.c_int64, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp,
                                            vp, C.c_int32]
    L.pikamd_solve_paths_device.restype = C.c_int32
    L.pikamd_path_kernel_name.argtypes = [vp, C.POINTER(Params), C.c_int64]
    L.pikamd_path_kernel_name.restype = C.c_char_p
    L.pikamd_search_batch.argtypes = [vp, C.POINTER(Params), C.c_int64, dp, dp, dp, C.c_uint64, C.c_int64, C.c_int32,
                                      dp, ip, dp, vp, ip, dp, ip]
    L.pikamd_search_batch.restype = C.c_int32
    L.pikamd_search_batch_device.argtypes = [vp, C.POINTER(Params), C.c_int64, vp, vp, vp, C.c_uint64, C.c_int64,
                                             C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int32]
    L.pikamd_search_batch_device.restype = C.c_int32
    L.pikamd_search_global_batch.argtypes = L.pikamd_search_batch.argtypes
    L.pikamd_search_global_batch.restype = C.c_int32
    L.pikamd_search_global_batch_device.argtypes = L.pikamd_search_batch_device.argtypes
    L.pikamd_search_global_batch_device.restype = C.c_int32
    L.pikamd_search_kernel_name.argtypes = [vp, C.POINTER(Params), C.c_int64, C.c_int32, ip]
    L.pikamd_search_kernel_name.restype = C.c_char_p
    L.pikamd_gate_batch.argtypes = [vp, C.POINTER(Params), C.POINTER(Gate), C.c_int64, dp, dp, dp, ip]
    L.pikamd_gate_batch.restype = C.c_int32
    L.pikamd_set_approximate_gate.argtypes = [vp, C.POINTER(Gate)]
    L.pikamd_set_approximate_gate.restype = C.c_int32
    L.pikamd_set_validity_model.argtypes = [vp, C.POINTER(ValidityModel)]
    L.pikamd_set_validity_model.restype = C.c_int32
    L.pikamd_set_path_validity.argtypes = [vp, C.c_int32]
    L.pikamd_set_path_validity.restype = C.c_int32
    L.pikamd_validity_batch.argtypes = [vp, C.c_int64, dp, ip, dp, dp]
    L.pikamd_validity_batch.restype = C.c_int32
    L.pikamd_validity_batch_device.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp]
    L.pikamd_validity_batch_device.restype = C.c_int32
    L.pikamd_search_paths.argtypes = [vp, C.POINTER(Params), C.c_int64, C.c_int32, dp, dp, dp, dp, C.c_uint64, C.c_int64,
                                      C.c_int32, dp, ip, dp, vp, ip, ip, vp]
    L.pikamd_search_paths.restype = C.c_int32
    L.pikamd_search_paths_device.argtypes = [vp, C.POINTER(Params), C.c_int64, C.c_int32, vp, vp, vp, vp, C.c_uint64,
                                             C.c_int64, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int32]
    L.pikamd_search_paths_device.restype = C.c_int32
    L.pikamd_search_paths_kernel_name.argtypes = [vp, C.POINTER(Params), C.c_int64]
    L.pikamd_search_paths_kernel_name.restype = C.c_char_p
    L.pikamd_search_global_paths.argtypes = L.pikamd_search_paths.argtypes
    L.pikamd_search_global_paths.restype = C.c_int32
    L.pikamd_search_global_paths_device.argtypes = L.pikamd_search_paths_device.argtypes
    L.pikamd_search_global_paths_device.restype = C.c_int32
    L.pikamd_search_global_paths_kernel_name.argtypes = [vp, C.POINTER(Params), C.c_int64]
    L.pikamd_search_global_paths_kernel_name.restype = C.c_char_p
    L.pikamd_interpolate_poses.argtypes = [C.POINTER(Cartesian), C.c_int64, C.c_int32, dp, dp, dp, ip]
    L.pikamd_interpolate_poses.restype = C.c_int32
    L.pikamd_cartesian_paths.argtypes = [vp, C.POINTER(Params), C.POINTER(Cartesian), C.c_int64, C.c_int32, dp, dp, dp, dp,
                                         ip, dp, vp, ip, ip, dp, dp]
    L.pikamd_cartesian_paths.restype = C.c_int32
    L.pikamd_cartesian_paths_device.argtypes = [vp, C.POINTER(Params), C.POINTER(Cartesian), C.c_int64, C.c_int32, vp, vp,
                                                vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int32]
    L.pikamd_cartesian_paths_device.restype = C.c_int32
    L.pikamd_cartesian_kernel_name.argtypes = [vp, C.POINTER(Params), C.c_int64]
    L.pikamd_cartesian_kernel_name.restype = C.c_char_p
    L.pikamd_cartesian_waypoints.argtypes = [vp, C.POINTER(Params), C.POINTER(Cartesian), C.c_int64, C.c_int32, C.c_int32,
                                             dp, dp, ip, dp, dp, ip, dp, vp, ip, ip, ip, dp, dp]
    L.pikamd_cartesian_waypoints.restype = C.c_int32
    L.pikamd_cartesian_waypoints_device.argtypes = [vp, C.POINTER(Params), C.POINTER(Cartesian), C.c_int64, C.c_int32,
                                                    C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                    C.c_int32]
    L.pikamd_cartesian_waypoints_device.restype = C.c_int32
    L.pikamd_cartesian_waypoints_kernel_name.argtypes = [vp, C.POINTER(Params), C.c_int64]
    L.pikamd_cartesian_waypoints_kernel_name.restype = C.c_char_p
    up = C.POINTER(C.c_uint32)
    L.pikamd_debug_regime.argtypes = [vp, C.c_int32, C.c_int64, C.c_int32, ip, up, up, ip]
    L.pikamd_debug_regime.restype = C.c_int32
    for name in ("pikamd_create", "pikamd_variables", "pikamd_fk_batch", "pikamd_cost_batch",
                 "pikamd_gd_step_batch", "pikamd_solve_batch", "pikamd_solve_batch_device",
                 "pikamd_fk_batch_device", "pikamd_solve_batches_device",
                 "pikamd_solve_batches_async", "pikamd_wait", "pikamd_solve_batches"):
        getattr(L, name).restype = C.c_int32
    _libs[strict] = L
    return L


def _check(rc: int, L=None):
    if rc != 0:
        L = L or lib()
        raise PickIkAmdError(f"pick_ik_amd error {rc}: {L.pikamd_last_error().decode()}")


def default_params(**kw) -> Params:
    p = Params()
    lib().pikamd_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _urdf_text(urdf: str) -> bytes:
    text = urdf if urdf.lstrip().startswith("<") else open(urdf).read()
    return text.encode()


def urdf_extract(urdf: str, base_link: str, tip_links, strict: bool = False):
    """pikamd_urdf_extract (no GPU needed): the chain the NATIVE reader finds, as a robots.Chain (one
    tip) or robots.MultiChain, plus the variable names (= the order of the joint vector).
    `urdf` is the XML text or a path; tip_links a name or a sequence of names."""
    from .robots import Chain, multi_chain
    L = lib(strict)
    tips = [tip_links] if isinstance(tip_links, str) else list(tip_links)
    arr = (C.c_char_p * len(tips))(*[t.encode() for t in tips])
    m = UrdfModel()
    _check(L.pikamd_urdf_extract(_urdf_text(urdf), base_link.encode(), arr, len(tips), C.byref(m)), L)
    d = m.dof
    names = [m.variable_names[i].value.decode() for i in range(d)]
    lim = [np.array(m.qmin[:d]), np.array(m.qmax[:d]), np.array(m.vmax[:d]), np.array(m.bounded[:d], dtype=np.uint8)]

    def tip_arrays(t):
        n = t.n_joints
        return (list(t.variable[:n]), np.array([list(r) for r in t.origin_xyz_rpy[:n]]).reshape(n, 6),
                np.array([list(r) for r in t.axis[:n]]).reshape(n, 3), np.array(t.joint_type[:n], dtype=np.int32),
                np.array(t.tip_xyz_rpy[:]))

    from .robots import MimicJoint
    import dataclasses
    mim = tuple(MimicJoint(after_variable=x.after_variable, master_variable=x.master_variable,
                           origin_xyz_rpy=tuple(x.origin_xyz_rpy), axis=tuple(x.axis), multiplier=x.multiplier,
                           offset=x.offset, joint_type=x.joint_type, tip=x.tip) for x in m.mimic[:m.n_mimic])
    if m.n_tips == 1:
        _, o, a, jt, tip = tip_arrays(m.tips[0])
        return Chain(name="urdf", origin_xyz_rpy=o, axis=a, joint_type=jt, tip_xyz_rpy=tip, qmin=lim[0],
                     qmax=lim[1], vmax=lim[2], bounded=lim[3], mimic=mim), names
    paths = [tip_arrays(m.tips[k]) for k in range(m.n_tips)]
    mc = multi_chain("urdf", paths, *lim)
    return (dataclasses.replace(mc, mimic=mim) if mim else mc), names


class Solver:
    """One solver handle = one serial chain (robots.Chain) or one multi-tip chain
    (robots.MultiChain: goals and FK results hold n_tips poses per problem) on one GPU
    (PickIKPlugin::initialize's role, reference src/pick_ik_plugin.cpp:22-71)."""

    def __init__(self, chain, device: int = 0, strict: bool = False, exact=None):
        """strict: the verification library (plain IEEE arithmetic, oracle math mode "portable");
        exact: None / True = the product library's DEFAULT, option arithmetic = exact (its exact kernels
        with fused multiply-adds at stated places, oracle math mode "fma": joint vectors identical to the
        reference algorithm's); False = arithmetic = fast (the Denavit-Hartenberg kernels, opt-in)."""
        self._L = lib(strict)
        self.strict = strict
        self.exact = (exact is None or bool(exact)) and not strict
        self.chain = chain
        self.dof = int(chain.dof)
        self.device = int(device)
        self.n_tips = int(getattr(chain, "n_tips", 1))
        h = C.c_void_p()
        lim = [_f64(chain.qmin), _f64(chain.qmax), _f64(chain.vmax),
               np.ascontiguousarray(chain.bounded, dtype=np.uint8)]
        if hasattr(chain, "tips"):  # robots.MultiChain: several tip frames
            keep, tips = [lim], (_Tip * self.n_tips)()
            for i, t in enumerate(chain.tips):
                a = [np.ascontiguousarray(t.variable, dtype=np.int32), _f64(t.origin_xyz_rpy),
                     _f64(t.axis), np.ascontiguousarray(t.joint_type, dtype=np.int32),
                     _f64(t.tip_xyz_rpy)]
                keep.append(a)
                tips[i] = _Tip(len(a[0]), _ip(a[0]), _dp(a[1]), _dp(a[2]), _ip(a[3]), _dp(a[4]))
            self._keep = (keep, tips)
            c = _MultiChain(self.dof, self.n_tips, tips, _dp(lim[0]), _dp(lim[1]), _dp(lim[2]),
                            lim[3].ctypes.data_as(C.POINTER(C.c_uint8)))
            self._chk(self._L.pikamd_create_multi(C.byref(c), self.device, C.byref(h)))
        else:
            k = [_f64(chain.origin_xyz_rpy), _f64(chain.axis),
                 np.ascontiguousarray(chain.joint_type, dtype=np.int32), _f64(chain.tip_xyz_rpy)]
            self._keep = (k, lim)
            c = _Chain(self.dof, _dp(k[0]), _dp(k[1]), _ip(k[2]), _dp(k[3]), _dp(lim[0]),
                       _dp(lim[1]), _dp(lim[2]), lim[3].ctypes.data_as(C.POINTER(C.c_uint8)))
            self._chk(self._L.pikamd_create(C.byref(c), self.device, C.byref(h)))
        self._h = h
        arr = mimic_array(chain)
        if arr is not None:
            self._chk(self._L.pikamd_set_mimic_joints(self._h, len(arr), arr))
        if not self.strict and exact is not None:  # (None: whatever the library defaults to -- exact)
            self.set_option("arithmetic", "exact" if exact else "fast")
        self._env_options()

    @classmethod
    def from_urdf(cls, urdf: str, base_link: str, tip_links, device: int = 0, strict: bool = False):
        """pikamd_create_from_urdf: the library reads the robot description itself (native reader).
        The handle's `chain` / `variable_names` are what pikamd_urdf_extract reports."""
        chain, names = urdf_extract(urdf, base_link, tip_links, strict)
        self = cls.__new__(cls)
        self._L = lib(strict)
        self.strict, self.chain, self.variable_names = strict, chain, names
        self.exact = not strict  # (the library's default arithmetic)
        self.dof, self.device, self.n_tips = int(chain.dof), int(device), int(getattr(chain, "n_tips", 1))
        tips = [tip_links] if isinstance(tip_links, str) else list(tip_links)
        arr = (C.c_char_p * len(tips))(*[t.encode() for t in tips])
        h = C.c_void_p()
        self._keep = None
        _check(self._L.pikamd_create_from_urdf(_urdf_text(urdf), base_link.encode(), arr, len(tips), self.device,
                                               C.byref(h)), self._L)
        self._h = h
        return self

    def _chk(self, rc: int):
        _check(rc, self._L)

    # ---- scheduling options (pikamd_set_option) -------------------------------------------
    def set_option(self, name: str, value) -> None:
        """Pin one scheduling choice of this handle ("lanes_per_elite", "lanes_per_elite_schedule",
        "passes", "two_per_simd", "regime", "device_regime", "regime_threshold", "search_schedule"; None / "" restores
        the default).  Results never depend on
        these."""
        v = b"" if value is None else str(value).encode()
        self._chk(self._L.pikamd_set_option(self._h, name.encode(), v))

    #: lanes per elite of the kernel variant ids pikamd_debug_regime reports (7: one lane, two wavefronts per SIMD)
    VARIANT_LANES = {5: 16, 4: 8, 3: 4, 2: 2, 1: 1, 7: 1}
    MAX_PASSES = 16

    def debug_regime(self, slot: int = 0, publish_load: int = -1):
        """pikamd_debug_regime (synchronises the device): what the routers of the LAST solve call on `slot` decided --
        None when that call was not routed (host rule), else a list with one (survivors, others_load, variant id)
        per pass.  publish_load >= 0 first sets the load `slot` shows the other slots' routers (an artificial load
        on a slot with no call in flight)."""
        n = C.c_int32(0)
        sv = np.zeros(self.MAX_PASSES, dtype=np.uint32)
        ol = np.zeros(self.MAX_PASSES, dtype=np.uint32)
        var = np.zeros(self.MAX_PASSES, dtype=np.int32)
        up = C.POINTER(C.c_uint32)
        self._chk(self._L.pikamd_debug_regime(self._h, slot, int(publish_load), self.MAX_PASSES, C.byref(n),
                                              sv.ctypes.data_as(up), ol.ctypes.data_as(up), _ip(var)))
        if n.value < 0:
            return None
        return [(int(sv[k]), int(ol[k]), int(var[k])) for k in range(n.value)]

    def self_test(self, params: Params, n: int = 64) -> int:
        """pikamd_self_test: every kernel variant against the one-lane kernel on n generated targets of this
        chain; returns the mask of variants that disagreed (and are now switched off for this handle)"""
        m = C.c_uint32(0)
        self._chk(self._L.pikamd_self_test(self._h, C.byref(params), n, C.byref(m)))
        return int(m.value)

    def self_test_cost(self):
        """pikamd_self_test_cost: (automatic self tests run on this handle, their wall-clock time in ms)"""
        runs, ms = C.c_int32(0), C.c_double(0.0)
        self._chk(self._L.pikamd_self_test_cost(self._h, C.byref(runs), C.byref(ms)))
        return int(runs.value), float(ms.value)

    #: Test / experiment hook of THIS binding (the library itself never reads the environment): these
    #: variables are turned into handle options before a solve whenever they have changed.
    ENV_OPTIONS = (("PIK_LPE", "lanes_per_elite"), ("PIK_LPE_SCHED", "lanes_per_elite_schedule"),
                   ("PIK_PASSES", "passes"), ("PIK_OCC2", "two_per_simd"), ("PIK_REGIME", "regime"),
                   ("PIK_SPECIALISED", "specialised"), ("PIK_SHARD_CHUNKS", "shard_chunks"),
                   ("PIK_SELF_TEST", "self_test"), ("PIK_DEVICE_REGIME", "device_regime"),
                   ("PIK_REGIME_THRESHOLD", "regime_threshold"))
    # (no environment form of "joint_layout": it changes what the arrays mean, callers set it explicitly)

    def _env_options(self) -> None:
        cur = tuple(os.environ.get(k) for k, _ in self.ENV_OPTIONS)
        seen = getattr(self, "_env_seen", (None,) * len(cur))
        if cur == seen:
            return
        for (_, name), new, old in zip(self.ENV_OPTIONS, cur, seen):
            if new != old:
                self.set_option(name, new)
        self._env_seen = cur

    def close(self):
        if getattr(self, "_h", None):
            self._L.pikamd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- parity hooks -------------------------------------------------------------------
    def variables(self) -> np.ndarray:
        out = np.empty((self.dof, 7))
        self._chk(self._L.pikamd_variables(self._h, _dp(out)))
        return out

    def fk(self, q) -> np.ndarray:
        """make_fk_fn: tip pose [n][7] = x y z qw qx qy qz for joint vectors q [n][dof]."""
        q = _f64(q).reshape(-1, self.dof)
        out = np.empty((q.shape[0], 7) if self.n_tips == 1 else (q.shape[0], self.n_tips, 7))
        self._chk(self._L.pikamd_fk_batch(self._h, q.shape[0], _dp(q), _dp(out)))
        return out

    def cost(self, params: Params, goal_pos_quat, seed, q):
        """cost_fn and solution_fn of n (goal, seed, q) triples (broadcast goal/seed if 1-D)."""
        q = _f64(q).reshape(-1, self.dof)
        n = q.shape[0]
        g7 = 7 * self.n_tips
        goal = np.ascontiguousarray(np.broadcast_to(_f64(goal_pos_quat).reshape(-1, g7), (n, g7)))
        seed = np.ascontiguousarray(np.broadcast_to(_f64(seed).reshape(-1, self.dof),
                                                    (n, self.dof)))
        cost = np.empty(n)
        sol = np.empty(n, dtype=np.int32)
        self._chk(self._L.pikamd_cost_batch(self._h, C.byref(params), n, _dp(goal), _dp(seed), _dp(q),
                                       _dp(cost), _ip(sol)))
        return cost, sol

    def gate(self, params: Params, gate: Gate, goal_pos_quat, seed, q) -> np.ndarray:
        """pikamd_gate_batch: pass [n] (bool) of n (goal, seed, q) triples (goal / seed broadcast if 1-D) -- the
        reference's approx_solution_valid: the solution test under the gate's cost threshold, then the joint limit."""
        q = _f64(q).reshape(-1, self.dof)
        n = q.shape[0]
        g7 = 7 * self.n_tips
        goal = np.ascontiguousarray(np.broadcast_to(_f64(goal_pos_quat).reshape(-1, g7), (n, g7)))
        seed = np.ascontiguousarray(np.broadcast_to(_f64(seed).reshape(-1, self.dof), (n, self.dof)))
        ok = np.zeros(n, dtype=np.int32)
        self._chk(self._L.pikamd_gate_batch(self._h, C.byref(params), C.byref(gate), n, _dp(goal), _dp(seed), _dp(q),
                                            _ip(ok)))
        return ok != 0

    def set_approximate_gate(self, cost_threshold: float = 0.0, joint_threshold: float = 0.0) -> None:
        """The gate search_batch / search_global_batch apply behind every attempt of a call with
        return_approximate_solution: a refused answer is GATE_REFUSED and the search restarts."""
        self._chk(self._L.pikamd_set_approximate_gate(self._h, C.byref(Gate(cost_threshold, joint_threshold))))

    def clear_approximate_gate(self) -> None:
        """no gate (the default): every result is what it was"""
        self._chk(self._L.pikamd_set_approximate_gate(self._h, None))

    def set_validity_model(self, spheres, pairs) -> None:
        """pikamd_set_validity_model: spheres = Sphere objects (or (after_variable, centre, radius) tuples), pairs =
        [n_pairs][2] sphere indices that must not overlap.  The model is the validity step of search_global_batch
        (a refused answer is VALIDITY_REFUSED and the search restarts) and what validity() tests."""
        sph = [s if isinstance(s, Sphere) else Sphere(*s) for s in spheres]
        arr = (Sphere * max(1, len(sph)))(*sph)
        pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        m = ValidityModel(len(sph), arr, pr.shape[0], pr.ctypes.data_as(C.POINTER(C.c_int32)))
        self._chk(self._L.pikamd_set_validity_model(self._h, C.byref(m)))
        self._n_spheres = len(sph)

    def clear_validity_model(self) -> None:
        """no model (the default): every result is what it was"""
        self._chk(self._L.pikamd_set_validity_model(self._h, None))
        self._n_spheres = None

    def set_path_validity(self, on: bool) -> None:
        """pikamd_set_path_validity: on -- solve_paths, cartesian_paths and cartesian_waypoints (and their _device
        forms) end a path at the first waypoint whose answer the handle's validity model refuses (VALIDITY_REFUSED);
        off (the default) -- they ignore the model.  Without a model the switch changes nothing."""
        self._chk(self._L.pikamd_set_path_validity(self._h, 1 if on else 0))

    def validity(self, q, centres: bool = False):
        """pikamd_validity_batch: (valid [n] bool, clearance [n]) of joint vectors q [n][dof]; centres=True: also the
        sphere centres [n][n_spheres][3] in the base frame, in the model's order."""
        q = _f64(q).reshape(-1, self.dof)
        n = q.shape[0]
        ns = getattr(self, "_n_spheres", None) or 0
        valid = np.zeros(n, dtype=np.int32)
        clearance = np.empty(n)
        cen = np.empty((n, ns, 3)) if centres else None
        self._chk(self._L.pikamd_validity_batch(self._h, n, _dp(q), _ip(valid), _dp(clearance),
                                                _dp(cen) if centres else None))
        return (valid != 0, clearance, cen) if centres else (valid != 0, clearance)

    def validity_device(self, n: int, d_q: int, d_valid: int, d_clearance: int = 0, d_centres: int = 0, stream: int = 0):
        """pikamd_validity_batch_device: device pointers, enqueued on `stream`"""
        self._chk(self._L.pikamd_validity_batch_device(self._h, n, d_q, d_valid, d_clearance or None, d_centres or None,
                                                       stream or None))

    def gd_step(self, params: Params, goal_pos_quat, seed, local, best, local_cost, best_cost):
        """One step() of src/ik_gradient.cpp:24-94 on n GradientIk states."""
        local = _f64(local).reshape(-1, self.dof).copy()
        n = local.shape[0]
        best = _f64(best).reshape(n, self.dof).copy()
        goal = _f64(goal_pos_quat).reshape(n, 7 * self.n_tips)
        seed = _f64(seed).reshape(n, self.dof)
        lc = _f64(local_cost).reshape(n).copy()
        bc = _f64(best_cost).reshape(n).copy()
        grad = np.empty((n, self.dof))
        imp = np.empty(n, dtype=np.int32)
        self._chk(self._L.pikamd_gd_step_batch(self._h, C.byref(params), n, _dp(goal), _dp(seed),
                                          _dp(local), _dp(best), _dp(lc), _dp(bc), _dp(grad),
                                          _ip(imp)))
        return local, best, lc, bc, grad, imp

    # ---- solvers ------------------------------------------------------------------------
    def _host_batch(self, goal_pos_quat, seed, initial_guess=None, problem_offset=0):
        """(pikamd_batch with host pointers, arrays to keep alive, outputs)"""
        goal = _f64(goal_pos_quat).reshape(-1, 7 * self.n_tips)
        B = goal.shape[0]
        seed = _f64(seed).reshape(B, self.dof)
        guess = None if initial_guess is None else _f64(initial_guess).reshape(B, self.dof)
        sol = np.empty((B, self.dof))
        status = np.empty(B, dtype=np.int32)
        cost = np.empty(B)
        stats = np.zeros(B, dtype=STATS_DTYPE)
        b = Batch(B, goal.ctypes.data, seed.ctypes.data, None if guess is None else guess.ctypes.data,
                  problem_offset, sol.ctypes.data, status.ctypes.data, cost.ctypes.data,
                  stats.ctypes.data, None)
        return b, (goal, seed, guess), (sol, status, cost, stats)

    def solve_batch(self, params: Params, goal_pos_quat, seed, rng_seed: int = 0,
                    problem_offset: int = 0, initial_guess=None):
        """ik_memetic / ik_gradient (params.mode) for B problems given as host arrays.
        seed = ik_seed_state (minimal-displacement reference, returned on failure); initial_guess =
        where the search starts (None = seed), src/pick_ik_plugin.cpp:199-245."""
        self._env_options()
        if initial_guess is None:
            goal = _f64(goal_pos_quat).reshape(-1, 7 * self.n_tips)
            B = goal.shape[0]
            seed = _f64(seed).reshape(B, self.dof)
            sol = np.empty((B, self.dof))
            status = np.empty(B, dtype=np.int32)
            cost = np.empty(B)
            stats = np.zeros(B, dtype=STATS_DTYPE)
            self._chk(self._L.pikamd_solve_batch(self._h, C.byref(params), B, _dp(goal), _dp(seed),
                                                 C.c_uint64(rng_seed), problem_offset, _dp(sol),
                                                 _ip(status), _dp(cost),
                                                 stats.ctypes.data_as(C.c_void_p)))
            return sol, status, cost, stats
        return self.solve_batches(params, [(goal_pos_quat, seed, initial_guess, problem_offset)],
                                  rng_seed=rng_seed)[0]

    def solve_batch_host(self, params: Params, goal_pos_quat, seed, cost_fn, rng_seed: int = 0, problem_offset: int = 0,
                         initial_guess=None):
        """pikamd_solve_batch_host: queries with a host cost function (kinematics::KinematicsBase::IKCostFn) -- one
        more goal of weight 1 per tip pose INSIDE the search (src/pick_ik_plugin.cpp:130-135) --, solved on the host
        with the exact kernels' arithmetic.  cost_fn(q: ndarray[dof], pose_index) -> float."""
        goal = _f64(goal_pos_quat).reshape(-1, 7 * self.n_tips)
        B = goal.shape[0]
        seed = _f64(seed).reshape(B, self.dof)
        guess = None if initial_guess is None else _f64(initial_guess).reshape(B, self.dof)
        sol = np.empty((B, self.dof))
        status = np.empty(B, dtype=np.int32)
        cost = np.empty(B)
        stats = np.zeros(B, dtype=STATS_DTYPE)
        cb = cost_fn if isinstance(cost_fn, COST_FN) else cost_callback(cost_fn)
        self._chk(self._L.pikamd_solve_batch_host(self._h, C.byref(params), B, _dp(goal), _dp(seed),
                                                  None if guess is None else _dp(guess), C.c_uint64(rng_seed),
                                                  problem_offset, cb, None, _dp(sol), _ip(status), _dp(cost),
                                                  stats.ctypes.data_as(C.c_void_p)))
        return sol, status, cost, stats

    def solve_batches(self, params: Params, batches, rng_seed: int = 0, job: int | None = None):
        """Several batches as one pool (pikamd_solve_batches).  batches: sequence of
        (goal_pos_quat, seed, initial_guess or None, problem_offset); returns a list of
        (solution, status, cost, stats).  With `job` the call is asynchronous
        (pikamd_solve_batches_async): the results are valid after wait(job)."""
        self._env_options()
        made = [self._host_batch(g, sd, ig, off) for g, sd, ig, off in batches]
        arr = (Batch * len(made))(*[m[0] for m in made])
        if job is None:
            self._chk(self._L.pikamd_solve_batches(self._h, C.byref(params), len(made), arr,
                                                   C.c_uint64(rng_seed)))
        else:
            self._chk(self._L.pikamd_solve_batches_async(self._h, C.byref(params), len(made), arr,
                                                         C.c_uint64(rng_seed), job))
            self._jobs = getattr(self, "_jobs", {})
            self._jobs[job] = made  # outputs must stay alive until wait()
        return [m[2] for m in made]

    def wait(self, job: int):
        self._chk(self._L.pikamd_wait(self._h, job))
        getattr(self, "_jobs", {}).pop(job, None)

    def solve_batch_device(self, params: Params, B: int, d_goal: int, d_seed: int, d_solution: int,
                           d_status: int, d_cost: int = 0, d_stats: int = 0, rng_seed: int = 0,
                           problem_offset: int = 0, stream: int = 0, slot: int = 0):
        """Enqueue a solve on HBM-resident buffers (raw device addresses, e.g. tensor.data_ptr());
        returns immediately -- the caller synchronises the stream."""
        self._env_options()
        self._chk(self._L.pikamd_solve_batch_device(
            self._h, C.byref(params), B, d_goal, d_seed, C.c_uint64(rng_seed), problem_offset,
            d_solution, d_status, d_cost or None, d_stats or None, stream or None, slot))

    def solve_batches_device(self, params: Params, batches, rng_seed: int = 0, stream: int = 0,
                             slot: int = 0):
        """Enqueue several HBM-resident batches as ONE pool (pikamd_solve_batches_device).
        batches: sequence of dicts / Batch with raw device addresses."""
        self._env_options()
        arr = (Batch * len(batches))(*[b if isinstance(b, Batch) else Batch(**b) for b in batches])
        self._chk(self._L.pikamd_solve_batches_device(self._h, C.byref(params), len(batches), arr,
                                                      C.c_uint64(rng_seed), stream or None, slot))

    def reserve(self, params: Params, B: int, slot: int = 0, stream: int = 0):
        """Allocate a slot's scratch + upload constants ahead of the first solve on it."""
        self._env_options()
        self._chk(self._L.pikamd_reserve(self._h, C.byref(params), B, slot, stream or None))

    def fk_device(self, n: int, d_q: int, d_pos_quat: int, stream: int = 0):
        self._chk(self._L.pikamd_fk_batch_device(self._h, n, d_q, d_pos_quat, stream or None))

    def kernel_name(self, params: Params) -> str:
        return self._L.pikamd_kernel_name(self._h, C.byref(params)).decode()

    # ---- Cartesian waypoint paths ---------------------------------------------------------
    def solve_paths(self, params: Params, goals, start, max_joint_step=None):
        """pikamd_solve_paths: P paths of W waypoints in local mode (params.mode = 1), every waypoint solved from the
        previous waypoint's answer, a path stopping at its first failure -- one launch.  goals [P][W][7]
        ([P][W][n_tips][7] for several tips), start [P][dof], max_joint_step [dof] or None (an entry <= 0: no limit for
        that variable).  Returns (solution [P][W][dof], status [P][W], cost [P][W], stats [P][W], reached [P]); the
        result is what the loop of solve_batch calls in include/pick_ik_amd.h returns, bit for bit."""
        self._env_options()
        goals = _f64(goals)
        tail = (7,) if self.n_tips == 1 else (self.n_tips, 7)
        if goals.ndim != 2 + len(tail) or goals.shape[2:] != tail:
            raise ValueError(f"goals: expected [P][W]{list(tail)}, got {list(goals.shape)}")
        P, W = goals.shape[:2]
        if W < 1:
            raise ValueError("goals: a path has at least one waypoint")
        start = _f64(start)
        if start.shape != (P, self.dof):
            raise ValueError(f"start: expected [{P}][{self.dof}], got {list(start.shape)}")
        step = None
        if max_joint_step is not None:
            step = _f64(max_joint_step)
            if step.shape != (self.dof,):
                raise ValueError(f"max_joint_step: expected [{self.dof}], got {list(step.shape)}")
        sol = np.empty((P, W, self.dof))
        status = np.empty((P, W), dtype=np.int32)
        cost = np.empty((P, W))
        stats = np.zeros((P, W), dtype=STATS_DTYPE)
        reached = np.empty(P, dtype=np.int32)
        self._chk(self._L.pikamd_solve_paths(self._h, C.byref(params), P, W, _dp(goals), _dp(start),
                                             None if step is None else _dp(step), _dp(sol), _ip(status), _dp(cost),
                                             stats.ctypes.data_as(C.c_void_p), _ip(reached)))
        return sol, status, cost, stats, reached

    def solve_paths_device(self, params: Params, P: int, W: int, d_goals: int, d_start: int, d_solution: int,
                           d_status: int, d_max_joint_step: int = 0, d_cost: int = 0, d_stats: int = 0,
                           d_reached: int = 0, stream: int = 0, slot: int = 0):
        """Enqueue a path solve on HBM-resident buffers (raw device addresses); returns immediately -- the caller
        synchronises the stream."""
        self._env_options()
        if P < 0 or W < 1:
            raise ValueError(f"{P} paths of {W} waypoints: expected P >= 0 and W >= 1")
        self._chk(self._L.pikamd_solve_paths_device(
            self._h, C.byref(params), P, W, d_goals or None, d_start or None, d_max_joint_step or None,
            d_solution or None, d_status or None, d_cost or None, d_stats or None, d_reached or None, stream or None,
            slot))

    def path_kernel_name(self, params: Params, P: int) -> str:
        """the kernel solve_paths launches for P paths (pikamd_path_kernel_name)"""
        self._env_options()
        return self._L.pikamd_path_kernel_name(self._h, C.byref(params), P).decode()

    # ---- computeCartesianPath in one call ---------------------------------------------------
    def cartesian_paths(self, params: Params, cartesian: Cartesian, start, target, W: int, max_joint_step=None,
                        optional: bool = True):
        """pikamd_cartesian_paths: P Cartesian motions in local mode (params.mode = 1), each from the start joint state
        start[p] to target[p] (a pose or an offset, cartesian.frame).  The poses are generated on the device, every
        path is walked for its own number of steps (steps[p]; a path with steps[p] > W is not walked: call again with
        a larger W), the absolute (max_joint_step) and the relative (cartesian.jump_factor) jump tests are applied and
        MoveIt's fraction comes out.  start [P][dof], target [P][7], max_joint_step [dof] or None.  Returns (solution
        [P][W][dof], status [P][W], cost [P][W], stats [P][W], reached [P], steps [P], fraction [P], goals [P][W][7]);
        optional=False leaves out every array the library can do without (cost, stats, reached, fraction and goals are
        None then).  The result is what fk + interpolate_poses + the loop of solve_paths calls in
        include/pick_ik_amd.h returns, bit for bit."""
        self._env_options()
        start = _f64(start)
        if start.ndim != 2 or start.shape[1] != self.dof:
            raise ValueError(f"start: expected [P][{self.dof}], got {list(start.shape)}")
        P = start.shape[0]
        target = _f64(target)
        if target.shape != (P, 7):
            raise ValueError(f"target: expected [{P}][7], got {list(target.shape)}")
        W = int(W)
        if W < 1:
            raise ValueError("W: a path has at least one waypoint")
        step = None
        if max_joint_step is not None:
            step = _f64(max_joint_step)
            if step.shape != (self.dof,):
                raise ValueError(f"max_joint_step: expected [{self.dof}], got {list(step.shape)}")
        sol = np.empty((P, W, self.dof))
        status = np.empty((P, W), dtype=np.int32)
        steps = np.empty(P, dtype=np.int32)
        cost = np.empty((P, W)) if optional else None
        stats = np.zeros((P, W), dtype=STATS_DTYPE) if optional else None
        reached = np.empty(P, dtype=np.int32) if optional else None
        fraction = np.empty(P) if optional else None
        goals = np.empty((P, W, 7)) if optional else None
        self._chk(self._L.pikamd_cartesian_paths(
            self._h, C.byref(params), C.byref(cartesian), P, W, _dp(start), _dp(target),
            None if step is None else _dp(step), _dp(sol), _ip(status), _dp(cost) if optional else None,
            stats.ctypes.data_as(C.c_void_p) if optional else None, _ip(reached) if optional else None, _ip(steps),
            _dp(fraction) if optional else None, _dp(goals) if optional else None))
        return sol, status, cost, stats, reached, steps, fraction, goals

    def cartesian_paths_device(self, params: Params, cartesian: Cartesian, P: int, W: int, d_start: int, d_target: int,
                               d_solution: int, d_status: int, d_steps: int, d_max_joint_step: int = 0, d_cost: int = 0,
                               d_stats: int = 0, d_reached: int = 0, d_fraction: int = 0, d_goals: int = 0,
                               stream: int = 0, slot: int = 0):
        """Enqueue cartesian_paths on HBM-resident buffers (raw device addresses); returns immediately -- the caller
        synchronises the stream.  Without d_goals the poses are kept in scratch of the handle's slot."""
        self._env_options()
        if P < 0 or W < 1:
            raise ValueError(f"{P} paths of {W} waypoints: expected P >= 0 and W >= 1")
        self._chk(self._L.pikamd_cartesian_paths_device(
            self._h, C.byref(params), C.byref(cartesian), P, W, d_start or None, d_target or None,
            d_max_joint_step or None, d_solution or None, d_status or None, d_cost or None, d_stats or None,
            d_reached or None, d_steps or None, d_fraction or None, d_goals or None, stream or None, slot))

    def cartesian_kernel_name(self, params: Params, P: int) -> str:
        """the kernel that walks P paths of cartesian_paths (pikamd_cartesian_kernel_name)"""
        self._env_options()
        return self._L.pikamd_cartesian_kernel_name(self._h, C.byref(params), P).decode()

    # ---- computeCartesianPath through waypoints ---------------------------------------------
    def cartesian_waypoints(self, params: Params, cartesian: Cartesian, start, targets, W: int, n_targets=None,
                            max_joint_step=None, optional: bool = True):
        """pikamd_cartesian_waypoints: P Cartesian motions in local mode (params.mode = 1), each from the start joint
        state start[p] through the targets targets[p][0..n_targets[p]-1] (poses or offsets, cartesian.frame; in the tip
        and offset frames relative to the tip pose of the state the previous segment ended in).  Segment after segment
        is interpolated and walked on the device with no host round trip; the relative jump test is applied once, to
        the stitched rows.  start [P][dof], targets [P][S][7], n_targets [P] or None (S for every path),
        max_joint_step [dof] or None, W >= S rows per path.  Returns (solution [P][W][dof], status [P][W], cost [P][W],
        stats [P][W], reached [P], steps [P], fraction [P], goals [P][W][7], segment_steps [P][S]); steps[p] > W: a
        segment did not fit, call again with W >= steps[p].  optional=False leaves out every array the library can do
        without (cost, stats, reached, fraction, goals and segment_steps are None then).  The result is what the loop
        of cartesian_paths calls in include/pick_ik_amd.h returns, bit for bit."""
        self._env_options()
        start = _f64(start)
        if start.ndim != 2 or start.shape[1] != self.dof:
            raise ValueError(f"start: expected [P][{self.dof}], got {list(start.shape)}")
        P = start.shape[0]
        targets = _f64(targets)
        if targets.ndim != 3 or targets.shape[0] != P or targets.shape[2] != 7:
            raise ValueError(f"targets: expected [{P}][S][7], got {list(targets.shape)}")
        S, W = targets.shape[1], int(W)
        if S < 1 or W < S:
            raise ValueError(f"{S} targets in {W} rows: expected W >= S >= 1 (every segment needs a row)")
        count = None
        if n_targets is not None:
            count = np.ascontiguousarray(n_targets, dtype=np.int32)
            if count.shape != (P,):
                raise ValueError(f"n_targets: expected [{P}], got {list(count.shape)}")
        step = None
        if max_joint_step is not None:
            step = _f64(max_joint_step)
            if step.shape != (self.dof,):
                raise ValueError(f"max_joint_step: expected [{self.dof}], got {list(step.shape)}")
        sol = np.empty((P, W, self.dof))
        status = np.empty((P, W), dtype=np.int32)
        steps = np.empty(P, dtype=np.int32)
        cost = np.empty((P, W)) if optional else None
        stats = np.zeros((P, W), dtype=STATS_DTYPE) if optional else None
        reached = np.empty(P, dtype=np.int32) if optional else None
        fraction = np.empty(P) if optional else None
        goals = np.empty((P, W, 7)) if optional else None
        segment_steps = np.empty((P, S), dtype=np.int32) if optional else None
        self._chk(self._L.pikamd_cartesian_waypoints(
            self._h, C.byref(params), C.byref(cartesian), P, S, W, _dp(start), _dp(targets),
            None if count is None else _ip(count), None if step is None else _dp(step), _dp(sol), _ip(status),
            _dp(cost) if optional else None, stats.ctypes.data_as(C.c_void_p) if optional else None,
            _ip(reached) if optional else None, _ip(steps), _ip(segment_steps) if optional else None,
            _dp(fraction) if optional else None, _dp(goals) if optional else None))
        return sol, status, cost, stats, reached, steps, fraction, goals, segment_steps

    def cartesian_waypoints_device(self, params: Params, cartesian: Cartesian, P: int, S: int, W: int, d_start: int,
                                   d_targets: int, d_solution: int, d_status: int, d_steps: int, d_n_targets: int = 0,
                                   d_max_joint_step: int = 0, d_cost: int = 0, d_stats: int = 0, d_reached: int = 0,
                                   d_segment_steps: int = 0, d_fraction: int = 0, d_goals: int = 0, stream: int = 0,
                                   slot: int = 0):
        """Enqueue cartesian_waypoints on HBM-resident buffers (raw device addresses); returns immediately -- the
        caller synchronises the stream.  The per-path state of the passes and, without d_goals, the poses are kept in
        scratch of the handle's slot."""
        self._env_options()
        if P < 0 or S < 1 or W < S:
            raise ValueError(f"{P} paths of {S} targets in {W} rows: expected P >= 0 and W >= S >= 1")
        self._chk(self._L.pikamd_cartesian_waypoints_device(
            self._h, C.byref(params), C.byref(cartesian), P, S, W, d_start or None, d_targets or None,
            d_n_targets or None, d_max_joint_step or None, d_solution or None, d_status or None, d_cost or None,
            d_stats or None, d_reached or None, d_steps or None, d_segment_steps or None, d_fraction or None,
            d_goals or None, stream or None, slot))

    def cartesian_waypoints_kernel_name(self, params: Params, P: int) -> str:
        """the kernel that walks the segments of P paths of cartesian_waypoints (pikamd_cartesian_waypoints_kernel_name)"""
        self._env_options()
        return self._L.pikamd_cartesian_waypoints_kernel_name(self._h, C.byref(params), P).decode()

    # ---- Cartesian paths from a pose: the start state restarted until the path holds -------
    def search_paths(self, params: Params, goals, seed, max_attempts: int, max_joint_step=None, rng_seed: int = 0,
                     problem_offset: int = 0, initial_guess=None):
        """pikamd_search_paths: P paths of W waypoints in local mode (params.mode = 1) from a pose: waypoint 0 is solved
        from the initial guess with `seed` as the displacement reference, the waypoints behind it as solve_paths does,
        and a path that did not hold throughout is tried again from a random valid configuration keyed by (rng_seed,
        problem_offset + p, attempt), up to max_attempts (1..MAX_ATTEMPTS) times; the attempt that held the most
        waypoints is kept, the first among equals -- one launch.  goals [P][W][7] ([P][W][n_tips][7] for several tips),
        seed [P][dof], initial_guess [P][dof] or None (= seed), max_joint_step [dof] or None.  Returns (solution
        [P][W][dof], status [P][W], cost [P][W], stats [P][W], reached [P], attempts [P], totals [P]); the result is
        what the loop of solve_batch and solve_paths calls in include/pick_ik_amd.h returns, bit for bit."""
        return self._search_paths("pikamd_search_paths", params, goals, seed, max_attempts, max_joint_step, rng_seed,
                                  problem_offset, initial_guess)

    def _search_paths(self, entry, params, goals, seed, max_attempts, max_joint_step, rng_seed, problem_offset,
                      initial_guess):
        """search_paths / search_global_paths; entry: the name of the library's entry point"""
        self._env_options()
        goals = _f64(goals)
        tail = (7,) if self.n_tips == 1 else (self.n_tips, 7)
        if goals.ndim != 2 + len(tail) or goals.shape[2:] != tail:
            raise ValueError(f"goals: expected [P][W]{list(tail)}, got {list(goals.shape)}")
        P, W = goals.shape[:2]
        if W < 1:
            raise ValueError("goals: a path has at least one waypoint")
        seed = _f64(seed)
        if seed.shape != (P, self.dof):
            raise ValueError(f"seed: expected [{P}][{self.dof}], got {list(seed.shape)}")
        guess = None
        if initial_guess is not None:
            guess = _f64(initial_guess)
            if guess.shape != (P, self.dof):
                raise ValueError(f"initial_guess: expected [{P}][{self.dof}], got {list(guess.shape)}")
        step = None
        if max_joint_step is not None:
            step = _f64(max_joint_step)
            if step.shape != (self.dof,):
                raise ValueError(f"max_joint_step: expected [{self.dof}], got {list(step.shape)}")
        K = int(max_attempts)
        if not 1 <= K <= MAX_ATTEMPTS:
            raise ValueError(f"max_attempts: expected 1..{MAX_ATTEMPTS}, got {max_attempts}")
        sol = np.empty((P, W, self.dof))
        status = np.empty((P, W), dtype=np.int32)
        cost = np.empty((P, W))
        stats = np.zeros((P, W), dtype=STATS_DTYPE)
        reached = np.empty(P, dtype=np.int32)
        attempts = np.empty(P, dtype=np.int32)
        totals = np.zeros(P, dtype=STATS_DTYPE)
        self._chk(getattr(self._L, entry)(
            self._h, C.byref(params), P, W, _dp(goals), _dp(seed), None if guess is None else _dp(guess),
            None if step is None else _dp(step), C.c_uint64(rng_seed), problem_offset, K, _dp(sol), _ip(status),
            _dp(cost), stats.ctypes.data_as(C.c_void_p), _ip(reached), _ip(attempts), totals.ctypes.data_as(C.c_void_p)))
        return sol, status, cost, stats, reached, attempts, totals

    def search_paths_device(self, params: Params, P: int, W: int, d_goals: int, d_seed: int, max_attempts: int,
                            d_solution: int, d_status: int, d_initial_guess: int = 0, d_max_joint_step: int = 0,
                            d_cost: int = 0, d_stats: int = 0, d_reached: int = 0, d_attempts: int = 0,
                            d_totals: int = 0, rng_seed: int = 0, problem_offset: int = 0, stream: int = 0,
                            slot: int = 0):
        """Enqueue search_paths on HBM-resident buffers (raw device addresses); returns immediately -- the caller
        synchronises the stream."""
        self._search_paths_device("pikamd_search_paths_device", params, P, W, d_goals, d_seed, max_attempts, d_solution,
                                  d_status, d_initial_guess, d_max_joint_step, d_cost, d_stats, d_reached, d_attempts,
                                  d_totals, rng_seed, problem_offset, stream, slot)

    def _search_paths_device(self, entry, params, P, W, d_goals, d_seed, max_attempts, d_solution, d_status,
                             d_initial_guess, d_max_joint_step, d_cost, d_stats, d_reached, d_attempts, d_totals,
                             rng_seed, problem_offset, stream, slot):
        """search_paths_device / search_global_paths_device; entry: the name of the library's entry point"""
        self._env_options()
        if P < 0 or W < 1:
            raise ValueError(f"{P} paths of {W} waypoints: expected P >= 0 and W >= 1")
        self._chk(getattr(self._L, entry)(
            self._h, C.byref(params), P, W, d_goals or None, d_seed or None, d_initial_guess or None,
            d_max_joint_step or None, C.c_uint64(rng_seed), problem_offset, max_attempts, d_solution or None,
            d_status or None, d_cost or None, d_stats or None, d_reached or None, d_attempts or None, d_totals or None,
            stream or None, slot))

    def search_paths_kernel_name(self, params: Params, P: int) -> str:
        """the kernel search_paths launches for P paths (pikamd_search_paths_kernel_name)"""
        self._env_options()
        return self._L.pikamd_search_paths_kernel_name(self._h, C.byref(params), P).decode()

    # ---- Cartesian paths from a pose, memetic start: waypoint 0 by the memetic solver, the path behind it ----
    def search_global_paths(self, params: Params, goals, seed, max_attempts: int, max_joint_step=None,
                            rng_seed: int = 0, problem_offset: int = 0, initial_guess=None):
        """pikamd_search_global_paths: search_paths with waypoint 0 of every attempt solved by the memetic solver
        (params.mode = 0; attempt a with rng_seed + (a << 32), as search_global_batch) and the waypoints behind it in
        local mode, as solve_paths does with mode = 1.  Arguments and returns as search_paths; the result is what the
        loop of solve_batches and solve_paths calls in include/pick_ik_amd.h returns, bit for bit."""
        return self._search_paths("pikamd_search_global_paths", params, goals, seed, max_attempts, max_joint_step,
                                  rng_seed, problem_offset, initial_guess)

    def search_global_paths_device(self, params: Params, P: int, W: int, d_goals: int, d_seed: int, max_attempts: int,
                                   d_solution: int, d_status: int, d_initial_guess: int = 0,
                                   d_max_joint_step: int = 0, d_cost: int = 0, d_stats: int = 0, d_reached: int = 0,
                                   d_attempts: int = 0, d_totals: int = 0, rng_seed: int = 0, problem_offset: int = 0,
                                   stream: int = 0, slot: int = 0):
        """Enqueue search_global_paths on HBM-resident buffers (raw device addresses): every attempt is enqueued,
        nothing synchronises -- the caller synchronises the stream."""
        self._search_paths_device("pikamd_search_global_paths_device", params, P, W, d_goals, d_seed, max_attempts,
                                  d_solution, d_status, d_initial_guess, d_max_joint_step, d_cost, d_stats, d_reached,
                                  d_attempts, d_totals, rng_seed, problem_offset, stream, slot)

    def search_global_paths_kernel_name(self, params: Params, P: int) -> str:
        """the kernel that walks the waypoints behind the first for P paths (pikamd_search_global_paths_kernel_name)"""
        self._env_options()
        return self._L.pikamd_search_global_paths_kernel_name(self._h, C.byref(params), P).decode()

    # ---- IK with random restarts: local mode (search_batch), the memetic solver (search_global_batch) ----
    def _search(self, entry, params, goal_pos_quat, seed, max_attempts, rng_seed, problem_offset, initial_guess, all_attempts):
        """search_batch / search_global_batch; entry: the name of the library's entry point"""
        self._env_options()
        goal = _f64(goal_pos_quat)
        if goal.ndim < 2 or goal.size != goal.shape[0] * 7 * self.n_tips:
            raise ValueError(f"goal_pos_quat: expected [B]{[7] if self.n_tips == 1 else [self.n_tips, 7]}, "
                             f"got {list(goal.shape)}")
        B = goal.shape[0]
        seed = _f64(seed)
        if seed.shape != (B, self.dof):
            raise ValueError(f"seed: expected [{B}][{self.dof}], got {list(seed.shape)}")
        guess = None
        if initial_guess is not None:
            guess = _f64(initial_guess)
            if guess.shape != (B, self.dof):
                raise ValueError(f"initial_guess: expected [{B}][{self.dof}], got {list(guess.shape)}")
        K = int(max_attempts)
        if not 1 <= K <= MAX_ATTEMPTS:
            raise ValueError(f"max_attempts: expected 1..{MAX_ATTEMPTS}, got {max_attempts}")
        sol = np.empty((B, self.dof))
        status = np.empty(B, dtype=np.int32)
        cost = np.empty(B)
        stats = np.zeros(B, dtype=STATS_DTYPE)
        attempts = np.empty(B, dtype=np.int32)
        all_sol = np.empty((B, K, self.dof)) if all_attempts else None
        all_st = np.empty((B, K), dtype=np.int32) if all_attempts else None
        # (C.c_uint64 takes any int modulo 2^64: a seed with the attempt in its high word may have wrapped)
        self._chk(getattr(self._L, entry)(
            self._h, C.byref(params), B, _dp(goal), _dp(seed), None if guess is None else _dp(guess), C.c_uint64(rng_seed),
            problem_offset, K, _dp(sol), _ip(status), _dp(cost), stats.ctypes.data_as(C.c_void_p), _ip(attempts),
            None if all_sol is None else _dp(all_sol), None if all_st is None else _ip(all_st)))
        if all_attempts:
            return sol, status, cost, stats, attempts, all_sol, all_st
        return sol, status, cost, stats, attempts

    def _search_device(self, entry, params, B, d_goal, d_seed, max_attempts, d_solution, d_status, d_initial_guess, d_cost,
                       d_stats, d_attempts, d_all_solution, d_all_status, rng_seed, problem_offset, stream, slot):
        """search_batch_device / search_global_batch_device; entry: the name of the library's entry point"""
        self._env_options()
        self._chk(getattr(self._L, entry)(
            self._h, C.byref(params), B, d_goal or None, d_seed or None, d_initial_guess or None, C.c_uint64(rng_seed),
            problem_offset, max_attempts, d_solution or None, d_status or None, d_cost or None, d_stats or None,
            d_attempts or None, d_all_solution or None, d_all_status or None, stream or None, slot))

    def search_batch(self, params: Params, goal_pos_quat, seed, max_attempts: int, rng_seed: int = 0,
                     problem_offset: int = 0, initial_guess=None, all_attempts: bool = False):
        """pikamd_search_batch: local mode (params.mode = 1) with up to max_attempts (1..MAX_ATTEMPTS) attempts per
        problem, every attempt after a failure from a random valid configuration keyed by (rng_seed, problem_offset + b,
        attempt) -- one launch.  Returns (solution [B][dof], status [B], cost [B], stats [B], attempts [B]) and, with
        all_attempts, (all_solution [B][max_attempts][dof], all_status [B][max_attempts]) behind them: every attempt
        of every problem, run without an early exit.  The result is what the loop of solve_batch calls in
        include/pick_ik_amd.h returns, bit for bit."""
        return self._search("pikamd_search_batch", params, goal_pos_quat, seed, max_attempts, rng_seed, problem_offset,
                            initial_guess, all_attempts)

    def search_batch_device(self, params: Params, B: int, d_goal: int, d_seed: int, max_attempts: int, d_solution: int,
                            d_status: int, d_initial_guess: int = 0, d_cost: int = 0, d_stats: int = 0,
                            d_attempts: int = 0, d_all_solution: int = 0, d_all_status: int = 0, rng_seed: int = 0,
                            problem_offset: int = 0, stream: int = 0, slot: int = 0):
        """Enqueue a restart search on HBM-resident buffers (raw device addresses); returns immediately -- the caller
        synchronises the stream."""
        self._search_device("pikamd_search_batch_device", params, B, d_goal, d_seed, max_attempts, d_solution, d_status,
                            d_initial_guess, d_cost, d_stats, d_attempts, d_all_solution, d_all_status, rng_seed,
                            problem_offset, stream, slot)

    def search_global_batch(self, params: Params, goal_pos_quat, seed, max_attempts: int, rng_seed: int = 0,
                            problem_offset: int = 0, initial_guess=None, all_attempts: bool = False):
        """pikamd_search_global_batch: global mode (params.mode = 0) with up to max_attempts (1..MAX_ATTEMPTS) attempts
        per problem; attempt a solves with rng_seed + (a << 32), every attempt after a failure from a random valid
        configuration keyed by (rng_seed, problem_offset + b, attempt).  Returns what search_batch returns; the result is
        what the loop of one-record solve_batches calls in include/pick_ik_amd.h returns, bit for bit."""
        return self._search("pikamd_search_global_batch", params, goal_pos_quat, seed, max_attempts, rng_seed, problem_offset,
                            initial_guess, all_attempts)

    def search_global_batch_device(self, params: Params, B: int, d_goal: int, d_seed: int, max_attempts: int,
                                   d_solution: int, d_status: int, d_initial_guess: int = 0, d_cost: int = 0,
                                   d_stats: int = 0, d_attempts: int = 0, d_all_solution: int = 0, d_all_status: int = 0,
                                   rng_seed: int = 0, problem_offset: int = 0, stream: int = 0, slot: int = 0):
        """Enqueue a global-mode restart search on HBM-resident buffers (raw device addresses): all max_attempts
        attempts; returns immediately -- the caller synchronises the stream."""
        self._search_device("pikamd_search_global_batch_device", params, B, d_goal, d_seed, max_attempts, d_solution, d_status,
                            d_initial_guess, d_cost, d_stats, d_attempts, d_all_solution, d_all_status, rng_seed,
                            problem_offset, stream, slot)

    def search_kernel_name(self, params: Params, B: int, max_attempts: int):
        """(the kernel search_batch launches for B problems of max_attempts attempts, attempts in flight per problem:
        1 = the sequential schedule, max_attempts = the parallel one) -- pikamd_search_kernel_name"""
        self._env_options()
        n = C.c_int32(0)
        name = self._L.pikamd_search_kernel_name(self._h, C.byref(params), B, max_attempts, C.byref(n)).decode()
        return name, int(n.value)


def interpolate_poses(cartesian: Cartesian, start_pose, target, W: int, strict: bool = False):
    """pikamd_interpolate_poses (a host function: no handle, no device): the waypoints of P Cartesian motions from
    start_pose [P][7] to target [P][7] (cartesian.frame says what a target is).  Returns (goals [P][W][7], steps [P]):
    steps[p] is MoveIt's step count, rows k < steps[p] are the interpolated poses, the rows behind them -- and every
    row of a path with steps[p] > W -- the resolved target."""
    start_pose = _f64(start_pose)
    if start_pose.ndim != 2 or start_pose.shape[1] != 7:
        raise ValueError(f"start_pose: expected [P][7], got {list(start_pose.shape)}")
    P = start_pose.shape[0]
    target = _f64(target)
    if target.shape != (P, 7):
        raise ValueError(f"target: expected [{P}][7], got {list(target.shape)}")
    W = int(W)
    if W < 1:
        raise ValueError("W: a path has at least one waypoint")
    goals = np.empty((P, W, 7))
    steps = np.empty(P, dtype=np.int32)
    L = lib(strict)
    _check(L.pikamd_interpolate_poses(C.byref(cartesian), P, W, _dp(start_pose), _dp(target), _dp(goals), _ip(steps)), L)
    return goals, steps


def shard_bounds(total: int, rank: int, world: int, strict: bool = False):
    """pikamd_shard_bounds: the contiguous range [lo, hi) device `rank` of `world` solves"""
    lo, hi = C.c_int64(), C.c_int64()
    lib(strict).pikamd_shard_bounds(total, rank, world, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def solve_batch_sharded(solvers, params: Params, goal_pos_quat, seed, rng_seed: int = 0, problem_offset: int = 0,
                        initial_guess=None):
    """pikamd_solve_batch_sharded: one batch over several handles (one per GPU), host arrays in and out."""
    s0 = solvers[0]
    for s in solvers:
        s._env_options()
    goal = _f64(goal_pos_quat).reshape(-1, 7 * s0.n_tips)
    B = goal.shape[0]
    seed = _f64(seed).reshape(B, s0.dof)
    guess = None if initial_guess is None else _f64(initial_guess).reshape(B, s0.dof)
    sol = np.empty((B, s0.dof))
    status = np.empty(B, dtype=np.int32)
    cost = np.empty(B)
    stats = np.zeros(B, dtype=STATS_DTYPE)
    arr = (C.c_void_p * len(solvers))(*[s._h for s in solvers])
    _check(s0._L.pikamd_solve_batch_sharded(arr, len(solvers), C.byref(params), B, _dp(goal), _dp(seed),
                                            None if guess is None else _dp(guess), C.c_uint64(rng_seed),
                                            problem_offset, _dp(sol), _ip(status), _dp(cost),
                                            stats.ctypes.data_as(C.c_void_p)), s0._L)
    return sol, status, cost, stats


def ik_memetic(solver: Solver, initial_guess, goal_pos_quat, params: Params | None = None,
               approx_solution: bool = False, rng_seed: int = 0):
    """Batch form of pick_ik::ik_memetic (src/ik_memetic.cpp:285-373): returns
    (solutions [B][dof], has_value [B]) where has_value mirrors std::optional."""
    p = params or default_params()
    p.mode = 0
    p.return_approximate_solution = int(approx_solution)
    sol, status, _, _ = solver.solve_batch(p, goal_pos_quat, initial_guess, rng_seed=rng_seed)
    return sol, status > 0


def ik_gradient(solver: Solver, initial_guess, goal_pos_quat, params: Params | None = None,
                approx_solution: bool = False):
    """Batch form of pick_ik::ik_gradient (src/ik_gradient.cpp:96-139)."""
    p = params or default_params()
    p.mode = 1
    p.return_approximate_solution = int(approx_solution)
    sol, status, _, _ = solver.solve_batch(p, goal_pos_quat, initial_guess)
    return sol, status > 0
