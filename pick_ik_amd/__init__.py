"""pick_ik_amd -- MI355X-native batched IK solver behind pick_ik's solver interface.

The package holds only the hot path BASELINE.json names: ``csrc/`` (HIP kernels + the C ABI of
include/pick_ik_amd.h), ``solver.py`` (ctypes mirror of the reference's solver interface),
``robots.py`` (serial-chain tables) and ``build.py``.
"""
from . import robots  # noqa: F401
from .solver import (APPROXIMATE, CARTESIAN_GLOBAL, CARTESIAN_OFFSET, CARTESIAN_TIP, GATE_REFUSED, MAX_ATTEMPTS,  # noqa: F401
                     NO_IK_SOLUTION, NOT_ATTEMPTED, PATH_JUMP, PATH_RELATIVE_JUMP, SUCCESS, Cartesian, Gate, Params,
                     PickIkAmdError, Solver, Sphere, VALIDITY_REFUSED, default_params, ik_gradient, ik_memetic,
                     interpolate_poses)
