"""Raw ctypes calls of the path / search entry points of include/pick_ik_amd.h -- every argument as the C ABI takes
it, any of them NULL -- for the tests of what they refuse, what they report and which optional arrays they need
(tests/test_gpu_abi_characterisation.py, test_gpu_path.py, test_gpu_search.py, test_gpu_search_global.py,
test_gpu_startpath.py, test_gpu_globalpath.py, test_gpu_cartesian.py, test_gpu_polyline.py)."""
import ctypes as C

import numpy as np

from pick_ik_amd.solver import STATS_DTYPE

DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)
#: the array arguments in the order of the C signatures
PATH_ARRAYS = ("goal", "start", "max_joint_step", "solution", "status", "final_cost", "stats", "reached")
SEARCH_ARRAYS = ("goal", "seed", "initial_guess", "solution", "status", "final_cost", "stats", "attempts",
                 "all_solution", "all_status")
STARTPATH_ARRAYS = ("goal", "seed", "initial_guess", "max_joint_step", "solution", "status", "final_cost", "stats",
                    "reached", "attempts", "totals")
CARTESIAN_ARRAYS = ("start", "target", "max_joint_step", "solution", "status", "final_cost", "stats", "reached", "steps",
                    "fraction", "goals")
WAYPOINT_ARRAYS = ("start", "targets", "n_targets", "max_joint_step", "solution", "status", "final_cost", "stats",
                   "reached", "steps", "segment_steps", "fraction", "goals")
PATH_OUTPUTS, SEARCH_OUTPUTS, STARTPATH_OUTPUTS = PATH_ARRAYS[3:], SEARCH_ARRAYS[3:], STARTPATH_ARRAYS[4:]
_CTYPE = {np.dtype(np.float64): DP, np.dtype(np.int32): IP}


def _ptr(a):
    """numpy array -> typed pointer, a device address (int) as it is, None -> NULL"""
    if a is None or isinstance(a, int):
        return a
    return a.ctypes.data_as(_CTYPE.get(a.dtype, C.c_void_p))


def _params(p):
    return None if p is None else C.byref(p)


def solve_paths(L, h, p, P, W, a, device=False, slot=0):
    """pikamd_solve_paths[_device]; a: name -> array of PATH_ARRAYS (absent or None: NULL)"""
    args = [_ptr(a.get(k)) for k in PATH_ARRAYS]
    if device:
        return L.pikamd_solve_paths_device(h, _params(p), P, W, *args, None, slot)
    return L.pikamd_solve_paths(h, _params(p), P, W, *args)


def search(L, h, p, B, K, a, device=False, slot=0, global_mode=False, rng_seed=0, problem_offset=0):
    """pikamd_search[_global]_batch[_device]; a: name -> array of SEARCH_ARRAYS (absent or None: NULL)"""
    x = [_ptr(a.get(k)) for k in SEARCH_ARRAYS]
    fn = getattr(L, "pikamd_search" + ("_global" if global_mode else "") + "_batch" + ("_device" if device else ""))
    args = [h, _params(p), B, *x[:3], C.c_uint64(rng_seed), problem_offset, K, *x[3:]]
    return fn(*args, None, slot) if device else fn(*args)


def search_paths(L, h, p, P, W, K, a, rng_seed=0, problem_offset=0, device=False, slot=0, global_mode=False):
    """pikamd_search[_global]_paths[_device]; a: name -> array of STARTPATH_ARRAYS (absent or None: NULL)"""
    x = [_ptr(a.get(k)) for k in STARTPATH_ARRAYS]
    fn = getattr(L, "pikamd_search" + ("_global" if global_mode else "") + "_paths" + ("_device" if device else ""))
    args = [h, _params(p), P, W, *x[:4], C.c_uint64(rng_seed), problem_offset, K, *x[4:]]
    return fn(*args, None, slot) if device else fn(*args)


def cartesian_paths(L, h, p, c, P, W, a, device=False, slot=0):
    """pikamd_cartesian_paths[_device]; c: the pikamd_cartesian (None: NULL); a: name -> array of CARTESIAN_ARRAYS"""
    args = [h, _params(p), _params(c), P, W, *[_ptr(a.get(k)) for k in CARTESIAN_ARRAYS]]
    return L.pikamd_cartesian_paths_device(*args, None, slot) if device else L.pikamd_cartesian_paths(*args)


def cartesian_waypoints(L, h, p, c, P, S, W, a, device=False, slot=0):
    """pikamd_cartesian_waypoints[_device]; c: the pikamd_cartesian (None: NULL); a: name -> array of WAYPOINT_ARRAYS"""
    args = [h, _params(p), _params(c), P, S, W, *[_ptr(a.get(k)) for k in WAYPOINT_ARRAYS]]
    return L.pikamd_cartesian_waypoints_device(*args, None, slot) if device else L.pikamd_cartesian_waypoints(*args)


def last_error(L):
    return L.pikamd_last_error().decode()


def _stats_pattern(shape):
    return np.full(int(np.prod(shape)) * STATS_DTYPE.itemsize, 0xAB, dtype=np.uint8).view(STATS_DTYPE).reshape(shape)


def path_arrays(s, goals, start, max_joint_step):
    """every array of a pikamd_solve_paths call, the outputs filled with a pattern no solve returns"""
    P, W = goals.shape[:2]
    return dict(goal=goals, start=start, max_joint_step=max_joint_step, solution=np.full((P, W, s.dof), -7.5),
                status=np.full((P, W), -77, dtype=np.int32), final_cost=np.full((P, W), -7.5),
                stats=_stats_pattern((P, W)), reached=np.full(P, -77, dtype=np.int32))


def search_arrays(s, goals, seed, initial_guess, K):
    """every array of a pikamd_search[_global]_batch call, the outputs filled with a pattern no solve returns"""
    B = len(seed)
    return dict(goal=goals, seed=seed, initial_guess=initial_guess, solution=np.full((B, s.dof), -7.5),
                status=np.full(B, -77, dtype=np.int32), final_cost=np.full(B, -7.5),
                stats=_stats_pattern((B,)), attempts=np.full(B, -77, dtype=np.int32),
                all_solution=np.full((B, K, s.dof), -7.5), all_status=np.full((B, K), -77, dtype=np.int32))


def startpath_arrays(s, goals, seed, guess, step):
    """every array of a pikamd_search[_global]_paths call, the outputs filled with a pattern no call returns"""
    P, W = goals.shape[:2]
    return dict(goal=goals, seed=seed, initial_guess=guess, max_joint_step=step, solution=np.full((P, W, s.dof), -7.5),
                status=np.full((P, W), -77, dtype=np.int32), final_cost=np.full((P, W), -7.5),
                stats=_stats_pattern((P, W)), reached=np.full(P, -77, dtype=np.int32),
                attempts=np.full(P, -77, dtype=np.int32), totals=_stats_pattern((P,)))


def cartesian_outputs(P, W, dof):
    """every output of a pikamd_cartesian_paths call, filled with a pattern no call returns"""
    return dict(solution=np.full((P, W, dof), -7.5), status=np.full((P, W), -77, dtype=np.int32),
                final_cost=np.full((P, W), -7.5), stats=_stats_pattern((P, W)), reached=np.full(P, -77, dtype=np.int32),
                steps=np.full(P, -77, dtype=np.int32), fraction=np.full(P, -7.5), goals=np.full((P, W, 7), -7.5))


def waypoint_outputs(P, S, W, dof):
    """... and of a pikamd_cartesian_waypoints call"""
    return dict(cartesian_outputs(P, W, dof), segment_steps=np.full((P, S), -77, dtype=np.int32))


def check_optional_arrays(call, fresh, optional, outputs):
    """call(arrays) -> rc; fresh() -> a new set of arrays.  The call with every array present is the reference; then
    with each array of `optional` absent in turn every output that is present must equal the reference's bit for bit
    (the optional INPUTS of fresh() are chosen so that leaving them out changes no answer)."""
    full = fresh()
    assert call(full) == 0
    for k in outputs:
        assert full[k].tobytes() != fresh()[k].tobytes(), f"{k} was not written"
    for gone in optional:
        a = fresh()
        a[gone] = None
        assert call(a) == 0, gone
        for k in outputs:
            if a[k] is not None:
                assert a[k].tobytes() == full[k].tobytes(), f"without {gone}: {k} differs"
    return full


def device_buffers(n, size=4096):
    """n device allocations of `size` bytes through the HIP runtime the library has loaded: (addresses, free())"""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64.so" in line)
    hip = C.CDLL(path)
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    ptrs = []
    for _ in range(n):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), size) == 0
        ptrs.append(p.value)

    def free():
        for p in ptrs:
            hip.hipFree(p)
    return ptrs, free
