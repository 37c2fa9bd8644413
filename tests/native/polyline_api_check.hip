// A HIP caller of the pikamd_cartesian_waypoints entry points: compiled by tests/test_polyline_cpu.py with hipcc for
// gfx950, host AND device pass (hipcc checks host function bodies in the device pass too, so every prototype must be
// visible there).
#include <hip/hip_runtime.h>

#include "../../include/pick_ik_amd.h"
#include "../../pick_ik_amd/host/pick_ik_amd.hpp"

__global__ void mark(int32_t* status) { status[threadIdx.x] = PIKAMD_NOT_ATTEMPTED; }

// what a caller holding a hipStream_t writes: device buffers, the stream-ordered entry point, no synchronise
int enqueue_cartesian_waypoints(pikamd_solver* s, const pikamd_params* p, int64_t P, int32_t S, int32_t W,
                                const double* d_start, const double* d_targets, const int32_t* d_n_targets,
                                double* d_solution, int32_t* d_status, int32_t* d_steps, int32_t* d_segment_steps,
                                double* d_fraction, hipStream_t stream) {
    hipLaunchKernelGGL(mark, dim3(1), dim3(64), 0, stream, d_status);
    const pikamd_cartesian c = {PIKAMD_CARTESIAN_OFFSET, 0, 0.01, 0.0, 2.0};
    const int rc = pikamd_cartesian_waypoints_device(s, p, &c, P, S, W, d_start, d_targets, d_n_targets, nullptr, d_solution,
                                                     d_status, nullptr, nullptr, nullptr, d_steps, d_segment_steps,
                                                     d_fraction, nullptr, stream, 1);
    return rc ? rc : (pikamd_cartesian_waypoints_kernel_name(s, p, P)[0] == 0);
}

int host_cartesian_waypoints(pikamd_solver* s, const pikamd_params* p, const double* start, const double* targets,
                             double* solution, int32_t* status, int32_t* steps) {
    const pikamd_cartesian c = {PIKAMD_CARTESIAN_TIP, 2, 0.0, 0.1, 0.0};
    return pikamd_cartesian_waypoints(s, p, &c, 1, 2, 8, start, targets, nullptr, nullptr, solution, status, nullptr, nullptr,
                                      nullptr, steps, nullptr, nullptr, nullptr);
}

pick_ik_amd::CartesianWaypointsResult mirror_cartesian_waypoints(const pick_ik_amd::Solver& s, const std::vector<double>& start,
                                                                 const std::vector<std::vector<pick_ik_amd::Pose>>& targets,
                                                                 int W) {
    const pikamd_cartesian c = {PIKAMD_CARTESIAN_GLOBAL, 0, 0.02, 0.05, 1.5};
    return s.compute_cartesian_waypoints(start, targets, W, c, pick_ik_amd::CostSpec{}, pick_ik_amd::GradientIkParams{});
}
