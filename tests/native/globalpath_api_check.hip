// A HIP caller of the pikamd_search_global_paths entry points: compiled by tests/test_globalpath_cpu.py with hipcc for
// gfx950, host AND device pass (hipcc checks host function bodies in the device pass too, so every prototype must be
// visible there).
#include <hip/hip_runtime.h>

#include "../../include/pick_ik_amd.h"
#include "../../pick_ik_amd/host/pick_ik_amd.hpp"

__global__ void touch(int32_t* status) { status[threadIdx.x] = PIKAMD_NOT_ATTEMPTED; }

// what a caller holding a hipStream_t writes: device buffers, the stream-ordered entry point, no synchronise
int enqueue_search_global_paths(pikamd_solver* s, const pikamd_params* p, int64_t P, int32_t W, const double* d_goals,
                                const double* d_seed, double* d_solution, int32_t* d_status, int32_t* d_reached,
                                hipStream_t stream) {
    hipLaunchKernelGGL(touch, dim3(1), dim3(64), 0, stream, d_status);
    const int rc = pikamd_search_global_paths_device(s, p, P, W, d_goals, d_seed, nullptr, nullptr, 1, 0,
                                                     PIKAMD_MAX_ATTEMPTS, d_solution, d_status, nullptr, nullptr,
                                                     d_reached, nullptr, nullptr, stream, 0);
    return rc ? rc : (pikamd_search_global_paths_kernel_name(s, p, P)[0] == 0);
}

int host_search_global_paths(pikamd_solver* s, const pikamd_params* p, const double* goals, const double* seed,
                             double* solution, int32_t* status) {
    return pikamd_search_global_paths(s, p, 1, 1, goals, seed, nullptr, nullptr, 0, 0, 4, solution, status, nullptr,
                                      nullptr, nullptr, nullptr, nullptr);
}

pick_ik_amd::SearchPathsResult mirror_search_global_paths(const pick_ik_amd::Solver& s, const std::vector<double>& seeds,
                                                          const std::vector<pick_ik_amd::Pose>& goals, int W) {
    return s.ik_memetic_search_paths(seeds, goals, W, pick_ik_amd::CostSpec{}, pick_ik_amd::MemeticIkParams{}, 4);
}
