// pik_validity_ops.hpp -- host side of the sphere validity test (pik_validity.hpp, pikamd_validity_batch and the step
// of the restart searches): the model as the kernels read it, the arguments of the rows kernel and the ops table a
// per-length translation unit of pik_validity_inst.hip exports.  No device code here; not read by pik_inst.hip.
#pragma once

#include "pik_dofs.hpp"
#include "pik_solver.hpp"

namespace pik {

constexpr int VALIDITY_MAX_SPHERES = PIKAMD_MAX_SPHERES;
constexpr int VALIDITY_MAX_PAIRS = PIKAMD_MAX_SPHERE_PAIRS;
constexpr int PIKAMD_VALIDITY_REFUSED_K = -1004; // PIKAMD_VALIDITY_REFUSED

// The model of a handle (pikamd_set_validity_model) as the kernels read it, wave-uniformly.  The spheres are SORTED by
// after_variable (stable: base-frame spheres first), so that one walk of the chain meets them in order; `index` keeps
// the caller's numbering, which `radius`, `pairs` and the centres a kernel stores use.
struct ValidityModelK {
    double centre[VALIDITY_MAX_SPHERES][3]; // sorted order: in the link's frame (after = -1: in the base frame)
    double radius[VALIDITY_MAX_SPHERES];    // caller's index
    int32_t after[VALIDITY_MAX_SPHERES];    // sorted order, ascending
    int32_t index[VALIDITY_MAX_SPHERES];    // sorted order -> caller's index
    int32_t pairs[VALIDITY_MAX_PAIRS][2];   // caller's indices
    int32_t n_spheres, n_pairs;
    uint32_t zero_mask; // bit k (sorted order): the local centre is all zeros -- the centre is the link frame's origin
    int32_t pad_;
};

// What validity_rows_kernel gets (device pointers): the rows of one attempt of pikamd_search_global_batch, exactly the
// fields restart_gate_kernel reads and rewrites of RestartArgs.
struct ValidityRows {
    long long B;
    int every;            // every attempt of every problem runs (all_* wanted)
    int pad_;
    const int* open;      // [B]
    double* row_solution; // [B][D]: a refused row becomes the seed
    int* row_status;      // [B]: ... and PIKAMD_VALIDITY_REFUSED
    const double* seed;   // [B][D]
};

struct ValidityOps {
    // the device image of a model for this chain length: the chain's constants in the exact flavour's layout and the
    // model behind them (a buffer of its own: no slot's constants are touched by the test)
    size_t image_bytes;
    void (*pack)(const pikamd_solver*, const ValidityModelK&, void* image);
    // pikamd_validity_batch_device: d_clear, d_centres may be null
    int (*check)(const void* d_image, int n_spheres, long long n, const double* d_q, int* d_valid, double* d_clear,
                 double* d_centres, hipStream_t);
    // the step of pikamd_search_global_batch*, behind the gate and in front of the fold
    int (*rows)(const void* d_image, int n_spheres, const ValidityRows&, hipStream_t);
};

PIK_DECLARE_OPS_FAMILY(ValidityOps, validity) // validity_ops_d<N>(), validity_ops(dof)

} // namespace pik
