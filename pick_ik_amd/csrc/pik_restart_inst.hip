// pik_restart_inst.hip -- the restart launcher (pik_restart.hpp) for ONE chain length (-DPIK_INST_D=<dof>); compiled
// once per supported length with the flags of the flavour whose memetic kernels it launches (pick_ik_amd/build.py).
// -DPIK_INST_STUB: nothing for this length (experiment builds).
//
// The memetic kernels are NOT compiled here: every variant the launcher names -- the forms for several tip frames
// included -- is declared as an explicit instantiation that lives elsewhere, in the flavour's pik_inst object of this
// length.  This object holds the prepare and fold kernels and undefined references to the memetic kernels' host stubs.
#ifndef PIK_INST_D
#error "compile with -DPIK_INST_D=<dof>"
#endif
#define PIK_CAT2(a, b) a##b
#define PIK_CAT(a, b) PIK_CAT2(a, b)

#if defined(PIK_INST_STUB)
#include "pik_restart_ops.hpp"
namespace pik {
const RestartOps* PIK_CAT(restart_ops_d, PIK_INST_D)() { return nullptr; }
} // namespace pik
#else
#include "pik_restart.hpp"
namespace pik {
#define PIK_EXTERN_MEMETIC(LPE, MULTI, OCC)                                                                       \
    extern template __global__ void memetic_kernel<PIK_INST_D, LPE, MULTI, OCC>(const ConstsK<PIK_INST_D>* __restrict__, \
                                                                                 SolveArgs);
PIK_EXTERN_MEMETIC(16, false, 1)
PIK_EXTERN_MEMETIC(8, false, 1)
PIK_EXTERN_MEMETIC(4, false, 1)
PIK_EXTERN_MEMETIC(2, false, 1)
PIK_EXTERN_MEMETIC(1, false, 1)
#if PIK_INST_D <= 9
PIK_EXTERN_MEMETIC(1, false, 2)
#endif
#if !defined(PIK_STRICT)
PIK_EXTERN_MEMETIC(16, true, 1)
PIK_EXTERN_MEMETIC(8, true, 1)
#endif
PIK_EXTERN_MEMETIC(2, true, 1)
PIK_EXTERN_MEMETIC(1, true, 1)
#undef PIK_EXTERN_MEMETIC
const RestartOps* PIK_CAT(restart_ops_d, PIK_INST_D)() { return make_restart_ops<PIK_INST_D>(); }
} // namespace pik
#endif
