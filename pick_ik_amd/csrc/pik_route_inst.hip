// pik_route_inst.hip -- the routed launcher (pik_route.hpp) for ONE chain length (-DPIK_INST_D=<dof>); compiled once
// per supported length with the flags of the flavour whose memetic kernels it launches (pick_ik_amd/build.py).
// -DPIK_INST_STUB: nothing for this length (experiment builds).
//
// The memetic kernels are NOT compiled here: every variant the launcher names is declared as an explicit
// instantiation that lives elsewhere -- the flavour's pik_inst object of this length, which launch_solve instantiates
// them in.  This object holds the router kernel and undefined references to the kernels' host stubs.
#ifndef PIK_INST_D
#error "compile with -DPIK_INST_D=<dof>"
#endif
#define PIK_CAT2(a, b) a##b
#define PIK_CAT(a, b) PIK_CAT2(a, b)

#if defined(PIK_INST_STUB)
#include "pik_route_ops.hpp"
namespace pik {
const RouteOps* PIK_CAT(route_ops_d, PIK_INST_D)() { return nullptr; }
} // namespace pik
#else
#include "pik_route.hpp"
namespace pik {
#define PIK_EXTERN_MEMETIC(LPE, OCC)                                                                             \
    extern template __global__ void memetic_kernel<PIK_INST_D, LPE, false, OCC>(const ConstsK<PIK_INST_D>* __restrict__, \
                                                                                 SolveArgs);
PIK_EXTERN_MEMETIC(16, 1)
PIK_EXTERN_MEMETIC(8, 1)
PIK_EXTERN_MEMETIC(4, 1)
PIK_EXTERN_MEMETIC(2, 1)
PIK_EXTERN_MEMETIC(1, 1)
#if PIK_INST_D <= 9
PIK_EXTERN_MEMETIC(1, 2)
#endif
#undef PIK_EXTERN_MEMETIC
const RouteOps* PIK_CAT(route_ops_d, PIK_INST_D)() { return make_route_ops<PIK_INST_D>(); }
} // namespace pik
#endif
