// pik_route_inst.hip -- the routed launcher (pik_route.hpp) for ONE chain length (-DPIK_INST_D=<dof>); compiled once
// per supported length with the flags of the flavour whose memetic kernels it launches (pick_ik_amd/build.py).
// -DPIK_INST_STUB: nothing for this length (experiment builds).
//
// The memetic kernels are NOT compiled here: every variant the shared launch code names (pik_launch.hpp
// with_variant_kernel: the forms for several tip frames too, which this launcher never enqueues) is declared as an
// explicit instantiation that lives elsewhere -- the flavour's pik_inst object of this length, which launch_solve
// instantiates them in (pik_dofs.hpp has the list).  This object holds the router kernel and undefined references to
// the kernels' host stubs.
#ifndef PIK_INST_D
#error "compile with -DPIK_INST_D=<dof>"
#endif
#if defined(PIK_INST_STUB)
#include "pik_route_ops.hpp"
#else
#include "pik_route.hpp"
#endif
namespace pik {
#if !defined(PIK_INST_STUB)
PIK_MEMETIC_ALL(PIK_EXTERN_MEMETIC)
#endif
PIK_DEFINE_OPS(RouteOps, route)
} // namespace pik
