// pik_restart_inst.hip -- the restart launcher (pik_restart.hpp) for ONE chain length (-DPIK_INST_D=<dof>); compiled
// once per supported length with the flags of the flavour whose memetic kernels it launches (pick_ik_amd/build.py).
// -DPIK_INST_STUB: nothing for this length (experiment builds).
//
// The memetic kernels are NOT compiled here: every variant the launcher names -- the forms for several tip frames
// included -- is declared as an explicit instantiation that lives elsewhere, in the flavour's pik_inst object of this
// length (pik_dofs.hpp has the list).  This object holds the prepare and fold kernels and undefined references to the
// memetic kernels' host stubs.
#ifndef PIK_INST_D
#error "compile with -DPIK_INST_D=<dof>"
#endif
#if defined(PIK_INST_STUB)
#include "pik_restart_ops.hpp"
#else
#include "pik_restart.hpp"
#endif
namespace pik {
#if !defined(PIK_INST_STUB)
PIK_MEMETIC_ALL(PIK_EXTERN_MEMETIC)
#endif
PIK_DEFINE_OPS(RestartOps, restart)
} // namespace pik
