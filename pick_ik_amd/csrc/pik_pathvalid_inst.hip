// pik_pathvalid_inst.hip -- the validity step of the path entry points (pik_pathvalid.hpp) and its launches for ONE
// chain length (-DPIK_INST_D=<dof>); compiled once per supported length for the flavour exact in the product library
// and strict in the verification library (pick_ik_amd/build.py), as pik_validity_inst.hip: one arithmetic serves every
// handle.  -DPIK_INST_STUB: no kernels for this length (experiment builds).
#ifndef PIK_INST_D
#error "compile with -DPIK_INST_D=<dof>"
#endif
#if defined(PIK_INST_STUB)
#include "pik_math.hpp"
#include "pik_pathvalid_ops.hpp"
#else
#include "pik_pathvalid.hpp"
#endif
namespace pik {
PIK_DEFINE_OPS(PathValidOps, pathvalid)
} // namespace pik
