// pik_validity_inst.hip -- the sphere validity kernels (pik_validity.hpp) and their launch for ONE chain length
// (-DPIK_INST_D=<dof>); compiled once per supported length for the flavour exact in the product library and strict in
// the verification library (pick_ik_amd/build.py): one arithmetic serves every handle.  -DPIK_INST_STUB: no kernels
// for this length (experiment builds).
#ifndef PIK_INST_D
#error "compile with -DPIK_INST_D=<dof>"
#endif
#if defined(PIK_INST_STUB)
#include "pik_math.hpp"
#include "pik_validity_ops.hpp"
#else
#include "pik_validity.hpp"
#endif
namespace pik {
PIK_DEFINE_OPS(ValidityOps, validity)
} // namespace pik
