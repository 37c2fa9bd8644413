// pik_path_inst.hip -- the waypoint-path kernels (pik_path.hpp) and their launch for ONE chain length
// (-DPIK_INST_D=<dof>); compiled once per supported length for the flavours fast, exact and strict
// (pick_ik_amd/build.py).  -DPIK_INST_STUB: no kernels for this length (experiment builds).
#ifndef PIK_INST_D
#error "compile with -DPIK_INST_D=<dof>"
#endif
#if defined(PIK_INST_STUB)
#include "pik_path_ops.hpp"
#else
#include "pik_path.hpp"
#endif
namespace pik {
PIK_DEFINE_OPS(PathOps, path)
} // namespace pik
