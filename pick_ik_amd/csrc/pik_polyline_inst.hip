// pik_polyline_inst.hip -- the waypoint-list kernels (pik_polyline.hpp) and their launches for ONE chain length
// (-DPIK_INST_D=<dof>); compiled once per supported length for the flavours fast, exact and strict
// (pick_ik_amd/build.py).  -DPIK_INST_STUB: no kernels for this length (experiment builds).
#ifndef PIK_INST_D
#error "compile with -DPIK_INST_D=<dof>"
#endif
#if defined(PIK_INST_STUB)
#include "pik_polyline_ops.hpp"
#else
#include "pik_polyline.hpp"
#endif
namespace pik {
PIK_DEFINE_OPS(PolylineOps, polyline)
} // namespace pik
