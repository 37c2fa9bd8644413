// pik_search_inst.hip -- the restart-search kernels (pik_search.hpp) and their launch for ONE chain length
// (-DPIK_INST_D=<dof>); compiled once per supported length for the flavours fast, exact and strict
// (pick_ik_amd/build.py).  -DPIK_INST_STUB: no kernels for this length (experiment builds).
#ifndef PIK_INST_D
#error "compile with -DPIK_INST_D=<dof>"
#endif
#define PIK_CAT2(a, b) a##b
#define PIK_CAT(a, b) PIK_CAT2(a, b)

#if defined(PIK_INST_STUB)
#include "pik_search_ops.hpp"
namespace pik {
const SearchOps* PIK_CAT(search_ops_d, PIK_INST_D)() { return nullptr; }
} // namespace pik
#else
#include "pik_search.hpp"
namespace pik {
const SearchOps* PIK_CAT(search_ops_d, PIK_INST_D)() { return make_search_ops<PIK_INST_D>(); }
} // namespace pik
#endif
