// kernels_essgraph.hip -- the kernels of xfh_essential_graph_device (essgraph.hip.h: k_eg_plan_* / _sims / _edges / _vertices / _begin / _fill / _ldlt_diag /
// _ldlt_panel / _subst / _update / _decide / _finish / _header, Optimizer::OptimizeEssentialGraph behind the Sim3 Fuse of LoopClosing).  Its own translation
// unit, as kernels_lba.hip is: the register contract of kernels_match.hip (tests/test_abi_and_host.py) is about the kernels there.
#include "ctx.h"
#include "search_common.hip.h"
#include "essgraph.hip.h"
