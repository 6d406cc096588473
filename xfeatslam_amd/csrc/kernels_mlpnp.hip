// kernels_mlpnp.hip -- the kernels of xfh_mlpnp_solve_device (mlpnp.hip.h: k_mlpnp_prepare / _fit / _count / _records / _refine / _decide, MLPnPsolver under
// Tracking::Relocalization's iterate(5) calls).  Its own translation unit, unlike the other solvers: k_mlpnp_fit and k_mlpnp_refine use scratch (1020 and
// 320 bytes per lane, profiles/mlpnp.md), and no kernel of kernels_match.hip may (tests/test_abi_and_host.py::test_search_kernel_register_contract).
#include "ctx.h"
#include "search_common.hip.h"
#include "mlpnp.hip.h"
