// kernels_lba.hip -- the kernels of xfh_local_ba_device (lba.hip.h: k_lba_plan_* / _linearize / _point_build / _begin / _schur / _solve / _update / _decide /
// _finish / _header, Optimizer::LocalBundleAdjustment behind the triangulate -> fuse chain of LocalMapping).  Its own translation unit, as kernels_mlpnp.hip
// is: the register contract of kernels_match.hip (tests/test_abi_and_host.py) is about the kernels there.
#include "ctx.h"
#include "search_common.hip.h"
#include "lba.hip.h"
