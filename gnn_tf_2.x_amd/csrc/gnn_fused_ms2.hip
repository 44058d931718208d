// Split-arithmetic (impl 2) instantiations of the fused iteration kernel for net_state with 2 Dense layers whose last layer has an
// activation of its own (ACTL == GNN_ACTL_FROM_ARGS): one kernel per hidden activation, the last one from GnnFusedArgs::act_last.
#include "gnn_fused_kernel.h"

bool gnn_fused_launch_ms2(int act, int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st)
{
    return gnn_fused_dev::launch_fused<2, true, true>(act, nt, ntl, how, a, grid, lds_bytes, st);
}
