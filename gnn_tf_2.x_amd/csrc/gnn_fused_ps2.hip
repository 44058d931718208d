// Seeded split-arithmetic (impl 2) instantiations of the fused iteration kernel for net_state with 2 Dense layers: the label projection
// (gnn_loop_set_label_projection) - layer 0 over [state | aggregated state], its accumulators started from GnnFusedArgs::seed.  One kernel per
// hidden activation, the last layer's activation from GnnFusedArgs::act_last.
#include "gnn_fused_kernel.h"

bool gnn_fused_launch_ps2(int act, int nt, int ntl, const GnnFusedLaunch &how, const GnnFusedArgs &a, unsigned grid, size_t lds_bytes, hipStream_t st)
{
    return gnn_fused_dev::launch_fused_seeded<2>(act, nt, ntl, how, a, grid, lds_bytes, st);
}
