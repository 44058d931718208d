// Persistent small-graph loop on 16-node tiles, hidden layers up to 64 wide (gnn_small16_kernel.h, WIDE): the instantiations for two- and
// three-layer nets whose last layer has an activation of its own (a.act_last), one kernel per hidden activation.
#include "gnn_small16_kernel.h"

bool gnn_small16w_launch_mixed(int layers, int act, int s0, const GnnFusedArgs &a, const GnnSmallCtl &c, unsigned grid, size_t lds_bytes, hipStream_t st)
{
    using namespace gnn_fused_dev;
    if (layers < 2) return false;
    return small_dispatch<GnnSmall16S0>(layers, act, s0, [&](auto L, auto A, auto S) {
        if constexpr (L.value >= 2) hipLaunchKernelGGL((k_small16<L.value, A.value, S.value, GNN_ACTL_FROM_ARGS, true>), grid, 64, lds_bytes, st, a, c);
    });
}
