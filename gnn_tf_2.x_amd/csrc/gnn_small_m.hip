// Persistent small-graph loop on 32-node tiles (gnn_small_kernel.h): the instantiations for two- and three-layer nets whose last layer has an
// activation of its own (a.act_last), one kernel per hidden activation.
#include "gnn_small_kernel.h"

bool gnn_small_launch_mixed(int layers, int act, int kk0, const GnnFusedArgs &a, const GnnSmallCtl &c, unsigned grid, size_t lds_bytes,
                            hipStream_t st)
{
    using namespace gnn_fused_dev;
    if (layers < 2) return false;
    return small_dispatch<GnnSmallKK0>(layers, act, kk0, [&](auto L, auto A, auto K) {
        if constexpr (L.value >= 2) hipLaunchKernelGGL((k_small_loop<L.value, A.value, K.value, GNN_ACTL_FROM_ARGS>), grid, 64, lds_bytes, st, a, c);
    });
}
