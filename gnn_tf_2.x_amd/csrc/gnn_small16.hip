// Persistent small-graph loop on 16-node tiles (gnn_small16_kernel.h): the instantiations for nets with one activation for all layers.
#include "gnn_small16_kernel.h"

bool gnn_small16_launch(int layers, int act, int s0, const GnnFusedArgs &a, const GnnSmallCtl &c, unsigned grid, size_t lds_bytes, hipStream_t st)
{
    using namespace gnn_fused_dev;
    return small_dispatch<GnnSmall16S0>(layers, act, s0, [&](auto L, auto A, auto S) {
        hipLaunchKernelGGL((k_small16<L.value, A.value, S.value>), grid, 64, lds_bytes, st, a, c);
    });
}
