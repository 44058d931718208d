// Persistent small-graph loop on 32-node tiles (gnn_small_kernel.h): the instantiations for nets with one activation for all layers.
#include "gnn_small_kernel.h"

bool gnn_small_launch(int layers, int act, int kk0, const GnnFusedArgs &a, const GnnSmallCtl &c, unsigned grid, size_t lds_bytes,
                      hipStream_t st)
{
    using namespace gnn_fused_dev;
    return small_dispatch<GnnSmallKK0>(layers, act, kk0, [&](auto L, auto A, auto K) {
        hipLaunchKernelGGL((k_small_loop<L.value, A.value, K.value>), grid, 64, lds_bytes, st, a, c);
    });
}
