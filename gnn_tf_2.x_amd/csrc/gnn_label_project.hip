// Label projection (gnn_loop_set_label_projection): P = inv . W1_label + b1, once per Loop, for the seeded fused kernels (gnn_fused_ps*.hip).
//
// inv [rows][IW] is the loop-invariant label block [nodes | aggregated nodes | aggregated arcs] of the owned rows, W1_label [IW][32 NT] the
// rows of net_state's first kernel that multiply it (columns past the layer's width zero) followed by one zero row, so that the second
// half of the last K-step of an odd width reads it unguarded, b1 [32 NT] the layer's bias (zero-padded).
// fp32 operands and fp32 accumulation on v_mfma_f32_32x32x2_f32, orientation as the fused kernels' exact layers: P^T[feature][node] =
// W^T . inv^T, so the result arrives in the accumulator-tile order the consumer loads it in (GnnFusedArgs::seed).  k ascending - an MFMA is a
// k-ordered fmaf chain, the K-steps follow each other in one accumulator - no atomics, every element one chain: run-to-run identical bits.
// The bias is added last, to the finished sum, so that an element is within (IW - 1) 2^-24 sum |x w| + half an ulp of the exact value.
#include "gnn_common.h"
#include "gnn_fused.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
constexpr int LP_WAVES = 4;          // waves per workgroup, one 32-row tile each; they share nothing
constexpr int LP_COLS = 64;          // label columns staged per round
constexpr int LP_STRIDE = LP_COLS + 1;      // odd row stride: the column reads of the B operand are conflict-free

// One wave per 32-row tile, all NT feature tiles of it.  Rows past n_rows of the last tile are rows of the padded, zeroed inv: they come out
// as the bias.  Reads: inv rows [32 tile, 32 tile + 32) x columns < IW; wl rows <= IW; writes: the tile's NT x 1024 floats of P.
template <int NT>
__global__ void __launch_bounds__(64 * LP_WAVES) k_label_project(int64_t n_tiles, int IW, const float *inv, const float *wl, const float *bias, float *P)
{
    __shared__ float xs[LP_WAVES][32 * LP_STRIDE];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile = (int64_t)blockIdx.x * LP_WAVES + wave;
    if (tile >= n_tiles) return;                      // wave-uniform; no workgroup barrier anywhere below
    float *X = xs[wave];
    const int node = lane & 31, half = lane >> 5;
    f32x16 acc[NT];
#pragma unroll
    for (int jt = 0; jt < NT; ++jt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[jt][r] = 0.0f;
    const float *src = inv + (size_t)tile * 32 * IW;
    for (int c0 = 0; c0 < IW; c0 += LP_COLS) {
        const int w = IW - c0 < LP_COLS ? IW - c0 : LP_COLS;
        // the tile's columns [c0, c0 + w): lane = column, row by row (256 contiguous bytes per row); zero behind the last column
#pragma unroll 8
        for (int r = 0; r < 32; ++r) X[r * LP_STRIDE + lane] = lane < w ? src[(size_t)r * IW + c0 + lane] : 0.0f;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const int steps = (w + 1) >> 1;
        for (int s = 0; s < steps; ++s) {
            const int k = c0 + 2 * s + half;          // == IW in the last step of an odd width: X holds a zero there, and row IW of wl is zero
            const float b = X[node * LP_STRIDE + 2 * s + half];
            float av[NT];
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) av[jt] = wl[(size_t)k * (32 * NT) + 32 * jt + node];
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) acc[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[jt], b, acc[jt], 0, 0, 0);
        }
        // the K-step loop ends in a branch and hipcc pads no wait states across a basic-block edge (persistent small-graph loop):
        // the 19 of the 16-pass MFMA, as in k_fused_generic - pinned, so that no read of an accumulator is scheduled in front of them
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the next round overwrites the staged columns
    }
    float *dst = P + (size_t)tile * (NT * 1024) + lane * 4;
#pragma unroll
    for (int jt = 0; jt < NT; ++jt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const v4f b = *reinterpret_cast<const v4f *>(bias + 32 * jt + 8 * q + 4 * half);
            v4f o = {acc[jt][4 * q], acc[jt][4 * q + 1], acc[jt][4 * q + 2], acc[jt][4 * q + 3]};
            o = o + b;
            *reinterpret_cast<v4f *>(dst + (jt * 4 + q) * 256) = o;
        }
}

}   // namespace

int gnn_label_project_launch(hipStream_t st, int64_t n_rows, int IW, int nt, const float *inv, const float *wl, const float *bias, float *P)
{
    ARGCHK(n_rows > 0 && IW > 0 && inv && wl && bias && P, "bad arguments");
    const int64_t n_tiles = (n_rows + 31) / 32;
    const unsigned grid = (unsigned)((n_tiles + LP_WAVES - 1) / LP_WAVES);
    switch (nt) {
    case 1: hipLaunchKernelGGL(k_label_project<1>, grid, 64 * LP_WAVES, 0, st, n_tiles, IW, inv, wl, bias, P); break;
    case 2: hipLaunchKernelGGL(k_label_project<2>, grid, 64 * LP_WAVES, 0, st, n_tiles, IW, inv, wl, bias, P); break;
    case 4: hipLaunchKernelGGL(k_label_project<4>, grid, 64 * LP_WAVES, 0, st, n_tiles, IW, inv, wl, bias, P); break;
    default: return gnn_fail(GNN_ERR_UNSUPPORTED, "no label-projection instantiation for %d feature tiles", nt);
    }
    HIPCHK(hipGetLastError());
    return GNN_OK;
}
