// gfx950 engine for the GNN fixed-point loop: errors, allocation, the per-op ("unfused") primitive kernels with their launchers, and the
// MLP handle and the RCCL table.  The graph handle is in gnn_graph.hip, communicators and the exchange layouts in gnn_comm.hip, the Loop in gnn_loop.hip.
//
// Every kernel here evaluates floating point in the order pinned by oracle/gnn_oracle.c (sequential fmaf chains,
// unfused BatchNormalization and norms), so results are bit-identical to that restatement.  The fused fast path is in
// gnn_fused.hip; these kernels are its fallback for shapes it does not cover and the GPU-side cross-check of it.
//
// Reference call sites replaced (paths relative to the reference root):
//   k_spmm        tf.sparse.sparse_dense_matmul   GNN/GNN.py:234, :259, :263
//   k_dense       Keras Dense + activation        GNN/MLP.py:62 (built), GNN/GNN.py:240, :279 (called)
//   k_softmax_bn  softmax activation + BatchNormalization (MLP.py:63)
//   k_check       condition()                     GNN/GNN.py:202-220
#include <dlfcn.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gnn_engine.h"

// ---------------------------------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";

int gnn_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

extern "C" const char *gnn_last_error(void) { return g_err; }
extern "C" int gnn_version(void) { return 1; }

extern "C" int gnn_device_count(int *count)
{
    ARGCHK(count, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { (void)hipGetLastError(); n = 0; }
    *count = n;
    return GNN_OK;
}

extern "C" int gnn_device_synchronize(int device)
{
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    return GNN_OK;
}

bool gnn_poison_enabled()
{
#ifdef GNN_DIAG
    static const bool on = [] {
        const bool v = getenv("GNN_POISON") != nullptr && atoi(getenv("GNN_POISON")) != 0;
        if (v) fprintf(stderr, "libgnn_hip (diagnostic build): GNN_POISON=1 - every device allocation and the fused kernels' LDS are filled with NaN before use\n");
        return v;
    }();
    return on;
#else
    return false;
#endif
}

hipError_t gnn_dev_malloc(void **p, size_t bytes)
{
    hipError_t e = hipMalloc(p, bytes);
#ifdef GNN_DIAG
    if (e == hipSuccess && gnn_poison_enabled()) {
        // null-stream fill + device-wide wait: complete before ANY stream of the engine can touch the block (diagnostic build only)
        e = hipMemset(*p, 0xFF, bytes);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
#endif
    return e;
}

// ---------------------------------------------------------------------------------------------------------------------
// RCCL (loaded lazily so that the library itself has no link-time dependency on it)
// ---------------------------------------------------------------------------------------------------------------------
Rccl g_rccl;

int rccl_load()
{
    if (g_rccl.h) return GNN_OK;
    void *h = nullptr;
    // GNN_RCCL_LIBRARY=<path>: the collectives library to load instead of the system's RCCL (another RCCL build; the multi-process tests
    // point it at their stand-in transport, tests/mock_rccl, to run several ranks on one GPU).  No fallback when it is set.
    if (const char *path = getenv("GNN_RCCL_LIBRARY")) {
        h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
        if (!h) return gnn_fail(GNN_ERR_COMM, "cannot load GNN_RCCL_LIBRARY=%s: %s", path, dlerror());
    }
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) return gnn_fail(GNN_ERR_COMM, "cannot load librccl: %s", dlerror());
#define SYM(field, name)                                                         \
    *(void **)(&g_rccl.field) = dlsym(h, name);                                  \
    if (!g_rccl.field) return gnn_fail(GNN_ERR_COMM, "librccl lacks %s", name);
    SYM(GetUniqueId, "ncclGetUniqueId") SYM(CommInitRank, "ncclCommInitRank") SYM(CommDestroy, "ncclCommDestroy")
    SYM(AllGather, "ncclAllGather") SYM(AllReduce, "ncclAllReduce") SYM(GroupStart, "ncclGroupStart")
    SYM(GroupEnd, "ncclGroupEnd") SYM(GetErrorString, "ncclGetErrorString") SYM(Send, "ncclSend") SYM(Recv, "ncclRecv")
#undef SYM
    g_rccl.h = h;
    return GNN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------

// out[r, :] = sum over the stored entries e of row r, in order, of w[e] * X[src(e), :]     (fmaf chain)
// lpr lanes (power of two <= 64) cooperate on a row, each owning VEC consecutive columns per chunk.
template <int VEC, bool INDEXED, int U = 4>
__global__ void __launch_bounds__(256) k_spmm(int64_t n_rows, const int32_t *__restrict__ indptr,
                                              const int32_t *__restrict__ idx, const float *__restrict__ w,
                                              const float *__restrict__ X, int width, int64_t ldx,
                                              float *__restrict__ out, int64_t ldo, int lpr, const int *gate, int world)
{
    if (!gnn_gate_open_block(gate, world)) return;
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t rows_per_pass = ((int64_t)gridDim.x * blockDim.x) / lpr;
    const int lane = (int)(gtid % lpr);
    for (int64_t row = gtid / lpr; row < n_rows; row += rows_per_pass) {
        const int beg = indptr[row], end = indptr[row + 1];
        for (int c0 = lane * VEC; c0 < width; c0 += lpr * VEC) {
            float acc[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;
            if constexpr (U == 4) {
                int e = beg;
                for (; e + 4 <= end; e += 4) {
                    float we[4];
                    float xv[4][VEC];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        we[u] = w[e + u];
                        const int64_t s = INDEXED ? (int64_t)idx[e + u] : (int64_t)(e + u);
                        const float *xp = X + s * ldx + c0;
                        if constexpr (VEC == 4) {
                            const float4 t = *reinterpret_cast<const float4 *>(xp);
                            xv[u][0] = t.x; xv[u][1] = t.y; xv[u][2] = t.z; xv[u][3] = t.w;
                        } else {
                            xv[u][0] = xp[0];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int v = 0; v < VEC; ++v) acc[v] = __builtin_fmaf(we[u], xv[u][v], acc[v]);
                }
                for (; e < end; ++e) {
                    const float we = w[e];
                    const int64_t s = INDEXED ? (int64_t)idx[e] : (int64_t)e;
                    const float *xp = X + s * ldx + c0;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] = __builtin_fmaf(we, xp[v], acc[v]);
                }
            } else {
                // narrow slices (feature-sliced exchange, 8 / 16 columns per rank): U entries requested together, the tail as a masked batch
                // (clamped to a real entry, result unused) instead of one dependent round trip per entry
                for (int e = beg; e < end; e += U) {
                    float we[U];
                    float xv[U][VEC];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int ee = e + u < end ? e + u : e;
                        we[u] = w[ee];
                        const int64_t s = INDEXED ? (int64_t)idx[ee] : (int64_t)ee;
                        const float *xp = X + s * ldx + c0;
                        if constexpr (VEC == 4) {
                            const float4 t = *reinterpret_cast<const float4 *>(xp);
                            xv[u][0] = t.x; xv[u][1] = t.y; xv[u][2] = t.z; xv[u][3] = t.w;
                        } else {
                            xv[u][0] = xp[0];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (e + u < end) {
#pragma unroll
                            for (int v = 0; v < VEC; ++v) acc[v] = __builtin_fmaf(we[u], xv[u][v], acc[v]);
                        }
                }
            }
            float *op = out + row * ldo + c0;
#pragma unroll
            for (int v = 0; v < VEC; ++v) op[v] = acc[v];
        }
    }
}

// Y[i, j] = epilogue( sum_k fmaf(X[i,k], W[k,j]) + b[j] );  R rows per block staged in LDS, one thread per column.
template <int R>
__global__ void __launch_bounds__(256) k_dense(int64_t n, int n_in, int n_in_pad, int n_out, const float *__restrict__ X,
                                               int64_t ldx, const float *__restrict__ W, const float *__restrict__ b,
                                               int act, const float *__restrict__ bn_scale,
                                               const float *__restrict__ bn_shift, float *__restrict__ Y, int64_t ldy,
                                               const int *gate, int world)
{
    extern __shared__ __attribute__((aligned(16))) float xs[];
    if (!gnn_gate_open_block(gate, world)) return;
    const int64_t i0 = (int64_t)blockIdx.x * R;
    for (int t = threadIdx.x; t < R * n_in_pad; t += blockDim.x) {
        const int r = t / n_in_pad, k = t - r * n_in_pad;
        xs[t] = (k < n_in && i0 + r < n) ? X[(i0 + r) * ldx + k] : 0.0f;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < n_out; j += blockDim.x) {
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.0f;
        int k = 0;
        for (; k + 4 <= n_in; k += 4) {
            const float w0 = W[(size_t)(k + 0) * n_out + j], w1 = W[(size_t)(k + 1) * n_out + j];
            const float w2 = W[(size_t)(k + 2) * n_out + j], w3 = W[(size_t)(k + 3) * n_out + j];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float4 x = *reinterpret_cast<const float4 *>(&xs[r * n_in_pad + k]);
                acc[r] = __builtin_fmaf(x.x, w0, acc[r]);
                acc[r] = __builtin_fmaf(x.y, w1, acc[r]);
                acc[r] = __builtin_fmaf(x.z, w2, acc[r]);
                acc[r] = __builtin_fmaf(x.w, w3, acc[r]);
            }
        }
        for (; k < n_in; ++k) {
            const float wk = W[(size_t)k * n_out + j];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = __builtin_fmaf(xs[r * n_in_pad + k], wk, acc[r]);
        }
        const float bj = b[j];
        const float sc = bn_scale ? bn_scale[j] : 1.0f, sh = bn_shift ? bn_shift[j] : 0.0f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (i0 + r >= n) break;
            float v = acc[r] + bj;
            if (act != GNN_ACT_SOFTMAX) {
                v = gnn_act(v, act);
                if (bn_scale) { float t = v * sc; v = t + sh; }
            }
            Y[(i0 + r) * ldy + j] = v;
        }
    }
}

// in-place row softmax (+ trailing BatchNormalization), one thread per row, sequential in j like the oracle
__global__ void k_softmax_bn(int64_t n, int n_out, float *Y, int64_t ldy, const float *bn_scale, const float *bn_shift,
                             const int *gate, int world)
{
    if (!gnn_gate_open_block(gate, world)) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float *y = Y + i * ldy;
    float m = y[0];
    for (int j = 1; j < n_out; ++j) m = y[j] > m ? y[j] : m;
    float s = 0.0f;
    for (int j = 0; j < n_out; ++j) { const float e = gnn_expf(y[j] - m); y[j] = e; s = s + e; }
    for (int j = 0; j < n_out; ++j) {
        float v = __fdiv_rn(y[j], s);
        if (bn_scale) { float t = v * bn_scale[j]; v = t + bn_shift[j]; }
        y[j] = v;
    }
}

// condition(): per owned node sqrt(sum (s-so)^2) > thr * sqrt(sum so^2); OR into the rank's flag.  so == nullptr: ones.
// One thread per row keeps the oracle's ascending-feature summation order; the rows of a block are staged through LDS in
// chunks of 32 features so that HBM is read in full 128-byte segments.
__global__ void __launch_bounds__(256) k_check(int64_t n_rows, int d, const float *__restrict__ s,
                                               const float *__restrict__ so, float thr, int *flag_out, const int *gate,
                                               int world)
{
    extern __shared__ float chk_sh[];                      // ts [256 * 33] (+ to [256 * 33] iff so)
    float *ts = chk_sh, *to = chk_sh + 256 * 33;
    if (!gnn_gate_open_block(gate, world)) return;
    const int64_t r0 = (int64_t)blockIdx.x * 256;
    const int64_t i = r0 + threadIdx.x;
    float dist = 0.0f, nrm = 0.0f;
    const bool v4 = (d & 3) == 0;
    for (int c0 = 0; c0 < d; c0 += 32) {
        const int cw = (d - c0) < 32 ? (d - c0) : 32;
        __syncthreads();
        if (v4) {
#pragma unroll
            for (int t = threadIdx.x; t < 256 * 8; t += 256) {
                const int r = t >> 3, c = (t & 7) * 4;
                if (c < cw && r0 + r < n_rows) {
                    const float4 a = *reinterpret_cast<const float4 *>(s + (r0 + r) * d + c0 + c);
                    float *p = ts + r * 33 + c;
                    p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w;
                    if (so) {
                        const float4 b = *reinterpret_cast<const float4 *>(so + (r0 + r) * d + c0 + c);
                        float *q = to + r * 33 + c;
                        q[0] = b.x; q[1] = b.y; q[2] = b.z; q[3] = b.w;
                    }
                }
            }
        } else {
            for (int t = threadIdx.x; t < 256 * 32; t += 256) {
                const int r = t >> 5, c = t & 31;
                if (c < cw && r0 + r < n_rows) {
                    ts[r * 33 + c] = s[(r0 + r) * d + c0 + c];
                    if (so) to[r * 33 + c] = so[(r0 + r) * d + c0 + c];
                }
            }
        }
        __syncthreads();
        if (i < n_rows)
            for (int c = 0; c < cw; ++c) {
                const float o = so ? to[threadIdx.x * 33 + c] : 1.0f;
                const float df = ts[threadIdx.x * 33 + c] - o;
                const float dd = df * df;
                dist = dist + dd;
                const float oo = o * o;
                nrm = nrm + oo;
            }
    }
    int f = 0;
    if (i < n_rows) {
        const float lhs = sqrtf(dist);
        const float rn = sqrtf(nrm);
        const float rhs = thr * rn;
        f = lhs > rhs;
    }
    if (__any(f) && (threadIdx.x & 63) == 0) gnn_flag_raise(flag_out);
}

// The first condition of a Loop (state vs ones, GNN.py:266, :271) as one streamed pass: k_check's sums, rows and flag word, another
// staging.  A one-wave block takes 64 consecutive rows, i.e. one contiguous 256 d bytes of the table, reads them in 16-byte pieces (all of
// a lane's pieces in flight at once, no barrier between chunks of features) and stores them to LDS in 16-byte pieces; lane r then runs
// row r's sums alone, in ascending feature order.  ld: row stride of the tile - d itself (the tile is then the flat image of the rows) or,
// where d / 4 is even, d + 4, which spreads the 16-byte row reads of 16 lanes over all banks.
#define GNN_CHECK1_MAX_D 124      // 64 rows of at most 128 floats: 32 KB of LDS per wave
__global__ void __launch_bounds__(64) k_check_first(int64_t n_rows, int d, int ld, const float *__restrict__ s, float thr, int *flag_out)
{
    extern __shared__ float chk1_sh[];                     // [64, ld]
    const int lane = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    const int rows = n_rows - r0 < 64 ? (int)(n_rows - r0) : 64;
    const float *src = s + r0 * d;                         // 16-byte aligned: s is (launch_check_first), and 64 rows are a multiple of 16 bytes
    const int n = rows * d, np = n >> 2;
    if (ld == d) {
#pragma unroll 8
        for (int p = lane; p < np; p += 64) {
            const float4 v = reinterpret_cast<const float4 *>(src)[p];
            reinterpret_cast<float4 *>(chk1_sh)[p] = v;
        }
        for (int t = 4 * np + lane; t < n; t += 64) chk1_sh[t] = src[t];
    } else {                                               // (d is a multiple of 4 here)
        const int q = d >> 2, dr = 64 / q, dc = 64 - dr * q;
        int r = lane / q, c = lane - r * q;
#pragma unroll 8
        for (int p = lane; p < np; p += 64) {
            const float4 v = reinterpret_cast<const float4 *>(src)[p];
            *reinterpret_cast<float4 *>(chk1_sh + r * ld + 4 * c) = v;
            r += dr; c += dc;
            if (c >= q) { c -= q; ++r; }
        }
    }
    __syncthreads();
    float dist = 0.0f, nrm = 0.0f;
    int f = 0;
    if (lane < rows) {
        const float *x = chk1_sh + lane * ld;
        const float o = 1.0f;
        if ((d & 3) == 0) {
            for (int c = 0; c < d; c += 4) {
                const float4 v = *reinterpret_cast<const float4 *>(x + c);
                const float xs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float df = xs[u] - o;
                    const float dd = df * df;
                    dist = dist + dd;
                    const float oo = o * o;
                    nrm = nrm + oo;
                }
            }
        } else {
            for (int c = 0; c < d; ++c) {
                const float df = x[c] - o;
                const float dd = df * df;
                dist = dist + dd;
                const float oo = o * o;
                nrm = nrm + oo;
            }
        }
        const float lhs = sqrtf(dist);
        const float rn = sqrtf(nrm);
        const float rhs = thr * rn;
        f = lhs > rhs;
    }
    if (__any(f) && lane == 0) gnn_flag_raise(flag_out);
}

// dst[r, 0:w) = src[r, 0:w) for r < n_rows (strided rows on both sides).  Own kernel instead of hipMemcpy2DAsync: the
// runtime's 2-D device-to-device copy was the only HIP call of the per-op path that the fused path never makes, and a
// profiled run (rocprofv3 --kernel-trace) of the per-op path died inside the runtime on its first use.
__global__ void k_copy_cols(int64_t n_rows, int w, const float *__restrict__ src, int64_t lds_, float *__restrict__ dst, int64_t ldd,
                            const int *gate, int world)
{
    if (!gnn_gate_open_block(gate, world)) return;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rows * w) return;
    const int64_t r = t / w;
    const int c = (int)(t - r * w);
    dst[r * ldd + c] = src[r * lds_ + c];
}

__global__ void k_fill(int64_t count, float v, float *out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < count) out[t] = v;
}

// ---------------------------------------------------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------------------------------------------------
int gnn_launch_spmm(hipStream_t st, int64_t n_rows, const int32_t *indptr, const int32_t *idx, const float *w,
                       const float *X, int width, int64_t ldx, float *out, int64_t ldo, const int *gate, int world)
{
    if (n_rows == 0 || width == 0) return GNN_OK;
    const bool vec4 = (width % 4 == 0) && (ldx % 4 == 0) && (((uintptr_t)X & 15) == 0);
    const int vec = vec4 ? 4 : 1;
    int lpr = 1;
    while (lpr * vec < width && lpr < 64) lpr <<= 1;
    const int64_t threads = n_rows * lpr;
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv(threads, 256), 256 * 32);
    const bool indexed = idx != nullptr;
    // (A one-lane-per-row form with eight entries in flight for the 8-column slices of the feature-sliced exchange was measured in round 3:
    //  257 us against 203 us for this kernel's two lanes per row - profiles/r03_exchange_layouts.txt - and removed.  Round 5: see below.)
    // narrow column slices (feature-sliced exchange at 4 / 8 ranks: 16 / 8 columns of all nodes): eight entries in flight per lane and the tail as a
    // masked batch - 183 against 204 us per rank and iteration at P = 8 (profiles/r05_slice_counters.txt).  The kernel is bound by the L2's miss path:
    // 11.4 M 64-byte fetches per launch for 10 M random 32-byte row pieces out of a 32 MB table that no XCD's 4 MiB L2 can hold (hit rate 23 %).
    if (vec4 && indexed && width <= 16) hipLaunchKernelGGL((k_spmm<4, true, 8>), grid, 256, 0, st, n_rows, indptr, idx, w, X, width, ldx, out, ldo, lpr, gate, world);
    else if (vec4 && indexed) hipLaunchKernelGGL((k_spmm<4, true>), grid, 256, 0, st, n_rows, indptr, idx, w, X, width, ldx, out, ldo, lpr, gate, world);
    else if (vec4) hipLaunchKernelGGL((k_spmm<4, false>), grid, 256, 0, st, n_rows, indptr, idx, w, X, width, ldx, out, ldo, lpr, gate, world);
    else if (indexed) hipLaunchKernelGGL((k_spmm<1, true>), grid, 256, 0, st, n_rows, indptr, idx, w, X, width, ldx, out, ldo, lpr, gate, world);
    else hipLaunchKernelGGL((k_spmm<1, false>), grid, 256, 0, st, n_rows, indptr, idx, w, X, width, ldx, out, ldo, lpr, gate, world);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

// one Dense layer without activation epilogue choices hidden: Y = act(X . W + b) [then x * scale + shift]; used by the
// training path (gnn_train.hip) for z = h . W + b and d h = d z . W^T
int gnn_launch_dense(hipStream_t st, int64_t n, int n_in, int n_out, const float *X, int64_t ldx, const float *W, const float *b,
                     int act, float *Y, int64_t ldy)
{
    if (n == 0) return GNN_OK;
    constexpr int R = 8;
    const int n_in_pad = (n_in + 3) & ~3;
    const size_t lds = sizeof(float) * R * n_in_pad;
    if (lds > 64 * 1024) return gnn_fail(GNN_ERR_UNSUPPORTED, "layer input width %d too large", n_in);
    if (act == GNN_ACT_SOFTMAX) return gnn_fail(GNN_ERR_ARG, "gnn_launch_dense: softmax is applied by the caller");
    const int threads = std::min(256, ((n_out + 63) / 64) * 64);
    hipLaunchKernelGGL((k_dense<R>), cdiv(n, R), threads, lds, st, n, n_in, n_in_pad, n_out, X, ldx, W, b, act, (const float *)nullptr,
                       (const float *)nullptr, Y, ldy, (const int *)nullptr, 1);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

int launch_check(hipStream_t st, int64_t n_rows, int d, const float *s, const float *so, float thr, int *flag_out,
                        const int *gate, int world)
{
    if (n_rows == 0) return GNN_OK;
    static bool lds_raised[64] = {false};      // two staged tiles are 66 KB of dynamic LDS
    HIPCHK(gnn_raise_dynamic_lds(reinterpret_cast<const void *>(k_check), 2 * 256 * 33 * 4, lds_raised));
    hipLaunchKernelGGL(k_check, cdiv(n_rows, 256), 256, sizeof(float) * 256 * 33 * (so ? 2 : 1), st, n_rows, d, s, so, thr, flag_out, gate, world);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

// the first condition of an inference Loop (against ones): the streamed form where a wave's 64 rows fit its LDS tile, k_check otherwise
int launch_check_first(hipStream_t st, int64_t n_rows, int d, const float *s, float thr, int *flag_out)
{
    if (n_rows == 0) return GNN_OK;
    if (d > GNN_CHECK1_MAX_D || ((uintptr_t)s & 15) != 0) return launch_check(st, n_rows, d, s, nullptr, thr, flag_out, nullptr, 1);
    const int ld = ((d & 3) == 0 && ((d >> 2) & 1) == 0) ? d + 4 : d;
    hipLaunchKernelGGL(k_check_first, cdiv(n_rows, 64), 64, sizeof(float) * 64 * ld, st, n_rows, d, ld, s, thr, flag_out);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

int gnn_launch_check(hipStream_t st, int64_t n_rows, int d, const float *s, const float *so, float thr, int *flag_rank_base)
{
    return launch_check(st, n_rows, d, s, so, thr, flag_rank_base, nullptr, 1);
}

// Sequential forward on device buffers: X[n, dims[0]] (ldx) -> Y[n, dims.back()] (ldy); t0/t1: [n, max hidden width]
int launch_mlp(hipStream_t st, const gnn_mlp *m, int64_t n, const float *X, int64_t ldx, float *Y, int64_t ldy,
                      float *t0, float *t1, const int *gate, int world)
{
    if (n == 0) return GNN_OK;
    const float *in = X;
    int64_t ldin = ldx;
    constexpr int R = 8;
    for (int l = 0; l < m->n_layers; ++l) {
        const bool last = l == m->n_layers - 1;
        float *out = last ? Y : ((l & 1) ? t1 : t0);
        const int64_t ldo = last ? ldy : m->dims[l + 1];
        const int n_in = m->dims[l], n_out = m->dims[l + 1], act = m->acts[l];
        const int n_in_pad = (n_in + 3) & ~3;
        const size_t lds = sizeof(float) * R * n_in_pad;
        if (lds > 64 * 1024) return gnn_fail(GNN_ERR_UNSUPPORTED, "layer input width %d too large", n_in);
        const int threads = std::min(256, ((n_out + 63) / 64) * 64);
        const float *sc = (last && m->has_bn) ? m->bn_scale : nullptr, *sh = (last && m->has_bn) ? m->bn_shift : nullptr;
        hipLaunchKernelGGL((k_dense<R>), cdiv(n, R), threads, lds, st, n, n_in, n_in_pad, n_out, in, ldin, m->W[l], m->b[l],
                           act, sc, sh, out, ldo, gate, world);
        HIPCHK(hipGetLastError());
        if (act == GNN_ACT_SOFTMAX) {
            hipLaunchKernelGGL(k_softmax_bn, cdiv(n, 256), 256, 0, st, n, n_out, out, ldo, sc, sh, gate, world);
            HIPCHK(hipGetLastError());
        }
        in = out;
        ldin = ldo;
    }
    return GNN_OK;
}

int gnn_launch_copy_cols(hipStream_t st, int64_t n_rows, int w, const float *src, int64_t lds_, float *dst, int64_t ldd, const int *gate, int world)
{
    if (n_rows == 0 || w == 0) return GNN_OK;
    hipLaunchKernelGGL(k_copy_cols, cdiv(n_rows * w, 256), 256, 0, st, n_rows, w, src, lds_, dst, ldd, gate, world);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// MLP
// ---------------------------------------------------------------------------------------------------------------------
__global__ void k_bn_inference_form(int f, float eps, const float *raw, float *scale, float *shift)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= f) return;
    // same expression order as oracle/gnn_oracle.c:orc_batchnorm.  sqrtf and operator/ are correctly rounded on the device;
    // __fsqrt_rn is NOT (tools/sqrt_check.hip: 16 % of 4 M inputs differ from the host's sqrtf by one ulp), so it is not used anywhere.
    const float g = raw[j], be = raw[f + j], mu = raw[2 * f + j], var = raw[3 * f + j];
    const float sc = (1.0f / sqrtf(var + eps)) * g;
    const float t = mu * sc;
    scale[j] = sc;
    shift[j] = be - t;
}

// scale / shift of the inference form from the raw BatchNormalization arrays on the device (after an upload or an optimizer step)
int gnn_mlp_refresh_bn(gnn_mlp *m, hipStream_t st)
{
    if (!m->has_bn) return GNN_OK;
    const int f = m->dims.back();
    hipLaunchKernelGGL(k_bn_inference_form, cdiv(f, 64), 64, 0, st, f, m->eps, m->bn_raw, m->bn_scale, m->bn_shift);
    HIPCHK(hipGetLastError());
    return GNN_OK;
}

static int mlp_upload(gnn_mlp *m, const float *const *W, const float *const *b, const float *bn)
{
    // one staging copy of the whole slab: a single transfer instead of two per layer
    std::vector<float> stage(m->slab_floats, 0.0f);
    for (int l = 0; l < m->n_layers; ++l) {
        ARGCHK(W[l] && b[l], "W[%d]/b[%d] is NULL", l, l);
        memcpy(stage.data() + (m->W[l] - m->slab), W[l], sizeof(float) * (size_t)m->dims[l] * m->dims[l + 1]);
        memcpy(stage.data() + (m->b[l] - m->slab), b[l], sizeof(float) * (size_t)m->dims[l + 1]);
    }
    HIPCHK(hipMemcpy(m->slab, stage.data(), sizeof(float) * m->slab_floats, hipMemcpyHostToDevice));
    if (m->has_bn) {
        ARGCHK(bn, "this MLP ends with BatchNormalization: bn is required");
        const int f = m->dims.back();
        HIPCHK(hipMemcpy(m->bn_raw, bn, sizeof(float) * 4 * f, hipMemcpyHostToDevice));
        int rc = gnn_mlp_refresh_bn(m, nullptr);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(nullptr));
    }
    m->version++;
    m->pack_dirty = true;       // packed images of the fused kernel: rebuilt lazily (gnn_loop_decide_form)
    return GNN_OK;
}

extern "C" int gnn_mlp_create(int n_layers, const int32_t *dims, const int32_t *acts, const float *const *W,
                              const float *const *b, const float *bn, float bn_eps, int device, gnn_mlp **out)
{
    ARGCHK(out, "out is NULL");
    *out = nullptr;
    ARGCHK(n_layers >= 1 && n_layers <= 16 && dims && acts && W && b, "bad MLP description");
    for (int l = 0; l <= n_layers; ++l) ARGCHK(dims[l] > 0 && dims[l] <= 8192, "dims[%d]=%d", l, dims[l]);
    for (int l = 0; l < n_layers; ++l) {
        ARGCHK(acts[l] >= GNN_ACT_LINEAR && acts[l] <= GNN_ACT_SOFTMAX, "unknown activation code %d", acts[l]);
        ARGCHK(acts[l] != GNN_ACT_SOFTMAX || dims[l + 1] <= 1024, "softmax width %d too large", dims[l + 1]);
    }
    HIPCHK(hipSetDevice(device));
    gnn_mlp *m = new gnn_mlp();
    m->device = device; m->n_layers = n_layers; m->eps = bn_eps; m->has_bn = bn != nullptr;
    m->dims.assign(dims, dims + n_layers + 1);
    m->acts.assign(acts, acts + n_layers);
    m->W.assign(n_layers, nullptr);
    m->b.assign(n_layers, nullptr);
    int rc = 0;
    auto pad = [](size_t n) { return (n + 63) & ~(size_t)63; };
    size_t off = 0;
    for (int l = 0; l < n_layers; ++l) off += pad((size_t)dims[l] * dims[l + 1]) + pad((size_t)dims[l + 1]);
    m->slab_floats = off;
    rc = dev_alloc(&m->slab, off);
    off = 0;
    for (int l = 0; l < n_layers && !rc; ++l) {
        m->W[l] = m->slab + off; off += pad((size_t)dims[l] * dims[l + 1]);
        m->b[l] = m->slab + off; off += pad((size_t)dims[l + 1]);
    }
    if (!rc && m->has_bn) {
        rc = dev_alloc(&m->bn_scale, (size_t)dims[n_layers]);
        if (!rc) rc = dev_alloc(&m->bn_shift, (size_t)dims[n_layers]);
        if (!rc) rc = dev_alloc(&m->bn_raw, (size_t)4 * dims[n_layers]);
    }
    if (!rc) rc = mlp_upload(m, W, b, bn);
    if (rc) { gnn_mlp_destroy(m); return rc; }
    *out = m;
    return GNN_OK;
}

extern "C" int gnn_mlp_set_weights(gnn_mlp *m, const float *const *W, const float *const *b, const float *bn)
{
    ARGCHK(m && W && b, "bad arguments");
    HIPCHK(hipSetDevice(m->device));
    return mlp_upload(m, W, b, bn);
}

extern "C" int gnn_mlp_get_weights(gnn_mlp *m, float *const *W, float *const *b, float *bn)
{
    ARGCHK(m && W && b, "bad arguments");
    ARGCHK(!m->has_bn || bn, "this MLP ends with BatchNormalization: bn [4 * width] is required");
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipDeviceSynchronize());                 // an optimizer step may still be running on a loop's stream
    std::vector<float> stage(m->slab_floats);
    HIPCHK(hipMemcpy(stage.data(), m->slab, sizeof(float) * m->slab_floats, hipMemcpyDeviceToHost));
    for (int l = 0; l < m->n_layers; ++l) {
        ARGCHK(W[l] && b[l], "W[%d]/b[%d] is NULL", l, l);
        memcpy(W[l], stage.data() + (m->W[l] - m->slab), sizeof(float) * (size_t)m->dims[l] * m->dims[l + 1]);
        memcpy(b[l], stage.data() + (m->b[l] - m->slab), sizeof(float) * (size_t)m->dims[l + 1]);
    }
    if (m->has_bn) HIPCHK(hipMemcpy(bn, m->bn_raw, sizeof(float) * 4 * m->dims.back(), hipMemcpyDeviceToHost));
    return GNN_OK;
}

extern "C" int gnn_mlp_reset_optimizer(gnn_mlp *m)
{
    ARGCHK(m, "mlp is NULL");
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipDeviceSynchronize());
    (void)hipFree(m->opt_a); (void)hipFree(m->opt_b); (void)hipFree(m->opt_c);
    m->opt_a = nullptr; m->opt_b = nullptr; m->opt_c = nullptr;      // allocated and zeroed again by the next device-side optimizer step
    m->opt_kind = -1;
    return GNN_OK;
}

extern "C" int gnn_mlp_set_regularizers(gnn_mlp *m, const double *l1, const double *l2)
{
    ARGCHK(m && ((l1 == nullptr) == (l2 == nullptr)), "mlp is NULL, or only one of l1 / l2 given (both NULL clears the regularizers)");
    const int n = 2 * m->n_layers;
    bool any = false;
    for (int a = 0; l1 && a < n; ++a) {
        ARGCHK(std::isfinite(l1[a]) && std::isfinite(l2[a]) && l1[a] >= 0.0 && l2[a] >= 0.0, "array %d: regularizer coefficients must be finite and >= 0", a);
        any = any || l1[a] != 0.0 || l2[a] != 0.0;
    }
    if (any) { m->reg_l1.assign(l1, l1 + n); m->reg_l2.assign(l2, l2 + n); }
    else { m->reg_l1.clear(); m->reg_l2.clear(); }
    return GNN_OK;
}

extern "C" int gnn_mlp_forward(gnn_mlp *m, int64_t n_rows, const float *x, float *y)
{
    ARGCHK(m && n_rows >= 0 && (n_rows == 0 || (x && y)), "bad arguments");
    if (n_rows == 0) return GNN_OK;
    HIPCHK(hipSetDevice(m->device));
    int maxw = 1;
    for (int l = 1; l <= m->n_layers; ++l) maxw = std::max(maxw, m->dims[l]);
    float *dx = nullptr, *dy = nullptr, *t0 = nullptr, *t1 = nullptr;
    int rc = dev_upload(&dx, x, (size_t)n_rows * m->dims[0]);
    if (!rc) rc = dev_alloc(&dy, (size_t)n_rows * m->dims.back());
    if (!rc) rc = dev_alloc(&t0, (size_t)n_rows * maxw);
    if (!rc) rc = dev_alloc(&t1, (size_t)n_rows * maxw);
    if (!rc) rc = launch_mlp(nullptr, m, n_rows, dx, m->dims[0], dy, m->dims.back(), t0, t1, nullptr, 1);
    if (!rc) {
        hipError_t e = hipMemcpy(y, dy, sizeof(float) * (size_t)n_rows * m->dims.back(), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = gnn_fail(GNN_ERR_HIP, "copy back: %s", hipGetErrorString(e));
    }
    (void)hipFree(dx); (void)hipFree(dy); (void)hipFree(t0); (void)hipFree(t1);
    return rc;
}

extern "C" int gnn_mlp_destroy(gnn_mlp *m)
{
    if (!m) return GNN_OK;
    (void)hipSetDevice(m->device);
    (void)hipFree(m->slab);
    (void)hipFree(m->bn_scale); (void)hipFree(m->bn_shift); (void)hipFree(m->bn_raw);
    (void)hipFree(m->opt_a); (void)hipFree(m->opt_b); (void)hipFree(m->opt_c);
    gnn_fused_release(m);
    delete m;
    return GNN_OK;
}
