// A15 -- the spatial gradient of element-nodal GLL fields, as fields: the physical gradient gr = G grad_ref u that the
// stiffness kernel (mm_diffusion.hip) forms at every node and folds into its flux, written out, with its norm and its
// split into the radial derivative and the lateral part.
//
//   mm_gll_gradient : grad[c][d][e][.] = (G grad_ref u[c])[d],  norm = |grad|,  radial = rh . grad,  lateral = |grad - radial rh|
//
// Bit parity with the NumPy statement (tests/gradient_cases.py): the table comes from the host, every product is rounded on
// its own (-ffp-contract=off), every sum starts from its first term and adds in ascending a, the one division and the square
// roots are IEEE operations; J, det and G are the expressions of gll_diffusion_kernel, term for term, and the order of
// everything else is written out in include/multimesh_hip.h.
//
// The kernel is the first half of gll_diffusion_kernel: a 256-thread block takes a tile of 256 / P whole elements, which
// are contiguous in memory; the coordinates (three coalesced 8-byte loads per thread) and one component of u (one load) go
// into LDS, lane t of the block is node t of the tile.  A lane is the same node (i, j, k) of every tile, so its three rows
// of D live in registers (no columns: nothing is transposed here).  J is recomputed from the coordinates of every tile; G
// and the unit radius stay in registers over the components of the tile.  Per tile and component: three tensor-line reads
// of u from LDS, the gr sums, the stores.  No flux, no pull-back, nothing written to LDS after the loads, so the only
// hazard is the next step's u (or coordinates) landing while a slower wave still reads this step's: both arrays are double
// buffered, which leaves ONE barrier per tile and component -- a buffer is written again two steps later, and every lane
// that writes it then has passed the barrier of the step between, which no lane reaches before its reads are done.  The
// next step's loads are issued before the current one is computed.  Which outputs are written is decided by pointer
// tests, the same for every lane of the grid.  HBM bytes per node: 24 + 8 C read, 8 per written plane.
//
// LDS layout: as gll_diffusion_kernel.  u is indexed by the node of the tile, so a tensor line is read with the strides 1,
// m, m^2 doubles; the 32 lanes of a half-wave (the conflict group of ds_read_b64, 32 banks of 8 bytes) read, along
// direction d, one address per line that crosses them: lanes that differ only in i_d read the same address (a broadcast),
// the others are consecutive nodes with i_d removed -- distinct addresses less than 32 doubles apart at m = 5, so no two
// fall on one bank.  The coordinates keep the [node][dim] layout, read once per tile.  Stores go to planes
// [component][direction]: consecutive lanes write consecutive doubles.
#include "mm_common.h"

namespace {

constexpr int kThreads = 256;
constexpr i64 kMaxBlocks = 2048;   // 256 CUs x 8 resident blocks; blocks stride over the rest

constexpr int ipow(int b, int e) { return e == 0 ? 1 : b * ipow(b, e - 1); }

template <int ORDER, int DIM>
__global__ __launch_bounds__(kThreads) void gll_gradient_kernel(const double *__restrict__ gp, i64 nelem,
                                                                const double *__restrict__ deriv,
                                                                const double *__restrict__ u, i64 ncomp,
                                                                double *__restrict__ grad, double *__restrict__ radial,
                                                                double *__restrict__ lateral, double *__restrict__ norm)
{
    constexpr int M = ORDER + 1;
    constexpr int P = ipow(M, DIM);
    constexpr int TILE = kThreads / P;            // elements per block and step
    constexpr int TILE_NODES = TILE * P;          // <= 256
    constexpr int TILE_DOUBLES = TILE_NODES * DIM;
    constexpr int LOADS = (TILE_DOUBLES + kThreads - 1) / kThreads;
    __shared__ double xs[2][TILE_DOUBLES];
    __shared__ double us[2][TILE_NODES];
    __shared__ double tab[M * M];

    const int tid = threadIdx.x;
    if (tid < M * M) tab[tid] = deriv[tid];
    __syncthreads();

    // this lane's node of the tile
    const bool node_lane = tid < TILE_NODES;
    const int el = node_lane ? tid / P : 0;
    const int p = node_lane ? tid - el * P : 0;
    const int i = p % M, j = (p / M) % M, k = DIM == 3 ? p / (M * M) : 0;
    double di[M], dj[M], dk[M];   // rows of D: D[i][a]
#pragma unroll
    for (int a = 0; a < M; ++a) {
        di[a] = tab[i * M + a];
        dj[a] = tab[j * M + a];
        dk[a] = tab[k * M + a];
    }
    // offsets (in nodes of the tile) of the first node of this lane's three tensor lines
    const int nbase = el * P;
    const int node_i = nbase + (p - i);
    const int node_j = nbase + (p - j * M);
    const int node_k = nbase + (p - k * M * M);

    const i64 ntiles = (nelem + TILE - 1) / TILE;
    const i64 nnodes = nelem * P;
    const bool want_rh = DIM == 3 && (radial != nullptr || lateral != nullptr);
    // valid nodes of a tile: the last one may hold fewer elements
    auto tile_nodes = [&](i64 t) -> int {
        const i64 left = nelem - t * TILE;
        return (int)(left < TILE ? left : TILE) * P;
    };
    double stage_x[LOADS];
    double stage_u = 0.0;
    auto fetch_x = [&](i64 t) {
        const int nd = tile_nodes(t) * DIM;
        const double *src = gp + t * (i64)TILE_DOUBLES;
#pragma unroll
        for (int r = 0; r < LOADS; ++r) {
            const int idx = r * kThreads + tid;
            stage_x[r] = idx < nd ? src[idx] : 0.0;
        }
    };
    auto fetch_u = [&](i64 t, i64 c) {
        const double *src = u + (c * nnodes + t * (i64)TILE_NODES);
        stage_u = tid < tile_nodes(t) ? src[tid] : 0.0;
    };

    i64 tile = blockIdx.x;
    if (tile < ntiles) {
        fetch_x(tile);
        fetch_u(tile, 0);
    }
    double G[3][3] = {}, rh[3] = {};
    int xbuf = 0, ubuf = 0;   // the halves of xs and us this step fills and reads
    for (; tile < ntiles; tile += gridDim.x, xbuf ^= 1) {
        const int nn = tile_nodes(tile);
        const bool active = node_lane && tid < nn;
        const i64 tile0 = tile * (i64)TILE_NODES;   // the tile's first node: the same for every lane, as all of an output's
                                                    // address but the lane's own 8 * tid
        const double *xt = xs[xbuf];
        for (i64 c = 0; c < ncomp; ++c, ubuf ^= 1) {
            if (c == 0) {
#pragma unroll
                for (int r = 0; r < LOADS; ++r) {
                    const int idx = r * kThreads + tid;
                    if (idx < TILE_DOUBLES) xs[xbuf][idx] = stage_x[r];
                }
            }
            if (node_lane) us[ubuf][tid] = stage_u;
            __syncthreads();
            // the next step's loads
            if (c + 1 < ncomp) {
                fetch_u(tile, c + 1);
            } else if (tile + gridDim.x < ntiles) {
                fetch_x(tile + gridDim.x);
                fetch_u(tile + gridDim.x, 0);
            }
            if (!active) continue;
            if (c == 0) {
                // (the unit radius first, while neither J nor G is live: its square root and divisions are the widest
                // stretch of the kernel)
                if constexpr (DIM == 3) {
                    if (want_rh) {
                        const double x0 = xt[tid * DIM], x1 = xt[tid * DIM + 1], x2 = xt[tid * DIM + 2];
                        const double rn = sqrt((x0 * x0 + x1 * x1) + x2 * x2);
                        const bool off_centre = rn > 0.0;
                        rh[0] = off_centre ? x0 / rn : 0.0;
                        rh[1] = off_centre ? x1 / rn : 0.0;
                        rh[2] = off_centre ? x2 / rn : 0.0;
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                double J[3][3];
                const int line_i = node_i * DIM, line_j = node_j * DIM, line_k = node_k * DIM;
                // one tensor direction at a time, the scheduler kept from hoisting the next direction's LDS reads over this
                // one's sums: all 3 m DIM values in flight at once cost the order-4 3-D instance an occupancy step
#pragma unroll
                for (int cc = 0; cc < DIM; ++cc) J[0][cc] = di[0] * xt[line_i + cc];
#pragma unroll
                for (int a = 1; a < M; ++a)
#pragma unroll
                    for (int cc = 0; cc < DIM; ++cc) J[0][cc] = J[0][cc] + di[a] * xt[line_i + a * DIM + cc];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int cc = 0; cc < DIM; ++cc) J[1][cc] = dj[0] * xt[line_j + cc];
#pragma unroll
                for (int a = 1; a < M; ++a)
#pragma unroll
                    for (int cc = 0; cc < DIM; ++cc) J[1][cc] = J[1][cc] + dj[a] * xt[line_j + a * M * DIM + cc];
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (DIM == 3) {
#pragma unroll
                    for (int cc = 0; cc < DIM; ++cc) J[2][cc] = dk[0] * xt[line_k + cc];
#pragma unroll
                    for (int a = 1; a < M; ++a)
#pragma unroll
                        for (int cc = 0; cc < DIM; ++cc) J[2][cc] = J[2][cc] + dk[a] * xt[line_k + a * M * M * DIM + cc];
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (DIM == 3) {
                    const double det = (J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) -
                                        J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0])) +
                                       J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
                    const double rdet = 1.0 / det;
                    G[0][0] = (J[1][1] * J[2][2] - J[1][2] * J[2][1]) * rdet;
                    G[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * rdet;
                    G[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * rdet;
                    G[1][0] = (J[1][2] * J[2][0] - J[1][0] * J[2][2]) * rdet;
                    G[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * rdet;
                    G[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * rdet;
                    G[2][0] = (J[1][0] * J[2][1] - J[1][1] * J[2][0]) * rdet;
                    G[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * rdet;
                    G[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * rdet;
                } else {
                    const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
                    const double rdet = 1.0 / det;
                    G[0][0] = J[1][1] * rdet;
                    G[0][1] = (-J[0][1]) * rdet;
                    G[1][0] = (-J[1][0]) * rdet;
                    G[1][1] = J[0][0] * rdet;
                }
            }
            // the reference gradient
            const double *ut = us[ubuf];
            double g[3];
            g[0] = di[0] * ut[node_i];
            g[1] = dj[0] * ut[node_j];
            if constexpr (DIM == 3) g[2] = dk[0] * ut[node_k];
#pragma unroll
            for (int a = 1; a < M; ++a) {
                g[0] = g[0] + di[a] * ut[node_i + a];
                g[1] = g[1] + dj[a] * ut[node_j + a * M];
                if constexpr (DIM == 3) g[2] = g[2] + dk[a] * ut[node_k + a * M * M];
            }
            // the physical gradient and what is asked of it
            double gr[3];
#pragma unroll
            for (int cc = 0; cc < DIM; ++cc) {
                gr[cc] = G[cc][0] * g[0] + G[cc][1] * g[1];
                if constexpr (DIM == 3) gr[cc] = gr[cc] + G[cc][2] * g[2];
            }
            const i64 at = c * nnodes + tile0;
            if (grad) {
#pragma unroll
                for (int cc = 0; cc < DIM; ++cc) (grad + ((c * DIM + cc) * nnodes + tile0))[tid] = gr[cc];
            }
            if (norm) {
                double sq = gr[0] * gr[0] + gr[1] * gr[1];
                if constexpr (DIM == 3) sq = sq + gr[2] * gr[2];
                (norm + at)[tid] = sqrt(sq);
            }
            if constexpr (DIM == 3) {
                if (want_rh) {
                    const double s = (rh[0] * gr[0] + rh[1] * gr[1]) + rh[2] * gr[2];
                    if (radial) (radial + at)[tid] = s;
                    if (lateral) {
                        const double l0 = gr[0] - s * rh[0], l1 = gr[1] - s * rh[1], l2 = gr[2] - s * rh[2];
                        (lateral + at)[tid] = sqrt((l0 * l0 + l1 * l1) + l2 * l2);
                    }
                }
            }
        }
    }
}

template <int ORDER, int DIM>
void launch_gradient(mm_context *ctx, const double *gp, i64 nelem, const double *deriv, const double *u, i64 ncomp,
                     double *grad, double *radial, double *lateral, double *norm)
{
    constexpr int TILE = kThreads / ipow(ORDER + 1, DIM);
    const i64 ntiles = (nelem + TILE - 1) / TILE;
    const dim3 grid((unsigned)(ntiles < kMaxBlocks ? ntiles : kMaxBlocks));
    hipLaunchKernelGGL((gll_gradient_kernel<ORDER, DIM>), grid, dim3(kThreads), 0, ctx->stream, gp, nelem, deriv, u, ncomp,
                       grad, radial, lateral, norm);
}

// [a, a + na) and [b, b + nb) share a byte
bool overlap(const double *a, i64 na, const double *b, i64 nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb * 8 && b0 < a0 + (uintptr_t)na * 8;
}

}  // namespace

extern "C" int mm_gll_gradient(mm_context *ctx, int order, int dim, const double *gll_points_d, int64_t nelem,
                               const double *deriv_d, const double *u_d, int64_t ncomp, double *grad_d, double *radial_d,
                               double *lateral_d, double *norm_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(order == 1 || order == 2 || order == 4, "order must be 1, 2 or 4");
    MM_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
    MM_REQUIRE(nelem >= 0 && nelem < ((i64)1 << 48), "nelem out of range");
    MM_REQUIRE(ncomp >= 0 && ncomp < 65536, "ncomp out of range");
    MM_REQUIRE(deriv_d != nullptr, "null table");
    MM_REQUIRE(grad_d != nullptr || radial_d != nullptr || lateral_d != nullptr || norm_d != nullptr,
               "at least one output is needed");
    MM_REQUIRE(dim == 3 || (radial_d == nullptr && lateral_d == nullptr), "the radial / lateral split needs a 3-D mesh");
    if (nelem == 0 || ncomp == 0) return MM_OK;
    MM_REQUIRE(gll_points_d != nullptr && u_d != nullptr, "null array");
    i64 P = order + 1;
    P = dim == 3 ? P * P * P : P * P;
    const i64 plane = (i64)ncomp * nelem * P;          // doubles of u and of every scalar output
    const double *arr[5] = {u_d, grad_d, radial_d, lateral_d, norm_d};
    const i64 len[5] = {plane, plane * dim, plane, plane, plane};
    for (int a = 0; a < 5; ++a)
        for (int b = a + 1; b < 5; ++b)
            MM_REQUIRE(arr[a] == nullptr || arr[b] == nullptr || !overlap(arr[a], len[a], arr[b], len[b]),
                       "an output must not alias u_d or another output");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
#define MM_GRAD_CASE(O, D)      \
    if (order == O && dim == D) \
    launch_gradient<O, D>(ctx, gll_points_d, nelem, deriv_d, u_d, ncomp, grad_d, radial_d, lateral_d, norm_d)
    MM_GRAD_CASE(1, 2);
    MM_GRAD_CASE(2, 2);
    MM_GRAD_CASE(4, 2);
    MM_GRAD_CASE(1, 3);
    MM_GRAD_CASE(2, 3);
    MM_GRAD_CASE(4, 3);
#undef MM_GRAD_CASE
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}
