// A15 -- the spatial gradient of element-nodal GLL fields, as fields: the physical gradient gr = G grad_ref u that the
// stiffness kernel (mm_diffusion.hip) forms at every node and folds into its flux, written out, with its norm and its
// split into the radial derivative and the lateral part.
//
//   mm_gll_gradient : grad[c][d][e][.] = (G grad_ref u[c])[d],  norm = |grad|,  radial = rh . grad,  lateral = |grad - radial rh|
//
// Bit parity with the NumPy statement (tests/gradient_cases.py): the table comes from the host, every product is rounded on
// its own (-ffp-contract=off), every sum starts from its first term and adds in ascending a, the one division and the square
// roots are IEEE operations; J, det, G, g and gr are the shared expressions of mm_gll_tile.h, and the order of everything
// else is written out in include/multimesh_hip.h.
//
// The kernel is the first half of gll_diffusion_kernel on the element tile of mm_gll_tile.h: the coordinates and one
// component of u go into LDS, a lane keeps its three rows of D in registers (no columns: nothing is transposed here).  J is
// recomputed from the coordinates of every tile; G and the unit radius stay in registers over the components of the tile.
// Per tile and component: three tensor-line reads of u from LDS, the gr sums, the stores.  No flux, no pull-back, nothing
// written to LDS after the loads, so the only hazard is the next step's u (or coordinates) landing while a slower wave
// still reads this step's: both arrays are double buffered, which leaves ONE barrier per tile and component -- a buffer is
// written again two steps later, and every lane that writes it then has passed the barrier of the step between, which no
// lane reaches before its reads are done.  The next step's loads are issued before the current one is computed.  Which
// outputs are written is decided by pointer tests, the same for every lane of the grid.  Stores go to planes
// [component][direction]: consecutive lanes write consecutive doubles.  HBM bytes per node: 24 + 8 C read, 8 per written
// plane.
#include "mm_common.h"
#include "mm_gll_tile.h"

namespace {

using gll::kThreads;

template <int ORDER, int DIM>
__global__ __launch_bounds__(kThreads) void gll_gradient_kernel(const double *__restrict__ gp, i64 nelem,
                                                                const double *__restrict__ deriv,
                                                                const double *__restrict__ u, i64 ncomp,
                                                                double *__restrict__ grad, double *__restrict__ radial,
                                                                double *__restrict__ lateral, double *__restrict__ norm)
{
    using T = gll::Tile<ORDER, DIM>;
    __shared__ double xs[2][T::TILE_DOUBLES];
    __shared__ double us[2][T::TILE_NODES];
    __shared__ double tab[T::TABLE];

    const int tid = threadIdx.x;
    T::load_tables(tab, deriv);
    const typename T::Lane ln(tab);

    const i64 ntiles = (nelem + T::TILE - 1) / T::TILE;
    const i64 nnodes = nelem * T::P;
    const bool want_rh = DIM == 3 && (radial != nullptr || lateral != nullptr);
    double stage_x[T::LOADS];
    double stage_u = 0.0;

    i64 tile = blockIdx.x;
    if (tile < ntiles) {
        T::fetch_x(gp, nelem, tile, stage_x);
        stage_u = T::fetch_u(u, nelem, tile, 0);
    }
    double G[3][3] = {}, rh[3] = {};
    int xbuf = 0, ubuf = 0;   // the halves of xs and us this step fills and reads
    for (; tile < ntiles; tile += gridDim.x, xbuf ^= 1) {
        const bool active = tid < T::tile_nodes(nelem, tile);
        const i64 tile0 = tile * (i64)T::TILE_NODES;   // the tile's first node: the same for every lane, as all of an
                                                       // output's address but the lane's own 8 * tid
        const double *xt = xs[xbuf];
        for (i64 c = 0; c < ncomp; ++c, ubuf ^= 1) {
            if (c == 0) T::store_x(xs[xbuf], stage_x);
            if (ln.node_lane) us[ubuf][tid] = stage_u;
            __syncthreads();
            // the next step's loads
            if (c + 1 < ncomp) {
                stage_u = T::fetch_u(u, nelem, tile, c + 1);
            } else if (tile + gridDim.x < ntiles) {
                T::fetch_x(gp, nelem, tile + gridDim.x, stage_x);
                stage_u = T::fetch_u(u, nelem, tile + gridDim.x, 0);
            }
            if (!active) continue;
            if (c == 0) {
                // (the unit radius first, while neither J nor G is live: its square root and divisions are the widest
                // stretch of the kernel; then J one direction at a time -- both for the registers of the order-4 3-D
                // instance)
                if constexpr (DIM == 3) {
                    if (want_rh) {
                        T::unit_radius(xt, rh);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                double J[3][3];
                T::template jacobian<true>(xt, ln.row, ln.line, J);
                T::inverse(J, T::det(J), G);
            }
            double g[3], gr[3];
            T::ref_gradient(us[ubuf], ln.row, ln.line, g);
            T::phys_gradient(G, g, gr);
            // what is asked of the physical gradient
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
    const dim3 grid(gll::grid_size(nelem, gll::Tile<ORDER, DIM>::TILE));
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
