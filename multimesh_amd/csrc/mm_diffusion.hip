// A14 -- the matrix-free stiffness operator of an element-nodal GLL mesh (the weak Laplacian with a lateral / radial
// diffusivity), and the streaming kernels of the preconditioned conjugate-gradient loop that smooths a field with it.
//
//   mm_gll_diffusion_apply : y[c][e][.] = K_e u[c][e][.], K_e = sum_n mass_n (G_n grad phi_p) . kappa_n (G_n grad phi_q)
//   mm_pcg_combine         : out[c][i] = mass[i] * p[c][i] + tau * kp[c][i]              (A p = M p + tau K p, M u, -tau K u)
//   mm_pcg_scalars         : the convergence test, beta and alpha of every component, from the device-resident dots
//   mm_pcg_direction       : p[c] = z[c] + beta[c] * p[c]                                 (active components only)
//   mm_pcg_advance         : x[c] = x[c] + alpha[c] * p[c],  r[c] = r[c] - alpha[c] * ap[c]  (active components only)
//
// Bit parity with the NumPy statement (tests/diffusion_cases.py): the tables come from the host, every product is rounded
// on its own (-ffp-contract=off), every sum starts from its first term and adds in ascending a, and the one division and the
// one square root per node are IEEE operations; the order of everything else is written out in include/multimesh_hip.h.
//
// mm_gll_diffusion_apply works on the element tile of mm_gll_tile.h and calls its geometry functions (J, det, G, the
// unit radius, g, gr) with its own rows of D and line starts; the lane set-up, the loads and the stores are written out
// here, since the kernel also needs the columns of D.  A lane keeps three rows of D (for the gradient) and three columns
// of D (for the transposed derivative) in registers.  J is recomputed from the coordinates of every tile (24 B per node)
// rather than read as six geometric factors (48 B); G = J^-1, the mass and the unit radius stay in registers over the
// components of the tile.  Per tile and component: the reference gradient from LDS, the flux, its pull-back written to
// LDS (one array per direction), a barrier, the transposed derivative from LDS, one store.  Every buffer is single: two
// barriers per tile and component; the next step's loads are issued before the current one is computed.
// HBM bytes per node: 24 + 16 C, plus 8 per kappa array.
#include "mm_gll_tile.h"

namespace {

using gll::ipow;
using mm_stream::kThreads;
constexpr int kStateStride = 8;    // doubles per component of the PCG state block (MM_PCG_* in the header)

template <int ORDER, int DIM, bool ANISO>
__global__ __launch_bounds__(kThreads) void gll_diffusion_kernel(const double *__restrict__ gp, i64 nelem,
                                                                 const double *__restrict__ deriv,
                                                                 const double *__restrict__ weights,
                                                                 const double *__restrict__ u, i64 ncomp, double kh_s,
                                                                 const double *__restrict__ kh_a, double kr_s,
                                                                 const double *__restrict__ kr_a, double *__restrict__ y)
{
    using T = gll::Tile<ORDER, DIM>;
    constexpr int M = T::M, P = T::P, TILE = T::TILE, TILE_NODES = T::TILE_NODES, TILE_DOUBLES = T::TILE_DOUBLES,
                  LOADS = T::LOADS;
    __shared__ double xs[TILE_DOUBLES];
    __shared__ double us[TILE_NODES];
    __shared__ double fs[DIM][TILE_NODES];
    __shared__ double tab[M * M + M];

    const int tid = threadIdx.x;
    if (tid < M * M) tab[tid] = deriv[tid];
    else if (tid < M * M + M) tab[tid] = weights[tid - M * M];
    __syncthreads();

    // this lane's node of the tile
    const bool node_lane = tid < TILE_NODES;
    const int el = node_lane ? tid / P : 0;
    const int p = node_lane ? tid - el * P : 0;
    const int ix[3] = {p % M, (p / M) % M, DIM == 3 ? p / (M * M) : 0};
    double row[DIM][M];   // rows of D:    D[i_d][a]
    double col[DIM][M];   // columns of D: D[a][i_d]
#pragma unroll
    for (int a = 0; a < M; ++a) {
#pragma unroll
        for (int d = 0; d < DIM; ++d) row[d][a] = tab[ix[d] * M + a];
#pragma unroll
        for (int d = 0; d < DIM; ++d) col[d][a] = tab[a * M + ix[d]];
    }
    const double *w = tab + M * M;
    const double wprod = DIM == 3 ? (w[ix[2]] * w[ix[1]]) * w[ix[0]] : w[ix[1]] * w[ix[0]];
    // offsets (in nodes of the tile) of the first node of this lane's tensor lines
    int line[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) line[d] = el * P + (p - ix[d] * ipow(M, d));

    const i64 ntiles = (nelem + TILE - 1) / TILE;
    const i64 nnodes = nelem * P;
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
        stage_u = tid < tile_nodes(t) ? u[c * nnodes + t * (i64)TILE_NODES + tid] : 0.0;
    };

    i64 tile = blockIdx.x;
    if (tile < ntiles) {
        fetch_x(tile);
        fetch_u(tile, 0);
    }
    double G[3][3] = {}, rh[3] = {};
    double mass = 0.0, kh = 0.0, kd = 0.0;   // kd = kr - kh
    for (; tile < ntiles; tile += gridDim.x) {
        const int nn = tile_nodes(tile);
        const bool active = node_lane && tid < nn;
        const i64 node = tile * (i64)TILE_NODES + tid;
        for (i64 c = 0; c < ncomp; ++c) {
            // (the previous step's reads of fs are behind every lane that passes the barrier below; its reads of xs and us
            // were done before its second barrier)
            if (c == 0) {
#pragma unroll
                for (int r = 0; r < LOADS; ++r) {
                    const int idx = r * kThreads + tid;
                    if (idx < TILE_DOUBLES) xs[idx] = stage_x[r];
                }
            }
            if (node_lane) us[tid] = stage_u;
            __syncthreads();
            // the next step's loads
            if (c + 1 < ncomp) {
                fetch_u(tile, c + 1);
            } else if (tile + gridDim.x < ntiles) {
                fetch_x(tile + gridDim.x);
                fetch_u(tile + gridDim.x, 0);
            }
            if (active) {
                if (c == 0) {
                    double J[3][3];
                    T::template jacobian<false>(xs, row, line, J);
                    const double det = T::det(J);
                    T::inverse(J, det, G);
                    mass = wprod * fabs(det);
                    kh = kh_a ? kh_s * kh_a[node] : kh_s;
                    if constexpr (ANISO) {
                        const double kr = kr_a ? kr_s * kr_a[node] : kr_s;
                        kd = kr - kh;
                        T::unit_radius(xs, rh);
                    }
                }
                // the reference and the physical gradient, the flux and its pull-back
                double g[3], gr[3], F[3];
                T::ref_gradient(us, row, line, g);
                T::phys_gradient(G, g, gr);
                if constexpr (ANISO) {
                    const double s = (rh[0] * gr[0] + rh[1] * gr[1]) + rh[2] * gr[2];
                    const double ks = kd * s;
#pragma unroll
                    for (int cc = 0; cc < DIM; ++cc) F[cc] = mass * (kh * gr[cc] + ks * rh[cc]);
                } else {
                    const double mk = mass * kh;
#pragma unroll
                    for (int cc = 0; cc < DIM; ++cc) F[cc] = mk * gr[cc];
                }
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    double f = G[0][d] * F[0] + G[1][d] * F[1];
                    if constexpr (DIM == 3) f = f + G[2][d] * F[2];
                    fs[d][tid] = f;
                }
            }
            __syncthreads();
            if (active) {
                // the transposed derivative: sum_a D[a][i_d] * f_d[a along d], then over d
                double sd[DIM];
#pragma unroll
                for (int d = 0; d < DIM; ++d) sd[d] = col[d][0] * fs[d][line[d]];
#pragma unroll
                for (int a = 1; a < M; ++a)
#pragma unroll
                    for (int d = 0; d < DIM; ++d) sd[d] = sd[d] + col[d][a] * fs[d][line[d] + a * ipow(M, d)];
                double out = sd[0] + sd[1];
                if constexpr (DIM == 3) out = out + sd[2];
                y[c * nnodes + node] = out;
            }
        }
    }
}

template <int ORDER, int DIM>
void launch_diffusion(mm_context *ctx, const double *gp, i64 nelem, const double *deriv, const double *weights,
                      const double *u, i64 ncomp, double kh_s, const double *kh_a, bool aniso, double kr_s,
                      const double *kr_a, double *y)
{
    const dim3 grid(gll::grid_size(nelem, gll::Tile<ORDER, DIM>::TILE));
    if constexpr (DIM == 3) {
        if (aniso) {
            hipLaunchKernelGGL((gll_diffusion_kernel<ORDER, DIM, true>), grid, dim3(kThreads), 0, ctx->stream, gp, nelem, deriv,
                               weights, u, ncomp, kh_s, kh_a, kr_s, kr_a, y);
            return;
        }
    }
    hipLaunchKernelGGL((gll_diffusion_kernel<ORDER, DIM, false>), grid, dim3(kThreads), 0, ctx->stream, gp, nelem, deriv,
                       weights, u, ncomp, kh_s, kh_a, kr_s, kr_a, y);
}

// ---- the streaming kernels of the PCG loop.  state: kStateStride doubles per component (MM_PCG_* slots).
__global__ __launch_bounds__(kThreads) void pcg_combine_kernel(const double *__restrict__ mass, const double *__restrict__ p,
                                                               double tau, const double *__restrict__ kp, i64 n, i64 ncomp,
                                                               double *__restrict__ out)
{
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += stride) {
        const double m = mass ? mass[idx] : 0.0;
        for (i64 c = 0; c < ncomp; ++c) {
            const i64 at = c * n + idx;
            double v;
            if (mass && kp) v = m * p[at] + tau * kp[at];
            else if (mass) v = m * p[at];
            else v = tau * kp[at];
            out[at] = v;
        }
    }
}

__global__ void pcg_scalars_kernel(double *state, i64 ncomp, int phase, double rtol, long long *nactive)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long count = 0;
    for (i64 c = 0; c < ncomp; ++c) {
        double *s = state + c * kStateStride;
        if (phase == MM_PCG_PHASE_START) {
            s[MM_PCG_ACTIVE] = 1.0;
            s[MM_PCG_RZ_OLD] = 0.0;
            s[MM_PCG_ALPHA] = 0.0;
            s[MM_PCG_BETA] = 0.0;
        } else if (phase == MM_PCG_PHASE_BETA) {
            const double rz = s[MM_PCG_RZ];
            // (a NaN residual stays active: the loop then ends at max_iter with an error, not with a NaN field)
            if (s[MM_PCG_ACTIVE] != 0.0 && sqrt(rz) <= rtol * sqrt(s[MM_PCG_BB])) s[MM_PCG_ACTIVE] = 0.0;
            const double old = s[MM_PCG_RZ_OLD];
            s[MM_PCG_BETA] = s[MM_PCG_ACTIVE] != 0.0 && old != 0.0 ? rz / old : 0.0;
            if (s[MM_PCG_ACTIVE] != 0.0) s[MM_PCG_RZ_OLD] = rz;
        } else {
            s[MM_PCG_ALPHA] = s[MM_PCG_ACTIVE] != 0.0 ? s[MM_PCG_RZ_OLD] / s[MM_PCG_PAP] : 0.0;
        }
        if (s[MM_PCG_ACTIVE] != 0.0) ++count;
    }
    if (nactive) *nactive = count;
}

__global__ __launch_bounds__(kThreads) void pcg_direction_kernel(const double *__restrict__ state,
                                                                 const double *__restrict__ z, i64 n, double *p)
{
    const i64 c = blockIdx.y;
    const double *s = state + c * kStateStride;
    if (s[MM_PCG_ACTIVE] == 0.0) return;
    const double beta = s[MM_PCG_BETA];
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += stride) {
        const i64 at = c * n + idx;
        p[at] = z[at] + beta * p[at];
    }
}

__global__ __launch_bounds__(kThreads) void pcg_advance_kernel(const double *__restrict__ state,
                                                               const double *__restrict__ p, const double *__restrict__ ap,
                                                               i64 n, double *x, double *r)
{
    const i64 c = blockIdx.y;
    const double *s = state + c * kStateStride;
    if (s[MM_PCG_ACTIVE] == 0.0) return;
    const double alpha = s[MM_PCG_ALPHA];
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += stride) {
        const i64 at = c * n + idx;
        x[at] = x[at] + alpha * p[at];
        r[at] = r[at] - alpha * ap[at];
    }
}

unsigned stream_blocks(i64 n) { return mm_blocks(n, kThreads, 8192); }

}  // namespace

extern "C" int mm_gll_diffusion_apply(mm_context *ctx, int order, int dim, const double *gll_points_d, int64_t nelem,
                                      const double *deriv_d, const double *weights_d, const double *u_d, int64_t ncomp,
                                      double kappa_h, const double *kappa_h_d, int anisotropic, double kappa_r,
                                      const double *kappa_r_d, double *y_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(order == 1 || order == 2 || order == 4, "order must be 1, 2 or 4");
    MM_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
    MM_REQUIRE(nelem >= 0 && nelem < ((i64)1 << 48), "nelem out of range");
    MM_REQUIRE(ncomp >= 0 && ncomp < 65536, "ncomp out of range");
    MM_REQUIRE(deriv_d != nullptr && weights_d != nullptr, "null table");
    MM_REQUIRE(anisotropic == 0 || anisotropic == 1, "anisotropic must be 0 or 1");
    MM_REQUIRE(!anisotropic || dim == 3, "the radial / lateral split needs a 3-D mesh");
    MM_REQUIRE(anisotropic || kappa_r_d == nullptr, "kappa_r_d without anisotropic");
    if (nelem == 0 || ncomp == 0) return MM_OK;
    MM_REQUIRE(gll_points_d != nullptr && u_d != nullptr && y_d != nullptr, "null array");
    MM_REQUIRE(u_d != y_d, "y_d must not be u_d");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
#define MM_DIFF_CASE(O, D)                                                                                          \
    if (order == O && dim == D)                                                                                     \
    launch_diffusion<O, D>(ctx, gll_points_d, nelem, deriv_d, weights_d, u_d, ncomp, kappa_h, kappa_h_d, anisotropic != 0, \
                           kappa_r, kappa_r_d, y_d)
    MM_DIFF_CASE(1, 2);
    MM_DIFF_CASE(2, 2);
    MM_DIFF_CASE(4, 2);
    MM_DIFF_CASE(1, 3);
    MM_DIFF_CASE(2, 3);
    MM_DIFF_CASE(4, 3);
#undef MM_DIFF_CASE
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}

extern "C" int mm_pcg_combine(mm_context *ctx, const double *mass_d, const double *p_d, double tau, const double *kp_d,
                              int64_t n, int64_t ncomp, double *out_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(n >= 0 && n < ((i64)1 << 48), "n out of range");
    MM_REQUIRE(ncomp >= 0 && ncomp < 65536, "ncomp out of range");
    MM_REQUIRE(mass_d != nullptr || kp_d != nullptr, "one of mass_d and kp_d is needed");
    MM_REQUIRE(mass_d == nullptr || p_d != nullptr, "mass_d needs p_d");
    if (n == 0 || ncomp == 0) return MM_OK;
    MM_REQUIRE(out_d != nullptr, "null array");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(pcg_combine_kernel, dim3(stream_blocks(n)), dim3(kThreads), 0, ctx->stream, mass_d, p_d, tau, kp_d, n,
                       ncomp, out_d);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}

extern "C" int mm_pcg_scalars(mm_context *ctx, double *state_d, int64_t ncomp, int phase, double rtol, int64_t *nactive_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(ncomp >= 0 && ncomp < 65536, "ncomp out of range");
    MM_REQUIRE(phase == MM_PCG_PHASE_START || phase == MM_PCG_PHASE_BETA || phase == MM_PCG_PHASE_ALPHA, "unknown phase");
    MM_REQUIRE(rtol >= 0.0, "rtol must be >= 0");
    MM_REQUIRE(state_d != nullptr || ncomp == 0, "null state");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(pcg_scalars_kernel, dim3(1), dim3(64), 0, ctx->stream, state_d, ncomp, phase, rtol,
                       (long long *)nactive_d);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}

extern "C" int mm_pcg_direction(mm_context *ctx, const double *state_d, const double *z_d, int64_t n, int64_t ncomp,
                                double *p_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(n >= 0 && n < ((i64)1 << 48), "n out of range");
    MM_REQUIRE(ncomp >= 0 && ncomp < 65536, "ncomp out of range");
    if (n == 0 || ncomp == 0) return MM_OK;
    MM_REQUIRE(state_d && z_d && p_d, "null array");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(pcg_direction_kernel, dim3(stream_blocks(n), (unsigned)ncomp), dim3(kThreads), 0, ctx->stream, state_d,
                       z_d, n, p_d);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}

extern "C" int mm_pcg_advance(mm_context *ctx, const double *state_d, const double *p_d, const double *ap_d, int64_t n,
                              int64_t ncomp, double *x_d, double *r_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(n >= 0 && n < ((i64)1 << 48), "n out of range");
    MM_REQUIRE(ncomp >= 0 && ncomp < 65536, "ncomp out of range");
    if (n == 0 || ncomp == 0) return MM_OK;
    MM_REQUIRE(state_d && p_d && ap_d && x_d && r_d, "null array");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(pcg_advance_kernel, dim3(stream_blocks(n), (unsigned)ncomp), dim3(kThreads), 0, ctx->stream, state_d,
                       p_d, ap_d, n, x_d, r_d);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}
