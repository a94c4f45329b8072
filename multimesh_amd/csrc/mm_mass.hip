// A13 -- the diagonal GLL mass matrix of an element-nodal mesh, the volume integrals it gives, and the elementwise
// quotient the mass-weighted adjoint ends in.  The inner product of two nodal fields of a spectral-element mesh is
// a^T M b with M[e][p] = w_p |det J_e(xi_p)|; the transposes of mm_transpose.hip are adjoint in the plain dot product.
//
//   mm_gll_mass      : mass[e][p] = ((w_k * w_j) * w_i) * |det J|, det J from the tensor-line sums of the header
//   mm_weighted_sum  : out[c] = sum_i mass[i] * field[c][i] in the fixed order of the header (chunks of 4096, 256 lanes)
//   mm_divide_rows   : out[c][i] = num[c][i] / den[i]
//
// Bit parity with the NumPy statement (tests/mass_cases.py): the derivative matrix and the weights come from the host, so
// the device does only + and *, every product rounded on its own (-ffp-contract=off), every sum from its first term in
// ascending a.
//
// mm_gll_mass is a streaming kernel on the element tile of mm_gll_tile.h: 24 B read and 8 B written per node, ~110 flops.
// Only the coordinates go into LDS, in one buffer: a barrier before it is overwritten and one after, the next tile's loads
// issued before the current one is computed.
#include "mm_gll_tile.h"

namespace {

using namespace mm_stream;   // kThreads, kChunk

template <int ORDER, int DIM>
__global__ __launch_bounds__(kThreads) void gll_mass_kernel(const double *__restrict__ gp, i64 nelem,
                                                            const double *__restrict__ deriv,
                                                            const double *__restrict__ weights,
                                                            double *__restrict__ mass, double *__restrict__ det_out,
                                                            unsigned long long *__restrict__ nbad)
{
    using T = gll::Tile<ORDER, DIM>;
    __shared__ double xs[T::TILE_DOUBLES];
    __shared__ double tab[T::TABLE + T::M];

    const int tid = threadIdx.x;
    T::load_tables(tab, deriv, weights);
    const typename T::Lane ln(tab);
    const double wprod = ln.wprod(tab);

    const i64 ntiles = (nelem + T::TILE - 1) / T::TILE;
    unsigned bad = 0;
    double stage[T::LOADS];
    i64 tile = blockIdx.x;
    if (tile < ntiles) T::fetch_x(gp, nelem, tile, stage);
    for (; tile < ntiles; tile += gridDim.x) {
        __syncthreads();   // (the previous step's reads of xs are done)
        T::store_x(xs, stage);
        __syncthreads();
        if (tile + gridDim.x < ntiles) T::fetch_x(gp, nelem, tile + gridDim.x, stage);
        if (tid < T::tile_nodes(nelem, tile)) {
            double J[3][3];
            T::template jacobian<false>(xs, ln.row, ln.line, J);
            const double det = T::det(J);
            const i64 node = tile * (i64)T::TILE_NODES + tid;
            mass[node] = wprod * fabs(det);
            if (det_out) det_out[node] = det;
            if (!(det > 0.0)) ++bad;
        }
    }
    mm_count_to(nbad, bad);
}

template <int ORDER, int DIM>
void launch_mass(mm_context *ctx, const double *gp, i64 nelem, const double *deriv, const double *weights, double *mass,
                 double *det, unsigned long long *nbad)
{
    hipLaunchKernelGGL((gll_mass_kernel<ORDER, DIM>), dim3(gll::grid_size(nelem, gll::Tile<ORDER, DIM>::TILE)),
                       dim3(kThreads), 0, ctx->stream, gp, nelem, deriv, weights, mass, det, nbad);
}

// ---- the weighted sum.  One block per chunk of kChunk values and component: mm_chunk_sum from the lane's first term.
// a: the weights (component stride sa, 0 for a shared mass); f: the fields (nullable; component stride n).
// partial[c * nchunks + chunk].
__global__ __launch_bounds__(kThreads) void weighted_sum_kernel(const double *__restrict__ a, i64 sa,
                                                                const double *__restrict__ f, i64 n,
                                                                double *__restrict__ partial)
{
    __shared__ double s[kThreads];
    const i64 c = blockIdx.y;
    const double *ac = a + c * sa;
    const double *fc = f ? f + c * n : nullptr;
    const double sum = mm_chunk_sum<true>(s, (i64)blockIdx.x * kChunk, n,
                                          [&](i64 idx) { return fc ? ac[idx] * fc[idx] : ac[idx]; });
    if (threadIdx.x == 0) partial[c * gridDim.x + blockIdx.x] = sum;
}

__global__ __launch_bounds__(kThreads) void divide_rows_kernel(const double *num, const double *__restrict__ den, i64 n,
                                                               i64 ncomp, double *out)
{
    // (out may be num: each thread reads its value before writing it)
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += stride) {
        const double d = den[idx];
        for (i64 c = 0; c < ncomp; ++c) out[c * n + idx] = num[c * n + idx] / d;
    }
}

}  // namespace

extern "C" int64_t mm_gll_mass(mm_context *ctx, int order, int dim, const double *gll_points_d, int64_t nelem,
                               const double *deriv_d, const double *weights_d, double *mass_d, double *det_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(order == 1 || order == 2 || order == 4, "order must be 1, 2 or 4");
    MM_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
    MM_REQUIRE(nelem >= 0 && nelem < ((i64)1 << 48), "nelem out of range");
    MM_REQUIRE(deriv_d != nullptr && weights_d != nullptr, "null table");
    if (nelem == 0) return 0;
    MM_REQUIRE(gll_points_d != nullptr && mass_d != nullptr, "null array");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    unsigned long long *nbad = mm_counters_begin(ctx, 2, 1);
    if (!nbad) return MM_ERR_HIP;
#define MM_MASS_CASE(O, D)                                                                              \
    if (order == O && dim == D) launch_mass<O, D>(ctx, gll_points_d, nelem, deriv_d, weights_d, mass_d, det_d, nbad)
    MM_MASS_CASE(1, 2);
    MM_MASS_CASE(2, 2);
    MM_MASS_CASE(4, 2);
    MM_MASS_CASE(1, 3);
    MM_MASS_CASE(2, 3);
    MM_MASS_CASE(4, 3);
#undef MM_MASS_CASE
    const i64 *count = mm_counters_end(ctx, 2, 1);
    return count ? count[0] : MM_ERR_HIP;
}

extern "C" int mm_weighted_sum(mm_context *ctx, const double *mass_d, const double *fields_d, int64_t n, int64_t ncomp,
                               double *out_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(n >= 0 && n < ((i64)1 << 42), "n out of range");
    MM_REQUIRE(ncomp >= 0 && ncomp < 65536, "ncomp out of range");
    MM_REQUIRE(fields_d != nullptr || ncomp <= 1, "without fields there is one sum");
    if (ncomp == 0) return MM_OK;
    MM_REQUIRE(out_d != nullptr && (mass_d != nullptr || n == 0), "null array");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    mm_sum_levels levels(n);   // one row of chunk sums per component
    if (levels.n) {
        mm_scratch_layout lay;
        levels.add_to(lay, ncomp);
        const int rc = lay.commit(ctx, __func__);
        if (rc != MM_OK) return rc;
    }
    const double *a = mass_d, *f = fields_d;
    i64 sa = 0, count = n;
    for (int level = 0; level <= levels.n; ++level) {
        const i64 nchunks = levels.chunks_at(level);
        double *dst = level == levels.n ? out_d : levels.partial[level];
        hipLaunchKernelGGL(weighted_sum_kernel, dim3((unsigned)nchunks, (unsigned)ncomp), dim3(kThreads), 0, ctx->stream, a,
                           sa, f, count, dst);
        a = dst;          // the next level sums the chunk sums: no fields, one row per component
        f = nullptr;
        sa = nchunks;
        count = nchunks;
    }
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}

extern "C" int mm_divide_rows(mm_context *ctx, const double *num_d, const double *den_d, int64_t n, int64_t ncomp,
                              double *out_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(n >= 0 && ncomp >= 0, "negative size");
    MM_REQUIRE(n < ((i64)1 << 48) && ncomp < (1 << 20), "size out of range");
    if (n == 0 || ncomp == 0) return MM_OK;
    MM_REQUIRE(num_d && den_d && out_d, "null array");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(divide_rows_kernel, dim3(mm_blocks(n, kThreads, 8192)), dim3(kThreads), 0, ctx->stream, num_d, den_d,
                       n, ncomp, out_d);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}
