// Geographic (geodetic) coordinates: points seen on an ellipsoid of revolution (include/multimesh_geodesy.h, which holds the
// statement; tests/geodesy_cases.py is its NumPy form).
//
//   mm_geographic_points : p -> the pseudo-point with the geodetic latitude of p as its geocentric latitude, the longitude
//                          of p and the radius R + height (direction 0), or back (direction 1), over f64[n][3]
//
// Bit parity with the statement: every product, quotient, sum and square root is rounded on its own (-ffp-contract=off; the
// f64 quotient and square root of the device are correctly rounded), nothing is special-cased, no atomics.  The constants of
// the ellipsoid travel in the kernel's arguments as the caller formed them: the kernel derives nothing.
//
// One lane per point, 256-lane workgroups, at most 8192 of them and a stride loop over the rest: the shape of
// rotate_points_kernel, which streams the same [n][3] layout.  24 B read + 24 B written per point (+ 8 B each for the
// optional radius and height), no reuse, no LDS.  Direction 0 executes 10 quotients and 6 square roots per point, direction
// 1 five and three -- most of them links of one dependent chain, the iteration, so the code is the statement as written and
// the waves in flight hide the chains ("Geographic coordinates", records the resources and what bounds the kernel).
#include "mm_stream.h"

#include <math.h>

#include "mm_node_layout.h"
#include "multimesh_geodesy.h"

namespace {

using mm_stream::kThreads;
using mm_layout::kMaxExtent;

constexpr int kPasses = 3;   // of Bowring's iteration: the statement's count

struct Ellipsoid {
    double a, b, e2, one_minus_e2, one_minus_f, ep2b, e2a, R;
};

// cos and sin of the longitude of (x, y) at the distance s from the axis: the rule of mm_local_components
__device__ __forceinline__ void longitude(double x, double y, double s, double &cl, double &sl)
{
    const bool off_axis = s > 0.0;
    cl = off_axis ? x / s : 1.0;
    sl = off_axis ? y / s : 0.0;
}

// (in and out may be the same array: no __restrict__ on them; each lane reads its point before writing it)
__global__ __launch_bounds__(kThreads) void to_geographic_kernel(const double *in, double *out, i64 npoints, const Ellipsoid E,
                                                                 const double *__restrict__ radius,
                                                                 double *__restrict__ height_out)
{
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < npoints; i += stride) {
        const double x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
        const double s = sqrt(x * x + y * y);
        double cl, sl;
        longitude(x, y, s, cl, sl);
        double u = E.b * s, v = E.a * z, zn, sn;
#pragma unroll
        for (int pass = 0; pass < kPasses; ++pass) {
            const double nb = sqrt(u * u + v * v);
            const double cb = u / nb, sb = v / nb;
            zn = z + E.ep2b * ((sb * sb) * sb);
            sn = s - E.e2a * ((cb * cb) * cb);
            u = sn;
            v = E.one_minus_f * zn;
        }
        const double nn = sqrt(sn * sn + zn * zn);
        const double cphi = sn / nn, sphi = zn / nn;
        const double h = (s * cphi + z * sphi) - E.a * sqrt(1.0 - E.e2 * (sphi * sphi));
        const double rho = radius ? radius[i] : E.R + h;
        out[3 * i] = (rho * cphi) * cl;
        out[3 * i + 1] = (rho * cphi) * sl;
        out[3 * i + 2] = rho * sphi;
        if (height_out) height_out[i] = h;
    }
}

__global__ __launch_bounds__(kThreads) void from_geographic_kernel(const double *in, double *out, i64 npoints, const Ellipsoid E)
{
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < npoints; i += stride) {
        const double x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
        const double r = mm_norm3(x, y, z);
        const double s = sqrt(x * x + y * y);
        double cl, sl;
        longitude(x, y, s, cl, sl);
        const double sphi = z / r, cphi = s / r, h = r - E.R;
        const double N = E.a / sqrt(1.0 - E.e2 * (sphi * sphi));
        out[3 * i] = ((N + h) * cphi) * cl;
        out[3 * i + 1] = ((N + h) * cphi) * sl;
        out[3 * i + 2] = (N * E.one_minus_e2 + h) * sphi;
    }
}

// whether [p, p + np) and [q, q + nq) of doubles share no byte
bool apart(const double *p, i64 np, const double *q, i64 nq) { return p + np <= q || q + nq <= p; }

}  // namespace

extern "C" int mm_geographic_points(mm_context *ctx, int64_t n, const double *in_d, double *out_d, const double *ell,
                                    int direction, const double *radius_d, double *height_out_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(n >= 0, "negative n");
    MM_REQUIRE(n <= (kMaxExtent - 1) / 3, "3 * n at or past 2^48");
    MM_REQUIRE(ell != nullptr, "ell is null");
    for (int k = 0; k < MM_GEODESY_NCONST; ++k) MM_REQUIRE(isfinite(ell[k]), "ell is not finite");
    MM_REQUIRE(ell[0] > 0.0 && ell[1] > 0.0, "the semi-axes a and b must be positive");
    MM_REQUIRE(direction == MM_GEODESY_TO_GEOGRAPHIC || direction == MM_GEODESY_TO_CARTESIAN, "direction must be 0 or 1");
    MM_REQUIRE(direction == MM_GEODESY_TO_GEOGRAPHIC || (radius_d == nullptr && height_out_d == nullptr),
               "radius_d and height_out_d go with direction 0 only");
    if (n == 0) return MM_OK;
    MM_REQUIRE(in_d && out_d, "null array");
    MM_REQUIRE(out_d == in_d || apart(out_d, 3 * n, in_d, 3 * n), "out_d overlaps in_d without being it");
    MM_REQUIRE(radius_d == nullptr || apart(radius_d, n, out_d, 3 * n), "radius_d overlaps out_d");
    MM_REQUIRE(height_out_d == nullptr || apart(height_out_d, n, out_d, 3 * n), "height_out_d overlaps out_d");
    MM_REQUIRE(height_out_d == nullptr || apart(height_out_d, n, in_d, 3 * n), "height_out_d overlaps in_d");
    MM_REQUIRE(height_out_d == nullptr || radius_d == nullptr || apart(height_out_d, n, radius_d, n),
               "height_out_d overlaps radius_d");
    const Ellipsoid E = {ell[0], ell[1], ell[2], ell[3], ell[4], ell[5], ell[6], ell[7]};
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    const dim3 grid(mm_blocks(n, kThreads, 8192));   // grid-stride beyond 2 M lanes
    if (direction == MM_GEODESY_TO_GEOGRAPHIC)
        hipLaunchKernelGGL(to_geographic_kernel, grid, dim3(kThreads), 0, ctx->stream, in_d, out_d, (i64)n, E, radius_d,
                           height_out_d);
    else
        hipLaunchKernelGGL(from_geographic_kernel, grid, dim3(kThreads), 0, ctx->stream, in_d, out_d, (i64)n, E);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}
