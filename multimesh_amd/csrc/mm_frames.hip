// Frames: points and vector fields rotated by a 3 x 3 matrix, and vector components between the Cartesian basis and the
// local spherical basis at every node (include/multimesh_frames.h, which holds the statement; tests/frames_cases.py is its
// NumPy form).
//
//   mm_rotate_points    : p' = R p over f64[n][3]
//   mm_rotate_vectors   : v' = R v over three addressed components of a field
//   mm_local_components : (vx, vy, vz) <-> (radial, south, east) or (up, north, east) at the node's position
//
// Bit parity with the statement: every product, quotient, sum and square root is rounded on its own (-ffp-contract=off; the
// f64 quotient and square root of the device are correctly rounded), nothing is special-cased, no atomics.
//
// One lane per point or node, 256-lane workgroups, at most 8192 of them and a stride loop over the rest: the shape of
// map_to_sphere_kernel, which streams the same [n][3] layout.  The matrix travels in the kernel's arguments, transposed on
// the host when the caller asks for the transpose: the kernels know one form.  HBM-bound: 24 B read + 24 B written per
// point or node (+ 24 B of position for the local basis), no reuse, no LDS (DESIGN.md section 5 records the resources).
#include "mm_stream.h"

#include <math.h>

#include "mm_node_layout.h"
#include "multimesh_frames.h"

namespace {

using mm_stream::kThreads;
using namespace mm_layout;   // kMaxExtent, Span, check_array, same_array, disjoint

unsigned grid_for(i64 n) { return mm_blocks(n, kThreads, 8192); }   // grid-stride beyond 2 M lanes

struct Matrix {
    double m[9];   // row-major, as the kernels apply it
};

__device__ __forceinline__ void rotate(const Matrix &R, double x, double y, double z, double &xo, double &yo, double &zo)
{
    xo = (R.m[0] * x + R.m[1] * y) + R.m[2] * z;
    yo = (R.m[3] * x + R.m[4] * y) + R.m[5] * z;
    zo = (R.m[6] * x + R.m[7] * y) + R.m[8] * z;
}

__global__ __launch_bounds__(kThreads) void rotate_points_kernel(const double *in, double *out, i64 npoints, const Matrix R)
{
    // (in and out may be the same array: no __restrict__ on them; each lane reads its point before writing it)
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < npoints; i += stride) {
        const double x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
        double xo, yo, zo;
        rotate(R, x, y, z, xo, yo, zo);
        out[3 * i] = xo;
        out[3 * i + 1] = yo;
        out[3 * i + 2] = zo;
    }
}

// where the three components of an array's nodes are: base[e * group_stride + cols[c] * comp_stride + p]
struct Layout {
    double *base;
    i64 group_stride, comp_stride;
    int cols[3];
};

struct FieldArgs {
    i64 ngroups;
    int P;
    Layout in, out;
};

__device__ __forceinline__ void load_node(const Layout &a, i64 at, double &x, double &y, double &z)
{
    x = a.base[at + a.cols[0] * a.comp_stride];
    y = a.base[at + a.cols[1] * a.comp_stride];
    z = a.base[at + a.cols[2] * a.comp_stride];
}

__device__ __forceinline__ void store_node(const Layout &a, i64 at, double x, double y, double z)
{
    a.base[at + a.cols[0] * a.comp_stride] = x;
    a.base[at + a.cols[1] * a.comp_stride] = y;
    a.base[at + a.cols[2] * a.comp_stride] = z;
}

// (out may be the input: every lane has read its node's three inputs before it writes)
__global__ __launch_bounds__(kThreads) void rotate_vectors_kernel(const FieldArgs a, const Matrix R)
{
    const i64 n = a.ngroups * a.P;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const i64 e = i / a.P, p = i - e * a.P;
        double x, y, z, xo, yo, zo;
        load_node(a.in, e * a.in.group_stride + p, x, y, z);
        rotate(R, x, y, z, xo, yo, zo);
        store_node(a.out, e * a.out.group_stride + p, xo, yo, zo);
    }
}

template <int DIRECTION>
__global__ __launch_bounds__(kThreads) void local_components_kernel(const FieldArgs a, const double *__restrict__ points,
                                                                    const int basis)
{
    const i64 n = a.ngroups * a.P;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const i64 e = i / a.P, p = i - e * a.P;
        const double x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
        const double r = mm_norm3(x, y, z);
        const double s = sqrt(x * x + y * y);
        const bool off_axis = s > 0.0;
        const double cp = off_axis ? x / s : 1.0, sp = off_axis ? y / s : 0.0;
        const double ct = z / r, st = s / r;
        double u, v, w, uo, vo, wo;
        load_node(a.in, e * a.in.group_stride + p, u, v, w);
        if constexpr (DIRECTION == MM_FRAMES_TO_LOCAL) {
            uo = ((st * cp) * u + (st * sp) * v) + ct * w;
            vo = ((ct * cp) * u + (ct * sp) * v) - st * w;
            wo = cp * v - sp * u;
            if (basis == MM_FRAMES_BASIS_ZNE) vo = -vo;
        } else {
            if (basis == MM_FRAMES_BASIS_ZNE) v = -v;
            uo = ((st * cp) * u + (ct * cp) * v) - sp * w;
            vo = ((st * sp) * u + (ct * sp) * v) + cp * w;
            wo = ct * u - st * v;
        }
        store_node(a.out, e * a.out.group_stride + p, uo, vo, wo);
    }
}

// ---- the checks, on the host: nothing below touches the device (one array's: mm_node_layout.h)
int matrix_of(const char *who, const double *R, int transpose, Matrix *out)
{
    MM_REQUIRE_AS(who, R != nullptr, "R is null");
    for (int k = 0; k < 9; ++k) MM_REQUIRE_AS(who, isfinite(R[k]), "R is not finite");
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out->m[3 * i + j] = transpose ? R[3 * j + i] : R[3 * i + j];
    return MM_OK;
}

Layout layout_of(const double *base, i64 group_stride, i64 comp_stride, const int *cols)
{
    Layout l;
    l.base = const_cast<double *>(base);
    l.group_stride = group_stride;
    l.comp_stride = comp_stride;
    for (int c = 0; c < 3; ++c) l.cols[c] = cols[c];
    return l;
}

// the shared refusals of the two field entry points; on MM_OK, a holds the launch's arguments and *out_span the output's span
int field_args(const char *who, i64 ngroups, i64 P, const double *in_d, i64 in_group_stride, i64 in_comp_stride,
               const int *in_cols, double *out_d, i64 out_group_stride, i64 out_comp_stride, const int *out_cols,
               FieldArgs *a, Span *out_span)
{
    MM_REQUIRE_AS(who, ngroups >= 0, "negative ngroups");
    MM_REQUIRE_AS(who, ngroups < kMaxExtent, "ngroups at or past 2^48");
    MM_REQUIRE_AS(who, P >= 1 && P <= MM_PARAM_MAX_P, "P must lie in [1, 4096]");
    Span in;
    int rc = check_array(who, "in", ngroups, P, in_d, in_group_stride, in_comp_stride, in_cols, 3, false, &in);
    if (rc != MM_OK) return rc;
    rc = check_array(who, "out", ngroups, P, out_d, out_group_stride, out_comp_stride, out_cols, 3, true, out_span);
    if (rc != MM_OK) return rc;
    MM_REQUIRE_AS(who, ngroups == 0 || same_array(*out_span, in) || disjoint(*out_span, in),
                  "out overlaps in without being that array with its strides");
    a->ngroups = ngroups;
    a->P = (int)P;
    a->in = layout_of(in_d, in_group_stride, in_comp_stride, in_cols);
    a->out = layout_of(out_d, out_group_stride, out_comp_stride, out_cols);
    return MM_OK;
}

}  // namespace

extern "C" int mm_rotate_points(mm_context *ctx, int64_t n, const double *in_d, double *out_d, const double *R, int transpose)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(n >= 0, "negative n");
    MM_REQUIRE(n <= (kMaxExtent - 1) / 3, "3 * n at or past 2^48");
    Matrix m;
    const int rc = matrix_of(__func__, R, transpose, &m);
    if (rc != MM_OK) return rc;
    if (n == 0) return MM_OK;
    MM_REQUIRE(in_d && out_d, "null array");
    MM_REQUIRE(out_d == in_d || out_d + 3 * n <= in_d || in_d + 3 * n <= out_d, "out_d overlaps in_d without being it");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(rotate_points_kernel, dim3(grid_for(n)), dim3(kThreads), 0, ctx->stream, in_d, out_d, (i64)n, m);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}

extern "C" int mm_rotate_vectors(mm_context *ctx, int64_t ngroups, int64_t P, const double *in_d, int64_t in_group_stride,
                                 int64_t in_comp_stride, const int *in_cols, double *out_d, int64_t out_group_stride,
                                 int64_t out_comp_stride, const int *out_cols, const double *R, int transpose)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    FieldArgs a;
    Span out;
    int rc = field_args(__func__, ngroups, P, in_d, in_group_stride, in_comp_stride, in_cols, out_d, out_group_stride,
                        out_comp_stride, out_cols, &a, &out);
    if (rc != MM_OK) return rc;
    Matrix m;
    rc = matrix_of(__func__, R, transpose, &m);
    if (rc != MM_OK) return rc;
    if (ngroups == 0) return MM_OK;
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(rotate_vectors_kernel, dim3(grid_for(ngroups * P)), dim3(kThreads), 0, ctx->stream, a, m);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}

extern "C" int mm_local_components(mm_context *ctx, int64_t ngroups, int64_t P, const double *points_d, const double *in_d,
                                   int64_t in_group_stride, int64_t in_comp_stride, const int *in_cols, double *out_d,
                                   int64_t out_group_stride, int64_t out_comp_stride, const int *out_cols, int direction,
                                   int basis)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(direction == MM_FRAMES_TO_LOCAL || direction == MM_FRAMES_TO_CARTESIAN, "direction must be 0 or 1");
    MM_REQUIRE(basis == MM_FRAMES_BASIS_RTP || basis == MM_FRAMES_BASIS_ZNE, "basis must be 0 or 1");
    FieldArgs a;
    Span out;
    const int rc = field_args(__func__, ngroups, P, in_d, in_group_stride, in_comp_stride, in_cols, out_d, out_group_stride,
                              out_comp_stride, out_cols, &a, &out);
    if (rc != MM_OK) return rc;
    if (ngroups == 0) return MM_OK;
    MM_REQUIRE(points_d != nullptr, "points: null array");
    MM_REQUIRE(3 * ngroups * P < kMaxExtent, "points: extent at or past 2^48 elements");
    MM_REQUIRE(points_d + 3 * ngroups * P <= out.base || out.base + out.extent <= points_d, "points overlap out");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    const dim3 grid(grid_for(ngroups * P));
    if (direction == MM_FRAMES_TO_LOCAL)
        hipLaunchKernelGGL(local_components_kernel<MM_FRAMES_TO_LOCAL>, grid, dim3(kThreads), 0, ctx->stream, a, points_d, basis);
    else
        hipLaunchKernelGGL(local_components_kernel<MM_FRAMES_TO_CARTESIAN>, grid, dim3(kThreads), 0, ctx->stream, a, points_d,
                           basis);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}
