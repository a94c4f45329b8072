// Parametrisations: models and sensitivity kernels converted between iso_velocity, iso_lame, iso_bulk, vti_velocity and
// vti_love, node by node (include/multimesh_params.h, which holds the statement; tests/parametrisation_cases.py is its NumPy
// form).
//
//   mm_convert_parameters : out = the route's steps applied to in
//   mm_convert_kernels    : kout = J^T kin at the model: the route forward with every step's input kept in registers, then
//                           the steps' transposed Jacobians in reverse order
//
// Bit parity with the statement: every product, quotient, sum and square root is rounded on its own (-ffp-contract=off; the
// f64 quotient and square root of the device are correctly rounded), nothing is special-cased, no float atomics; the count
// of nodes with a non-finite output is an integer sum (mm_count_to).
//
// One lane per node, 256-lane workgroups, at most kMaxBlocks of them and a stride loop over the rest, as clamp_kernel.
// Consecutive lanes read consecutive doubles of a component's run of P; 8 * (C_in + C_out) bytes per node, no LDS.  The
// route is uniform over the launch and travels as up to four step codes in the kernel's arguments: the loops over the steps
// are unrolled, so every state array has constant indices (registers), and each step is a switch on a scalar register.  Two
// kernels serve the 20 ordered pairs; a template per (from, to) would be 40 (DESIGN.md section 5 records the resources).
#include "mm_stream.h"

#include <math.h>

#include "mm_node_layout.h"
#include "multimesh_params.h"

namespace {

using namespace mm_stream;   // kThreads, kMaxBlocks
using namespace mm_layout;   // kMaxExtent, Span, check_array, same_array, disjoint
constexpr int kMaxComp = MM_PARAM_MAX_COMPONENTS;
constexpr int kMaxSteps = 4;
constexpr int kNumParams = 5;
typedef unsigned long long u64;

enum Step {
    kVelocityToLame = 1,
    kLameToVelocity,
    kLameToBulk,
    kBulkToLame,
    kVtiVelocityToLove,
    kLoveToVtiVelocity,
    kEmbed,
    kVoigt
};

const int kNcomp[kNumParams] = {3, 3, 3, 6, 6};

// the route from -> to: the fewest steps around the ring (0 ends a route)
const int kRoute[kNumParams][kNumParams][kMaxSteps] = {
    {{0}, {1}, {1, 3}, {7}, {7, 5}},
    {{2}, {0}, {3}, {2, 7}, {2, 7, 5}},
    {{4, 2}, {4}, {0}, {4, 2, 7}, {4, 2, 7, 5}},
    {{5, 8, 4, 2}, {5, 8, 4}, {5, 8}, {0}, {5}},
    {{8, 4, 2}, {8, 4}, {8}, {6}, {0}},
};

// ---- the statement, step by step: v holds the step's input on entry and its output on return
__device__ __forceinline__ void step_forward(int step, double (&v)[kMaxComp])
{
    switch (step) {
    case kVelocityToLame: {
        const double vp = v[0], vs = v[1], rho = v[2];
        const double mu = rho * (vs * vs);
        v[0] = rho * (vp * vp) - 2.0 * mu;
        v[1] = mu;
        break;
    }
    case kLameToVelocity: {
        const double lam = v[0], mu = v[1], rho = v[2];
        v[1] = sqrt(mu / rho);
        v[0] = sqrt((lam + 2.0 * mu) / rho);
        break;
    }
    case kLameToBulk:
        v[0] = v[0] + (2.0 * v[1]) / 3.0;
        break;
    case kBulkToLame:
        v[0] = v[0] - (2.0 * v[1]) / 3.0;
        break;
    case kVtiVelocityToLove: {
        const double vpv = v[0], vph = v[1], vsv = v[2], vsh = v[3], eta = v[4], rho = v[5];
        const double A = rho * (vph * vph), L = rho * (vsv * vsv);
        v[0] = A;
        v[1] = rho * (vpv * vpv);
        v[2] = L;
        v[3] = rho * (vsh * vsh);
        v[4] = eta * (A - 2.0 * L);
        break;
    }
    case kLoveToVtiVelocity: {
        const double A = v[0], C = v[1], L = v[2], N = v[3], F = v[4], rho = v[5];
        v[0] = sqrt(C / rho);
        v[1] = sqrt(A / rho);
        v[2] = sqrt(L / rho);
        v[3] = sqrt(N / rho);
        v[4] = F / (A - 2.0 * L);
        break;
    }
    case kEmbed: {
        const double vp = v[0], vs = v[1], rho = v[2];
        v[0] = vp, v[1] = vp, v[2] = vs, v[3] = vs, v[4] = 1.0, v[5] = rho;
        break;
    }
    case kVoigt: {
        const double A = v[0], C = v[1], L = v[2], N = v[3], F = v[4], rho = v[5];
        v[0] = (((C + 4.0 * A) - 4.0 * N) + 4.0 * F) / 9.0;
        v[1] = ((((A + C) + 6.0 * L) + 5.0 * N) - 2.0 * F) / 15.0;
        v[2] = rho;
        v[3] = 0.0, v[4] = 0.0, v[5] = 0.0;
        break;
    }
    default:
        break;
    }
}

// ---- the transposed Jacobian of a step at its input m: k holds K' (with respect to the outputs) on entry, K on return
__device__ __forceinline__ void step_transposed(int step, const double (&m)[kMaxComp], double (&k)[kMaxComp])
{
    switch (step) {
    case kVelocityToLame: {
        const double vp = m[0], vs = m[1], rho = m[2], r2 = 2.0 * rho;
        const double klam = k[0], kmu = k[1], krho = k[2];
        k[0] = (r2 * vp) * klam;
        k[1] = (r2 * vs) * (kmu - 2.0 * klam);
        k[2] = (krho + (vp * vp - 2.0 * (vs * vs)) * klam) + (vs * vs) * kmu;
        break;
    }
    case kLameToVelocity: {
        const double lam = m[0], mu = m[1], rho = m[2], r2 = 2.0 * rho;
        const double vs = sqrt(mu / rho), vp = sqrt((lam + 2.0 * mu) / rho);
        const double kvp = k[0], kvs = k[1], krho = k[2];
        k[0] = kvp / (r2 * vp);
        k[1] = kvp / (rho * vp) + kvs / (r2 * vs);
        k[2] = (krho - (vp / r2) * kvp) - (vs / r2) * kvs;
        break;
    }
    case kLameToBulk:
        k[1] = k[1] + (2.0 * k[0]) / 3.0;
        break;
    case kBulkToLame:
        k[1] = k[1] - (2.0 * k[0]) / 3.0;
        break;
    case kVtiVelocityToLove: {
        const double vpv = m[0], vph = m[1], vsv = m[2], vsh = m[3], eta = m[4], rho = m[5], r2 = 2.0 * rho;
        const double A = rho * (vph * vph), L = rho * (vsv * vsv);
        const double kA = k[0], kC = k[1], kL = k[2], kN = k[3], kF = k[4], krho = k[5];
        const double ef = eta * kF, a = kA + ef, l = kL - 2.0 * ef;
        k[0] = (r2 * vpv) * kC;
        k[1] = (r2 * vph) * a;
        k[2] = (r2 * vsv) * l;
        k[3] = (r2 * vsh) * kN;
        k[4] = (A - 2.0 * L) * kF;
        k[5] = (((krho + (vph * vph) * a) + (vpv * vpv) * kC) + (vsv * vsv) * l) + (vsh * vsh) * kN;
        break;
    }
    case kLoveToVtiVelocity: {
        const double A = m[0], C = m[1], L = m[2], N = m[3], F = m[4], rho = m[5], r2 = 2.0 * rho;
        const double vpv = sqrt(C / rho), vph = sqrt(A / rho), vsv = sqrt(L / rho), vsh = sqrt(N / rho);
        const double d = A - 2.0 * L, eta = F / d, g = eta / d;
        const double kvpv = k[0], kvph = k[1], kvsv = k[2], kvsh = k[3], keta = k[4], krho = k[5];
        k[0] = kvph / (r2 * vph) - g * keta;
        k[1] = kvpv / (r2 * vpv);
        k[2] = kvsv / (r2 * vsv) + (2.0 * g) * keta;
        k[3] = kvsh / (r2 * vsh);
        k[4] = keta / d;
        k[5] = (((krho - (vpv / r2) * kvpv) - (vph / r2) * kvph) - (vsv / r2) * kvsv) - (vsh / r2) * kvsh;
        break;
    }
    case kEmbed: {
        const double kvp = k[0] + k[1], kvs = k[2] + k[3], krho = k[5];
        k[0] = kvp, k[1] = kvs, k[2] = krho;
        k[3] = 0.0, k[4] = 0.0, k[5] = 0.0;
        break;
    }
    case kVoigt: {
        const double a = k[0] / 9.0, b = k[1] / 15.0, krho = k[2];
        k[0] = 4.0 * a + b;
        k[1] = a + b;
        k[2] = 6.0 * b;
        k[3] = 5.0 * b - 4.0 * a;
        k[4] = 4.0 * a - 2.0 * b;
        k[5] = krho;
        break;
    }
    default:
        break;
    }
}

// where the components of an array's nodes are: base[e * group_stride + cols[c] * comp_stride + p]
struct Layout {
    double *base;
    i64 group_stride, comp_stride;
    int cols[kMaxComp];
    int ncomp;
};

struct ConvertArgs {
    i64 ngroups;
    int P;
    int nsteps, steps[kMaxSteps];
    Layout model, kin, out;   // mm_convert_parameters: model = the input, kin is not used
    u64 *nbad;
};

__device__ __forceinline__ void load_node(const Layout &a, i64 at, double (&v)[kMaxComp])
{
#pragma unroll
    for (int c = 0; c < kMaxComp; ++c) v[c] = c < a.ncomp ? a.base[at + a.cols[c] * a.comp_stride] : 0.0;
}

// (out may be an input: no __restrict__ anywhere, every lane has read its node's inputs before it writes)
template <bool KERNELS>
__global__ __launch_bounds__(kThreads) void convert_kernel(const ConvertArgs a)
{
    const i64 n = a.ngroups * a.P;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    unsigned mine = 0;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const i64 e = i / a.P, p = i - e * a.P;
        double v[kMaxComp];
        load_node(a.model, e * a.model.group_stride + p, v);
        if constexpr (KERNELS) {
            double k[kMaxComp];
            load_node(a.kin, e * a.kin.group_stride + p, k);
            double m[kMaxSteps][kMaxComp];   // m[t]: the input of step t
#pragma unroll
            for (int t = 0; t < kMaxSteps; ++t) {
#pragma unroll
                for (int c = 0; c < kMaxComp; ++c) m[t][c] = v[c];   // (past the route's end: never read)
                if (t + 1 < a.nsteps) step_forward(a.steps[t], v);
            }
#pragma unroll
            for (int t = kMaxSteps - 1; t >= 0; --t)
                if (t < a.nsteps) step_transposed(a.steps[t], m[t], k);
#pragma unroll
            for (int c = 0; c < kMaxComp; ++c) v[c] = k[c];
        } else {
#pragma unroll
            for (int t = 0; t < kMaxSteps; ++t)
                if (t < a.nsteps) step_forward(a.steps[t], v);
        }
        const i64 at = e * a.out.group_stride + p;
        bool bad = false;
#pragma unroll
        for (int c = 0; c < kMaxComp; ++c) {
            if (c < a.out.ncomp) {
                a.out.base[at + a.out.cols[c] * a.out.comp_stride] = v[c];
                bad = bad || !mm_is_finite(v[c]);
            }
        }
        if (bad) ++mine;
    }
    if (a.nbad) mm_count_to(a.nbad, mine);
}

// ---- the checks, on the host: nothing below touches the device (one array's: mm_node_layout.h)
Layout layout_of(const double *base, i64 group_stride, i64 comp_stride, const int *cols, int ncomp)
{
    Layout l;
    l.base = const_cast<double *>(base);
    l.group_stride = group_stride;
    l.comp_stride = comp_stride;
    l.ncomp = ncomp;
    for (int c = 0; c < kMaxComp; ++c) l.cols[c] = c < ncomp ? cols[c] : 0;
    return l;
}

int check_pair(const char *who, int from, int to, i64 ngroups, i64 P)
{
    MM_REQUIRE_AS(who, from >= 0 && from < kNumParams && to >= 0 && to < kNumParams, "from and to must lie in 0..4");
    MM_REQUIRE_AS(who, from != to, "from == to: nothing to convert");
    MM_REQUIRE_AS(who, ngroups >= 0, "negative ngroups");
    MM_REQUIRE_AS(who, ngroups < kMaxExtent, "ngroups at or past 2^48");
    MM_REQUIRE_AS(who, P >= 1 && P <= MM_PARAM_MAX_P, "P must lie in [1, 4096]");
    return MM_OK;
}

template <bool KERNELS>
int launch(mm_context *ctx, int from, int to, ConvertArgs &a, int64_t *nbad_d)
{
    a.nsteps = 0;
    for (int t = 0; t < kMaxSteps; ++t) {
        a.steps[t] = kRoute[from][to][t];
        if (a.steps[t] != 0) a.nsteps = t + 1;
    }
    a.nbad = (u64 *)nbad_d;
    if (a.ngroups == 0) return MM_OK;
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(convert_kernel<KERNELS>, dim3(mm_blocks(a.ngroups * a.P, kThreads, kMaxBlocks)), dim3(kThreads), 0,
                       ctx->stream, a);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}

}  // namespace

extern "C" int mm_convert_parameters(mm_context *ctx, int from, int to, int64_t ngroups, int64_t P, const double *in_d,
                                     int64_t in_group_stride, int64_t in_comp_stride, const int *in_cols, double *out_d,
                                     int64_t out_group_stride, int64_t out_comp_stride, const int *out_cols, int64_t *nbad_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    int rc = check_pair(__func__, from, to, ngroups, P);
    if (rc != MM_OK) return rc;
    Span in, out;
    rc = check_array(__func__, "in", ngroups, P, in_d, in_group_stride, in_comp_stride, in_cols, kNcomp[from], false, &in);
    if (rc != MM_OK) return rc;
    rc = check_array(__func__, "out", ngroups, P, out_d, out_group_stride, out_comp_stride, out_cols, kNcomp[to], true, &out);
    if (rc != MM_OK) return rc;
    MM_REQUIRE(ngroups == 0 || same_array(out, in) || disjoint(out, in),
               "out overlaps in without being that array with its strides");
    ConvertArgs a;
    a.ngroups = ngroups;
    a.P = (int)P;
    a.model = layout_of(in_d, in_group_stride, in_comp_stride, in_cols, kNcomp[from]);
    a.kin = a.model;
    a.out = layout_of(out_d, out_group_stride, out_comp_stride, out_cols, kNcomp[to]);
    return launch<false>(ctx, from, to, a, nbad_d);
}

extern "C" int mm_convert_kernels(mm_context *ctx, int from, int to, int64_t ngroups, int64_t P, const double *model_d,
                                  int64_t model_group_stride, int64_t model_comp_stride, const int *model_cols,
                                  const double *kin_d, int64_t kin_group_stride, int64_t kin_comp_stride, const int *kin_cols,
                                  double *kout_d, int64_t kout_group_stride, int64_t kout_comp_stride, const int *kout_cols,
                                  int64_t *nbad_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    int rc = check_pair(__func__, from, to, ngroups, P);
    if (rc != MM_OK) return rc;
    Span model, kin, kout;
    rc = check_array(__func__, "model", ngroups, P, model_d, model_group_stride, model_comp_stride, model_cols, kNcomp[from],
                     false, &model);
    if (rc != MM_OK) return rc;
    rc = check_array(__func__, "kin", ngroups, P, kin_d, kin_group_stride, kin_comp_stride, kin_cols, kNcomp[to], false, &kin);
    if (rc != MM_OK) return rc;
    rc = check_array(__func__, "kout", ngroups, P, kout_d, kout_group_stride, kout_comp_stride, kout_cols, kNcomp[from], true,
                     &kout);
    if (rc != MM_OK) return rc;
    MM_REQUIRE(ngroups == 0 || same_array(kout, model) || disjoint(kout, model),
               "kout overlaps model without being that array with its strides");
    MM_REQUIRE(ngroups == 0 || same_array(kout, kin) || disjoint(kout, kin),
               "kout overlaps kin without being that array with its strides");
    ConvertArgs a;
    a.ngroups = ngroups;
    a.P = (int)P;
    a.model = layout_of(model_d, model_group_stride, model_comp_stride, model_cols, kNcomp[from]);
    a.kin = layout_of(kin_d, kin_group_stride, kin_comp_stride, kin_cols, kNcomp[to]);
    a.out = layout_of(kout_d, kout_group_stride, kout_comp_stride, kout_cols, kNcomp[from]);
    return launch<true>(ctx, from, to, a, nbad_d);
}
