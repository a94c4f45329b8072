// Spherical-harmonic models: coefficients per radial knot evaluated on the nodes of a mesh (include/multimesh_harmonics.h,
// which holds the statement; tests/harmonic_cases.py is its NumPy form).
//
//   mm_harmonic_model_apply : s = lerp over the knot interval of sum_lk (A_lk cos k phi + B_lk sin k phi) P_lk(cos theta);
//                             out = s, in + s or in + in * s
//
// Bit parity with the statement: every product, quotient, sum and square root is rounded on its own (-ffp-contract=off; the
// f64 quotient and square root of the device are correctly rounded), no libm, no float atomics, no matrix instructions (their
// internal summation order cannot be stated); the count of nodes outside the table is an integer sum per workgroup.
//
// Shape.  The tile of mm_radial_model_apply (gll::RunTile): a 256-lane workgroup takes 256 / P whole elements per step, at
// most kMaxBlocks workgroups stride over the tiles; the coordinates go to LDS coalesced, lane e < tile forms element e's centre
// and finds its layer (mm_radial_table, the same device function as the radial kernel), then lane t is node t: one lane per
// node.  A lane holds its direction, its knot interval i and weight t, and per order k two Legendre values, C_k, S_k and
// 4 NC partial sums (U and V at the rows i and i + 1 of NC components) besides the 2 NC running sums S_i, S_{i+1}.
// The (k, l) loops have wave-uniform trip counts and indices, so the recurrence tables d, a, b are uniform addresses: they are
// read through const __restrict__ kernel arguments, which the compiler turns into scalar loads (one per wave, not 64).  The
// coefficient rows depend on i.  The nodes of an element mostly share it: where every live lane of a wave has the same i
// (a ballot), i is read into a scalar register and the rows come through scalar loads too; otherwise each lane gathers its own
// rows (the same arithmetic in the same order: the two paths give the same bits).  Lanes without work (past the tile, a NaN
// centre, an element outside the table) adopt the wave's i and their sums are dropped; a wave with no live lane skips the loops.
// Components: NC = 1..4 unrolled; more than four are served four at a time by further launches (the Legendre recurrence,
// 5 of the 8 NC + 5 operations per term, is repeated per launch; the partial sums of more components would not fit registers).
#include "mm_gll_tile.h"
#include "mm_harmonic_node.h"   // what an element and a node are to this kernel and to its transpose

#include "multimesh_harmonics.h"

namespace {

using namespace mm_stream;   // kThreads, kWave, kMaxBlocks
using namespace mm_harmonic;
constexpr i64 kMaxExtent = (i64)1 << 48;
constexpr int kMaxUnrolled = 4;        // components per launch
typedef unsigned long long u64;

struct HarmonicArgs {
    i64 ngroups;
    int P, m, nlayers, lmax, nlm, mode, extend;
    i64 n;          // values per component of in and out
    const double *in;
    double *out;    // (may be in: no __restrict__, every lane reads its value before writing)
    u64 *noutside;
};

// One order k of the lateral sums: U (and, SINE, V) at the knot rows i and i + 1 of NC components, over l = k .. L.
// rows: the cosine plane of knot row i of the first component; base = idx(k, k); pkk = P_kk.  SINE is false for k = 0
// alone: B[.][idx(l, 0)] is never read.
template <int NC, bool SINE>
__device__ __forceinline__ void order_sums(int k, int L, int base, i64 knot, i64 comp, int nlm,
                                           const double *__restrict__ ta, const double *__restrict__ tb,
                                           const double *__restrict__ rows, double ct, double pkk, double (&U0)[NC],
                                           double (&U1)[NC], double (&V0)[NC], double (&V1)[NC])
{
    // q = idx(l, k); the first term starts every sum
    auto add = [&](int q, double Plk, bool first) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const double *A = rows + c * comp + q;
            const double u0 = A[0] * Plk, u1 = A[knot] * Plk;
            U0[c] = first ? u0 : U0[c] + u0;
            U1[c] = first ? u1 : U1[c] + u1;
            if constexpr (SINE) {
                const double v0 = A[nlm] * Plk, v1 = A[knot + nlm] * Plk;
                V0[c] = first ? v0 : V0[c] + v0;
                V1[c] = first ? v1 : V1[c] + v1;
            }
        }
    };
    add(base, pkk, true);
    double p1 = pkk, p2 = pkk;
    if (k + 1 <= L) {
        p1 = legendre_second(ta[base + 1], ct, pkk);
        add(base + 1, p1, false);
    }
    for (int l = k + 2; l <= L; ++l) {
        const int q = base + (l - k);
        const double Plk = legendre_next(ta[q], tb[q], ct, p1, p2);
        p2 = p1;
        p1 = Plk;
        add(q, Plk, false);
    }
}

// The lateral sums S_i and S_{i+1} of NC components at one direction.  rows: as above -- a scalar (the wave shares i) or one
// pointer per lane; the same statements either way.
template <int NC>
__device__ __forceinline__ void lateral_sums(const HarmonicArgs &args, const double *__restrict__ td,
                                             const double *__restrict__ ta, const double *__restrict__ tb,
                                             const double *__restrict__ rows, double ct, double st, double cp, double sp,
                                             double (&S0)[NC], double (&S1)[NC])
{
    const int L = args.lmax, nlm = args.nlm;
    const i64 knot = 2 * (i64)nlm, comp = (i64)args.m * knot;   // doubles per knot row, per component
    double U0[NC], U1[NC], V0[NC], V1[NC];
    order_sums<NC, false>(0, L, 0, knot, comp, nlm, ta, tb, rows, ct, 1.0, U0, U1, V0, V1);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        S0[c] = U0[c];
        S1[c] = U1[c];
    }
    double pkk = 1.0, C = 1.0, S = 0.0;
    int base = L + 1;   // idx(k, k)
    for (int k = 1; k <= L; ++k) {
        fourier_step(k, cp, sp, C, S);
        pkk = sectoral_step(td[k], st, pkk);
        order_sums<NC, true>(k, L, base, knot, comp, nlm, ta, tb, rows, ct, pkk, U0, U1, V0, V1);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            S0[c] = S0[c] + (U0[c] * C + V0[c] * S);
            S1[c] = S1[c] + (U1[c] * C + V1[c] * S);
        }
        base += L + 1 - k;
    }
}

// NC components starting at coef, args.in and args.out.  (The tables are arguments of their own: __restrict__ on a kernel
// argument is what lets their uniform reads become scalar loads.)
template <int NC>
__global__ __launch_bounds__(kThreads, 4) void harmonic_apply_kernel(const HarmonicArgs args, const double *__restrict__ points,
                                                                  const double *__restrict__ R,
                                                                  const int *__restrict__ lstart,
                                                                  const double *__restrict__ td,
                                                                  const double *__restrict__ ta,
                                                                  const double *__restrict__ tb,
                                                                  const double *__restrict__ coef)
{
    __shared__ double xs[3 * kThreads];
    __shared__ int s_a[kThreads], s_b[kThreads];   // the rows [a, b] of every element's layer; a = kDead, kOutside: none
    __shared__ unsigned s_count[kThreads / kWave];

    const int tid = threadIdx.x, P = args.P, m = args.m;
    const gll::RunTile T(args.ngroups, P);
    const i64 n = args.n;
    const double *in = args.in;
    double *out = args.out;
    const i64 knot = 2 * (i64)args.nlm;
    unsigned mine = 0;   // nodes of elements outside the table

    for (i64 t = blockIdx.x; t < T.ntiles; t += gridDim.x) {
        const int nel = T.nel(t), nnodes = T.nnodes(t);
        const double *src = T.coords(points, t);
        __syncthreads();   // (the previous step's reads of xs, s_a and s_b are done)
        for (int q = tid; q < 3 * nnodes; q += kThreads) xs[q] = src[q];
        __syncthreads();
        if (tid < nel) {
            int a, b;
            element_layer(xs + 3 * tid * P, P, R, m, lstart, args.nlayers, args.extend, a, b);
            s_a[tid] = a;
            s_b[tid] = b;
        }
        __syncthreads();
        const bool node = tid < nnodes;
        const int a = node ? s_a[T.el] : kDead, b = node ? s_b[T.el] : kDead;
        const bool live = a >= 0;
        const double x = node ? xs[3 * tid] : 0.0, y = node ? xs[3 * tid + 1] : 0.0, z = node ? xs[3 * tid + 2] : 0.0;
        if (node && a == kOutside) ++mine;
        int i = 0;
        double w = 0.0;
        const double r = mm_norm3(x, y, z);
        if (live) mm_radial_table::interval_of(R, a, b, r, i, w);
        double S0[NC], S1[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) S0[c] = S1[c] = 0.0;
        const u64 livemask = __ballot(live);
        if (livemask != 0) {   // (the same for every lane of the wave)
            // the direction
            double ct, st, cp, sp;
            direction(x, y, z, r, ct, st, cp, sp);
            const int iu = __builtin_amdgcn_readlane(i, (int)__builtin_ctzll(livemask));   // the first live lane's interval
            if (!live) i = iu;
            if (__ballot(i != iu) == 0)
                lateral_sums<NC>(args, td, ta, tb, coef + iu * knot, ct, st, cp, sp, S0, S1);
            else
                lateral_sums<NC>(args, td, ta, tb, coef + i * knot, ct, st, cp, sp, S0, S1);
        }
        if (node) {
            const i64 at = T.first_node(t) + tid;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const double s = live ? mm_lerp(w, S0[c], S1[c]) : (a == kOutside ? 0.0 : __builtin_nan(""));
                double o = s;
                if (args.mode != 0) {
                    const double v = in[c * n + at];
                    o = args.mode == 1 ? v + s : v + v * s;
                }
                out[c * n + at] = o;
            }
        }
    }
    if (args.noutside) {   // one integer sum per workgroup, one atomic
        mine = wave_sum(mine);
        if ((tid & (kWave - 1)) == 0) s_count[tid / kWave] = mine;
        __syncthreads();
        if (tid == 0) {
            unsigned total = 0;
#pragma unroll
            for (int wv = 0; wv < kThreads / kWave; ++wv) total += s_count[wv];
            if (total != 0) atomicAdd(args.noutside, (u64)total);
        }
    }
}

template <int NC>
void launch(mm_context *ctx, unsigned grid, const HarmonicArgs &a, const double *points, const double *R, const int *lstart,
            const double *td, const double *ta, const double *tb, const double *coef)
{
    hipLaunchKernelGGL(harmonic_apply_kernel<NC>, dim3(grid), dim3(kThreads), 0, ctx->stream, a, points, R, lstart, td, ta,
                       tb, coef);
}

}  // namespace

extern "C" int mm_harmonic_model_apply(mm_context *ctx, const double *points_d, int64_t ngroups, int64_t P,
                                       const double *radius_d, int64_t m, int lmax, const double *coef_d, int64_t ncomp,
                                       int mode, int extend, const double *in_d, double *out_d, int64_t *noutside_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(ngroups >= 0 && ngroups < kMaxExtent, "ngroups out of range");
    MM_REQUIRE(P >= 1 && P <= MM_HARMONIC_MAX_P, "P must lie in [1, 256]");
    MM_REQUIRE(m >= 2 && m < ((i64)1 << 24), "the table needs between 2 and 2^24 rows");
    MM_REQUIRE(lmax >= 0 && lmax <= MM_HARMONIC_MAX_LMAX, "lmax must lie in [0, 255]");
    MM_REQUIRE(ncomp >= 0 && ncomp < 65536, "ncomp out of range");
    MM_REQUIRE(mode >= 0 && mode <= 2, "mode must be 0 .. 2");
    MM_REQUIRE(extend == 0 || extend == 1, "extend must be 0 or 1");
    MM_REQUIRE(radius_d != nullptr && (coef_d != nullptr || ncomp == 0), "null table");
    const i64 nlm = (i64)(lmax + 1) * (lmax + 2) / 2;
    const i64 n = ngroups * P;   // (< 2^56)
    MM_REQUIRE((unsigned __int128)ncomp * (unsigned __int128)n < (unsigned __int128)kMaxExtent,
               "in and out: extent at or past 2^48 elements");
    MM_REQUIRE((unsigned __int128)ncomp * (unsigned __int128)(m * 2 * nlm) < (unsigned __int128)kMaxExtent,
               "coef: extent at or past 2^48 elements");
    const bool work = ngroups > 0 && ncomp > 0;
    MM_REQUIRE(!work || (points_d != nullptr && out_d != nullptr), "null array");
    MM_REQUIRE(!work || mode == 0 || in_d != nullptr, "modes 1 and 2 read in_d");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    // what the kernels need besides the caller's arrays is queued BEFORE the one wait: the recurrence tables from the host,
    // the layer starts from the radii on the device
    std::vector<double> tab;
    double *tab_d = nullptr;
    int *lstart_d = nullptr;
    if (work) {
        recurrence_tables(lmax, tab);
        mm_scratch_layout lay;
        lay.add(&tab_d, tab.size());
        lay.add(&lstart_d, (size_t)m + 1);
        const int rc = lay.commit(ctx, __func__);
        if (rc != MM_OK) return rc;
        MM_HIP_CHECK(hipMemcpyAsync(tab_d, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(layer_starts_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, radius_d, (int)m, lstart_d);
    }
    // the table's radii, checked on the host
    std::vector<double> R((size_t)m);
    MM_HIP_CHECK(hipMemcpyAsync(R.data(), radius_d, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MM_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // (tab and R leave scope with this call)
    std::vector<int> lstart;
    const int table_rc = mm_radial_table_layers(__func__, R.data(), m, lstart);
    if (table_rc != MM_OK) return table_rc;
    if (!work) return MM_OK;
    HarmonicArgs a;
    a.ngroups = ngroups;
    a.P = (int)P;
    a.m = (int)m;
    a.nlayers = (int)lstart.size() - 1;
    a.lmax = lmax;
    a.nlm = (int)nlm;
    a.mode = mode;
    a.extend = extend;
    a.n = n;
    const unsigned grid = mm_blocks(ngroups, kThreads / P, kMaxBlocks);
    const double *td = tab_d, *ta = tab_d + (lmax + 1), *tb = ta + nlm;
    for (i64 c0 = 0; c0 < ncomp; c0 += kMaxUnrolled) {
        const int nc = (int)(ncomp - c0 < kMaxUnrolled ? ncomp - c0 : kMaxUnrolled);
        a.in = in_d ? in_d + c0 * n : nullptr;
        a.out = out_d + c0 * n;
        a.noutside = c0 == 0 ? (u64 *)noutside_d : nullptr;   // (every launch sees the same elements: counted once)
        const double *coef = coef_d + c0 * (m * 2 * nlm);
        switch (nc) {
        case 1: launch<1>(ctx, grid, a, points_d, radius_d, lstart_d, td, ta, tb, coef); break;
        case 2: launch<2>(ctx, grid, a, points_d, radius_d, lstart_d, td, ta, tb, coef); break;
        case 3: launch<3>(ctx, grid, a, points_d, radius_d, lstart_d, td, ta, tb, coef); break;
        default: launch<4>(ctx, grid, a, points_d, radius_d, lstart_d, td, ta, tb, coef); break;
        }
    }
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}
