// A10 -- GLL elements (order 1, 2, 4; 2-D and 3-D): element search by Newton inversion of the
// isoparametric map, tensor-product Lagrange interpolation coefficients, element-nodal gather.
// Replaces the per-point Python loops of reference multi_mesh/components/interpolator.py:
//   get_element_weights.check_inside :1181-1233 (control flow reproduced here),
//   inverse_transform :1370-1386 and get_coefficients :1337-1347 (thin wrappers over the
//   proprietary salvus.fem package, which is absent: PARITY UNPINNED -- the numerics below are
//   this project's own definition, identical to oracle/mm_oracle.c "A10", pinned by analytic
//   properties: partition of unity, Kronecker property at the nodes, exact reproduction of
//   polynomials up to the element order, order-1 == the hex8 path),
//   and the gather np.sum(coeffs * field[elem_indices], axis=1) :976.
//
// Numerics: tensor-product Lagrange basis on the GLL nodes (order 1: -1,1; order 2: -1,0,1;
// order 4: -1,-sqrt(3/7),0,sqrt(3/7),1), node index p = i + (n+1) j + (n+1)^2 k; Newton from
// xi = 0 with the analytic Jacobian and a cofactor solve; converged when the largest update
// component is < 1e-10, at most 25 updates; NaN when an iterate leaves [-10,10] or the iteration
// does not converge.  Same operation order as the oracle, no fused multiply-add.
//
// One lane per target, control nodes streamed from L1/L2 each Newton step.  Targets are visited in
// the order of their FIRST candidate element (a counting sort by nn[:,0] on the device), so the
// lanes of a wave mostly work on the same element and their control-node loads collapse to one
// cache line per instruction instead of up to 64.  (An element-centric LDS-tiled variant is the
// next step, see DESIGN.md.)
//
// Each step once: gll_judge is THE ACCEPTANCE RULE, gll_settle the end of an unfound target, GllWaveQueue the wave's
// re-queue, gll_next_candidate the id skip -- shared by locate_gll_first_pass_kernel (which owns the LDS staging turns)
// and locate_gll_pass_kernel (which owns the queue it reads and the walk loop); the bounding-box kernel has its own
// control flow and shares the id skip and gll_store_row.  The host helpers are named gll_* as well.
#include <math.h>

#include <type_traits>

#include "mm_common.h"
#include "mm_grid_cell.h"
#include "mm_newton_hex8.h"

namespace {

template <int ORDER>
__device__ __forceinline__ void gll_nodes(double (&g)[ORDER + 1])
{
    if (ORDER == 1) {
        g[0] = -1.0;
        g[ORDER] = 1.0;
    } else if (ORDER == 2) {
        g[0] = -1.0;
        g[1] = 0.0;
        g[ORDER] = 1.0;
    } else {
        const double a = 0x1.4f2ec413cb52ap-1;  // sqrt(3/7)
        g[0] = -1.0;
        g[1] = -a;
        g[ORDER / 2] = 0.0;
        g[ORDER - 1] = a;
        g[ORDER] = 1.0;
    }
}

// 1-D Lagrange values and derivatives: product formulas in a fixed loop order with precomputed
// reciprocals of the node differences (compile-time constants here), identical to the oracle:
//   e[i][m] = (x - g[m]) * (1 / (g[i] - g[m]));  l[i] = prod_{m != i} e[i][m];
//   dl[i] = sum_{m != i} (1/(g[i]-g[m])) * prod_{q != i,m} e[i][q]
template <int ORDER>
__device__ __forceinline__ void lagrange_1d(const double (&g)[ORDER + 1], double x, double (&l)[ORDER + 1],
                                            double (&dl)[ORDER + 1])
{
    constexpr int n = ORDER + 1;
    double inv[n][n], e[n][n];
#pragma unroll
    for (int i = 0; i < n; ++i)
#pragma unroll
        for (int m = 0; m < n; ++m)
            if (m != i) {
                inv[i][m] = 1.0 / (g[i] - g[m]);
                e[i][m] = (x - g[m]) * inv[i][m];
            }
#pragma unroll
    for (int i = 0; i < n; ++i) {
        double v = 1.0;
#pragma unroll
        for (int m = 0; m < n; ++m)
            if (m != i) v = v * e[i][m];
        l[i] = v;
        double d = 0.0;
#pragma unroll
        for (int m = 0; m < n; ++m) {
            if (m == i) continue;
            double t = inv[i][m];
#pragma unroll
            for (int q = 0; q < n; ++q)
                if (q != i && q != m) t = t * e[i][q];
            d = d + t;
        }
        dl[i] = d;
    }
}

// The node loads of the unrolled sum-factorised loops are kept from being hoisted to the top (all (order+1)^3 x 3
// values live at once: spills) by a compiler fence every kGllFenceEvery rows of nodes (cfg5's locate stage, ms:
// every row 5.04, every 2nd 4.92, every 3rd / 5th 5.06 / 5.03, none: 470 registers spilled).  Pinning the running sums
// there as well (round 4) serialised the walking passes' node loads: 0.46 -> 1.0 ms a pass.
constexpr int kGllFenceEvery = 2;
#define MM_GLL_ROW_FENCE(row) do { if ((row) % kGllFenceEvery == 0) asm volatile("" ::: "memory"); } while (0)
// Waves per SIMD the register allocator must leave room for in the GLL locate kernels.  1: it takes what the kernel
// needs -- at order 4 in 3-D 256 VGPRs + ~90 AGPRs, one wave per SIMD, nothing in scratch memory -- and the lower orders
// still run 2 to 5 waves (95 - 211 VGPRs).  Asking for 3 (168 VGPRs, rounds 1 - 2) left 340 registers of the order-4
// kernels in scratch: cfg5's locate stage 6.2 ms at 3, 5.5 at 2 (150 spilled), 5.1 at 1.
constexpr int kGllWaves = 1;
constexpr int kGllValuesWaves = 2;   // waves per SIMD gll_values_kernel is compiled for
constexpr int kGllGuessTrips = 8;    // hex8 trips of the corner solve that starts a 3-D inverse transform (as the oracle's)
constexpr double kGllGuessMax = 3.0;    // a start beyond this (or NaN) is not used

template <int ORDER, int DIM>
struct Gll {
    static constexpr int n = ORDER + 1;
    static constexpr int P = DIM == 3 ? n * n * n : n * n;

    // reference coordinates of pnt inside the element whose control nodes start at ctrl
    // ([P][DIM]); NaNs when the iteration fails
    static __device__ __forceinline__ void inverse_transform(const double (&pnt)[DIM],
                                                             const double *__restrict__ ctrl, double (&xi)[DIM])
    {
        double g[n];
        gll_nodes<ORDER>(g);
#pragma unroll
        for (int d = 0; d < DIM; ++d) xi[d] = 0.0;
        if (DIM == 3 && ORDER >= 2) {
            // Start from the solution of the element's eight CORNERS' trilinear map (newton_hex8_start of
            // mm_newton_hex8.h: at most kGllGuessTrips trips of ~80 fp64 instructions -- the polynomial form of the map,
            // round 4; rounds 2-3 ran the reference-order hex8 iteration here, ~300 a trip -- against ~1.2 k for one step
            // here): a straight-sided element -- its nodes the trilinear images of the GLL points -- is then left
            // after one or two steps instead of five, a curved one after three.  Same arithmetic as the oracle's start
            // (mmo_gll_inverse_transform -> mmo_hex8_start; bit-identical: tests/test_newton_host.py).  A start
            // that is not finite or far outside is not used.
            double cx[8], cy[8], cz[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int node = (MM_R(c) > 0 ? n - 1 : 0) + n * ((MM_S(c) > 0 ? n - 1 : 0) + n * (MM_T(c) > 0 ? n - 1 : 0));
                cx[c] = ctrl[3 * node + 0];
                cy[c] = ctrl[3 * node + 1];
                cz[c] = ctrl[3 * node + 2];
            }
            double q[3];
            newton_hex8_start(pnt[0], pnt[1], pnt[DIM - 1], cx, cy, cz, q, kGllGuessTrips);
            if (fabs(q[0]) <= kGllGuessMax && fabs(q[1]) <= kGllGuessMax && fabs(q[2]) <= kGllGuessMax) {
                xi[0] = q[0];
                xi[1] = q[1];
                xi[DIM - 1] = q[2];
            }
        }
        for (int it = 0; it < 25; ++it) {
            double l[DIM][n], dl[DIM][n];
#pragma unroll
            for (int d = 0; d < DIM; ++d) lagrange_1d<ORDER>(g, xi[d], l[d], dl[d]);
            double x[DIM], J[DIM][DIM];
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                x[a] = 0.0;
#pragma unroll
                for (int b = 0; b < DIM; ++b) J[a][b] = 0.0;
            }
            // Tensor-product (sum-factorised) evaluation of the map and its Jacobian, in exactly the
            // oracle's order of partial sums (mmo_gll_inverse_transform): innermost over i with l0 /
            // dl0, then over j, then over k -- and every partial sum accumulated with ONE fused multiply-add
            // (this path's arithmetic is our own definition, the oracle uses fma() at the same places):
            // ~1.2 k fp64 instructions per step at order 4 instead of 2.1 k, a third of the live registers
            // of the plain triple sum.
            if (DIM == 3) {
#pragma unroll
                for (int k = 0; k < n; ++k) {
                    double b00[3] = {0.0, 0.0, 0.0}, b01[3] = {0.0, 0.0, 0.0}, b10[3] = {0.0, 0.0, 0.0};
#pragma unroll
                    for (int j = 0; j < n; ++j) {
                        // keep the scheduler from hoisting all (order+1)^3 node loads to the top of
                        // the unrolled loop: one row of nodes at a time
                        MM_GLL_ROW_FENCE(j);
                        double a0[3] = {0.0, 0.0, 0.0}, a1[3] = {0.0, 0.0, 0.0};
#pragma unroll
                        for (int i = 0; i < n; ++i) {
                            const double *X = ctrl + 3 * (i + n * (j + n * k));
#pragma unroll
                            for (int a = 0; a < 3; ++a) {
                                const double Xa = X[a];
                                a0[a] = __builtin_fma(l[0][i], Xa, a0[a]);
                                a1[a] = __builtin_fma(dl[0][i], Xa, a1[a]);
                            }
                        }
#pragma unroll
                        for (int a = 0; a < 3; ++a) {
                            b00[a] = __builtin_fma(l[1][j], a0[a], b00[a]);
                            b01[a] = __builtin_fma(dl[1][j], a0[a], b01[a]);
                            b10[a] = __builtin_fma(l[1][j], a1[a], b10[a]);
                        }
                    }
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        x[a] = __builtin_fma(l[DIM - 1][k], b00[a], x[a]);
                        J[a][0] = __builtin_fma(l[DIM - 1][k], b10[a], J[a][0]);
                        J[a][1] = __builtin_fma(l[DIM - 1][k], b01[a], J[a][1]);
                        J[a][DIM - 1] = __builtin_fma(dl[DIM - 1][k], b00[a], J[a][DIM - 1]);
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < n; ++j) {
                    double a0[2] = {0.0, 0.0}, a1[2] = {0.0, 0.0};
#pragma unroll
                    for (int i = 0; i < n; ++i) {
                        const double *X = ctrl + 2 * (i + n * j);
#pragma unroll
                        for (int a = 0; a < 2; ++a) {
                            const double Xa = X[a];
                            a0[a] = __builtin_fma(l[0][i], Xa, a0[a]);
                            a1[a] = __builtin_fma(dl[0][i], Xa, a1[a]);
                        }
                    }
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        x[a] = __builtin_fma(l[1][j], a0[a], x[a]);
                        J[a][0] = __builtin_fma(l[1][j], a1[a], J[a][0]);
                        J[a][1] = __builtin_fma(dl[1][j], a0[a], J[a][1]);
                    }
                }
            }
            double r[DIM], dxi[DIM];
#pragma unroll
            for (int a = 0; a < DIM; ++a) r[a] = x[a] - pnt[a];
            if (DIM == 3) {
                const double c00 = J[1][1] * J[DIM - 1][DIM - 1] - J[1][DIM - 1] * J[DIM - 1][1];
                const double c01 = J[1][DIM - 1] * J[DIM - 1][0] - J[1][0] * J[DIM - 1][DIM - 1];
                const double c02 = J[1][0] * J[DIM - 1][1] - J[1][1] * J[DIM - 1][0];
                const double det = (J[0][0] * c00 + J[0][1] * c01) + J[0][DIM - 1] * c02;
                const double rdet = 1.0 / det;
                const double i00 = c00 * rdet;
                const double i01 = (J[0][DIM - 1] * J[DIM - 1][1] - J[0][1] * J[DIM - 1][DIM - 1]) * rdet;
                const double i02 = (J[0][1] * J[1][DIM - 1] - J[0][DIM - 1] * J[1][1]) * rdet;
                const double i10 = c01 * rdet;
                const double i11 = (J[0][0] * J[DIM - 1][DIM - 1] - J[0][DIM - 1] * J[DIM - 1][0]) * rdet;
                const double i12 = (J[0][DIM - 1] * J[1][0] - J[0][0] * J[1][DIM - 1]) * rdet;
                const double i20 = c02 * rdet;
                const double i21 = (J[0][1] * J[DIM - 1][0] - J[0][0] * J[DIM - 1][1]) * rdet;
                const double i22 = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * rdet;
                dxi[0] = (i00 * r[0] + i01 * r[1]) + i02 * r[DIM - 1];
                dxi[1] = (i10 * r[0] + i11 * r[1]) + i12 * r[DIM - 1];
                dxi[DIM - 1] = (i20 * r[0] + i21 * r[1]) + i22 * r[DIM - 1];
            } else {
                const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
                const double rdet = 1.0 / det;
                dxi[0] = (J[1][1] * r[0] - J[0][1] * r[1]) * rdet;
                dxi[1] = (J[0][0] * r[1] - J[1][0] * r[0]) * rdet;
            }
            double step = 0.0;
            bool bad = false;
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                xi[a] = xi[a] - dxi[a];
                if (fabs(dxi[a]) > step) step = fabs(dxi[a]);
                if (!(fabs(xi[a]) <= 10.0)) bad = true;  // also catches NaN
            }
            if (bad) break;
            if (step < 1e-10) return;   // (the update just applied: what is left is its square)
        }
#pragma unroll
        for (int d = 0; d < DIM; ++d) xi[d] = NAN;
    }

    static __device__ __forceinline__ void coefficients(const double (&xi)[DIM], double *__restrict__ out)
    {
        double g[n];
        gll_nodes<ORDER>(g);
        double l[DIM][n], dl[DIM][n];
#pragma unroll
        for (int d = 0; d < DIM; ++d) lagrange_1d<ORDER>(g, xi[d], l[d], dl[d]);
        if (DIM == 3) {
#pragma unroll
            for (int k = 0; k < n; ++k)
#pragma unroll
                for (int j = 0; j < n; ++j)
#pragma unroll
                    for (int i = 0; i < n; ++i) out[i + n * (j + n * k)] = (l[0][i] * l[1][j]) * l[DIM - 1][k];
        } else {
#pragma unroll
            for (int j = 0; j < n; ++j)
#pragma unroll
                for (int i = 0; i < n; ++i) out[i + n * j] = l[0][i] * l[1][j];
        }
    }

    // sum_p coeff[p] * f[p] in NumPy's row-sum order (np.sum(coeffs * field[elem], axis=1), reference
    // interpolator.py:976; the order is spelled out in mm_gather.hip), coeff[p] formed exactly as
    // coefficients() forms it -- or 0.0 for a point that was not found (`zero`).  One lane, all P
    // terms: the values-only pipeline uses this at the point of acceptance instead of writing the
    // P coefficients (1 kB per target at order 4) for a gather kernel to read back.
    // LEAN (gll_values_kernel): the innermost 1-D values are made opaque at every row, so that the row's coefficient
    // products cannot be formed before it -- left alone the scheduler forms all P of them first (250 registers at
    // order 4 in 3-D: one wave per SIMD)
    template <bool LEAN = false>
    static __device__ __forceinline__ double weighted_sum(const double (&l)[DIM][n], bool zero,
                                                          const double *__restrict__ f)
    {
        constexpr int tail = P & 7, nfull = P - tail;
        double r[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
        double res = 0.;
        constexpr int nk = DIM == 3 ? n : 1;
        double m[n];
#pragma unroll
        for (int i = 0; i < n; ++i) m[i] = l[0][i];
#pragma unroll
        for (int k = 0; k < nk; ++k)
#pragma unroll
            for (int j = 0; j < n; ++j) {
                // one row of field values at a time (see inverse_transform): hoisting all P loads
                // to the top of the unrolled loop spills
                if (LEAN) {
                    // (... and the running sums are pinned at every row: without that the scheduler keeps every loaded
                    // field value in a register and adds them all up at the end)
#pragma unroll
                    for (int i = 0; i < n; ++i) asm volatile("" : "+v"(m[i])::"memory");
#pragma unroll
                    for (int q = 0; q < 8; ++q) asm volatile("" : "+v"(r[q])::"memory");
                    asm volatile("" : "+v"(res)::"memory");
                } else {
                    MM_GLL_ROW_FENCE(j);
                }
#pragma unroll
                for (int i = 0; i < n; ++i) {
                    const int p = i + n * (j + n * k);
                    double c = DIM == 3 ? (m[i] * l[1][j]) * l[DIM - 1][k] : m[i] * l[1][j];
                    if (zero) c = 0.0;
                    const double a = c * f[p];
                    if (P < 8) {
                        res += a;
                    } else if (p < 8) {
                        r[p] = a;
                    } else if (p < nfull) {
                        r[p & 7] += a;
                    }
                    if (P >= 8 && p == nfull - 1)
                        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
                    if (P >= 8 && p >= nfull) res += a;
                }
            }
        return 0.0 + res;   // NumPy starts the reduction from the identity (-0.0 reads +0.0)
    }
};

// What a located target leaves behind: element id and coefficients (the staged mm_locate_gll), and /
// or the interpolated values themselves (mm_interpolate_gll without operator outputs).
struct GllEmit {
    i64 *elem;             // [N] or null
    double *coeffs;        // [N][P] or null
    const double *fields;  // [ncomp][nelem][P] or null
    double *out;           // [N][ncomp] or null
    int ncomp;
    // Deferred values (round 4): with xi_defer the locate kernels only leave {element or -1, reference coordinates}
    // per target and gll_values_kernel forms the weighted sums afterwards -- the same arithmetic in a kernel of its
    // own.  Inside the order-4 locate kernels the unrolled 125-term sum cost 1.4 of the stage's 4.4 ms at cfg5's
    // shape and, worse, registers: those kernels run ONE wave per SIMD (256 VGPRs + ~120 AGPRs).
    double *xi_defer = nullptr;   // [N][DIM] or null
    int *elem_defer = nullptr;    // [N]
};

// The values of one target from {element, xi}: store(c, sum_p coeff_p(xi) * fields[c][e][p]) per component, in NumPy's
// row-sum order (Gll::weighted_sum); a target that was not found reads the LAST element with zero coefficients, like
// NumPy's field[-1] * 0.  (LEAN: the 125 coefficient products do not depend on c -- left alone, the compiler forms them
// all in front of the component loop: 250 registers, one wave per SIMD; weighted_sum<true> forms them row by row.)
template <int ORDER, int DIM, bool LEAN, typename STORE>
__device__ __forceinline__ void gll_target_values(i64 e, const double *xi, bool found, const double *__restrict__ fields,
                                                  i64 nelem, int ncomp, STORE store)
{
    using G = Gll<ORDER, DIM>;
    double g[G::n];
    gll_nodes<ORDER>(g);
    double l[DIM][G::n], dl[DIM][G::n];
#pragma unroll
    for (int d = 0; d < DIM; ++d) lagrange_1d<ORDER>(g, found ? xi[d] : 0.0, l[d], dl[d]);
    const i64 ef = found ? e : nelem - 1;
    for (int c = 0; c < ncomp; ++c)
        store(c, G::template weighted_sum<LEAN>(l, !found, fields + ((i64)c * nelem + ef) * G::P));
}

// Row i of the operator: the element and its P coefficients, or the reference's "-1 and zero coefficients"
template <int ORDER, int DIM>
__device__ __forceinline__ void gll_store_row(i64 *__restrict__ elem, double *__restrict__ coeffs, i64 i, i64 e,
                                              const double (&xi)[DIM], bool found)
{
    using G = Gll<ORDER, DIM>;
    elem[i] = found ? e : -1;
    if (found) G::coefficients(xi, coeffs + i * G::P);
    else
        for (int p = 0; p < G::P; ++p) coeffs[i * G::P + p] = 0.0;
}

template <int ORDER, int DIM, bool DEFER = false>
__device__ __forceinline__ void gll_emit(const GllEmit &em, i64 i, i64 e, const double (&xi)[DIM], bool found, i64 nelem)
{
    if (DEFER) {   // (compile-time: the instance carries neither the coefficient products nor the sums)
        em.elem_defer[i] = found ? (int)e : -1;
#pragma unroll
        for (int d = 0; d < DIM; ++d) em.xi_defer[i * DIM + d] = found ? xi[d] : 0.0;
        return;
    }
    if (em.coeffs) gll_store_row<ORDER, DIM>(em.elem, em.coeffs, i, e, xi, found);   // (the two come together)
    if (em.out)
        gll_target_values<ORDER, DIM, false>(e, xi, found, em.fields, nelem, em.ncomp,
                                             [&](int c, double v) { em.out[i * em.ncomp + c] = v; });
}

// The deferred half of gll_emit (GllEmit::xi_defer): out[i][c] point-major.  One lane per target; neighbouring targets
// lie in the same or neighbouring elements, so a wave's loads of a field row fall on a few lines.
template <int ORDER, int DIM>
__global__ __launch_bounds__(256, kGllValuesWaves) void gll_values_kernel(i64 npoints, const int *__restrict__ elem,
                                                         const double *__restrict__ xi_all,
                                                         const double *__restrict__ fields, i64 nelem, int ncomp,
                                                         double *__restrict__ out)
{
    // (its own copy of gll_target_values<LEAN>, which see: through that function cfg5's gather stage ran 0.542 ms, not 0.534)
    using G = Gll<ORDER, DIM>;
    constexpr int P = G::P;
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npoints) return;
    const int e = elem[i];
    const bool found = e >= 0;
    double g[G::n];
    gll_nodes<ORDER>(g);
    double l[DIM][G::n], dl[DIM][G::n];
#pragma unroll
    for (int d = 0; d < DIM; ++d) lagrange_1d<ORDER>(g, found ? xi_all[i * DIM + d] : 0.0, l[d], dl[d]);
    const i64 ef = found ? (i64)e : nelem - 1;
    for (int c = 0; c < ncomp; ++c)
        out[i * ncomp + c] = G::template weighted_sum<true>(l, !found, fields + ((i64)c * nelem + ef) * P);
}

constexpr int kGllLazyK = 8;   // candidates asked of the kNN stage up front by mm_interpolate_gll
constexpr int kGllWalkFrom = 1; // passes that advance one candidate before the lanes walk their lists (round 4: 1 -- with the
                                // values formed in a kernel of their own the one-candidate passes 1 and 2 cost more than they save: 3.12 -> 2.92 ms)

// The next valid candidate of a list row: j moves past ids outside [0, nelem); returns the id at j, or -1 with
// j == kavail when the row is used up.
template <typename IDX>
__device__ __forceinline__ i64 gll_next_candidate(const IDX *__restrict__ row, int kavail, i64 nelem, int &j)
{
    for (; j < kavail; ++j) {
        const i64 e = (i64)row[j];
        if (e >= 0 && e < nelem) return e;
    }
    return -1;
}

// The least-outside candidate a target has seen so far.  With snap_to_nearest it travels between the passes in two
// scratch arrays: best_state [N][kGllSnapDoubles] (val, then xi -- DIM + 1 of each row's doubles are used) and
// best_elem_state [N]; locate_gll_run puts them into its scratch layout.
constexpr int kGllSnapDoubles = 4;
template <int DIM>
struct GllBest {
    double val = 10e9;
    i64 elem = 0;
    double xi[DIM];
    __device__ __forceinline__ GllBest()
    {
#pragma unroll
        for (int d = 0; d < DIM; ++d) xi[d] = 10e9;
    }
    __device__ __forceinline__ void load(const double *__restrict__ state, const i64 *__restrict__ elem_state, i64 i)
    {
        val = state[i * (DIM + 1)];
#pragma unroll
        for (int d = 0; d < DIM; ++d) xi[d] = state[i * (DIM + 1) + 1 + d];
        elem = elem_state[i];
    }
    __device__ __forceinline__ void save(double *__restrict__ state, i64 *__restrict__ elem_state, i64 i) const
    {
        state[i * (DIM + 1)] = val;
#pragma unroll
        for (int d = 0; d < DIM; ++d) state[i * (DIM + 1) + 1 + d] = xi[d];
        elem_state[i] = elem;
    }
};

// THE ACCEPTANCE RULE (reference interpolator.py:1181-1233, the oracle's mmo_locate_gll): xi = the inverse transform of
// target i in candidate e.  A NaN is skipped; otherwise the candidate becomes the least-outside one if max |xi_d| is
// smaller than the best so far, and it is accepted -- emitted, true returned -- when every |xi_d| < tolerance.
template <int ORDER, int DIM, bool DEFER>
__device__ __forceinline__ bool gll_judge(const double (&xi)[DIM], i64 e, GllBest<DIM> &best, double tolerance,
                                          const GllEmit &em, i64 i, i64 nelem)
{
    bool isnan_any = false;
    double worst = 0.0;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
        if (xi[d] != xi[d]) isnan_any = true;
        if (fabs(xi[d]) > worst) worst = fabs(xi[d]);
    }
    if (isnan_any) return false;
    if (worst < best.val) {
        best.val = worst;
        best.elem = e;
#pragma unroll
        for (int d = 0; d < DIM; ++d) best.xi[d] = xi[d];
    }
    bool inside = true;
#pragma unroll
    for (int d = 0; d < DIM; ++d)
        if (!(fabs(xi[d]) < tolerance)) inside = false;
    if (inside) gll_emit<ORDER, DIM, DEFER>(em, i, e, xi, true, nelem);
    return inside;
}

// A target this pass did not find, next candidate j of k: re-queued (returns true; the snap state saved) while
// candidates are left -- also when the short list is used up and the full one is needed -- else emitted: the
// least-outside candidate clamped to +-1.02 under snap_to_nearest, or "not found" (`missing`).
template <int ORDER, int DIM, bool DEFER>
__device__ __forceinline__ bool gll_settle(i64 i, int j, i64 k, int snap_to_nearest, GllBest<DIM> &best,
                                           double *__restrict__ best_state, i64 *__restrict__ best_elem_state,
                                           const GllEmit &em, i64 nelem, bool &missing)
{
    if (j < k) {
        if (snap_to_nearest) best.save(best_state, best_elem_state, i);
        return true;
    }
    if (snap_to_nearest) {
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
            double v = best.xi[d];
            if (v < -1.02) v = -1.02;
            if (v > 1.02) v = 1.02;
            best.xi[d] = v;
        }
        gll_emit<ORDER, DIM, DEFER>(em, i, best.elem, best.xi, true, nelem);
    } else {
        gll_emit<ORDER, DIM, DEFER>(em, i, 0, best.xi, false, nelem);
        missing = true;
    }
    return false;
}

// Re-queue entries {target, next candidate} are batched per wave in LDS and flushed with one global atomic per ~200
// entries: when a further trip (up to 64 entries) might not fit, and after the wave's last trip.
constexpr int kGllWaveQueue = 256;
constexpr int kGllWaveQueueFlush = kGllWaveQueue - 64;
struct GllWaveQueue {
    int2 *slots;   // [kGllWaveQueue] in LDS, the wave's own
    int held = 0;
    unsigned long long missing_total = 0;
    // every lane of the wave, once per trip
    __device__ __forceinline__ void end_trip(bool requeue, i64 i, int j, bool missing, bool last_trip,
                                             int2 *__restrict__ q_out, int *__restrict__ q_out_count)
    {
        const int lane = threadIdx.x;
        missing_total += __popcll(__ballot(missing));
        const unsigned long long vote = __ballot(requeue);
        if (requeue) slots[held + __popcll(vote & ((1ull << lane) - 1ull))] = make_int2((int)i, j);
        held += __popcll(vote);
        if (held > kGllWaveQueueFlush || (last_trip && held > 0)) {
            int base = 0;
            if (lane == 0) base = atomicAdd(q_out_count, held);
            base = __shfl(base, 0);
            for (int t = lane; t < held; t += 64) q_out[base + t] = slots[t];
            held = 0;
        }
    }
    __device__ __forceinline__ void finish(unsigned long long *__restrict__ nmissing) const
    {
        if (threadIdx.x == 0 && missing_total) atomicAdd(nmissing, missing_total);
    }
};

// Control flow of reference interpolator.py:1181-1233 (see the oracle's mmo_locate_gll), scheduled
// as COMPACTING PASSES like the hex8 locate: a pass performs at most one inverse transform per
// still-open target (candidate j of its list) and re-queues the unresolved ones densely as (target,
// j+1), so a wave never waits for its unluckiest lane's whole candidate walk.  k passes are launched
// (each advances every open target by at least one candidate), the late ones over a nearly empty
// queue.  This kernel owns the per-lane schedule: the queue it reads and the `walk` loop.
template <int ORDER, int DIM, typename IDX, bool DEFER = false>
__global__ __launch_bounds__(64, kGllWaves) void locate_gll_pass_kernel(i64 k, int kavail, i64 npoints,
                                                             const IDX *__restrict__ nn,
                                                             const double *__restrict__ gll_points, i64 nelem,
                                                             const double *__restrict__ points, double tolerance,
                                                             int snap_to_nearest, GllEmit em,
                                                             unsigned long long *__restrict__ nmissing,
                                                             const int *__restrict__ order,
                                                             const int2 *__restrict__ q_in,
                                                             const int *__restrict__ q_in_count,
                                                             int2 *__restrict__ q_out, int *__restrict__ q_out_count,
                                                             double *__restrict__ best_state,
                                                             i64 *__restrict__ best_elem_state,
                                                             int walk)
{
    using G = Gll<ORDER, DIM>;
    constexpr int P = G::P;
    __shared__ int2 s_queue[kGllWaveQueue];
    GllWaveQueue wq{s_queue};

    const i64 total = q_in ? (i64)*q_in_count : npoints;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    const i64 first = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const i64 trips = (total + stride - 1) / stride;
    for (i64 trip = 0; trip < trips; ++trip) {
        const i64 q = first + trip * stride;
        bool requeue = false, missing = false;
        i64 i = 0;
        int j = 0;
        if (q < total) {
            if (q_in) {
                const int2 e = q_in[q];
                i = e.x;
                j = e.y;
            } else {
                i = order ? (i64)order[q] : q;
            }
            double pnt[DIM];
#pragma unroll
            for (int d = 0; d < DIM; ++d) pnt[d] = points[i * DIM + d];
            GllBest<DIM> best;   // (fresh in the first pass)
            if (snap_to_nearest && q_in) best.load(best_state, best_elem_state, i);
            bool found = false;
            do {   // one candidate, or (walk) one after the other until the point is found or the list ends
                // (this array holds the first kavail <= k of the target's list)
                const i64 e = gll_next_candidate(nn + i * kavail, kavail, nelem, j);
                if (e < 0) break;
                double xi[DIM];
                G::inverse_transform(pnt, gll_points + e * (i64)(P * DIM), xi);
                found = gll_judge<ORDER, DIM, DEFER>(xi, e, best, tolerance, em, i, nelem);
                ++j;
            } while (walk && !found);
            if (!found)
                requeue = gll_settle<ORDER, DIM, DEFER>(i, j, k, snap_to_nearest, best, best_state, best_elem_state, em,
                                                        nelem, missing);
        }
        wq.end_trip(requeue, i, j, missing, trip == trips - 1, q_out, q_out_count);
    }
    wq.finish(nmissing);
}

// First pass with the control nodes in LDS.  Targets arrive sorted by their first candidate element
// (~90 per element at cfg5's shape), so the 64 lanes of a wave need one to three elements: up to kStaged
// of them are copied into LDS once per solve (coalesced) and every Newton step reads them from there -- all
// lanes of an element the same address (broadcast) -- instead of going back to L1/L2 for 3 KB per step.  A
// wave with more distinct elements (thinly populated elements) takes further turns of the stage/solve
// loop.  Same arithmetic, same results as locate_gll_pass_kernel with q_in == null.  This kernel owns the staging
// turns, kStaged, the pinned per-lane offset and the wave fences.
template <int ORDER, int DIM, typename IDX, bool DEFER = false>
__global__ __launch_bounds__(64, kGllWaves) void locate_gll_first_pass_kernel(
    i64 k, int kavail, i64 npoints, const IDX *__restrict__ nn, const double *__restrict__ gll_points, i64 nelem,
    const double *__restrict__ points, double tolerance, int snap_to_nearest, GllEmit em,
    unsigned long long *__restrict__ nmissing, const int *__restrict__ order,
    int2 *__restrict__ q_out, int *__restrict__ q_out_count, double *__restrict__ best_state,
    i64 *__restrict__ best_elem_state)
{
    // (Round 4 also sent the LATER passes through this kernel, {target, next candidate} queue entries in the visiting
    // order: slower -- a wave of open targets spans many more than two elements and takes a turn of the stage / solve
    // loop for every pair: 0.9 ms a pass at cfg5's shape against 0.4 for the per-lane kernel.  Taken out again.)
    using G = Gll<ORDER, DIM>;
    constexpr int P = G::P;
    constexpr int kNodeDoubles = P * DIM;
    __shared__ int2 s_queue[kGllWaveQueue];
    GllWaveQueue wq{s_queue};
    // elements staged per turn: two at order 4 in 3-D (3 KB each; four measured slower: 7.9 vs 7.6 ms at cfg5's
    // shape -- a tenth of the waves span more than two elements, every wave pays the LDS), more for small elements
    constexpr int kStaged = kNodeDoubles <= 81 ? 4 : 2;
    __shared__ double s_ctrl[kStaged][kNodeDoubles];
    const int lane = threadIdx.x;

    const i64 stride = (i64)gridDim.x * blockDim.x;
    const i64 first = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const i64 trips = (npoints + stride - 1) / stride;
    for (i64 trip = 0; trip < trips; ++trip) {
        const i64 q = first + trip * stride;
        const bool active = q < npoints;
        bool requeue = false, missing = false;
        i64 i = 0, e = -1;
        int j = 0;
        double pnt[DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) pnt[d] = 0.0;
        if (active) {
            i = order ? (i64)order[q] : q;
#pragma unroll
            for (int d = 0; d < DIM; ++d) pnt[d] = points[i * DIM + d];
            e = gll_next_candidate(nn + i * kavail, kavail, nelem, j);
        }
        bool pending = e >= 0;
        bool found = false;
        GllBest<DIM> best;
        while (__any(pending)) {
            // the (up to) kStaged elements of this turn: the first pending lane's, the first other one, ...
            int which = -1;   // this lane's element among the staged ones (an offset into s_ctrl)
            unsigned long long left = __ballot(pending);
#pragma unroll
            for (int m = 0; m < kStaged; ++m) {
                if (left == 0) break;   // (wave-uniform)
                const i64 em = __shfl(e, __ffsll((long long)left) - 1);
                for (int t = lane; t < kNodeDoubles; t += 64) s_ctrl[m][t] = gll_points[em * (i64)kNodeDoubles + t];
                const bool hit = pending && e == em;
                if (hit) which = m * kNodeDoubles;
                left &= ~__ballot(hit);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const bool mine = which >= 0;
            if (mine) {
                double xi[DIM];
                // a per-lane OFFSET into the staged nodes: with a select between the arrays the compiler
                // reads every node of all of them and picks the values lane by lane (750 v_cndmask_b32 and
                // twice the LDS reads per Newton step at order 4 with two arrays)
                asm volatile("" : "+v"(which));
                G::inverse_transform(pnt, &s_ctrl[0][0] + which, xi);
                found = gll_judge<ORDER, DIM, DEFER>(xi, e, best, tolerance, em, i, nelem);
                ++j;
                pending = false;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();   // every lane is done with the staged nodes
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if (active && !found)
            requeue = gll_settle<ORDER, DIM, DEFER>(i, j, k, snap_to_nearest, best, best_state, best_elem_state, em, nelem,
                                                    missing);
        wq.end_trip(requeue, i, j, missing, trip == trips - 1, q_out, q_out_count);
    }
    wq.finish(nmissing);
}

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v)
{
    int lo = __double2loint(v);
    int hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}

// Element-nodal gather with NumPy's row-sum order (see mm_gather.hip): 8 lanes per target, lane j
// owns the running partial r[j]; the node "ids" are implicit: elem * P + p.
template <bool POINT_MAJOR>
__global__ __launch_bounds__(256) void gather_elem_kernel(const double *__restrict__ fields, i64 nelem, int ncomp,
                                                          const i64 *__restrict__ elem,
                                                          const double *__restrict__ coeffs, i64 npoints, int P,
                                                          double *__restrict__ out)
{
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const i64 n_raw = t >> 3;
    const int j = (int)(t & 7);
    const int group_base = (threadIdx.x & 63) & ~7;
    const bool valid = n_raw < npoints;
    const i64 n = valid ? n_raw : npoints - 1;
    const i64 e_raw = elem[n];
    // -1 (not found, zero coefficients) reads the LAST element like NumPy's field[-1]: the sign of the zero
    const i64 e = (unsigned long long)e_raw < (unsigned long long)nelem ? e_raw
                  : (e_raw < 0 && e_raw >= -nelem ? e_raw + nelem : 0);
    const double *crow = coeffs + n * P;
    const int tail = P & 7;
    const int nfull = P - tail;
    for (int c = 0; c < ncomp; ++c) {
        const double *f = fields + ((i64)c * nelem + e) * P;
        double res;
        if (P < 8) {
            const double a = j < P ? crow[j] * f[j] : 0.0;
            res = 0.;
            for (int i = 0; i < P; ++i) res += __shfl(a, group_base + i);
        } else {
            double r = crow[j] * f[j];
            for (int i = 8; i < nfull; i += 8) r += crow[i + j] * f[i + j];
            double s = r + dpp_f64<0xB1>(r);
            s = s + dpp_f64<0x4E>(s);
            s = s + dpp_f64<0x141>(s);
            const double a = j < tail ? crow[nfull + j] * f[nfull + j] : 0.0;
            res = s;
            for (int i = 0; i < tail; ++i) res += __shfl(a, group_base + i);
        }
        if (valid && j == 0) {
            // NumPy starts a reduction from the identity: 0.0 + (row sum), visible where the sum is -0.0
            if (POINT_MAJOR) out[n * ncomp + c] = 0.0 + res;
            else out[(i64)c * npoints + n] = 0.0 + res;
        }
    }
}

// Lazily evaluated candidate lists (fused pipeline): nn holds only the kavail nearest; after kavail
// passes the still-open targets get their full lists from the generic kNN kernel (list mode) and
// the remaining passes read those.  The k' nearest are the first k' of the k nearest, so results
// do not depend on it.
struct GllLazy {
    const mm_knn_index *index;
    int *nn_full;   // [N][k], rows filled on demand
};

// The fused entries' candidate lists: kavail per target up front (all k, or kGllLazyK when evaluated lazily), int32 rows
struct GllLists {
    bool lazy;
    int kavail;
    int *nn = nullptr, *nn_full = nullptr;
    GllLists(const mm_context *ctx, i64 k) : lazy(ctx->lazy_lists && k > kGllLazyK), kavail(lazy ? kGllLazyK : (int)k) {}
    int get(mm_context *ctx, i64 rows, i64 k)
    {
        int rc = mm_buffer_get(ctx, MM_BUF_NN, (size_t)rows * kavail * sizeof(int), (void **)&nn);
        if (rc == MM_OK && lazy) rc = mm_buffer_get(ctx, MM_BUF_NN_FULL, (size_t)rows * k * sizeof(int), (void **)&nn_full);
        return rc;
    }
};

__global__ __launch_bounds__(256) void gll_queue_ids_kernel(const int2 *__restrict__ q, const int *__restrict__ q_count,
                                                            int *__restrict__ list)
{
    const i64 total = *q_count;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) list[t] = q[t].x;
}

template <int ORDER, int DIM, typename IDX, bool DEFER = false>
int launch_locate(mm_context *ctx, i64 k, int kavail, i64 npoints, const IDX *nn, const double *gll, i64 nelem,
                  const double *pts, double tol, int snap, const GllEmit &em, unsigned long long *nmiss,
                  const int *order, int2 *qa, int2 *qb, int *counters, double *best_state, i64 *best_elem_state,
                  const GllLazy *lazy, int *id_list)
{
    const i64 full_grid = (npoints + 63) / 64;
    // Pass c reads queue c (pass 0: every target) and advances each open target by ONE candidate -- so that a
    // wave never waits for its unluckiest lane while most lanes still have work -- until pass kGllWalkFrom: by
    // then the queue is a sliver of the targets (mostly points that lie outside every candidate and will use
    // up their list) and each further launch would cost a full Newton solve of latency over a nearly empty
    // chip (17 such passes: 2.9 of cfg5's 8.6 ms), so from there a lane walks its list to the end.  With lazy
    // lists the walk ends at the short list's end, the open targets' full lists are fetched once, and one
    // more walking pass finishes them.
    i64 jdone = 0;        // candidates every open target is past
    bool full = false;    // the passes read the full lists (lazy only)
    for (int c = 0; c == 0 || jdone < k; ++c) {
        const int2 *q_in = c == 0 ? nullptr : ((c & 1) ? qa : qb);
        int2 *q_out = (c & 1) ? qb : qa;
        // persistent waves; later passes only know their size on the device
        i64 grid = full_grid >> (c < 6 ? c : 6);
        if (grid > 16384) grid = 16384;
        if (grid < 256) grid = full_grid < 256 ? full_grid : 256;
        if (lazy && !full && jdone >= kavail) {
            hipLaunchKernelGGL(gll_queue_ids_kernel, dim3(64), dim3(256), 0, ctx->stream, q_in, counters + c, id_list);
            int rc = mm_knn_query_list_impl(ctx, lazy->index, pts, npoints, k, lazy->nn_full, id_list, counters + c, -1);
            if (rc != MM_OK) return rc;
            full = true;
        }
        const i64 avail = full ? k : (i64)kavail;
        const int walk = c >= kGllWalkFrom ? 1 : 0;
        if (c == 0 && k > 0 && nelem > 0) {
            hipLaunchKernelGGL((locate_gll_first_pass_kernel<ORDER, DIM, IDX, DEFER>), dim3((unsigned)grid), dim3(64), 0,
                               ctx->stream, k, kavail, npoints, nn, gll, nelem, pts, tol, snap, em, nmiss, order, q_out,
                               counters + c + 1, best_state, best_elem_state);
        } else if (full) {
            hipLaunchKernelGGL((locate_gll_pass_kernel<ORDER, DIM, int, DEFER>), dim3((unsigned)grid), dim3(64), 0, ctx->stream,
                               k, (int)k, npoints, (const int *)lazy->nn_full, gll, nelem, pts, tol, snap, em, nmiss,
                               (const int *)nullptr, q_in, counters + c, q_out, counters + c + 1, best_state,
                               best_elem_state, walk);
        } else {
            hipLaunchKernelGGL((locate_gll_pass_kernel<ORDER, DIM, IDX, DEFER>), dim3((unsigned)grid), dim3(64), 0, ctx->stream,
                               k, kavail, npoints, nn, gll, nelem, pts, tol, snap, em, nmiss, c == 0 ? order : nullptr,
                               q_in, c == 0 ? nullptr : counters + c, q_out, counters + c + 1, best_state,
                               best_elem_state, walk);
        }
        jdone = (walk && c > 0) || (walk && !(k > 0 && nelem > 0)) ? avail : jdone + 1;
    }
    return MM_OK;
}

// ---- variant 1 (reference interpolator.py:1350-1367, :1409-1473; oracle mmo_locate_gll_v1) ----------
// Per element: axis-aligned bounding box of the control nodes and their mean (sequential sum from 0.0
// in node order, divided by P) -- boxes[e] = {min[dim], max[dim], centre[dim]}.  The reference
// recomputes them per candidate and point; they only depend on the element.
template <int ORDER, int DIM>
__global__ __launch_bounds__(256) void gll_box_kernel(i64 nelem, const double *__restrict__ gll_points,
                                                      double *__restrict__ boxes)
{
    constexpr int P = Gll<ORDER, DIM>::P;
    const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nelem) return;
    const double *X = gll_points + e * (i64)(P * DIM);
    double *b = boxes + e * (i64)(3 * DIM);
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
        double mn = X[d], mx = X[d], sum = 0.0;
        for (int p = 0; p < P; ++p) {
            const double v = X[p * DIM + d];
            if (v < mn) mn = v;
            if (v > mx) mx = v;
            sum = sum + v;
        }
        b[d] = mn;
        b[DIM + d] = mx;
        b[2 * DIM + d] = sum / (double)P;
    }
}

// One lane per target, candidates in order (lock-step: this variant is the completeness path, the
// tolerance/snap variant above is the tuned one).
template <int ORDER, int DIM>
__global__ __launch_bounds__(64, kGllWaves) void locate_gll_v1_kernel(i64 k, i64 npoints, const i64 *__restrict__ nn,
                                                              const double *__restrict__ gll_points, i64 nelem,
                                                              const double *__restrict__ boxes,
                                                              const double *__restrict__ points,
                                                              i64 *__restrict__ elem, double *__restrict__ coeffs,
                                                              unsigned long long *__restrict__ nhard,
                                                              const int *__restrict__ order)
{
    using G = Gll<ORDER, DIM>;
    constexpr int P = G::P;
    const i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    bool hard = false;
    if (q < npoints) {
        const i64 i = order ? (i64)order[q] : q;
        double pnt[DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) pnt[d] = points[i * DIM + d];
        i64 first_inside = -1, nearest = -1;
        double nearest_d2 = INFINITY;
        bool found = false;
        double xi[DIM];
        for (int j = 0; !found; ++j) {
            const i64 e = gll_next_candidate(nn + i * k, (int)k, nelem, j);
            if (e < 0) break;
            const double *b = boxes + e * (i64)(3 * DIM);
            bool inside = true;
#pragma unroll
            for (int d = 0; d < DIM; ++d)
                if (!(pnt[d] >= b[d] && pnt[d] <= b[DIM + d])) inside = false;
            if (inside) {
                if (first_inside < 0) first_inside = j;
                G::inverse_transform(pnt, gll_points + e * (i64)(P * DIM), xi);
                bool ok = true;
#pragma unroll
                for (int d = 0; d < DIM; ++d)
                    if (!(fabs(xi[d]) <= 1.04)) ok = false;   // NaN fails the comparison too
                if (ok) {
                    gll_store_row<ORDER, DIM>(elem, coeffs, i, e, xi, true);
                    found = true;
                }
            } else {
                double d2 = 0.0;
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    const double t = pnt[d] - b[2 * DIM + d];
                    d2 = d2 + t * t;
                }
                if (d2 < nearest_d2) {
                    nearest_d2 = d2;
                    nearest = j;
                }
            }
        }
        if (!found) {
            const i64 ind = first_inside >= 0 ? first_inside : nearest;
            if (ind < 0) {
                gll_store_row<ORDER, DIM>(elem, coeffs, i, -1, xi, false);
                hard = true;
            } else {
                const i64 e = nn[i * k + ind];
                G::inverse_transform(pnt, gll_points + e * (i64)(P * DIM), xi);
                bool isnan_any = false, far = false;
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    if (xi[d] != xi[d]) isnan_any = true;
                    if (fabs(xi[d]) >= 1.04) far = true;
                }
                hard = isnan_any;
                if (isnan_any || far) {
                    const double hard_xi[3] = {0.645, -0.5, 0.22};   // reference :1468-1471
#pragma unroll
                    for (int d = 0; d < DIM; ++d) xi[d] = hard_xi[d];
                }
                gll_store_row<ORDER, DIM>(elem, coeffs, i, e, xi, true);
            }
        }
    }
    const unsigned long long mask = __ballot(hard);
    if (threadIdx.x == 0 && mask) atomicAdd(nhard, (unsigned long long)__popcll(mask));
}

// visiting order: counting sort of the targets by their first candidate element
template <typename IDX>
__global__ __launch_bounds__(256) void gll_key_kernel(i64 k, i64 npoints, const IDX *__restrict__ nn, i64 nelem,
                                                      int2 *__restrict__ key_rank, int *__restrict__ counts)
{
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = t < npoints;
    int key = -1;
    if (live) {
        const i64 e = (i64)nn[t * k];
        key = (unsigned long long)e < (unsigned long long)nelem ? (int)e : (int)nelem;  // invalid -> last bin
    }
    // (targets in mesh order arrive in runs with the same first candidate: one atomic per run inside the wave)
    const int rank = count_and_rank(key, live, counts);
    if (live) key_rank[t] = make_int2(key, rank);
}

__global__ __launch_bounds__(256) void gll_order_kernel(i64 npoints, const int2 *__restrict__ key_rank,
                                                        const int *__restrict__ start, int *__restrict__ order)
{
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= npoints) return;
    const int2 kr = key_rank[t];
    order[start[kr.x] + kr.y] = (int)t;
}

}  // namespace

// calls f(std::integral_constant<int, ORDER>, std::integral_constant<int, DIM>) for the (order, dim) the kernels are
// instantiated for; the entry points have refused every other pair before
template <typename F>
static void gll_dispatch(int order, int dim, F &&f)
{
#define MM_GLL_PAIR(O, D) if (order == O && dim == D) f(std::integral_constant<int, O>{}, std::integral_constant<int, D>{});
    MM_GLL_PAIR(1, 2) MM_GLL_PAIR(1, 3) MM_GLL_PAIR(2, 2) MM_GLL_PAIR(2, 3) MM_GLL_PAIR(4, 2) MM_GLL_PAIR(4, 3)
#undef MM_GLL_PAIR
}

// Visiting order: the targets counting-sorted by their first candidate element (invalid ids: the last bin).  add() puts
// its arrays into the caller's layout -- none when there is nothing to sort by --, run() sorts after the caller's commit;
// *visit = the order, or null.
namespace {
struct GllVisit {
    int2 *key_rank = nullptr;
    int *ord = nullptr, *counts = nullptr, *start = nullptr, *tile_sums = nullptr;
    i64 npoints = 0, nbins = 0;
    int kavail = 0;

    void add(mm_scratch_layout &lay, int kavail_, i64 npoints_, i64 nelem)
    {
        if (kavail_ <= 0 || nelem <= 0) return;
        kavail = kavail_;
        npoints = npoints_;
        nbins = nelem + 1;
        lay.add(&key_rank, (size_t)npoints);
        lay.add(&ord, (size_t)npoints);
        lay.add(&counts, (size_t)(nbins + 1));
        lay.add(&start, (size_t)(nbins + 1));
        lay.add(&tile_sums, mm_scan_scratch_ints(nbins));
    }
    template <typename IDX>
    int run(mm_context *ctx, const IDX *nn, const int **visit) const
    {
        *visit = nullptr;
        if (!ord) return MM_OK;
        MM_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)(nbins + 1) * sizeof(int), ctx->stream));
        const unsigned gp = (unsigned)((npoints + 255) / 256);
        hipLaunchKernelGGL((gll_key_kernel<IDX>), dim3(gp), dim3(256), 0, ctx->stream, (i64)kavail, npoints, nn, nbins - 1,
                           key_rank, counts);
        const int rc = mm_exclusive_scan_int(ctx, counts, nbins, start, tile_sums);
        if (rc != MM_OK) return rc;
        hipLaunchKernelGGL(gll_order_kernel, dim3(gp), dim3(256), 0, ctx->stream, npoints, key_rank, start, ord);
        *visit = ord;
        return MM_OK;
    }
};
}  // namespace

// The locate stage on ctx->stream: visiting order, passes, no synchronisation.  nn holds the first
// kavail (<= k) candidates of every target (kavail < k only with `lazy`).  The number of targets
// that were not found is added to ctx->d_counters[0].
template <typename IDX>
static int locate_gll_run(mm_context *ctx, int order, int dim, i64 k, int kavail, i64 npoints, const IDX *nn,
                          const double *gll_points_d, i64 nelem, const double *points_d, double tolerance,
                          int snap_to_nearest, const GllEmit &em, const GllLazy *lazy)
{
    unsigned long long *nm = (unsigned long long *)ctx->d_counters;
    // scratch: two pass queues, their counters, the ids of the open targets, snap state, visiting order
    const size_t snap = snap_to_nearest ? (size_t)npoints : 0;   // rows of the snap state
    int2 *qa, *qb;
    int *counters, *id_list;
    double *best_state = nullptr;
    i64 *best_elem_state = nullptr;
    GllVisit order_work;
    mm_scratch_layout lay;
    lay.add(&qa, (size_t)npoints);
    lay.add(&qb, (size_t)npoints);
    lay.add(&counters, (size_t)(MM_KNN_MAX_K + 8));
    lay.add(&id_list, (size_t)npoints);
    if (snap) {
        lay.add(&best_state, snap * kGllSnapDoubles);
        lay.add(&best_elem_state, snap);
    }
    order_work.add(lay, kavail, npoints, nelem);
    int rc = lay.commit(ctx, __func__, MM_ERR_ARG);   // (MM_ERR_ARG: this stage has always reported a failed carve with MM_REQUIRE)
    if (rc != MM_OK) return rc;
    MM_HIP_CHECK(hipMemsetAsync(counters, 0, sizeof(int) * (MM_KNN_MAX_K + 8), ctx->stream));
    const int *visit = nullptr;
    rc = order_work.run(ctx, nn, &visit);
    if (rc != MM_OK) return rc;
    // (deferred values: only the fused pipeline's int32 lists ask for them)
    constexpr bool kCanDefer = sizeof(IDX) == sizeof(int);
    const bool defer = kCanDefer && em.xi_defer != nullptr;
    gll_dispatch(order, dim, [&](auto o, auto d) {
        constexpr int O = decltype(o)::value, D = decltype(d)::value;
        rc = defer ? launch_locate<O, D, IDX, kCanDefer>(ctx, k, kavail, npoints, nn, gll_points_d, nelem, points_d,
                                                         tolerance, snap_to_nearest, em, nm, visit, qa, qb, counters,
                                                         best_state, best_elem_state, lazy, id_list)
                   : launch_locate<O, D, IDX>(ctx, k, kavail, npoints, nn, gll_points_d, nelem, points_d, tolerance,
                                              snap_to_nearest, em, nm, visit, qa, qb, counters, best_state,
                                              best_elem_state, lazy, id_list);
    });
    if (rc != MM_OK) return rc;
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}

// mm_locate_gll and mm_locate_gll_bbox: their argument rules; the counter cleared before `stage` and read back after it
template <typename F>
static int64_t gll_staged_call(const char *who, mm_context *ctx, int order, int dim, int64_t k, int64_t npoints,
                               const int64_t *nn_d, const double *gll_points_d, int64_t nelem, const double *points_d,
                               const int64_t *elem_d, const double *coeffs_d, F &&stage)
{
    MM_REQUIRE_AS(who, ctx != nullptr, "ctx is null");
    MM_REQUIRE_AS(who, order == 1 || order == 2 || order == 4, "order must be 1, 2 or 4");
    MM_REQUIRE_AS(who, dim == 2 || dim == 3, "dim must be 2 or 3");
    MM_REQUIRE_AS(who, k >= 0 && npoints >= 0 && nelem >= 0, "negative size");
    MM_REQUIRE_AS(who, k <= MM_KNN_MAX_K, "nelem_to_search must be <= MM_KNN_MAX_K");
    MM_REQUIRE_AS(who, npoints == 0 || (elem_d && coeffs_d && points_d), "null array");
    MM_REQUIRE_AS(who, npoints == 0 || k == 0 || (nn_d && gll_points_d), "null array");
    MM_REQUIRE_AS(who, npoints < (int64_t)0x7fffffff && nelem < (int64_t)0x7ffffff0, "too many targets / elements");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    mm_stage_reset(ctx);
    MM_HIP_CHECK(hipMemsetAsync(ctx->d_counters, 0, sizeof(i64), ctx->stream));
    if (npoints > 0) {
        mm_stage_begin(ctx, MM_STAGE_LOCATE);
        const int rc = stage(who);
        mm_stage_end(ctx, MM_STAGE_LOCATE);
        if (rc != MM_OK) return rc;
    }
    MM_HIP_CHECK(hipMemcpyAsync(ctx->h_counters, ctx->d_counters, sizeof(i64), hipMemcpyDeviceToHost, ctx->stream));
    MM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return ctx->h_counters[0];
}

extern "C" int64_t mm_locate_gll(mm_context *ctx, int order, int dim, int64_t k, int64_t npoints,
                                 const int64_t *nn_d, const double *gll_points_d, int64_t nelem,
                                 const double *points_d, double tolerance, int snap_to_nearest, int64_t *elem_d,
                                 double *coeffs_d)
{
    return gll_staged_call(__func__, ctx, order, dim, k, npoints, nn_d, gll_points_d, nelem, points_d, elem_d, coeffs_d,
                           [&](const char *) {
        const GllEmit em = {(i64 *)elem_d, coeffs_d, nullptr, nullptr, 0};
        return locate_gll_run<i64>(ctx, order, dim, k, (int)k, npoints, (const i64 *)nn_d, gll_points_d, nelem, points_d,
                                   tolerance, snap_to_nearest, em, nullptr);
    });
}

// Mean of the control nodes of every element, summed in node order like NumPy's mean(axis=1)
// (reference salvus_mesh_reader.py:99-100) -- the source points of the GLL path's centroid tree.
template <int DIM>
__global__ __launch_bounds__(256) void centroid_nodal_kernel(i64 nelem, int P, const double *__restrict__ gll_points,
                                                             double *__restrict__ out)
{
    const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nelem) return;
    const double *row = gll_points + e * (i64)P * DIM;
    double acc[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) acc[a] = row[a];
    for (int p = 1; p < P; ++p)
#pragma unroll
        for (int a = 0; a < DIM; ++a) acc[a] = acc[a] + row[p * DIM + a];
#pragma unroll
    for (int a = 0; a < DIM; ++a) out[e * DIM + a] = acc[a] / (double)P;
}

// mm_interpolate_gll and mm_sample_columns_gll: the elements' centroid tree (`timed`: as two stages of the call's timers)
static int gll_centroid_tree(mm_context *ctx, int order, int dim, const double *gll_points_d, i64 nelem, bool timed,
                             mm_knn_index **ix)
{
    const int P = dim == 3 ? (order + 1) * (order + 1) * (order + 1) : (order + 1) * (order + 1);
    double *cen = nullptr;
    int rc = mm_buffer_get(ctx, MM_BUF_CENTROID, (size_t)nelem * dim * sizeof(double), (void **)&cen);
    if (rc != MM_OK) return rc;
    if (timed) mm_stage_begin(ctx, MM_STAGE_CENTROID);
    const dim3 g((unsigned)((nelem + 255) / 256)), b(256);
    if (dim == 3) hipLaunchKernelGGL((centroid_nodal_kernel<3>), g, b, 0, ctx->stream, nelem, P, gll_points_d, cen);
    else hipLaunchKernelGGL((centroid_nodal_kernel<2>), g, b, 0, ctx->stream, nelem, P, gll_points_d, cen);
    if (timed) {
        mm_stage_end(ctx, MM_STAGE_CENTROID);
        mm_stage_begin(ctx, MM_STAGE_KNN_BUILD);
    }
    rc = mm_knn_build_impl(ctx, cen, nelem, dim, ix, /*use_context_buffers=*/true, nullptr, 0);
    if (timed) mm_stage_end(ctx, MM_STAGE_KNN_BUILD);
    return rc;
}

static int gll_clear_missing(mm_context *ctx)
{
    const hipError_t e = hipMemsetAsync(ctx->d_counters, 0, sizeof(i64), ctx->stream);
    if (e != hipSuccess) mm_set_error(MM_ERR_HIP, "memset: %s", hipGetErrorString(e));
    return e == hipSuccess ? MM_OK : MM_ERR_HIP;
}

// The end of both calls: the number of missing targets read back (or rc, after the stream has drained), the tree given up
static int64_t gll_finish(mm_context *ctx, int rc, mm_knn_index *ix, const char *what)
{
    int64_t result = rc;
    if (rc == MM_OK) {
        hipError_t e = hipMemcpyAsync(ctx->h_counters, ctx->d_counters, sizeof(i64), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            mm_set_error(MM_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
            result = MM_ERR_HIP;
        } else {
            result = ctx->h_counters[0];
        }
    } else {
        (void)hipStreamSynchronize(ctx->stream);
    }
    if (ix) mm_knn_destroy(nullptr, ix);   // borrowed arrays stay in the context cache
    return result;
}

// The GLL form of the whole path on resident arrays (reference interpolator.py:931-977, and the core of
// gll_2_gll :700-830): element centroids -> k nearest -> element + reference coordinates by the
// acceptance loop of :1181-1233 -> sum of coefficient x element-nodal field value.  Without operator
// outputs the weighted sum is formed where a target is accepted (no [N][P] coefficient array), and
// the candidate lists are evaluated lazily (mm_set_lazy_lists) exactly as in mm_interpolate_hex8.
extern "C" int64_t mm_interpolate_gll(mm_context *ctx, int order, int dim, const double *gll_points_d, int64_t nelem,
                                      const double *points_d, int64_t npoints, const double *fields_d,
                                      int64_t ncomp, int64_t k, double tolerance, int snap_to_nearest,
                                      double *out_d, int64_t *elem_out_d, double *coeffs_out_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(order == 1 || order == 2 || order == 4, "order must be 1, 2 or 4");
    MM_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
    MM_REQUIRE(k >= 1 && k <= MM_KNN_MAX_K, "nelem_to_search must be in 1..MM_KNN_MAX_K");
    MM_REQUIRE(npoints >= 0 && nelem >= 1 && ncomp >= 0, "bad sizes");
    MM_REQUIRE(npoints < (int64_t)0x7fffffff && nelem < (int64_t)0x7ffffff0, "too many targets / elements");
    MM_REQUIRE(ncomp < (1 << 20), "ncomp too large");
    MM_REQUIRE(gll_points_d && (npoints == 0 || points_d), "null array");
    MM_REQUIRE(ncomp == 0 || npoints == 0 || (fields_d && out_d), "null array");
    MM_REQUIRE((elem_out_d == nullptr) == (coeffs_out_d == nullptr), "element and coefficient outputs come together");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    mm_stage_reset(ctx);
    if (npoints == 0) return 0;

    mm_knn_index *ix = nullptr;
    int rc = gll_centroid_tree(ctx, order, dim, gll_points_d, nelem, /*timed=*/true, &ix);
    if (rc != MM_OK) return rc;
    GllLists ls(ctx, k);
    rc = ls.get(ctx, npoints, k);
    if (rc == MM_OK) {
        mm_stage_begin(ctx, MM_STAGE_KNN_QUERY);
        rc = mm_knn_query_impl(ctx, ix, points_d, npoints, ls.kavail, ls.nn, nullptr, /*idx_is_int32=*/true);
        mm_stage_end(ctx, MM_STAGE_KNN_QUERY);
    }
    if (rc == MM_OK) rc = gll_clear_missing(ctx);
    if (rc == MM_OK) {
        mm_stage_begin(ctx, MM_STAGE_LOCATE);
        GllEmit em = {(i64 *)elem_out_d, coeffs_out_d, ncomp > 0 ? fields_d : nullptr, ncomp > 0 ? out_d : nullptr,
                      (int)ncomp};
        // values without the operator: the locate kernels leave {element, xi}, the sums are formed afterwards
        const bool defer = em.out && !em.coeffs;
        if (defer) {
            rc = mm_buffer_get(ctx, MM_BUF_W, (size_t)npoints * dim * sizeof(double), (void **)&em.xi_defer);
            if (rc == MM_OK) rc = mm_buffer_get(ctx, MM_BUF_ENC, (size_t)npoints * sizeof(int), (void **)&em.elem_defer);
        }
        GllLazy lz = {ix, ls.nn_full};
        if (rc == MM_OK)
            rc = locate_gll_run<int>(ctx, order, dim, k, ls.kavail, npoints, ls.nn, gll_points_d, nelem, points_d,
                                     tolerance, snap_to_nearest, em, ls.lazy ? &lz : nullptr);
        mm_stage_end(ctx, MM_STAGE_LOCATE);
        if (rc == MM_OK && defer) {
            mm_stage_begin(ctx, MM_STAGE_GATHER);
            const dim3 g((unsigned)((npoints + 255) / 256)), b(256);
            gll_dispatch(order, dim, [&](auto o, auto d) {
                hipLaunchKernelGGL((gll_values_kernel<decltype(o)::value, decltype(d)::value>), g, b, 0, ctx->stream,
                                   (i64)npoints, (const int *)em.elem_defer, (const double *)em.xi_defer, fields_d,
                                   (i64)nelem, (int)ncomp, out_d);
            });
            mm_stage_end(ctx, MM_STAGE_GATHER);
            if (hipGetLastError() != hipSuccess) {
                mm_set_error(MM_ERR_HIP, "gll_values_kernel launch failed");
                rc = MM_ERR_HIP;
            }
        }
    }
    return gll_finish(ctx, rc, ix, "pipeline");
}

// ---- mm_sample_columns_gll: a model sampled on latitude x longitude x depth columns --------------------------------
// Target t = d * ncol + h of a chunk [t0, t0 + n): radius d, column h -- latitude h / nlon and longitude h % nlon on a
// grid, latitude h and longitude h of a path (paired).  The host gives the trig tables; the point is formed with the
// operations of latlondepth_to_xyz (reference utils.py:526-542) in its order, x = (r * sin colat) * cos lon, ... (no
// fused multiply-add: -ffp-contract=off), so that it is that function's row bit for bit.
__global__ __launch_bounds__(256) void sample_points_kernel(i64 t0, i64 n, i64 ncol, i64 nlon, int paired,
                                                            const double *__restrict__ lat,
                                                            const double *__restrict__ lon,
                                                            const double *__restrict__ radius, double *__restrict__ pts)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const i64 t = t0 + i;
    const i64 d = t / ncol, h = t - d * ncol;
    const i64 a = paired ? h : h / nlon;
    const i64 b = paired ? h : h - a * nlon;
    const double r = radius[d];
    const double rs = r * lat[2 * a];
    pts[3 * i + 0] = rs * lon[2 * b];
    pts[3 * i + 1] = rs * lon[2 * b + 1];
    pts[3 * i + 2] = r * lat[2 * a + 1];
}

// gll_values_kernel for the sampled columns: the same weighted sums (NumPy's row-sum order), written component-major
// out[c * stride + i] (out starts at the chunk's first target), and fill for a target without an element instead of
// NumPy's +-0 of field[-1] * 0.
template <int ORDER>
__global__ __launch_bounds__(256, kGllValuesWaves) void gll_column_values_kernel(i64 npoints, const int *__restrict__ elem,
                                                                 const double *__restrict__ xi_all,
                                                                 const double *__restrict__ fields, i64 nelem,
                                                                 int ncomp, double fill, i64 stride,
                                                                 double *__restrict__ out)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npoints) return;
    const int e = elem[i];
    if (e < 0) {
        for (int c = 0; c < ncomp; ++c) out[(i64)c * stride + i] = fill;
        return;
    }
    gll_target_values<ORDER, 3, true>((i64)e, xi_all + i * 3, true, fields, nelem, ncomp,
                                      [&](int c, double v) { out[(i64)c * stride + i] = v; });
}

// Targets per chunk a call takes when the caller leaves it open (see MM_SAMPLE_CHUNK_BYTES in the header).
static i64 sample_chunk_auto(i64 k, int kavail, bool lazy, bool points_out)
{
    const i64 per = 4 * (i64)kavail + (lazy ? 4 * k : 0) + 3 * 8 + 4 + (points_out ? 0 : 3 * 8) + MM_SAMPLE_STAGE_BYTES;
    const i64 c = MM_SAMPLE_CHUNK_BYTES / per;
    return c < 1 ? 1 : c;
}

// One centroid tree for the whole call, then chunk after chunk: targets generated into the chunk's point buffer (or
// straight into points_out), the k nearest centroids, the acceptance loop of interpolator.py:1181-1233 with deferred
// values (locate_gll_run, as mm_interpolate_gll without operator outputs), the sums into the chunk's slice of out.
// Every target's result depends on its point alone, so the chunking cannot change it.
extern "C" int64_t mm_sample_columns_gll(mm_context *ctx, int order, const double *gll_points_d, int64_t nelem,
                                         const double *fields_d, int64_t ncomp, const double *lat_d, int64_t nlat,
                                         const double *lon_d, int64_t nlon, int paired, const double *radius_d,
                                         int64_t ndepth, int64_t k, double tolerance, double fill_value,
                                         int64_t chunk_points, double *out_d, double *points_out_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(order == 1 || order == 2 || order == 4, "order must be 1, 2 or 4");
    MM_REQUIRE(k >= 1 && k <= MM_KNN_MAX_K, "nelem_to_search must be in 1..MM_KNN_MAX_K");
    MM_REQUIRE(nelem >= 1 && nelem < (int64_t)0x7ffffff0, "nelem must be in 1..0x7ffffff0");
    MM_REQUIRE(ncomp >= 0 && ncomp < (1 << 20), "bad ncomp");
    MM_REQUIRE(nlat >= 0 && nlon >= 0 && ndepth >= 0 && chunk_points >= 0, "negative size");
    MM_REQUIRE(nlat < ((int64_t)1 << 31) && nlon < ((int64_t)1 << 31), "too many latitudes / longitudes");
    MM_REQUIRE(paired == 0 || paired == 1, "paired must be 0 or 1");
    MM_REQUIRE(!paired || nlat == nlon, "a path pairs latitude h with longitude h: nlat must equal nlon");
    const i64 ncol = paired ? nlat : nlat * nlon;
    MM_REQUIRE(ncol == 0 || ndepth <= INT64_MAX / 8 / ncol / (ncomp > 3 ? ncomp : 3), "too many targets");
    const i64 total = ncol * ndepth;
    MM_REQUIRE(total == 0 || (gll_points_d && lat_d && lon_d && radius_d), "null array");
    MM_REQUIRE(total == 0 || ncomp == 0 || (fields_d && out_d), "null array");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    mm_stage_reset(ctx);
    if (total == 0) return 0;

    mm_knn_index *ix = nullptr;
    int rc = gll_centroid_tree(ctx, order, 3, gll_points_d, nelem, /*timed=*/false, &ix);
    if (rc != MM_OK) return rc;
    GllLists ls(ctx, k);
    i64 chunk = chunk_points > 0 ? chunk_points : sample_chunk_auto(k, ls.kavail, ls.lazy, points_out_d != nullptr);
    if (chunk > MM_SAMPLE_CHUNK_MAX) chunk = MM_SAMPLE_CHUNK_MAX;   // the locate stage's int32 target indices
    if (chunk > total) chunk = total;
    int *elem = nullptr;
    double *xi = nullptr, *pts_buf = nullptr;
    rc = ls.get(ctx, chunk, k);
    if (rc == MM_OK) rc = mm_buffer_get(ctx, MM_BUF_W, (size_t)chunk * 3 * sizeof(double), (void **)&xi);
    if (rc == MM_OK) rc = mm_buffer_get(ctx, MM_BUF_ENC, (size_t)chunk * sizeof(int), (void **)&elem);
    if (rc == MM_OK && !points_out_d)
        rc = mm_buffer_get(ctx, MM_BUF_SAMPLE_POINTS, (size_t)chunk * 3 * sizeof(double), (void **)&pts_buf);
    if (rc == MM_OK) rc = gll_clear_missing(ctx);
    GllEmit em = {nullptr, nullptr, nullptr, nullptr, 0};
    em.xi_defer = xi;
    em.elem_defer = elem;
    const GllLazy lz = {ix, ls.nn_full};
    for (i64 t0 = 0; rc == MM_OK && t0 < total; t0 += chunk) {
        const i64 n = total - t0 < chunk ? total - t0 : chunk;
        double *pts = points_out_d ? points_out_d + 3 * t0 : pts_buf;
        const dim3 g((unsigned)((n + 255) / 256)), b(256);
        hipLaunchKernelGGL(sample_points_kernel, g, b, 0, ctx->stream, t0, n, ncol, (i64)nlon, paired, lat_d, lon_d,
                           radius_d, pts);
        rc = mm_knn_query_impl(ctx, ix, pts, n, ls.kavail, ls.nn, nullptr, /*idx_is_int32=*/true);
        if (rc == MM_OK)
            rc = locate_gll_run<int>(ctx, order, 3, k, ls.kavail, n, ls.nn, gll_points_d, nelem, pts, tolerance, 0, em,
                                     ls.lazy ? &lz : nullptr);
        if (rc == MM_OK && ncomp > 0)
            gll_dispatch(order, 3, [&](auto o, auto) {
                hipLaunchKernelGGL((gll_column_values_kernel<decltype(o)::value>), g, b, 0, ctx->stream, n,
                                   (const int *)elem, (const double *)xi, fields_d, (i64)nelem, (int)ncomp, fill_value,
                                   total, out_d + t0);
            });
        if (rc == MM_OK && hipGetLastError() != hipSuccess) {
            mm_set_error(MM_ERR_HIP, "mm_sample_columns_gll: kernel launch failed");
            rc = MM_ERR_HIP;
        }
    }
    return gll_finish(ctx, rc, ix, "mm_sample_columns_gll");
}

extern "C" int mm_gather_elem(mm_context *ctx, const double *fields_d, int64_t nelem, int64_t ncomp,
                              const int64_t *elem_d, const double *coeffs_d, int64_t npoints, int64_t P,
                              double *out_d, int out_point_major)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(nelem >= 0 && ncomp >= 0 && npoints >= 0, "negative size");
    MM_REQUIRE(P >= 1 && P <= 128, "P must be in 1..128");
    MM_REQUIRE(ncomp < (1 << 20), "ncomp too large");
    MM_REQUIRE(npoints == 0 || ncomp == 0 || (fields_d && elem_d && coeffs_d && out_d), "null array");
    MM_REQUIRE(npoints == 0 || ncomp == 0 || nelem >= 1, "empty source mesh");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    mm_stage_reset(ctx);
    if (npoints == 0 || ncomp == 0) return MM_OK;
    const i64 grid = (npoints * 8 + 255) / 256;
    MM_REQUIRE(grid < (i64)0x7fffffff, "too many targets for one launch");
    mm_stage_begin(ctx, MM_STAGE_GATHER);
    if (out_point_major)
        hipLaunchKernelGGL((gather_elem_kernel<true>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, fields_d, nelem,
                           (int)ncomp, (const i64 *)elem_d, coeffs_d, npoints, (int)P, out_d);
    else
        hipLaunchKernelGGL((gather_elem_kernel<false>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, fields_d,
                           nelem, (int)ncomp, (const i64 *)elem_d, coeffs_d, npoints, (int)P, out_d);
    mm_stage_end(ctx, MM_STAGE_GATHER);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}

// Variant 1 of the GLL acceptance loop (bounding-box pre-test; reference interpolator.py:1409-1473).
extern "C" int64_t mm_locate_gll_bbox(mm_context *ctx, int order, int dim, int64_t k, int64_t npoints,
                                      const int64_t *nn_d, const double *gll_points_d, int64_t nelem,
                                      const double *points_d, int64_t *elem_d, double *coeffs_d)
{
    return gll_staged_call(__func__, ctx, order, dim, k, npoints, nn_d, gll_points_d, nelem, points_d, elem_d, coeffs_d,
                           [&](const char *who) -> int {
        double *boxes;
        GllVisit order_work;
        mm_scratch_layout lay;
        lay.add(&boxes, (size_t)(nelem > 0 ? nelem : 1) * 9);
        order_work.add(lay, (int)k, npoints, nelem);
        int rc = lay.commit(ctx, who, MM_ERR_ARG);   // (MM_ERR_ARG, as MM_REQUIRE_AS reported it)
        if (rc != MM_OK) return rc;
        const int *visit = nullptr;
        rc = order_work.run(ctx, (const i64 *)nn_d, &visit);
        if (rc != MM_OK) return rc;
        unsigned long long *nh = (unsigned long long *)ctx->d_counters;
        const unsigned ge = (unsigned)((nelem + 255) / 256), gt = (unsigned)((npoints + 63) / 64);
        gll_dispatch(order, dim, [&](auto o, auto d) {
            constexpr int O = decltype(o)::value, D = decltype(d)::value;
            if (nelem > 0)
                hipLaunchKernelGGL((gll_box_kernel<O, D>), dim3(ge), dim3(256), 0, ctx->stream, nelem, gll_points_d, boxes);
            hipLaunchKernelGGL((locate_gll_v1_kernel<O, D>), dim3(gt), dim3(64), 0, ctx->stream, k, npoints,
                               (const i64 *)nn_d, gll_points_d, nelem, boxes, points_d, (i64 *)elem_d, coeffs_d, nh, visit);
        });
        MM_HIP_CHECK(hipGetLastError());
        return MM_OK;
    });
}
