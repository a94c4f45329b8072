/*
 * multimesh_harmonics.h -- an EXTENSION of the C ABI of multi_mesh_hip.so (multimesh_hip.h): a model given as
 * spherical-harmonic coefficients per radial knot, f(r, theta, phi) = sum_lm c_lm(r) Y_lm(theta, phi), evaluated on the nodes
 * of a mesh or on points that stay in HBM.  The entry point lives in the same library; it is declared here and not in
 * multimesh_hip.h because that header's set of functions is pinned by the binding tests (DESIGN.md section 5,
 * "Spherical-harmonic models").  Bound by multimesh_amd/harmonics.py.
 *
 * ARRAYS, all on the device.  L = lmax, NLM = (L + 1)(L + 2) / 2, n = ngroups * P.
 *   points_d  f64[ngroups][P][3], P nodes per element, 1 <= P <= 256 (P = 1: a point cloud, hex8 nodes).  z is the pole,
 *             latitude is geocentric, longitude runs from x towards y: the geometry of mm_sample_grid.
 *   radius_d  f64[m], ascending; a REPEATED radius marks a discontinuity.  The table rule is mm_radial_model_apply's
 *             (multimesh_hip.h): the layers are the maximal strictly ascending runs; a run of length 1 (m == 1, three equal
 *             radii), a descending step or a non-finite radius is refused with MM_ERR_ARG (the radii are read back and checked
 *             on the host, nothing is written).
 *   coef_d    f64[ncomp][m][2][NLM]: per component and knot row, plane 0 the cosine coefficients A, plane 1 the sine
 *             coefficients B, at idx(l, k) = k * (L + 1) - k * (k - 1) / 2 + (l - k) for degree l and order k, 0 <= k <= l <= L:
 *             the order is the major index, the degrees of one order are contiguous.  B[.][idx(l, 0)] is never read.
 *   in_d      f64[ncomp][n] (modes 1 and 2, else ignored); out_d of that shape, may be in_d (every lane reads its value
 *             before it writes, and touches no other node); otherwise the two may share no byte.
 *   noutside_d int64[1] or NULL: see RADIUS.
 *
 * THE STATEMENT.  Every operation is an IEEE-754 binary64 operation rounded on its own, as written and bracketed here; there is
 * no fused multiply-add (the library is built with -ffp-contract=off) and no libm call: only + - * / sqrt, all correctly
 * rounded, so the result is bit for bit what NumPy gives for the same expressions (tests/harmonic_cases.py).  Sums run left to
 * right from their first term.
 *   DIRECTION of a node (x, y, z):
 *     r = sqrt((x*x + y*y) + z*z);  rho = sqrt(x*x + y*y)
 *     ct = z / r, st = rho / r;     when r == 0:   ct = 0, st = 1   (the equator, as mm_sample_grid's latitude)
 *     cp = x / rho, sp = y / rho;   when rho == 0: cp = 1, sp = 0   (longitude 0, as atan2(0, 0))
 *     Nothing else is special-cased: a NaN coordinate makes the node's outputs NaN, an infinite one gives what the quotients
 *     give (the payload and sign of a NaN that an operation produces are the processor's).
 *   FOURIER FACTORS, by complex multiplication (not by the three-term Chebyshev form):
 *     C_0 = 1, S_0 = 0, C_1 = cp, S_1 = sp;  C_k = C_{k-1} * cp - S_{k-1} * sp;  S_k = S_{k-1} * cp + C_{k-1} * sp
 *   ASSOCIATED LEGENDRE FUNCTIONS, 4-pi-normalised (the integral of Y^2 over the sphere is 4 pi), real, WITHOUT the
 *   Condon-Shortley phase:
 *     P_00 = 1;  P_kk = (d_k * st) * P_{k-1,k-1},  d_1 = sqrt(3.0),  d_k = sqrt((2k + 1) / (2k)) for k >= 2
 *     P_{k+1,k} = (a_{k+1,k} * ct) * P_kk;  P_lk = a_lk * (ct * P_{l-1,k} - b_lk * P_{l-2,k}) for l >= k + 2
 *     a_lk = sqrt(((2l + 1)(2l - 1)) / ((l - k)(l + k)));  b_lk = sqrt(((l - 1 - k)(l - 1 + k)) / ((2l - 1)(2l - 3)))
 *     The integer products are exact in binary64; then one division, then one sqrt.  The library computes d, a and b on the
 *     host and hands them to the kernel.  Nothing is rescaled against underflow: below degree 256 a sectoral term that
 *     underflows near a pole (st^k) is a term whose true value is negligible beside the zonal terms, and gradual underflow
 *     is IEEE arithmetic like the rest.
 *   LATERAL SUM at knot row j, component c:
 *     U_jk = sum_{l = k .. L} A[c][j][idx(l, k)] * P_lk,  V_jk likewise with B (k >= 1)
 *     S_j = term_0 + term_1 + ... + term_L,  term_0 = U_j0,  term_k = U_jk * C_k + V_jk * S_k
 *   RADIUS.  The layer of an element is decided once by its centre, and r', i and t are mm_radial_model_apply's, operation for
 *   operation (one device function serves both kernels): c = (((X[0] + X[1]) + ...) + X[P-1]) / P per coordinate,
 *   rc = sqrt((cx*cx + cy*cy) + cz*cz), the layer with r_lo <= rc < r_hi (below the first layer the first, above the last
 *   the last); a NaN rc makes every output of the element NaN; within the layer's rows [a, b]: r' = min(max(r, R[a]), R[b]),
 *   i = clip(upper_bound(R[a..b], r') - 1, a, b - 1), t = (r' - R[i]) / (R[i+1] - R[i]).  A node on a discontinuity takes the
 *   side of its own element; with P = 1 a point on a discontinuity takes the upper side.
 *     s = (1.0 - t) * S_i + t * S_{i+1}
 *     extend = 1: radii outside the table are clamped, as in mm_radial_model_apply.
 *     extend = 0: an element whose centre radius is below R[0] or above R[m-1] gets s = +0.0 for all its nodes (a mantle
 *       model does not leak into crust or core), whatever their coordinates hold.  The nodes of such elements are counted:
 *       their number is ADDED to *noutside_d (integer sums, one atomic per workgroup: the same on every run); it is not
 *       zeroed.  The nodes of an element inside the table are clamped to its layer like any other.
 *   MODE.  0: out = s    1: out = in + s    2: out = in + in * s  (a relative perturbation such as dlnVs applied to the
 *   mesh's own value)
 *
 * Runs on the context's stream.  Synchronises once, for the table check, before its kernels are queued, and not after.
 * Components are served four at a time (one launch per four); P_lk is computed once per node and launch.
 * MM_ERR_ARG, decided on the host and with nothing written, for a null ctx; a negative ngroups or one at or past 2^48; P
 * outside [1, 256]; m outside [2, 2^24); lmax outside [0, 255]; ncomp outside [0, 65536); a mode outside 0..2; extend other
 * than 0 or 1; a null radius_d, or a null coef_d with ncomp > 0; ncomp * ngroups * P or ncomp * m * 2 * NLM at or past 2^48
 * elements; with ngroups > 0 and ncomp > 0, a null points_d or out_d, or a null in_d in modes 1 and 2; and for the table (see
 * radius_d).  ngroups == 0 and ncomp == 0 are valid: the table is still checked, nothing is computed or counted.
 */
#ifndef MULTIMESH_HARMONICS_H
#define MULTIMESH_HARMONICS_H

#include "multimesh_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MM_HARMONIC_MAX_LMAX 255
#define MM_HARMONIC_MAX_P 256
#define MM_HARMONIC_REPLACE 0
#define MM_HARMONIC_ADD 1
#define MM_HARMONIC_RELATIVE 2

int mm_harmonic_model_apply(mm_context *ctx, const double *points_d, int64_t ngroups, int64_t P,
                            const double *radius_d, int64_t m, int lmax, const double *coef_d, int64_t ncomp,
                            int mode, int extend, const double *in_d, double *out_d, int64_t *noutside_d);

#ifdef __cplusplus
}
#endif
#endif /* MULTIMESH_HARMONICS_H */
