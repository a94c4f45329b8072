/*
 * multimesh_frames.h -- an EXTENSION of the C ABI of multi_mesh_hip.so (multimesh_hip.h): FRAMES -- points and the three
 * components of a vector field rotated by a 3 x 3 matrix, and vector components moved between the Cartesian basis and the
 * local spherical basis at every node, on arrays that stay in HBM.  The three entry points live in the same library; they
 * are declared here and not in multimesh_hip.h because that header's set of functions is pinned by the binding tests
 * ("Frames").  Bound by multimesh_amd/frames.py.
 *
 * THE STATEMENT.  Every product, quotient, sum and square root is an IEEE-754 binary64 operation rounded on its own, as
 * written and bracketed here, sums left to right; no fused multiply-add (the library is built with -ffp-contract=off), no
 * libm.  Nothing is special-cased beyond what is written: NaN, +-inf, -0.0 and denormals give what IEEE arithmetic gives (the
 * payload and sign of a NaN that an operation produces are the processor's).  tests/frames_cases.py is the NumPy form.
 *
 * ROTATION of (x, y, z) by R, a HOST array of nine doubles, row-major (Rij = R[3 * i + j]), copied into the kernel's
 * arguments:
 *     x' = (R00*x + R01*y) + R02*z
 *     y' = (R10*x + R11*y) + R12*z
 *     z' = (R20*x + R21*y) + R22*z
 * With transpose != 0 the statement reads Rji where it says Rij.  R is any nine finite doubles: that it is orthogonal is the
 * caller's business (multimesh_amd.frames.Rotation checks it).
 *
 * LOCAL BASIS at a node with position (x, y, z):
 *     r = sqrt((x*x + y*y) + z*z);  s = sqrt(x*x + y*y)
 *     cp = x / s and sp = y / s where s > 0, else cp = 1.0 and sp = 0.0   (cos and sin of the longitude; a node on the polar
 *                                                                          axis, or with a NaN s, takes longitude 0)
 *     ct = z / r;  st = s / r                                             (of the colatitude; r = 0 gives NaN by 0 / 0)
 *   direction 0, Cartesian (vx, vy, vz) -> local:
 *     a_r = ((st*cp)*vx + (st*sp)*vy) + ct*vz
 *     a_t = ((ct*cp)*vx + (ct*sp)*vy) - st*vz
 *     a_p = cp*vy - sp*vx
 *   direction 1, local -> Cartesian:
 *     vx = ((st*cp)*a_r + (ct*cp)*a_t) - sp*a_p
 *     vy = ((st*sp)*a_r + (ct*sp)*a_t) + cp*a_p
 *     vz = ct*a_r - st*a_t
 *   basis 0: the three local components are (radial, south, east) = (a_r, a_t, a_p).
 *   basis 1: (up, north, east) = (a_r, -a_t, a_p): the second component is the exact negation (the sign bit flipped, of a
 *            NaN too) of a_t, on the way out in direction 0 and on the way in in direction 1.
 *
 * ARRAYS, all on the device.
 *   mm_rotate_points: in_d and out_d are f64[n][3] -- also the flat form of element-nodal points [E][P][3].  out_d == in_d is
 *     allowed (a lane reads its point before it writes it); any other overlap of the two extents is refused.
 *   mm_rotate_vectors and mm_local_components address the three components of a field by the ADDRESSING paragraph of
 *     multimesh_params.h: component c of node p of group e is base[e * group_stride + cols[c] * comp_stride + p], in elements;
 *     field planes [C][E][P] have group_stride = P, comp_stride = E * P; MODEL/data rows [E][C_total][P] have
 *     group_stride = C_total * P, comp_stride = P.  cols are HOST arrays of three ints.  The output may be the input array
 *     with the same strides (every lane reads its node's three inputs before it writes, and touches no other node; the
 *     columns may then be permuted); otherwise it may share no byte with the input.
 *   points_d of mm_local_components is f64[ngroups * P][3], the position of node e * P + p; it may share no byte with out_d.
 *
 * All three run on the context's stream and do not synchronise; one launch each, one lane per point or node, no atomics.
 * MM_ERR_ARG, decided on the host with nothing written and before the device is touched:
 *   all:  a null ctx.
 *   mm_rotate_points: a negative n, or 3 * n at or past 2^48; a null R or an R that is not finite; with n > 0, a null in_d
 *     or out_d, or extents that overlap without out_d == in_d.  n == 0 is valid.
 *   mm_rotate_vectors, mm_local_components: what multimesh_params.h refuses of an array -- a null array (allowed when
 *     ngroups == 0) or cols; a negative ngroups, or one at or past 2^48; P outside [1, MM_PARAM_MAX_P]; a negative column
 *     or stride; two equal output columns; an output layout in which two nodes or components share an element; an extent
 *     (ngroups - 1) * group_stride + max(cols) * comp_stride + P at or past 2^48 elements; an output that overlaps the
 *     input without being that array with its strides.  mm_rotate_vectors: R and transpose as above.  mm_local_components:
 *     direction or basis outside {0, 1}; with ngroups > 0, a null points_d, 3 * ngroups * P at or past 2^48, or points that
 *     overlap the output's extent.
 *     ngroups == 0 is valid.
 */
#ifndef MULTIMESH_FRAMES_H
#define MULTIMESH_FRAMES_H

#include "multimesh_hip.h"
#include "multimesh_params.h" /* MM_PARAM_MAX_P */

#ifdef __cplusplus
extern "C" {
#endif

#define MM_FRAMES_TO_LOCAL 0
#define MM_FRAMES_TO_CARTESIAN 1
#define MM_FRAMES_BASIS_RTP 0
#define MM_FRAMES_BASIS_ZNE 1

/* out = R p (transpose != 0: R^T p), point by point. */
int mm_rotate_points(mm_context *ctx, int64_t n, const double *in_d, double *out_d, const double *R, int transpose);

/* out = R v (transpose != 0: R^T v) of the three components of a vector field, node by node. */
int mm_rotate_vectors(mm_context *ctx, int64_t ngroups, int64_t P,
                      const double *in_d, int64_t in_group_stride, int64_t in_comp_stride, const int *in_cols,
                      double *out_d, int64_t out_group_stride, int64_t out_comp_stride, const int *out_cols,
                      const double *R, int transpose);

/* The components of a vector field in the local basis at each node's position (direction 0), or back (direction 1). */
int mm_local_components(mm_context *ctx, int64_t ngroups, int64_t P, const double *points_d,
                        const double *in_d, int64_t in_group_stride, int64_t in_comp_stride, const int *in_cols,
                        double *out_d, int64_t out_group_stride, int64_t out_comp_stride, const int *out_cols,
                        int direction, int basis);

#ifdef __cplusplus
}
#endif
#endif /* MULTIMESH_FRAMES_H */
