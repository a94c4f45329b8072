/*
 * multimesh_harmonic_adjoint.h -- a second EXTENSION header of the C ABI of multi_mesh_hip.so, on top of
 * multimesh_harmonics.h: the TRANSPOSE of mm_harmonic_model_apply (mode 0).  The forward call evaluates coefficients per radial
 * knot on the nodes of a mesh, f = H c; this one brings values on the nodes onto the coefficients, grad = H^T (w o v): the
 * gradient of a misfit with respect to c_lm(r) from a sensitivity kernel on the mesh, and, with the forward call, the two
 * halves of a least-squares expansion of a mesh field in spherical harmonics.  It has a header of its own because the
 * contents of multimesh_harmonics.h are pinned by that unit's tests ("Spherical-harmonic transpose").
 * Bound by multimesh_amd/harmonic_adjoint.py.
 *
 * ARRAYS, all on the device.  L = lmax, NLM = (L + 1)(L + 2) / 2, n = ngroups * P.  points_d, radius_d, idx(l, k) and the
 * table rule are multimesh_harmonics.h's.
 *   weight_d  f64[n] or NULL (no weights): a mass matrix, say
 *   values_d  f64[ncomp][n]
 *   grad_d    f64[ncomp][m][2][NLM], the layout of coef_d: OVERWRITTEN, every entry, not added to.  It may share no byte with
 *             an input.
 *   noutside_d int64[1] or NULL: added to, as in the forward call
 *
 * THE STATEMENT.  Every operation is an IEEE-754 binary64 operation rounded on its own, as written and bracketed here; no
 * fused multiply-add, no libm, no float atomics: the result is bit for bit what NumPy gives for the same expressions
 * (tests/harmonic_adjoint_cases.py), on every run.
 *   A NODE.  Everything about a node is mm_harmonic_model_apply's, operation for operation (the two kernels share the device
 *   functions): the direction ct, st, cp, sp; C_k, S_k and P_lk with the tables d, a, b; the element's centre picking the
 *   layer; r', i, t; and the meaning of extend.
 *   PER NODE AND COMPONENT c:
 *     g = weight[n] * values[c][n]                 (without weight_d: g = values[c][n])
 *     e0 = (1.0 - t) * g,  e1 = t * g
 *     order k >= 1: a0 = e0 * C_k, b0 = e0 * S_k, a1 = e1 * C_k, b1 = e1 * S_k;  order 0: a0 = e0, a1 = e1, no b
 *     the node's terms for its interval i, at q = idx(l, k):
 *       cosine plane: a0 * P_lk into Lo_i, a1 * P_lk into Hi_i;   sine plane (k >= 1): b0 * P_lk into Lo_i, b1 * P_lk into Hi_i
 *   WHICH NODES TAKE PART.  The nodes of an element with a NaN centre take no part (the forward call writes NaN there: the
 *   transpose of "untouched" is nothing).  With extend = 0 the nodes of an element outside the table take no part either; their
 *   number is ADDED to *noutside_d exactly as in the forward call (once per call, whatever the number of components or passes).
 *   A NaN in a live node's coordinates, weight or value goes where the arithmetic takes it: into every term of the node.
 *   THE ORDER OF THE SUMS: a definition, not a launch shape.
 *     Gs = max(1, 16384 / P) (integer division); segment s holds the groups [s * Gs, (s + 1) * Gs).
 *     For every output value, interval i and side (Lo, Hi) the SEGMENT SUM starts from +0.0 and adds the terms of the
 *     segment's nodes that lie in interval i, in ascending node index; the other nodes are skipped (a sum that starts from
 *     +0.0 is never -0.0, so skipping and adding +0.0 are the same bits).
 *     The segment sums are added in ascending s, from +0.0: Lo_i and Hi_i.
 *     grad[c][j][plane][q] = Lo_j + Hi_{j-1},  with Hi_{-1} = +0.0 and Lo_{m-1} = +0.0.
 *     The last row of a layer has an empty Lo (no node has the interval between the two rows of a repeated radius), the
 *     first an empty Hi: across a discontinuity nothing mixes.  The sine plane at k = 0 is +0.0.  No output is -0.0.
 *
 * SCRATCH.  The segment sums live in the context's scratch: 4 (m - 1) nseg doubles per component and (l, k), nseg =
 * ceil(ngroups / Gs).  scratch_limit bounds them in bytes (0: MM_HARMONIC_ADJOINT_SCRATCH, 1 GiB).  When they do not all fit,
 * the call runs several passes, each over a range of orders k of one or two components; a pass starts its recurrences at its
 * first order (P_kk and C_k, S_k cost O(k) to reach).  The order of every sum is defined per output value, so the bits do not
 * depend on the split.  MM_ERR_UNSUPPORTED, with nothing written, when order 0 of one component (the largest) does not fit.
 * The recurrence tables, the layer starts (m + 1 int32) and nothing else come on top of the limit.
 *
 * Runs on the context's stream.  Synchronises once, for the table check, before its kernels are queued, and not after.
 * MM_ERR_ARG, decided on the host and with nothing written: the conditions of mm_harmonic_model_apply on ctx, ngroups, P,
 * m, lmax, ncomp, extend, radius_d, the extents and the table; a negative scratch_limit; with ncomp > 0 a null grad_d; with
 * ngroups > 0 and ncomp > 0 a null points_d or values_d.  ngroups == 0 with ncomp > 0 writes +0.0 everywhere.  ncomp == 0
 * checks the table only: nothing is computed or counted.
 */
#ifndef MULTIMESH_HARMONIC_ADJOINT_H
#define MULTIMESH_HARMONIC_ADJOINT_H

#include "multimesh_harmonics.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MM_HARMONIC_SEGMENT_NODES 16384
#define MM_HARMONIC_ADJOINT_SCRATCH ((int64_t)1 << 30)

int mm_harmonic_model_transpose(mm_context *ctx, const double *points_d, int64_t ngroups, int64_t P,
                                const double *radius_d, int64_t m, int lmax, const double *weight_d,
                                const double *values_d, int64_t ncomp, int extend, double *grad_d, int64_t *noutside_d,
                                int64_t scratch_limit);

#ifdef __cplusplus
}
#endif
#endif /* MULTIMESH_HARMONIC_ADJOINT_H */
