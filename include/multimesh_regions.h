/*
 * multimesh_regions.h -- an EXTENSION of the C ABI of multi_mesh_hip.so (multimesh_hip.h): REGIONS drawn on the sphere as rings
 * of great-circle edges -- a continent, the area with ray coverage, the footprint of a regional model.  One entry point gives
 * for every node whether it lies inside the region and its distance to the region's outline up to a cutoff.  It lives in the
 * same library; it is declared here and not in multimesh_hip.h because that header's set of functions is pinned by the binding
 * tests ("Regions").  Bound by multimesh_amd/regions.py.
 *
 * ARRAYS, all on the device.
 *   points_d  f64[ngroups][P][3], 1 <= P <= 256, as in mm_point_taper (P = 1: a point cloud or the nodes of a hex8 mesh).  Only
 *             a node's direction counts: z is the pole, as in mm_sample_grid.
 *   edges_d   f64[E][9], 0 <= E <= 2^20: one row (U, V, N) per edge, the shorter great-circle arc from the unit vector U to the
 *             unit vector V, and N the unit normal of U x V FORMED BY THESE OPERATIONS (the device checks the bits):
 *               c = (U1*V2 - U2*V1, U2*V0 - U0*V2, U0*V1 - U1*V0);  n = sqrt((c0*c0 + c1*c1) + c2*c2);  N = (c0/n, c1/n, c2/n)
 *             Rings, holes and several polygons are all just edges: inside is even-odd.  The two rows that share a vertex must
 *             hold the same three doubles for it, which makes the half-open rule below consistent.
 *   anchor_d  f64[3]: a unit vector a, not near the outline, whose status anchor_inside (0 / 1) the caller states.
 *   signed_out_d  f64[n] or NULL, inside_out_d int32[n] or NULL (n = ngroups * P); not both NULL.
 *   info_d    int64[2] or NULL: receives {nodes with hit, invalid nodes}.
 * cutoff is a chord on the unit sphere, 0 < cutoff <= 2; scale is metres per unit chord, positive and finite.
 *
 * THE STATEMENT.  Every operation is an IEEE-754 binary64 operation rounded on its own, as written and bracketed here; no
 * fused multiply-add (the library is built with -ffp-contract=off), nothing but + - * / sqrt and comparisons: the whole
 * result is bit for bit what NumPy gives for the same expressions (tests/regions_cases.py).  dot(x, y) = (x0*y0 + x1*y1) +
 * x2*y2;  cross(x, y) = (x1*y2 - x2*y1, x2*y0 - x0*y2, x0*y1 - x1*y0).  Per node x, for the edges in ascending order:
 *
 *   r = sqrt((x0*x0 + x1*x1) + x2*x2)
 *   if r is not finite or not >= 2^-500:   s = -(scale*cutoff), inside = 0, the node is counted as INVALID, done
 *        (the centre, and a node so near it that the squares of its coordinates leave the normal range: its p would be no unit
 *        vector, which the exactness of the culls needs)
 *   p = (x0/r, x1/r, x2/r);   m = cross(p, a)
 *   q = cutoff*cutoff;  hit = 0;  ncross = 0
 *   per edge (U, V, N):
 *     su = dot(m, U);  sv = dot(m, V);  tp = dot(N, p);  ta = dot(N, a)
 *     if ((su >= 0) != (sv >= 0)) and ((tp >= 0) != (ta >= 0)) and ((ta >= 0) == (su >= 0)):  ncross += 1
 *     w1 = dot(cross(U, p), N);  w2 = dot(cross(p, V), N)
 *     if w1 >= 0 and w2 >= 0:  g = 1.0 - tp*tp;  if (g < 0.0) g = 0.0;  qe = (2.0*(tp*tp)) / (1.0 + sqrt(g))
 *     else:                    qe = min(|p-U|^2, |p-V|^2)   with |d|^2 = (d0*d0 + d1*d1) + d2*d2, d = p - U
 *     if (qe < q) { q = qe; hit = 1 }
 *   inside = anchor_inside ^ (ncross & 1)
 *   d = hit ? scale*sqrt(q) : scale*cutoff;   s = inside ? d : -d
 *
 * The crossing rule is the four-orientation test of the arcs a -> p and U -> V with a half-open sign (>= 0 is one side, -0.0
 * included): an arc a -> p that passes exactly through a vertex is counted once.  2h^2 / (1 + sqrt(1 - h^2)) is the squared
 * chord to the great circle without cancellation at small distances.  q is a minimum and ncross a sum: neither depends on the
 * order of the edges.  DEGENERATE: p == a and p == -a give m = (+-0, +-0, +-0), every su and sv passes >= 0, nothing crosses:
 * the anchor and its antipode have the anchor's status.  A node on a vertex or an edge has d == 0.0 or within rounding of it and
 * the status the signs give.
 *
 * Returns the number of inside nodes (>= 0).  Integer sums, one atomic per workgroup and count: the same on every run.
 * Synchronises.  Runs on the context's stream; its scratch (68 bytes per 32 edges, rounded up) is the context's.
 * MM_ERR_ARG with nothing written for a null ctx; a null points_d with ngroups > 0, a null edges_d with E > 0, a null anchor_d;
 * both outputs NULL; ngroups negative or at or past 2^48; P outside [1, 256]; E outside [0, 2^20]; cutoff not in (0, 2]; scale
 * not positive and finite; anchor_inside not 0 / 1 -- all decided before the device is touched -- and, checked on the device:
 * an anchor that is not finite or whose dot(a, a) differs from 1 by more than 2^-48; an edge entry that is not finite; a U or
 * V whose dot with itself differs from 1 by more than 2^-48; |U - V|^2 or |U + V|^2 below 2^-40 (an edge shorter than a chord
 * of 2^-20, six metres on the Earth, or that close to antipodal: its great circle is not determined); an N that is not the
 * formula above, bit for bit.  E == 0 is valid: every valid node has the anchor's status and |s| = scale*cutoff.  ngroups == 0
 * is valid.
 */
#ifndef MULTIMESH_REGIONS_H
#define MULTIMESH_REGIONS_H

#include "multimesh_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MM_REGION_MAX_EDGES 1048576
#define MM_REGION_EDGE_CHUNK 32

int64_t mm_region_distance(mm_context *ctx, const double *points_d, int64_t ngroups, int64_t P, const double *edges_d, int64_t E,
                           const double *anchor_d, int anchor_inside, double cutoff, double scale,
                           double *signed_out_d, int *inside_out_d, int64_t *info_d);

#ifdef __cplusplus
}
#endif
#endif /* MULTIMESH_REGIONS_H */
