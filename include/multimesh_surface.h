/*
 * multimesh_surface.h -- an EXTENSION of the C ABI of multi_mesh_hip.so (multimesh_hip.h): the boundary faces of a mesh as
 * triangles through their GLL nodes, and the exact distance of points to that triangulated surface, with a cutoff or with
 * none.  The two entry points live in the same library; they are declared here and not in multimesh_hip.h because that
 * header's set of functions is pinned by the binding tests ("Boundaries").  Bound by
 * multimesh_amd/surface.py.  mm_cutoff_distance (multimesh_hip.h) is the distance to the nearest boundary NODE; this is the
 * distance to the faces between them.
 *
 * THE STATEMENTS, in NumPy's terms: every difference, product, sum, quotient and root is an IEEE-754 binary64 operation
 * rounded on its own, sums run as the parentheses say, no fused multiply-add.  tests/surface_cases.py holds them as code.
 *
 * mm_boundary_triangles.  Inputs as mm_boundary_nodes: points_d f64[nelem][P][3], P = (order + 1)^3, order 1, 2 or 4, node
 * p = i + m j + m m k of an element (m = order + 1); faces_d int64[nb] codes 6 e + f (local face f = 2 * axis + side);
 * side_d int[nb] or NULL (every face is selected); side_mask: bit (1 << side).  The m * m nodes of a face in ascending node
 * index p form a grid q[j][i], i the faster of the face's two free tensor indices.  Each of the order^2 sub-quads (j, i),
 * j-major, gives two triangles, in this order:
 *     (q[j][i], q[j][i+1], q[j+1][i+1])        (q[j][i], q[j+1][i+1], q[j+1][i])
 * written face by face in the order of faces_d into tri_d f64[T][3][3] (triangle, vertex, coordinate: copies of the nodes'
 * bits), which has room for nb * 2 * order^2 triangles.  Returns T = 2 order^2 per selected face.  The surface is therefore
 * the PIECEWISE-LINEAR surface through the faces' nodes: for order 1 the corner quad split along the diagonal q[0][0] --
 * q[1][1]; for a curved order-4 face 32 flat facets whose vertices lie on it, not the polynomial patch itself.
 * MM_ERR_ARG as mm_boundary_nodes: a null ctx, a null array with nb > 0, an order other than 1, 2, 4, nelem outside
 * [0, 2^27), nb outside [0, 6 nelem], side_mask outside [0, 7] (host); a code outside [0, 6 nelem) or a side outside [0, 2]
 * (checked on the device before anything is read through them).  Nothing is written on MM_ERR_ARG.  nb == 0 returns 0.
 *
 * mm_surface_distance.  points_d f64[n][3], tri_d f64[T][3][3], cutoff, dist_d f64[n]:
 *     d_i = cutoff
 *     for every triangle (a, b, c):  q = closest(p_i; a, b, c);  dx, dy, dz = p_i - q;
 *                                    r = sqrt((dx*dx + dy*dy) + dz*dz);  if (r < d_i) d_i = r
 * closest is the region walk of Ericson ("Real-Time Collision Detection", 5.1.5), with u.v = (u0*v0 + u1*v1) + u2*v2 and
 * vector operations component by component; the first condition that holds decides:
 *     ab = b - a; ac = c - a; ap = p - a; d1 = ab.ap; d2 = ac.ap;      if (d1 <= 0 && d2 <= 0) q = a
 *     bp = p - b; d3 = ab.bp; d4 = ac.bp;                              else if (d3 >= 0 && d4 <= d3) q = b
 *     vc = d1*d4 - d3*d2;   else if (vc <= 0 && d1 >= 0 && d3 <= 0) { v = d1 / (d1 - d3); q = a + v*ab }
 *     cp = p - c; d5 = ab.cp; d6 = ac.cp;                              else if (d6 >= 0 && d5 <= d6) q = c
 *     vb = d5*d2 - d1*d6;   else if (vb <= 0 && d2 >= 0 && d6 <= 0) { w = d2 / (d2 - d6); q = a + w*ac }
 *     va = d3*d6 - d5*d4;   else if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0)
 *                               { w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); q = b + w*(c - b) }
 *     else { den = 1.0 / ((va + vb) + vc); v = vb*den; w = vc*den; q = (a + ab*v) + ac*w }
 * (a comparison with a NaN is false, so a NaN falls through to the last branch).  Properties:
 *   - a minimum does not depend on its order: the result is defined by the SET of triangles, bit for bit, whatever their
 *     order and however often one occurs;
 *   - a point that is a vertex of a triangle gets exactly +0.0: the vertex branches return the vertex's own bits;
 *   - a degenerate triangle whose walk produces a NaN (two equal vertices: 0 / 0) is skipped by the test r < d_i; its edges
 *     are still covered by its neighbours in a mesh;
 *   - a point with a coordinate that is not finite keeps cutoff;
 *   - cutoff is positive and at least 2^-500 (as in mm_cutoff_distance); it may be +inf: no cutoff, and with T == 0 every
 *     d is +inf;
 *   - the return value is the number of points with d < cutoff.
 * The device evaluates this statement and nothing else; which triangles a point evaluates is decided by a search that
 * never skips one that could lower d (a grid of cells of about a triangle's size, walked ring by ring outwards from the
 * point until a lower bound on everything beyond the rings reaches d; DESIGN.md section 5 derives the bound and its
 * margin).  The cost depends on how far the nearest triangle is, not on the cutoff; a point that is far outside the
 * triangles' box (more than about 2^20 box sizes) scans every triangle.  Integer atomics only: the same bits on every run.
 * MM_ERR_ARG, with nothing written: a null ctx, a null points_d or dist_d with n > 0, a null tri_d with T > 0; n outside
 * [0, 2^48); T outside [0, 2^30); a cutoff that is not positive, is a NaN or is below 2^-500; a triangle coordinate that is
 * not finite (checked on the device); a bounding box of the triangles whose extent overflows.  T == 0 and n == 0 are valid.
 * Scratch (the context's pool): 72 bytes per ENTRY, an entry being a triangle in a cell its bounding box overlaps -- at
 * most 16 T entries, else the cells are enlarged; about 3 T on a mesh's faces --, and 8 bytes per cell plus the scan's tile
 * sums, at most 2^22 cells; 8 KiB for the histogram that picks the cell edge.
 * Both entry points run on the context's stream and return after it has drained (they read their counts back).
 */
#ifndef MULTIMESH_SURFACE_H
#define MULTIMESH_SURFACE_H

#include "multimesh_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t mm_boundary_triangles(mm_context *ctx, const double *points_d, int64_t nelem, int order, const int64_t *faces_d,
                              const int *side_d, int64_t nb, int side_mask, double *tri_d);

int64_t mm_surface_distance(mm_context *ctx, const double *points_d, int64_t n, const double *tri_d, int64_t T, double cutoff,
                            double *dist_d);

#ifdef __cplusplus
}
#endif
#endif /* MULTIMESH_SURFACE_H */
