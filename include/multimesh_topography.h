/*
 * multimesh_topography.h -- an EXTENSION of the C ABI of multi_mesh_hip.so (multimesh_hip.h): a RADIAL STRETCHING of the nodes
 * of a mesh between anchor radii, driven by a latitude x longitude map of interface positions (surface elevation, Moho, any
 * honoured discontinuity), and its inverse, the FLATTENING, which returns every node's 1-D reference radius.  The entry point
 * lives in the same library; it is declared here and not in multimesh_hip.h because that header's set of functions is pinned by
 * the binding tests ("Topography").  Bound by multimesh_amd/topography.py.
 *
 * ARRAYS, all on the device.
 *   points_d  f64[n][3].  z is the pole, latitude is geocentric, longitude runs from x towards y: the geometry of mm_sample_grid.
 *   ref_radius_d  f64[n] or NULL: the 1-D reference radius of every node, for direction = 0 (a mesh that carries z_node_1D
 *             passes z_node_1D * 6371000).  It must be NULL with direction = 1, which computes it.
 *   lat_d     f64[nlat], lon_d f64[nlon]: strictly ascending, in degrees, prepared by the host exactly as for mm_sample_grid
 *             and mm_layered_model_apply (descending axes flipped; a global longitude axis closed at lon[0] + 360 and
 *             lon_periodic = 1).  They are the caller's word: the entry point does not read them back.
 *   anchors_d f64[na]: the reference radii A_0 > A_1 > ... > A_{na-1} in metres, top first, 2 <= na <= 64.  The caller's word,
 *             as the axes are (multimesh_amd.topography.InterfaceMap checks them).
 *   shifts_d  f64[nlat][nlon][na]: shifts[ja][io][j] is the radial displacement of anchor j at a map node in metres, positive
 *             up.  COLUMN-MAJOR -- the column of one map node is one contiguous run -- for the reason multimesh_layered.h gives:
 *             a lane walks down one column (four, in bilinear mode) and stops at its interval.
 *   points_out_d  f64[n][3] or NULL.  It may be points_d itself (in place): a node's coordinates are read before they are
 *             written and no node reads another's.  Any other overlap with points_d is not allowed.
 *   radius_out_d  f64[n] or NULL: the radius the node was given (direction = 0: r'; direction = 1: rho).
 *   latlondepth_out_d  f64[n][3] or NULL: the (lat, lon, depth) the device computed, depth = 6371000 - r.
 *   noutside_d  int64[1] or NULL: the number of outside nodes is ADDED to it (integer sums, one atomic per workgroup: the same
 *             on every run); it is not zeroed.
 *
 * THE STATEMENT.  Every operation is an IEEE-754 binary64 operation rounded on its own, as written and bracketed here; no
 * fused multiply-add (the library is built with -ffp-contract=off), no libm beyond the acos and atan2 of step 1.
 * lerp(t, p, q) = (1.0 - t) * p + t * q.
 *   1. COORDINATES of a node p = (x, y, z), mm_sample_grid's operation for operation (one device function serves all):
 *        r = sqrt((x*x + y*y) + z*z);  depth = 6371000 - r;  lat = 90 - acos(r > 0 ? z / r : 0) * (180 / pi)
 *        lon = atan2(y, x) * (180 / pi);  with lon_periodic: if lon < lon[0]: lon += 360; if lon >= lon[0] + 360: lon -= 360
 *      lat and lon depend on the device's acos and atan2; latlondepth_out_d hands them back.  r has no libm in it and is
 *      NumPy's bit for bit, and everything below is bit for bit what NumPy gives for the same expressions ON THOSE ANGLES
 *      (tests/topography_cases.py).  A radial move changes neither angle: both directions read the same column.
 *   2. THE COLUMN.  The cells (ja, ja1, ta) on the latitude and (io, io1, to) on the longitude axis are
 *      mm_layered_model_apply's (multimesh_layered.h, step 3; with outside = 1 the angle is clamped to its axis first), and
 *        lateral = 1 (bilinear):  s_j = lerp(ta, lerp(to, S[ja][io][j], S[ja][io1][j]), lerp(to, S[ja1][io][j], S[ja1][io1][j]))
 *        lateral = 0 (cell):      s_j is the entry of the nearest map node's column, per axis t < 0.5 ? i : i1, unchanged.
 *      B_j = A_j + s_j is the deformed anchor.
 *   3. direction = 0 (APPLY).  rho = ref_radius[i] if given, else r.
 *        rho >= A_0:  d = s_0 (the shell above the top anchor moves rigidly);
 *        else, with the first j in 0 .. na-2 such that rho >= A_{j+1}:
 *                     u = (rho - A_{j+1}) / (A_j - A_{j+1});  d = lerp(u, s_{j+1}, s_j);
 *        no such j (below the last anchor; a NaN rho):  d = s_{na-1}.
 *      r' = rho + d;  scale = r' / r;  p' = (x * scale, y * scale, z * scale);  radius_out = r'.
 *      A node with d == 0 and no ref_radius has r' == r, scale == 1.0 exactly, and keeps its bits.
 *   4. direction = 1 (FLATTEN).
 *        r >= B_0:  rho = r - s_0;
 *        else, with the first j in 0 .. na-2 such that r >= B_{j+1}:
 *                     u = (r - B_{j+1}) / (B_j - B_{j+1});  rho = lerp(u, A_{j+1}, A_j)
 *                     (r < B_j by the way j is found, so the divisor is positive whatever the order of the B);
 *        no such j:   rho = r - s_{na-1}.
 *      radius_out = rho;  scale = rho / r;  p' = (x * scale, y * scale, z * scale).
 *      Flattening inverts the stretching where the B_j descend strictly (InterfaceMap refuses a map whose interfaces cross);
 *      the round trip is exact to a few roundings times (A_j - A_{j+1}) / (B_j - B_{j+1}).
 *   5. OUTSIDE.  A node is outside when r, lat or lon is a NaN (a NaN among x, y, z makes r one), when r == 0, or when lat
 *      or lon lies off the closed span of its axis (an axis of length 1 is constant: every angle is on it).
 *        outside = 0 (keep):  an outside node is copied to points_out unchanged, bit for bit, and its radius_out is r.
 *        outside = 1 (clamp): lat and lon are clamped as in find_cell, so the edge column extends; NaN nodes and the centre
 *                             stay outside and are treated as under keep.
 *      Outside nodes are counted in both modes.
 *
 * Runs on the context's stream and does not synchronise.  One launch.
 * MM_ERR_ARG, decided on the host with nothing written and before the device is touched, for a null ctx; a negative n or 3 * n
 * at or past 2^48; na outside [2, 64]; nlat or nlon < 1; nlat * nlon * na at or past 2^48; direction, lateral or outside
 * outside {0, 1}; a null lat_d, lon_d, anchors_d or shifts_d; with n > 0 a null points_d; a ref_radius_d that is not null with
 * direction = 1.  n == 0 is valid: nothing is computed or counted; so is a call that asks for no output at all.
 */
#ifndef MULTIMESH_TOPOGRAPHY_H
#define MULTIMESH_TOPOGRAPHY_H

#include "multimesh_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MM_STRETCH_MAX_NA 64
#define MM_STRETCH_DIRECTION_APPLY 0
#define MM_STRETCH_DIRECTION_FLATTEN 1
#define MM_STRETCH_LATERAL_CELL 0
#define MM_STRETCH_LATERAL_BILINEAR 1
#define MM_STRETCH_OUTSIDE_KEEP 0
#define MM_STRETCH_OUTSIDE_CLAMP 1

int mm_radial_stretch(mm_context *ctx, const double *points_d, int64_t n, const double *ref_radius_d,
                      const double *lat_d, int nlat, const double *lon_d, int nlon, int lon_periodic,
                      const double *anchors_d, int na, const double *shifts_d,
                      int direction, int lateral, int outside,
                      double *points_out_d, double *radius_out_d,
                      double *latlondepth_out_d, int64_t *noutside_d);

#ifdef __cplusplus
}
#endif
#endif /* MULTIMESH_TOPOGRAPHY_H */
