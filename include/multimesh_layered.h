/*
 * multimesh_layered.h -- an EXTENSION of the C ABI of multi_mesh_hip.so (multimesh_hip.h): a LAYERED COLUMN MODEL -- on a
 * latitude x longitude map the depths of a stack of interfaces and one value per layer and parameter, the form crustal
 * models are distributed in -- evaluated on the nodes of a mesh or on points that stay in HBM.  The entry point lives in the
 * same library; it is declared here and not in multimesh_hip.h because that header's set of functions is pinned by the binding
 * tests ("Layered column models").  Bound by multimesh_amd/layered.py.
 *
 * ARRAYS, all on the device.  nlayer = nb - 1, n = ngroups * P.
 *   points_d  f64[ngroups][P][3], P nodes per element, 1 <= P <= 256 (P = 1: a point cloud, hex8 nodes).  z is the pole,
 *             latitude is geocentric, longitude runs from x towards y: the geometry of mm_sample_grid.
 *   lat_d     f64[nlat], lon_d f64[nlon]: strictly ascending, in degrees, prepared by the host exactly as for
 *             mm_sample_grid (descending axes flipped; a global longitude axis closed at lon[0] + 360 and lon_periodic = 1).
 *             They are the caller's word: the entry point does not read them back.
 *   bounds_d  f64[nlat][nlon][nb]: the depths of the interfaces of every column in metres, positive down from 6371000 m (a
 *             negative value lies above that radius), top first.  2 <= nb <= 256.
 *   values_d  f64[nlat][nlon][nlayer][ncomp]: one value per column, layer and component.
 *             Both tables are COLUMN-MAJOR -- the column of one map node is one contiguous run -- because a lane walks down
 *             one column (four, in bilinear mode) and stops at its layer: with the map as the minor index every step of that
 *             walk would touch another cache line.
 *   out_d     f64[ncomp][n].  ncomp = 0 is valid and means layers only (out_d and values_d may then be NULL).
 *   layer_out_d  int32[n] or NULL: the layer index, -1 outside.
 *   span_out_d   f64[n][2] or NULL: the top and the bottom depth of the node's layer at the node's column, NaN outside.
 *   latlondepth_out_d  f64[n][3] or NULL: the (lat, lon, depth) the device computed.
 *   noutside_d   int64[1] or NULL: the number of outside nodes is ADDED to it (integer sums, one atomic per workgroup: the
 *             same on every run); it is not zeroed.
 *
 * THE STATEMENT.  Every operation is an IEEE-754 binary64 operation rounded on its own, as written and bracketed here; no
 * fused multiply-add (the library is built with -ffp-contract=off), no libm beyond the acos and atan2 of step 1.
 * lerp(t, p, q) = (1.0 - t) * p + t * q.
 *   1. COORDINATES of a node (x, y, z), mm_sample_grid's operation for operation (one device function serves both):
 *        r = sqrt((x*x + y*y) + z*z);  depth = 6371000 - r;  lat = 90 - acos(r > 0 ? z / r : 0) * (180 / pi)
 *        lon = atan2(y, x) * (180 / pi);  with lon_periodic: if lon < lon[0]: lon += 360; if lon >= lon[0] + 360: lon -= 360
 *      These three are what latlondepth_out_d hands back; they depend on the device's acos and atan2.  Everything below is
 *      bit for bit what NumPy gives for the same expressions ON THOSE (tests/layered_cases.py).
 *   2. PICKING DEPTH dp.  pick = 0 (node): dp = depth.  pick = 1 (element): dp = 6371000 - rc with the centre of the node's
 *      element, c = (((X[0] + X[1]) + ...) + X[P-1]) / P per coordinate, rc = sqrt((cx*cx + cy*cy) + cz*cz): the centre of
 *      mm_radial_model_apply (one device function); no libm, so dp is NumPy's bit for bit.  Only the DEPTH comes from the
 *      centre; the lateral position is always the node's own: all nodes of an element compare the same dp, each against its
 *      own column.  On a mesh that honours an interface, a node on the interface takes the side of its own element.
 *   3. LATERAL CELLS.  Per axis a (length m) and coordinate v, mm_sample_grid's cell: m == 1: i = i1 = 0, t = 0, inside;
 *      else inside = a[0] <= v <= a[m-1] (with outside = 1, v is first clamped: v = v < a[0] ? a[0] : v, then
 *      v = v > a[m-1] ? a[m-1] : v, and the node is inside), i = clip(upper_bound(a, v) - 1, 0, m - 2), i1 = i + 1,
 *      t = (v - a[i]) / (a[i+1] - a[i]).  With (ja, ja1, ta) on the latitude and (io, io1, to) on the longitude axis:
 *        lateral = 1 (bilinear):  b_j = lerp(ta, lerp(to, B[ja][io][j], B[ja][io1][j]), lerp(to, B[ja1][io][j], B[ja1][io1][j]))
 *                                 and the value of component c in layer l likewise from V[..][..][l][c].
 *        lateral = 0 (cell): the model is piecewise constant around its map nodes: per axis the column is t < 0.5 ? i : i1,
 *                                 and b_j and the values are that column's entries, unchanged.
 *   4. LAYER.  With nlayer = nb - 1:  if dp >= b_0: the layer is the first j in 0 .. nlayer-1 with dp < b_{j+1}; if there is
 *      none and dp == b_{nb-1}, it is the LAST j with b_j < b_{j+1} (the model's bottom belongs to the model).  A layer of zero
 *      thickness is skipped by this rule without a special case.  Every comparison with a NaN is false: a NaN bound never stops
 *      the scan.  The rule is defined for any bounds; that they do not decrease downwards is the caller's business
 *      (multimesh_amd.layered.LayeredModel checks it).  span = (b_j, b_{j+1}) of the layer found.
 *   5. OUTSIDE.  A node is outside when lat, lon or dp is a NaN, when lat or lon lies outside the closed span of its axis, or
 *      when step 4 finds no layer.
 *        outside = 0 (fill): every component of an outside node is fill_value.
 *        outside = 1 (clamp): lat and lon are clamped (step 3); when step 4 finds no layer, dp < b_0 takes the FIRST j with
 *          b_j < b_{j+1}, dp >= b_0 the LAST such j.  What then has no layer -- a column without a layer of positive thickness,
 *          a NaN -- is outside and gets fill_value.
 *        outside = 2 (keep): the entries of out_d of an outside node are not written.  This is how a crust is laid over an
 *          existing model.
 *      Outside nodes get layer -1 and a NaN span, and are counted, in all three modes.
 *
 * Runs on the context's stream and does not synchronise.  One launch whatever ncomp is.
 * MM_ERR_ARG, decided on the host with nothing written and before the device is touched, for a null ctx; a negative ngroups or
 * one at or past 2^48; P outside [1, 256]; nb outside [2, 256]; nlat or nlon < 1; ncomp outside [0, 65536); 3 * n, ncomp * n,
 * nlat * nlon * nb or nlat * nlon * nlayer * ncomp at or past 2^48; lateral or pick outside {0, 1}; outside outside {0, 1, 2};
 * a null lat_d, lon_d or bounds_d; a null values_d with ncomp > 0; with ngroups > 0, a null points_d, or a null out_d with
 * ncomp > 0.  ngroups == 0 is valid: nothing is computed or counted.
 */
#ifndef MULTIMESH_LAYERED_H
#define MULTIMESH_LAYERED_H

#include "multimesh_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MM_LAYERED_MAX_P 256
#define MM_LAYERED_MAX_NB 256
#define MM_LAYERED_LATERAL_CELL 0
#define MM_LAYERED_LATERAL_BILINEAR 1
#define MM_LAYERED_PICK_NODE 0
#define MM_LAYERED_PICK_ELEMENT 1
#define MM_LAYERED_OUTSIDE_FILL 0
#define MM_LAYERED_OUTSIDE_CLAMP 1
#define MM_LAYERED_OUTSIDE_KEEP 2

int mm_layered_model_apply(mm_context *ctx, const double *points_d, int64_t ngroups, int64_t P,
                           const double *lat_d, int nlat, const double *lon_d, int nlon, int lon_periodic,
                           const double *bounds_d, int nb, const double *values_d, int64_t ncomp,
                           int lateral, int pick, int outside, double fill_value,
                           double *out_d, int32_t *layer_out_d, double *span_out_d,
                           double *latlondepth_out_d, int64_t *noutside_d);

#ifdef __cplusplus
}
#endif
#endif /* MULTIMESH_LAYERED_H */
