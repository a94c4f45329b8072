/*
 * multimesh_hip.h -- C ABI of multi_mesh_hip.so, the MI355X (gfx950) drop-in for the
 * MultiMesh interpolation hot path: element centroids -> k nearest centroids ->
 * point-in-hex8 location by Newton inversion -> shape-function weighted gather.
 *
 * Plain pointers and sizes only.  Two groups of entry points:
 *
 *  (1) LEGACY symbols with the exact signature and semantics of the reference's own C
 *      library (what reference multi_mesh/helpers.py:43-81 binds).  Host pointers in,
 *      host pointers out; the work runs on the GPU.
 *  (2) mm_* symbols taking DEVICE pointers, for callers that keep meshes resident in HBM
 *      (the benchmark, the multi-GPU driver, repeated queries against one source mesh).
 *
 * Error convention: the reference has no error channel (per-point failures are a count,
 * reference src/trilinearinterpolator.c:133-147).  Here: int / int64 returns are >= 0 on
 * success (a failed-point count where the reference returns one) and NEGATIVE MM_ERR_* on a
 * runtime error; mm_last_error() returns a message.  There is no CPU fallback: without a
 * usable GPU every compute entry point fails with MM_ERR_NODEVICE / MM_ERR_HIP.
 * Nothing is ever printed from device code (the reference's "not any" printf is dropped).
 */
#ifndef MULTIMESH_HIP_H
#define MULTIMESH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM_OK 0
#define MM_ERR_ARG (-1)         /* bad argument (null pointer, negative size, k too large ...) */
#define MM_ERR_HIP (-2)         /* a HIP runtime call failed; see mm_last_error() */
#define MM_ERR_NODEVICE (-3)    /* no usable GPU */
#define MM_ERR_ALLOC (-4)       /* device or host allocation failed */
#define MM_ERR_UNSUPPORTED (-5) /* valid request this build does not implement */

#define MM_KNN_MAX_K 64 /* largest nelem_to_search served (reference uses 20, 25, 30) */

/* ------------------------------------------------------------------------------------
 * (1) Legacy symbols -- replace the reference library one for one.
 * ---------------------------------------------------------------------------------- */

/* Replaces reference src/centroid.c:3-9 (bound at helpers.py:43-57).
 * centroid[e][a] = (sum over the element's nodes, in connectivity order) / npointsperelem.
 * connectivity int64[nelem][npointsperelem], points f64[npoints][ndim], centroid
 * f64[nelem][ndim], all C-contiguous host arrays.  ndim in {1,2,3}.  The signature has no
 * error channel: on failure the output is left untouched, a message goes to stderr and
 * mm_last_error()/mm_last_status() report it. */
void centroid(long long ndim, long long nelem, long long npointsperelem,
              long long *connectivity, double *points, double *centroid);

/* Replaces reference src/trilinearinterpolator.c:40-48 (bound at helpers.py:59-81).
 * For each of npoints targets walk its nelem_to_search candidate elements in the given
 * order, Newton-invert the trilinear map, accept the first with max|xi| < 1.025, else after
 * the last candidate fall back to the least-outside one if < 1.5; write the element's 8
 * node ids and 8 weights in place; rows of failed points are left untouched.  Returns the
 * number of failed points (>= 0) or a negative MM_ERR_*.  Host arrays:
 * nearest_element_indices int64[npoints][k], connectivity int64[nelem][8] (locator corner
 * order), enclosing_elem_indices int64[npoints][8] out, nodes f64[nnodes][3], weights
 * f64[npoints][8] out, points f64[npoints][3].  nelem / nnodes are not in the reference
 * signature; they are recovered as max index + 1. */
long long triLinearInterpolator(long long nelem_to_search, long long npoints,
                                long long *nearest_element_indices, long long *connectivity,
                                long long *enclosing_elem_indices, double *nodes,
                                double *weights, double *points);

/* ------------------------------------------------------------------------------------
 * (2) Device-pointer API.
 * ---------------------------------------------------------------------------------- */

/* Alignment: a device array needs the alignment of its element type and no more (8 bytes for f64 / int64, 4 for int32,
 * 1 for unsigned char), so a view that starts part-way into a larger buffer is a valid argument everywhere.  The hex8
 * locate and kNN kernels move connectivity rows, operator rows and rows of an even k 16 bytes at a time: mm_knn_query
 * (idx_d, dist_d), mm_locate_hex8 (connectivity_d -- which then needs nelem > 0, else MM_ERR_ARG --,
 * enclosing_elem_indices_d, weights_d), mm_interpolate_hex8 (connectivity_d, enc_d, w_d), mm_source_create
 * (connectivity_d) and mm_interpolate_hex8_on (enc_d, w_d) serve such an array that starts off 16 bytes through a copy of
 * their own (an allocation, device-to-device copies and a wait per call; the source keeps its copy): same results, slower.
 * Arrays on 16 bytes -- anything from mm_device_alloc, hipMalloc or a whole torch tensor -- take the direct path. */
typedef struct mm_context mm_context;     /* device, stream, scratch pool, stage timers */
typedef struct mm_knn_index mm_knn_index; /* device-resident search grid over source points */

int mm_device_count(void);
const char *mm_last_error(void); /* thread-local message of the last failure */
int mm_last_status(void);        /* thread-local MM_* code of the last legacy call */

/* hip_stream: a hipStream_t (NULL = the device's default stream).  All work of a context is
 * issued on that stream; entry points that return a count synchronise it. */
int mm_context_create(int device, void *hip_stream, mm_context **out);
void mm_context_destroy(mm_context *ctx);
int mm_synchronize(mm_context *ctx);

/* Resident-array helpers for hosts that have no other device allocator. */
int mm_device_alloc(mm_context *ctx, size_t bytes, void **dptr);
int mm_device_free(mm_context *ctx, void *dptr);
int mm_copy_h2d(mm_context *ctx, void *dst_d, const void *src_h, size_t bytes);
int mm_copy_d2h(mm_context *ctx, void *dst_h, const void *src_d, size_t bytes);
int mm_memset(mm_context *ctx, void *dst_d, int value, size_t bytes);

/* A1 -- element centroids (reference src/centroid.c:3-25), device arrays. */
int mm_centroid(mm_context *ctx, int64_t ndim, int64_t nelem, int64_t npointsperelem,
                const int64_t *connectivity_d, const double *points_d, double *centroid_d);

/* A2 -- exact k nearest neighbours; replaces scipy.spatial.cKDTree(src, balanced_tree=False)
 * + .query(pts, k) at reference scripts/cli.py:66-73.  build = the tree construction,
 * query = .query: idx_d int64[npts][k] ascending by Euclidean distance (squared distance
 * summed axis by axis in fp64, no fused multiply-add; equal distances ordered by index);
 * rows with fewer than k sources are padded with index nsrc (distance inf) like cKDTree.
 * dist_d (nullable) f64[npts][k] receives the distances.  ndim in {1,2,3}; k <= MM_KNN_MAX_K.
 * Non-finite coordinates (NaN, +-inf, or finite ones whose squared distance overflows): the call still returns MM_OK.
 *   targets: the rows of the finite targets are what they are without the others, bit for bit; in the row of a
 *     non-finite target every index lies in [0, nsrc] (nsrc: the padding) and the row is the same on every kernel
 *     route the dispatcher can take.
 *   sources: a source with a NaN coordinate is never nearer than anything (it is not listed); a non-finite source never
 *     precedes a finite one, and the finite sources' part of every row is the exact kNN over the finite sources.  (An
 *     infinite source coordinate makes the bounding box's extent along that axis non-finite; the grid then takes one
 *     cell of unit edge there, which is exact as long as the finite sources span at most that along the axis.) */
int mm_knn_build(mm_context *ctx, const double *src_d, int64_t nsrc, int64_t ndim,
                 mm_knn_index **out);
int mm_knn_query(mm_context *ctx, const mm_knn_index *index, const double *pts_d, int64_t npts,
                 int64_t k, int64_t *idx_d, double *dist_d);
void mm_knn_destroy(mm_context *ctx, mm_knn_index *index);

/* A4..A8 -- hex8 point location + weights (reference src/trilinearinterpolator.c:40-148),
 * device arrays, same in-place contract as the legacy symbol.  nelem > 0 enables a bounds
 * guard: candidates outside [0, nelem) (cKDTree's padding) count as "not in hull".
 * conn_is_exodus != 0 applies the reference's host-side column reorder
 * (scripts/cli.py:79-81) on the fly, so the caller can pass the mesh's own connectivity.
 * Degenerate elements (flat, zero-size, mirrored, tangled, collapsed edges or faces, duplicates) and non-finite node or
 * point coordinates are not special cases: the stage is the reference's arithmetic on whatever it is given, and every
 * row -- a NaN weight included -- is what the reference computes from the same arrays (MM_FP_EXACT: bit for bit;
 * MM_FP_TOL: see there).  A target no candidate accepts, a non-finite one among them, counts as failed and keeps its row. */
/* A connectivity_d that starts off 16 bytes (a view into a larger buffer) is copied by the call, which must then know its
 * size: with nelem == 0 (no bounds guard) such an array is refused with MM_ERR_ARG; on 16 bytes nelem == 0 is served. */
int64_t mm_locate_hex8(mm_context *ctx, int64_t nelem_to_search, int64_t npoints,
                       const int64_t *nearest_element_indices_d, const int64_t *connectivity_d,
                       int64_t nelem, int conn_is_exodus, int64_t *enclosing_elem_indices_d,
                       const double *nodes_d, double *weights_d, const double *points_d);

/* A9 -- weighted gather; replaces np.sum(field[enc] * w, axis=1) at reference
 * scripts/cli.py:98-100 (P = 8) and interpolator.py:976 (P = 27, 125), NumPy's summation
 * order.  fields_d f64[ncomp][nsrc] (one contiguous array per parameter, as the reference
 * keeps them); ids_d int64[npoints][P]; w_d f64[npoints][P]; out_d f64[npoints][ncomp] when
 * out_point_major (the layout reference interpolator.py:973-977 returns) else
 * f64[ncomp][npoints].  P <= 128. */
int mm_gather(mm_context *ctx, const double *fields_d, int64_t nsrc, int64_t ncomp,
              const int64_t *ids_d, const double *w_d, int64_t npoints, int64_t P, double *out_d,
              int out_point_major);

/* A10 -- GLL elements (order 1, 2, 4; dim 2, 3): element search + Lagrange coefficients; replaces
 * the per-point loop get_element_weights.check_inside at reference
 * components/interpolator.py:1181-1233 (tolerance and snap_to_nearest as there; 1.03 / 0 gives the
 * layered variant :1271-1297).  The inverse transform and the coefficients come from salvus.fem in
 * the reference (absent): PARITY UNPINNED, numerics defined in mm_locate_gll.hip / the oracle.
 * gll_points_d f64[nelem][P][dim] with P = (order+1)^dim, control node p = i + (order+1) j + ...;
 * nn_d int64[npoints][k]; elem_d int64[npoints] (-1 = not found); coeffs_d f64[npoints][P].
 * Degenerate (flat, zero-size, mirrored, folded, duplicated) elements and non-finite coordinates take the same path as
 * everything else: a transform that fails is NaN and the candidate is skipped, as the acceptance loop states; every row
 * equals the oracle's on the same arrays.  The same holds for mm_locate_gll_bbox and mm_interpolate_gll.
 * Returns the number of points without an element, or a negative MM_ERR_*. */
int64_t mm_locate_gll(mm_context *ctx, int order, int dim, int64_t nelem_to_search, int64_t npoints,
                      const int64_t *nearest_element_indices_d, const double *gll_points_d, int64_t nelem,
                      const double *points_d, double tolerance, int snap_to_nearest, int64_t *elem_d,
                      double *coeffs_d);

/* The other GLL acceptance loop of the reference: _check_if_inside_element + boundary_box_check
 * (components/interpolator.py:1350-1367, :1409-1473; used by gll_2_exodus :274, the layered drivers
 * :543 and the helpers :1523, :1572).  Candidates in order: bounding box of the control nodes first,
 * inside -> inverse transform, accept when every |xi| <= 1.04.  Otherwise the first candidate whose
 * box holds the point, else the one with the nearest control-node mean, is transformed again; NaN
 * or any |xi| >= 1.04 gives the reference's constant xi = (0.645, -0.5, 0.22) (:1468-1471).
 * Arrays as mm_locate_gll; PARITY UNPINNED like it.  Returns the number of points whose final
 * transform was NaN (where the reference raises unless ignore_hard_elements), or a negative MM_ERR_*. */
int64_t mm_locate_gll_bbox(mm_context *ctx, int order, int dim, int64_t nelem_to_search, int64_t npoints,
                           const int64_t *nearest_element_indices_d, const double *gll_points_d,
                           int64_t nelem, const double *points_d, int64_t *elem_d, double *coeffs_d);

/* Element-nodal gather np.sum(coeffs * field[elem_indices], axis=1) (reference interpolator.py:976):
 * fields_d f64[ncomp][nelem][P]; points with elem -1 give 0.  NumPy's summation order. */
int mm_gather_elem(mm_context *ctx, const double *fields_d, int64_t nelem, int64_t ncomp,
                   const int64_t *elem_d, const double *coeffs_d, int64_t npoints, int64_t P, double *out_d,
                   int out_point_major);

/* The GLL form of the whole path on resident arrays: what reference components/interpolator.py:931-977
 * (interpolate_to_points on a GLL mesh) and the core of gll_2_gll (:700-830) compute for an array
 * of points -- centroid of every element's control nodes (NumPy mean(axis=1) order,
 * salvus_mesh_reader.py:99-100), the nelem_to_search nearest centroids, the acceptance loop of
 * :1181-1233 (mm_locate_gll), then np.sum(coeffs * field[elem], axis=1) per component (:976).
 *   gll_points_d f64[nelem][P][dim], points_d f64[npoints][dim], fields_d f64[ncomp][nelem][P],
 *   out_d f64[npoints][ncomp]; points that are not found give +-0.0 like NumPy's field[-1] * 0.
 *   elem_out_d int64[npoints] and coeffs_out_d f64[npoints][P]: both or neither (the operator).
 * Without the operator outputs the sum is formed where a target is accepted (no coefficient array
 * in memory), and the candidate lists are evaluated lazily (mm_set_lazy_lists); results are
 * identical to the staged calls.  Returns the number of points not found, or a negative MM_ERR_*. */
int64_t mm_interpolate_gll(mm_context *ctx, int order, int dim, const double *gll_points_d, int64_t nelem,
                           const double *points_d, int64_t npoints, const double *fields_d, int64_t ncomp,
                           int64_t nelem_to_search, double tolerance, int snap_to_nearest, double *out_d,
                           int64_t *elem_out_d, double *coeffs_out_d);

/* A 3-D GLL model sampled on latitude x longitude x depth columns: extract_regular_grid (reference api.py:600-642,
 * components/interpolator.py:1600-1646), the depth slice of plot_depth_slice (plotter.py:89-102, :159-187) and the
 * radius x path section of plot_cross_section (plotter.py:360-391).  The targets are generated on the device:
 *   lat_d f64[nlat][2] = {sin colat, cos colat}, lon_d f64[nlon][2] = {cos lon, sin lon}, radius_d f64[ndepth]
 *   (6371000 - depth), all computed on the host as latlondepth_to_xyz computes them (reference utils.py:526-542);
 *   column h: latitude h / nlon and longitude h % nlon (paired == 0, ncol = nlat * nlon), or latitude h and
 *   longitude h (paired == 1, a path, nlat == nlon = ncol);
 *   target (d, h) = {(r_d * sin_colat) * cos_lon, (r_d * sin_colat) * sin_lon, r_d * cos_colat} in that order, no
 *   fused multiply-add: bit for bit latlondepth_to_xyz of the row (lat, lon, depth).
 * Every target is then served as mm_interpolate_gll (dim 3, snap_to_nearest 0) serves the same point -- same
 * element, same acceptance, same value -- except that a target without an element gets fill_value.
 *   gll_points_d f64[nelem][P][3], fields_d f64[ncomp][nelem][P], out_d f64[ncomp][ndepth][ncol] (component-major, in
 *   grid order), points_out_d (nullable) f64[ndepth][ncol][3] receives the generated targets.
 * The centroid tree is built once per call; the targets go through in chunks of chunk_points consecutive flat indices
 * d * ncol + h (0: automatic, MM_SAMPLE_CHUNK_BYTES / the per-target bytes 4 min(k, 8) + 4 k (k > 8) + 28 + 24 (no
 * points_out_d) + MM_SAMPLE_STAGE_BYTES; never more than MM_SAMPLE_CHUNK_MAX).  Results do not depend on the chunk size.
 * Returns the number of targets without an element, or a negative MM_ERR_*. */
#define MM_SAMPLE_CHUNK_BYTES ((int64_t)1 << 34) /* per-target scratch of one automatic chunk (16 GiB) */
#define MM_SAMPLE_STAGE_BYTES 96                 /* the kNN and locate stages' own per-target arrays, counted flat */
#define MM_SAMPLE_CHUNK_MAX ((int64_t)0x7fffff00) /* int32 target indices of the locate stage */
int64_t mm_sample_columns_gll(mm_context *ctx, int order, const double *gll_points_d, int64_t nelem,
                              const double *fields_d, int64_t ncomp, const double *lat_d, int64_t nlat,
                              const double *lon_d, int64_t nlon, int paired, const double *radius_d, int64_t ndepth,
                              int64_t nelem_to_search, double tolerance, double fill_value, int64_t chunk_points,
                              double *out_d, double *points_out_d);

/* The other direction: a regular (depth, latitude, longitude) grid sampled at arbitrary points -- a gridded model onto the
 * nodes of a mesh.  points_d f64[npoints][3] (an element-nodal [nelem][P][3] array read flat), the axes depth_d
 * f64[ndepth] (m below 6371000), lat_d f64[nlat] (geocentric degrees), lon_d f64[nlon] (degrees), each STRICTLY ASCENDING
 * (the caller guarantees it), grid_d f64[ncomp][ndepth][nlat][nlon], out_d f64[ncomp][npoints] (for an element-nodal mesh
 * the [C][E][P] layout mm_gather_elem reads), latlondepth_out_d (nullable) f64[npoints][3] = (lat, lon, depth) as computed.
 * Per point, every operation rounded on its own (no fused multiply-add):
 *   r = sqrt((x*x + y*y) + z*z)   depth = 6371000.0 - r   c = r > 0 ? z / r : 0.0
 *   lat = 90.0 - acos(c) * (180.0 / pi)   lon = atan2(y, x) * (180.0 / pi)          (the inverse of latlondepth_to_xyz)
 *   lon_periodic: if (lon < lon[0]) lon += 360.0; if (lon >= lon[0] + 360.0) lon -= 360.0; each once -- the caller
 *     guarantees -360 <= lon[0] <= 180 and lon[nlon-1] == lon[0] + 360
 *   per axis a[0..n-1] and value v: inside = (v >= a[0] && v <= a[n-1]) (NaN is outside); clamp mode first sets
 *     v = min(max(v, a[0]), a[n-1]) and counts the point as inside; i = clip(upper_bound(a, v) - 1, 0, n - 2)
 *     (np.searchsorted(a, v, side="right") - 1), t = (v - a[i]) / (a[i+1] - a[i]), i1 = i + 1; an axis of length 1 is
 *     constant along itself: i = i1 = 0, t = 0, always inside
 *   per component, with lerp(t, p, q) = (1.0 - t) * p + t * q: four lerps along longitude, two of those along latitude,
 *     one along depth, corners read at (k|k1, j|j1, i|i1).  A NaN corner propagates as IEEE arithmetic propagates it,
 *     also with weight 0.
 * So out_d is bit for bit that statement on latlondepth_out_d; the angles themselves are the device's acos / atan2.
 * outside_mode for points outside the grid: 0 fill (fill_value is written), 1 clamp (the edge value extends; nothing is
 * outside), 2 keep (out_d[c][n] is left untouched).  ncomp == 0 with latlondepth_out_d is valid (the coordinates alone),
 * and so is npoints == 0.  Returns the number of points outside the grid (0 in clamp mode; an integer sum, the same on
 * every run), or a negative MM_ERR_*: MM_ERR_ARG for a null table, ndepth / nlat / nlon < 1 or an unknown mode, nothing is
 * written then.  Synchronises. */
int64_t mm_sample_grid(mm_context *ctx, const double *points_d, int64_t npoints, const double *depth_d, int64_t ndepth,
                       const double *lat_d, int64_t nlat, const double *lon_d, int64_t nlon, const double *grid_d,
                       int64_t ncomp, int lon_periodic, int outside_mode, double fill_value, double *out_d,
                       double *latlondepth_out_d);

/* The grid import as an OPERATOR: the ids and weights that mm_sample_grid applies, written out so that they can be kept
 * (mm_gather imports any number of cubes without a new search) and turned round (mm_transpose_create_nodes / _apply give
 * G^T, the way back from the mesh to the cube).  points_d, the axes, lon_periodic and latlondepth_out_d as mm_sample_grid;
 * ids_d int64[npoints][8], w_d f64[npoints][8].  Every operation is rounded on its own (no fused multiply-add):
 *   (lat, lon, depth), the periodic wrap and per axis (i, i1, t, inside) are EXACTLY those of mm_sample_grid -- depth gives
 *     (k, k1, tz), latitude (j, j1, ty), longitude (i, i1, tx);
 *   corner c = 4 a + 2 b + e with a, b, e in {0, 1} selecting K = k|k1, J = j|j1, I = i|i1;
 *   ids[n][c] = (K * nlat + J) * nlon + I, the flat index into one component's [ndepth][nlat][nlon] cube;
 *   u(t, 0) = 1.0 - t, u(t, 1) = t;   w[n][c] = (u(tz, a) * u(ty, b)) * u(tx, e).
 * An axis of length 1 gives i = i1 = 0 and t = 0: two corners then share an id, with the weights 1 * ... and 0 * ...; ids
 * repeated in a row are valid input for mm_gather and mm_transpose_*.
 * clamp == 0: a point outside the grid (a NaN coordinate is outside) gets ids 0 and weights +0.0 in all eight slots and is
 * counted -- the all-zero row that a failed target is for mm_transpose_create_nodes.  clamp != 0: as mm_sample_grid's clamp
 * mode, nothing is outside; a NaN coordinate yields NaN weights on the ids its cell search gives.  The clamp is
 * v = v < a[0] ? a[0] : v, then v = v > a[n-1] ? a[n-1] : v: a coordinate of -0.0 on an axis that starts at +0.0 stays -0.0,
 * so that t = -0.0 and the weights it multiplies are -0.0 (mm_sample_grid's values cannot tell: its t * q is added to a term).
 * So ids_d and w_d are bit for bit this statement on latlondepth_out_d.  sum_c w[n][c] * g[ids[n][c]] in mm_gather's
 * (NumPy's) order is NOT bit-equal to mm_sample_grid's nested lerps: for finite corners and t in [0, 1] the two differ by at
 * most 32 eps max|corner| (ten roundings through the three lerp levels, seven through the weights, the products and the
 * 8-term sum).
 * Returns the number of points outside (0 with clamp; an integer sum, the same on every run), or a negative MM_ERR_*:
 * MM_ERR_ARG for a null table or ndepth / nlat / nlon < 1 (nothing is written), MM_ERR_UNSUPPORTED when an axis exceeds
 * INT_MAX nodes or the cube 2^63 - 1.  npoints == 0 is valid.  Synchronises. */
int64_t mm_grid_operator(mm_context *ctx, const double *points_d, int64_t npoints, const double *depth_d, int64_t ndepth,
                         const double *lat_d, int64_t nlat, const double *lon_d, int64_t nlon, int lon_periodic, int clamp,
                         int64_t *ids_d, double *w_d, double *latlondepth_out_d);

/* The TRANSPOSE of an interpolation operator: what comes back from the targets to the sources (a gradient on the event
 * mesh -> the inversion mesh, so that <P m, g> = <m, P^T g>; P^T 1 = the coverage map).  Deterministic: the result is bit for
 * bit np.add.at on zeros, i.e. the sequential loop, on every run (no float atomics, no reordering).
 *   node form (the hex8 operator of mm_interpolate_hex8 / mm_locate_hex8, any ids int64[N][P], w f64[N][P]):
 *     out[c][j] = (((+0.0 + t1) + t2) + ...), every t = w[n][p] * v[n][c] rounded as a product on its own (no fused
 *     multiply-add), over all (n, p) with ids[n][p] == j in ascending flat index n * P + p.  Every row takes part, the all-zero
 *     rows of failed targets included (as in NumPy); a destination nobody names is +0.0.
 *     = np.add.at(out[c], ids, w * v[:, c, None]).
 *   element form (the GLL operator of mm_interpolate_gll / mm_locate_gll: elem int64[N], coeffs f64[N][P]):
 *     out[c][e][p] = the same sequential sum from +0.0 of coeffs[n][p] * v[n][c] over the n with elem[n] == e, ascending n;
 *     rows with elem[n] == -1 are skipped (mm_gather_elem gives 0 for them).
 * create groups the contributions by destination ONCE (a stable sort; it synchronises); apply then runs for any number of
 * value sets -- the operator / gather split in the other direction.
 *   create: every id must lie in [0, nsrc) (element form: [-1, nelem)), else MM_ERR_ARG (one reduction over the ids, as in
 *     mm_first_occurrence).  P <= 128.  npoints * P (element form: npoints) must stay below 2^31 -- the sort carries the flat
 *     index as a 32-bit payload and counts with 32-bit signed offsets -- else MM_ERR_UNSUPPORTED, decided from the sizes alone
 *     before anything is allocated.  npoints == 0 is valid.
 *     The node-form handle OWNS what it sorted: the weights in destination order (8 B), the target index of each (4 B) and
 *     the row offsets (4 B per destination): 12 B per contribution, 0.97 GB + 0.04 GB for 10,077,696 hex8 targets onto as
 *     many nodes; ids_d / w_d are not needed after create.  While it runs, create also holds the sort's two key and payload
 *     buffers (24 B per contribution), freed before it returns.
 *     The element-form handle owns only the target permutation (4 B per target) and the offsets (4 B per element); it
 *     BORROWS coeffs_d, which must stay alive and unchanged until mm_transpose_destroy (as mm_source borrows its mesh).
 *   apply: values_d f64[N][C] when values_point_major (what mm_gather returns by default), else f64[C][N];
 *     out_d f64[C][nsrc] (the layout mm_gather reads fields in) or f64[C][nelem][P] (the layout mm_gather_elem reads);
 *     every element of out_d is written.  ncomp == 0 is valid.  Timed as MM_STAGE_GATHER. */
typedef struct mm_transpose mm_transpose;
int mm_transpose_create_nodes(mm_context *ctx, const int64_t *ids_d, const double *w_d, int64_t npoints, int64_t P,
                              int64_t nsrc, mm_transpose **out);
int mm_transpose_create_elem(mm_context *ctx, const int64_t *elem_d, const double *coeffs_d, int64_t npoints, int64_t P,
                             int64_t nelem, mm_transpose **out);
int mm_transpose_apply(mm_context *ctx, const mm_transpose *op, const double *values_d, int64_t ncomp,
                       int values_point_major, double *out_d);
void mm_transpose_destroy(mm_context *ctx, mm_transpose *op);

/* The diagonal GLL MASS MATRIX of an element-nodal mesh, M[e][p] = w_p |det J_e(xi_p)|: the inner product of a
 * spectral-element mesh is a^T M b, so that a density (a sensitivity kernel K with d chi = int K dm dV) goes from mesh to
 * mesh as M_c K_c = P^T (M_f K_f), and int f dV = sum M f.  The reference has no counterpart (its mass matrix lives in Salvus).
 *   gll_points_d f64[nelem][P][dim], P = (order+1)^dim, order 1, 2 or 4, dim 2 or 3, node p = i + m j + m^2 k with
 *   m = order + 1 (the layout mm_locate_gll takes); deriv_d f64[m][m] with D[i][a] = l_a'(g_i) and weights_d f64[m], the GLL
 *   rule's tables, made on the host (as the sine and cosine tables of mm_sample_columns_gll: the device then does only + and
 *   *, and the result is stated bit for bit).  mass_d f64[nelem][P]; det_d f64[nelem][P] or NULL, the signed determinant.
 * Every product is rounded on its own (no fused multiply-add), every sum starts from its first term and adds in ascending a:
 *   J[0][c] = sum_a D[i][a] * X[a,j,k][c]    J[1][c] = sum_a D[j][a] * X[i,a,k][c]    J[2][c] = sum_a D[k][a] * X[i,j,a][c]
 *   det3 = (J00*(J11*J22 - J12*J21) - J01*(J10*J22 - J12*J20)) + J02*(J10*J21 - J11*J20)          det2 = J00*J11 - J01*J10
 *   mass = ((w_k * w_j) * w_i) * |det3|                                                    (2-D: (w_j * w_i) * |det2|)
 * Returns the number of nodes whose determinant is not > 0 (zero, negative, NaN): positive for an inverted or collapsed
 * element, every node for a left-handed mesh; or a negative MM_ERR_* (order, dim or a null table: MM_ERR_ARG, nothing is
 * written).  nelem == 0 is valid.  Synchronises. */
int64_t mm_gll_mass(mm_context *ctx, int order, int dim, const double *gll_points_d, int64_t nelem, const double *deriv_d,
                    const double *weights_d, double *mass_d, double *det_d);

/* The volume integral of ncomp fields, out_d[c] = sum_i mass_d[i] * fields_d[c][i] over n values (fields_d f64[ncomp][n];
 * NULL with ncomp == 1: the sum of mass_d, the volume).  out_d f64[ncomp] on the device.  Deterministic: no float atomics, and
 * the order of the sum is fixed by this definition, not by a launch shape.  With t[i] = mass[i] * field[i], a product rounded
 * on its own (t[i] = mass[i] without fields), padded with +0.0 to whole chunks of 4096 values:
 *   in a chunk, lane l of 256 adds t[l], t[l + 256], ... t[l + 3840] in that order, from the first;
 *   the 256 lane sums are halved eight times, s[l] = s[l] + s[l + h] for h = 128, 64, ... 1; s[0] is the chunk's sum;
 *   the chunk sums are summed by the same rule (as t, without fields) until one value is left.  n == 0 gives +0.0.
 * Not synchronising (the result is on the device). */
int mm_weighted_sum(mm_context *ctx, const double *mass_d, const double *fields_d, int64_t n, int64_t ncomp, double *out_d);

/* out_d[c][i] = num_d[c][i] / den_d[i] for ncomp rows of n values: the last step of the mass-weighted adjoint,
 * K_c = (P^T (M_f K_f)) / M_c.  IEEE division: a zero den_d[i] gives inf or NaN.  out_d may be num_d. */
int mm_divide_rows(mm_context *ctx, const double *num_d, const double *den_d, int64_t n, int64_t ncomp, double *out_d);

/* The STIFFNESS OPERATOR of an element-nodal GLL mesh, applied matrix-free: y[c][e][.] = K_e u[c][e][.] with
 *   K_e[p][q] = sum_n mass_n (G_n grad phi_p(xi_n)) . kappa_n (G_n grad phi_q(xi_n)),   G_n = J_e(xi_n)^-1, mass_n = w_n |det J|,
 * the weak form of -div(kappa grad u) with natural boundaries, element by element and NOT assembled: u^T y summed over the
 * mesh is the roughness int grad u . kappa grad u dV, and M + tau A^T K A (A = the gather from unique nodes) is the matrix of
 * a backward-Euler diffusion step.  kappa = kappa_h (1 - r r^T) + kappa_r r r^T with r = x / |x| the unit radius at the node
 * when `anisotropic` (3-D only), else kappa_h.  Each kappa is its scalar argument times an optional element-nodal array
 * f64[nelem][P] (NULL = 1).  The reference has no counterpart.
 *   gll_points_d, order, dim, deriv_d, weights_d, the node numbering p = i + m j + m^2 k: as mm_gll_mass.
 *   u_d, y_d f64[ncomp][nelem][P], two different arrays.
 * Every product is rounded on its own, every sum starts from its first term and adds in ascending a.  At node (i, j, k):
 *   J, det3 / det2                      : as mm_gll_mass, from the coordinates
 *   rdet = 1 / det                      : the one division
 *   G[0][0] = (J11*J22 - J12*J21)*rdet   G[0][1] = (J02*J21 - J01*J22)*rdet   G[0][2] = (J01*J12 - J02*J11)*rdet
 *   G[1][0] = (J12*J20 - J10*J22)*rdet   G[1][1] = (J00*J22 - J02*J20)*rdet   G[1][2] = (J02*J10 - J00*J12)*rdet
 *   G[2][0] = (J10*J21 - J11*J20)*rdet   G[2][1] = (J01*J20 - J00*J21)*rdet   G[2][2] = (J00*J11 - J01*J10)*rdet
 *     (2-D: G[0][0] = J11*rdet, G[0][1] = (-J01)*rdet, G[1][0] = (-J10)*rdet, G[1][1] = J00*rdet)
 *   mass = ((w_k * w_j) * w_i) * |det|  (2-D: (w_j * w_i) * |det|)
 *   kh = kappa_h * kappa_h_d[n] (kappa_h without the array), kr likewise
 *   g[0] = sum_a D[i][a] * u[a,j,k]     g[1] = sum_a D[j][a] * u[i,a,k]     g[2] = sum_a D[k][a] * u[i,j,a]
 *   gr[c] = (G[c][0]*g[0] + G[c][1]*g[1]) + G[c][2]*g[2]                                    (2-D: the first two terms)
 *   isotropic:   F[c] = (mass * kh) * gr[c]
 *   anisotropic: rn = sqrt((x*x + y*y) + z*z),  rh[c] = x[c] / rn (0 where rn == 0),  s = (rh[0]*gr[0] + rh[1]*gr[1]) + rh[2]*gr[2],
 *                F[c] = mass * (kh * gr[c] + ((kr - kh) * s) * rh[c])
 *   f[d] = (G[0][d]*F[0] + G[1][d]*F[1]) + G[2][d]*F[2]                                     (2-D: the first two terms)
 *   y = (sum_a D[a][i] * f[0][a,j,k] + sum_a D[a][j] * f[1][i,a,k]) + sum_a D[a][k] * f[2][i,j,a]
 * Returns MM_OK or a negative MM_ERR_*; MM_ERR_ARG (nothing is written) for an order or dim without tables, a null table or
 * array, anisotropic with dim 2, kappa_r_d without anisotropic, u_d == y_d.  nelem == 0 and ncomp == 0 are valid.  Not
 * synchronising. */
int mm_gll_diffusion_apply(mm_context *ctx, int order, int dim, const double *gll_points_d, int64_t nelem,
                           const double *deriv_d, const double *weights_d, const double *u_d, int64_t ncomp, double kappa_h,
                           const double *kappa_h_d, int anisotropic, double kappa_r, const double *kappa_r_d, double *y_d);

/* The SPATIAL GRADIENT of element-nodal GLL fields, as fields: the physical gradient grad u = G grad_ref u that the stiffness
 * operator forms at every node, written out per element and NOT assembled (the gradient of a C0 field jumps across element
 * faces: the copies of a shared node differ), with its norm and, on a 3-D Earth mesh, its split into the radial derivative
 * and the lateral part -- what first-order regularisation, total variation and maps of |grad m| read.  Every (component,
 * direction) plane is an ordinary element-nodal field.  The reference has no counterpart.
 *   gll_points_d, order, dim, deriv_d, the node numbering p = i + m j + m^2 k: as mm_gll_mass (no weights are needed).
 *   u_d f64[ncomp][nelem][P].  Four nullable outputs, at least one of them given:
 *   grad_d f64[ncomp][dim][nelem][P];  radial_d, lateral_d (3-D only), norm_d f64[ncomp][nelem][P].
 * Every product is rounded on its own, every sum starts from its first term and adds in ascending a.  At node (i, j, k):
 *   J, det, rdet = 1 / det, G[c][d]     : as mm_gll_diffusion_apply (the same expressions, the one division)
 *   g[0] = sum_a D[i][a] * u[a,j,k]     g[1] = sum_a D[j][a] * u[i,a,k]     g[2] = sum_a D[k][a] * u[i,j,a]
 *   gr[c] = (G[c][0]*g[0] + G[c][1]*g[1]) + G[c][2]*g[2]                  (2-D: the first two terms)      -> grad_d[comp][c]
 *   norm = sqrt((gr[0]*gr[0] + gr[1]*gr[1]) + gr[2]*gr[2])                (2-D: sqrt(gr[0]*gr[0] + gr[1]*gr[1])) -> norm_d
 *   rn = sqrt((x*x + y*y) + z*z),  rh[c] = x[c] / rn (0 where rn == 0)
 *   s = (rh[0]*gr[0] + rh[1]*gr[1]) + rh[2]*gr[2]                                                          -> radial_d
 *   l[c] = gr[c] - s*rh[c],  lateral = sqrt((l[0]*l[0] + l[1]*l[1]) + l[2]*l[2])                           -> lateral_d
 * A node with det == 0 gives the inf or NaN that IEEE arithmetic gives.  Returns MM_OK or a negative MM_ERR_*; MM_ERR_ARG
 * (nothing is written) for an order or dim without tables, a null table or input, all four outputs null, radial_d or
 * lateral_d with dim 2, an output that overlaps u_d or another output.  nelem == 0 and ncomp == 0 are valid.  Not
 * synchronising. */
int mm_gll_gradient(mm_context *ctx, int order, int dim, const double *gll_points_d, int64_t nelem, const double *deriv_d,
                    const double *u_d, int64_t ncomp, double *grad_d, double *radial_d, double *lateral_d, double *norm_d);

/* The POLYNOMIAL ORDER of element-nodal GLL values changed on their own mesh: per element, the tensor product of one
 * rectangular 1-D table R = table_d f64[m_out][m_in] applied to the element's values, m = order + 1, P = m^dim, node
 * p = i + m j + m^2 k as everywhere.  With R[q][a] = l_a^in(g_q^out) it interpolates onto the GLL nodes of the other order
 * (up: exact for the polynomial the field is; down: the subsample on the coinciding nodes, whose rows are unit rows); with
 * the transposed table of the opposite direction it is the transpose of that interpolation; with scale_in_d = the fine mass
 * and div_out_d = the coarse mass (mm_gll_mass) it is the mass-weighted restriction K_c = M_c^-1 I^T M_f K_f of a sensitivity
 * kernel in one pass.  Every target node sits in a known element at a known reference coordinate: nothing is searched, no
 * node can fail, and a node on an element face takes its value from its own element.  The reference has no counterpart.
 *   layout: where component c of node p of element e sits, the same for in_d (with P_in) and out_d (with P_out):
 *     0 = [C][E][P], the field planes;  1 = [E][P][C], MODEL/coordinates;  2 = [E][C][P], MODEL/data.
 *   scale_in_d f64[nelem][P_in] and div_out_d f64[nelem][P_out], each nullable, shared by all components.
 * Every product is rounded on its own (no fused multiply-add), every sum starts from its first term and adds in ascending
 * index; 3-D (2-D drops the third sweep and out = t2):
 *   v[a,b,c]      = in[a,b,c]                        (scale_in_d == NULL)   or   in[a,b,c] * scale_in[e][p_in]
 *   t1[qi,b,c]    = sum_a R[qi][a] * v[a,b,c]
 *   t2[qi,qj,c]   = sum_b R[qj][b] * t1[qi,b,c]
 *   out[qi,qj,qk] = sum_c R[qk][c] * t2[qi,qj,c]     then   / div_out[e][p_out]   (one IEEE division) if given
 * Nothing is special-cased: 0 * NaN is NaN, so a NaN poisons the outputs of its element whose table entries multiply it.
 * Returns MM_OK or a negative MM_ERR_*; MM_ERR_ARG (nothing is written) for dim other than 2 or 3, an order other than
 * 1, 2, 4, order_in == order_out (copy instead), an unknown layout, a size out of range, a null table, a null in_d / out_d,
 * an out_d that shares a byte with in_d, scale_in_d or div_out_d -- all decided before the context or a device is touched
 * -- and a null ctx.  nelem == 0 and ncomp == 0 are valid.  Not synchronising. */
int mm_gll_tensor_apply(mm_context *ctx, int dim, int order_in, int order_out, const double *table_d, int layout,
                        const double *in_d, double *out_d, int64_t nelem, int64_t ncomp, const double *scale_in_d,
                        const double *div_out_d);

/* How far two sets of node coordinates of the same elements are apart, element by element, and the size of each element:
 * what gll_change_order compares before it writes.  a_d, b_d f64[nelem][npts][dim], dim 2 or 3:
 *   deviation_d[e] = max over p, d of |a[e][p][d] - b[e][p][d]|, NaN where one of these differences is NaN
 *   edge_d[e]      = fmax over d of (fmax over p of b[e][p][d] - fmin over p of b[e][p][d])   (fmax / fmin pass over a NaN)
 * Both are exact (one subtraction each, then comparisons), so the order of the reduction does not show.  Returns MM_OK or a
 * negative MM_ERR_*; MM_ERR_ARG (nothing is written) for dim other than 2 or 3, npts < 1, a size out of range, a null
 * array, an output that shares a byte with an input or the other output -- all decided before the context or a device is
 * touched -- and a null ctx.  nelem == 0 is valid.  Not synchronising. */
int mm_element_deviation(mm_context *ctx, int dim, int64_t npts, const double *a_d, const double *b_d, int64_t nelem,
                         double *deviation_d, double *edge_d);

/* RADIAL 1-D PROFILES: the radial bin of every point, a mass-weighted sum per bin in one pass, and a 1-D table (radius ->
 * value, with discontinuities) evaluated on the nodes.  The reference has no counterpart.
 *
 * mm_radial_bins: points_d f64[n][3]; edges_d f64[nbins + 1], strictly ascending and finite (checked on the device:
 * MM_ERR_ARG otherwise, nothing is written); bin_d int32[n]; radius_out_d f64[n] or NULL.
 *   r = sqrt((x*x + y*y) + z*z)            (every product and sum rounded on its own: bit for bit NumPy)
 *   b = upper_bound(edges, r) - 1, so that edges[b] <= r < edges[b + 1]; r == edges[nbins] belongs to bin nbins - 1;
 *   b = -1 for r < edges[0], r > edges[nbins] and a NaN r.
 * Returns the number of -1 entries (an integer sum, the same on every run) or a negative MM_ERR_*: MM_ERR_ARG for a null
 * ctx or array, n < 0 or nbins outside [1, 2^20].  n == 0 is valid.  Synchronises. */
int64_t mm_radial_bins(mm_context *ctx, const double *points_d, int64_t n, const double *edges_d, int64_t nbins,
                       int32_t *bin_d, double *radius_out_d);

/* out_d[c][b] = sum over the i with bin_d[i] == b of mass_d[i] * fields_d[c][i], for all bins in ONE pass over the arrays
 * per component.  mass_d f64[n]; fields_d f64[ncomp][n], or NULL with ncomp == 1: the sum of the mass (the volume per bin);
 * bin_d int32[n] (entries < 0 or >= nbins belong to no bin); square 0 / 1; out_d f64[ncomp][nbins]; count_d int64[nbins] or
 * NULL: the number of members of every bin (integer atomics).  Deterministic: no float atomics, and the order of every sum
 * is fixed by this definition, not by a launch shape.  For bin b,
 *   t[i] = mass[i] * f[i]   (square: (mass[i] * f[i]) * f[i];  without fields: mass[i]), every product rounded on its own,
 *          where bin[i] == b, and +0.0 elsewhere WHATEVER f[i] is (a NaN outside a bin does not reach it),
 * padded with +0.0 to whole chunks of 4096 values, then mm_weighted_sum's rule with every lane sum STARTING FROM +0.0:
 *   in a chunk, lane l of 256 computes ((((+0.0 + t[l]) + t[l + 256]) + ...) + t[l + 3840]);
 *   the 256 lane sums are halved eight times, s[l] = s[l] + s[l + h] for h = 128, 64, ... 1; s[0] is the chunk's sum;
 *   the chunk sums of bin b are summed by the same rule (as t) until one value is left.
 * A partial sum that starts from +0.0 is never -0.0, so adding +0.0 never changes it: skipping the non-members is bit for
 * bit this statement.  No result is -0.0; an empty bin is +0.0.  n == 0 gives zeros.
 * Scratch: 8 B * nbins * ceil(n / 4096) for one component at a time (the components are summed one after the other).
 * MM_ERR_ARG (nothing is written) for a null ctx or array, a negative size, nbins outside [1, 2^20], ncomp >= 65536,
 * n >= 2^42, fields_d NULL with ncomp > 1; MM_ERR_UNSUPPORTED when nbins * ceil(n / 4096^2) reaches 2^31.  ncomp == 0 is
 * valid (only count_d is filled).  Not synchronising. */
int mm_binned_weighted_sum(mm_context *ctx, const double *mass_d, const double *fields_d, const int32_t *bin_d, int64_t n,
                           int64_t ncomp, int64_t nbins, int square, double *out_d, int64_t *count_d);

/* A 1-D table on the nodes, optionally fused with the perturbation arithmetic.  points_d f64[ngroups][P][3], P nodes per
 * element, 1 <= P <= 256 (P = 1: a point cloud, hex8 nodes); radius_d f64[m] ascending, a REPEATED radius marks a
 * discontinuity; values_d f64[ncomp][m]; in_d f64[ncomp][ngroups * P] (modes 1-4, else ignored); out_d of that shape, may
 * be in_d.  The layers are the maximal strictly ascending runs of radius_d; a run of length 1 (m == 1, three equal radii),
 * a descending step or a non-finite radius is refused with MM_ERR_ARG (the table is read back and checked on the host,
 * nothing is written).
 *   the layer of an element, decided once by its centre: c = (((X[0] + X[1]) + ...) + X[P-1]) / P per coordinate,
 *     rc = sqrt((cx*cx + cy*cy) + cz*cz); the layer with r_lo <= rc < r_hi; below the first layer the first, above the last
 *     the last; a NaN rc makes every output of the element NaN.  A node on a discontinuity therefore takes the side of its
 *     own element however its radius rounds; with P = 1 a point on a discontinuity takes the upper side.
 *   the value at a node, within the layer's rows [a, b]: r = sqrt((x*x + y*y) + z*z), r' = min(max(r, R[a]), R[b]),
 *     i = clip(upper_bound(R[a..b], r') - 1, a, b - 1), t = (r' - R[i]) / (R[i+1] - R[i]),
 *     ref = (1.0 - t) * V[i] + t * V[i+1], every operation rounded on its own.
 *   mode 0: out = ref   1: out = in - ref   2: out = (in - ref) / ref   3: out = in + ref   4: out = ref + in * ref
 * The table is held in LDS when m * (1 + ncomp) <= 4096 doubles, else read from global memory.  MM_ERR_ARG also for a null
 * ctx or array, a negative size, P outside [1, 256], an unknown mode, in_d NULL in modes 1-4, ncomp >= 65536.
 * ngroups == 0 and ncomp == 0 are valid.  Synchronises once before its kernel is queued (the table check), not after. */
int mm_radial_model_apply(mm_context *ctx, const double *points_d, int64_t ngroups, int64_t P, const double *radius_d,
                          const double *values_d, int64_t m, int64_t ncomp, int mode, const double *in_d, double *out_d);

/* KERNEL PRECONDITIONING: the cut-out around sources and receivers, exact order statistics of a field and clipping at bounds
 * that are already on the device -- what stands between "sum the event kernels" and "smooth".  The reference has no counterpart.
 *
 * mm_point_taper: points_d f64[ngroups][P][3], 1 <= P <= 256 (P = 1: a point cloud, hex8 nodes); centres_d f64[K][3], inner_d
 * and outer_d f64[K], 0 <= K <= 2^20; in_d and out_d f64[ncomp][ngroups * P], out_d may be in_d; weight_out_d f64[ngroups * P]
 * or NULL; ncomp == 0 with weight_out_d is valid.  Per node x and centre k, every product, quotient and sum rounded on its own:
 *   dx = x0 - c0, dy = x1 - c1, dz = x2 - c2;   d = sqrt((dx*dx + dy*dy) + dz*dz)
 *   t_k = 0.0                      if d <= inner_k
 *         1.0                      else if d >= outer_k
 *         (s*s) * (3.0 - 2.0*s)    else, with s = (d - inner_k) / (outer_k - inner_k)
 *   w = 1.0;  for k ascending:  if (t_k < w) w = t_k      (a NaN t_k never wins: a node with a NaN coordinate keeps w = 1.0)
 *   out[c][i] = w * in[c][i]
 * outer == inner is a hard cut: the order of the tests makes it well defined, nothing is divided.  A minimum of values <= 1
 * does not depend on its order and a centre with d >= outer_k at every node of an element contributes exactly 1.0, so the
 * kernel skips such centres per element by a bounding-box test that goes through the statement's own roundings (margin zero:
 * mm_precondition.hip) -- bit for bit this statement.  An element that no centre reaches gets out = in and weight 1.0, and
 * nothing at all is written for it when out_d == in_d and weight_out_d == NULL.
 * Returns the number of nodes with w < 1 (an integer sum, the same on every run) or a negative MM_ERR_*: MM_ERR_ARG, with
 * nothing written, for a null ctx or array, P outside [1, 256], a negative size, K > 2^20, a centre that is not finite, an
 * inner or outer that is not finite, inner < 0 or outer < inner (the centres are checked on the device).  ngroups == 0 is
 * valid.  Synchronises. */
int64_t mm_point_taper(mm_context *ctx, const double *points_d, int64_t ngroups, int64_t P, const double *centres_d,
                       const double *inner_d, const double *outer_d, int64_t K, int64_t ncomp, const double *in_d,
                       double *out_d, double *weight_out_d);

/* Exact order statistics of ncomp rows of n values: values_d f64[ncomp][n]; q_d f64[m], every q in [0, 1], 1 <= m <= 16;
 * method 0 = lower, 1 = higher; out_d f64[ncomp][m]; nvalid_d int64[ncomp].  Per row:
 *   NaNs are excluded; nvalid = the number of the others, which are ordered by the key of their bits u (absolute: of the bits
 *   with the sign cleared):  key = sign(u) ? ~u : u | 2^63  as unsigned 64-bit integers -- the numeric order, -0.0 before +0.0;
 *   pos = q * (double)(nvalid - 1), one rounded product;  rank = floor(pos) (lower) or ceil(pos) (higher);
 *   out = the value whose key has that rank (absolute: |v|);  nvalid == 0: NaN.
 * The result is defined by the order alone and exact for every input: a most-significant-digit radix select over the keys, one
 * byte per pass, eight passes over the values for all m ranks and all rows together, integer histograms only.
 * Scratch: 32 KiB of histograms and 0.6 KiB of state per row, whatever n is.
 * MM_ERR_ARG (nothing is written) for a null ctx or array, a negative size, n >= 2^42, m outside [1, 16], an unknown method, a q
 * that is NaN or outside [0, 1].  n == 0 gives NaN and nvalid 0; ncomp == 0 is valid.  Synchronises once before its kernels are
 * queued (q is read back and checked on the host), not after: the results are on the device. */
int mm_order_statistics(mm_context *ctx, const double *values_d, int64_t n, int64_t ncomp, int absolute, const double *q_d,
                        int64_t m, int method, double *out_d, int64_t *nvalid_d);

/* Clipping: out[c][i] = v < lo[c] ? lo[c] : (v > hi[c] ? hi[c] : v) for in_d, out_d f64[ncomp][n], out_d may be in_d.  lower_d
 * and upper_d f64[ncomp] ON THE DEVICE (the output of mm_order_statistics with m = 1 as it stands), NULL: no bound on that
 * side; symmetric = 1 takes lower_d == NULL and uses lo[c] = -upper_d[c].  A NaN passes through (both comparisons are false),
 * -0.0 is kept against a bound of 0.0, a NaN bound bounds nothing.  changed_d int64[ncomp] or NULL: the number of values
 * replaced (integer atomics, one per workgroup).  MM_ERR_ARG (nothing is written) for a null ctx or array, a negative size,
 * symmetric other than 0 / 1, symmetric with lower_d or without upper_d.  n == 0 and ncomp == 0 are valid.  Not synchronising. */
int mm_clamp(mm_context *ctx, const double *in_d, int64_t n, int64_t ncomp, const double *lower_d, const double *upper_d,
             int symmetric, double *out_d, int64_t *changed_d);

/* BOUNDARIES: where a hexahedral mesh ends, which side of the domain each boundary face is, the distance of any point to
 * the nearest boundary node up to a cutoff, and a taper or blend of fields driven by that distance (a regional model put
 * inside a larger one without a step along its outline; a kernel damped towards absorbing sides).  3-D only.  The reference
 * has no counterpart.  Integer atomics only; every result is the same on every run.
 *
 * Conventions.  Tensor corner c = i + 2 j + 4 k with i, j, k in {0, 1}; for a GLL element of order n, m = n + 1, corner c is
 * node p = n i + m n j + m m n k; a hex8 connectivity in exodus order gives tensor order by its columns [0,1,3,2,4,5,7,6].
 * Local faces f = 0 .. 5 are i = 0, i = 1, j = 0, j = 1, k = 0, k = 1, with the corners
 *   (0,2,4,6) (1,3,5,7) (0,1,4,5) (2,3,6,7) (0,1,2,3) (4,5,6,7)      and, in cyclic order for the normal,
 *   (0,2,6,4) (1,3,7,5) (0,1,5,4) (2,3,7,6) (0,1,3,2) (4,5,7,6).
 * A face's nodes are the m m nodes with that index fixed, in ascending p.  The code of face f of element e is 6 e + f.
 *
 * mm_boundary_faces: corner_ids_d int64[nelem][8] in tensor order, every id in [0, nnodes), nnodes < 2^31, nelem < 2^27;
 * faces_d int64[6 * nelem] (room for the worst case); info_d int64[1] or NULL.
 *   keys = np.sort(corner_ids[:, FACE_CORNERS], axis=2).reshape(6 * nelem, 4)
 *   _, inverse, counts = np.unique(keys, axis=0, return_inverse=True, return_counts=True)
 *   faces = np.flatnonzero(counts[inverse] == 1);   info[0] = (counts[inverse] > 2).sum()
 * faces_d receives the codes ascending; the return value is their number.  Faces whose key occurs more than twice count as
 * interior: the mesh is then not a manifold.  A hash table of face indices claimed by compare-and-swap, matches found by
 * comparing the claimant's sorted ids, a count per class, flags, a prefix sum.  Scratch: 8 bytes per slot of a table of
 * 12 * nelem slots rounded up to a power of two, and 12 bytes per face.  MM_ERR_ARG, with nothing written to faces_d, for a
 * null ctx or array, a size out of range or an id outside [0, nnodes) (checked on the device).  nelem == 0 is valid.
 * Synchronises. */
int64_t mm_boundary_faces(mm_context *ctx, const int64_t *corner_ids_d, int64_t nelem, int64_t nnodes, int64_t *faces_d,
                          int64_t *info_d);

/* The side of every boundary face: corners_d f64[nelem][8][3] in tensor order, faces_d int64[nb] codes in [0, 6 * nelem)
 * (checked on the device: MM_ERR_ARG, nothing is read through a bad code), side_d int[nb].  Every product, sum and quotient
 * rounded on its own; with q0 .. q3 the face's corners in cyclic order and c0 .. c7 the element's:
 *   a = q2 - q0;  b = q3 - q1;  n = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0)
 *   fc = ((q0 + q1) + (q2 + q3)) * 0.25;  ec = (((((((c0 + c1) + c2) + c3) + c4) + c5) + c6) + c7) * 0.125;  g = fc - ec
 *   if ((n0*g0 + n1*g1) + n2*g2 < 0) n = -n                                  (outward)
 *   u = fc if radial (Earth-centred coordinates) else (upx, upy, upz)
 *   t = (n0*u0 + n1*u1) + n2*u2;  lim = cos_min * sqrt(((n0*n0 + n1*n1) + n2*n2) * ((u0*u0 + u1*u1) + u2*u2))
 *   side = 1 (top) if t >= lim, else 2 (bottom) if t <= -lim, else 0 (lateral side); a NaN gives 0.
 * MM_ERR_ARG also for a null ctx or array, a size out of range, nb > 6 * nelem, radial other than 0 / 1, cos_min outside
 * (0, 1], and without radial an up that is zero or not finite.  nb == 0 is valid.  Synchronises. */
int mm_boundary_classify(mm_context *ctx, const double *corners_d, int64_t nelem, const int64_t *faces_d, int64_t nb,
                         int radial, double upx, double upy, double upz, double cos_min, int *side_d);

/* The nodes of the selected boundary faces: points_d f64[nelem][P][3], P = (order + 1)^3, order 1, 2 or 4 (hex8: order 1 with
 * the gathered tensor-order corners); faces_d int64[nb], side_d int[nb] (NULL: every face is selected); a face is selected
 * when bit (1 << side) of side_mask is set; out_d f64[nb * (order + 1)^2][3] (room for the worst case).
 *   out = np.concatenate([points[e, FACE_NODES[f]] for (e, f) of the selected faces, in faces_d's order])
 * face by face, ascending p within a face; a node shared by two faces appears twice, which is harmless for a minimum.
 * Returns the number of points written, (order + 1)^2 per selected face.  MM_ERR_ARG, with nothing written, for a null ctx
 * or array, another order, a size out of range, nb > 6 * nelem, side_mask outside [0, 7], a code outside [0, 6 * nelem) or a
 * side outside [0, 2] (both checked on the device).  Synchronises. */
int64_t mm_boundary_nodes(mm_context *ctx, const double *points_d, int64_t nelem, int order, const int64_t *faces_d,
                          const int *side_d, int64_t nb, int side_mask, double *out_d);

/* The distance to the nearest source up to a cutoff: points_d f64[n][3], sources_d f64[K][3], dist_d f64[n].
 *   d_i = cutoff
 *   for every source j:  dx, dy, dz = the differences;  r = sqrt((dx*dx + dy*dy) + dz*dz);  if (r < d_i) d_i = r
 * A minimum does not depend on its order: the result is defined by the SET of sources alone, bit for bit.  A point with a
 * NaN coordinate keeps cutoff.  Returns the number of points with d < cutoff.  A cell grid over the sources' bounding box,
 * built by a counting sort (integer histogram, prefix sum, scatter), with an edge of cutoff * (1 + 2^-30) -- enlarged until
 * there are at most 1024 cells per axis and 2^22 in all --; a point scans the 27 cells around its own and a point outside
 * the box grown by one cell is done at once.  The margin covers the rounding of the cell index and of r itself (DESIGN.md
 * section 5): a source whose rounded r is below cutoff never sits outside the 27 cells.  The distance is to the nearest
 * NODE given, not to the surface they sample: its resolution is the node spacing.
 * Scratch: 28 bytes per source and 8 per cell.  MM_ERR_ARG (nothing is written) for a null ctx or array, a negative size,
 * K >= 2^30, a cutoff that is not finite, not positive or below 2^-500 (the margin's derivation needs the squares of the
 * offsets not to underflow), a source that is not finite (checked on the device), an extent of the sources that overflows.
 * K == 0 (every d is cutoff) and n == 0 are valid.  Synchronises. */
int64_t mm_cutoff_distance(mm_context *ctx, const double *points_d, int64_t n, const double *sources_d, int64_t K, double cutoff,
                           double *dist_d);

/* Taper or blend by a distance: dist_d f64[n]; a_d, b_d (or NULL), out_d f64[ncomp][n]; elem_d int64[n] or NULL;
 * weight_out_d f64[n] or NULL.  w is mm_point_taper's smoothstep of d, formula and order of the tests unchanged:
 *   w = 0.0 if d <= inner, else 1.0 if d >= outer, else (s*s) * (3.0 - 2.0*s) with s = (d - inner) / (outer - inner)
 *   with elem_d: w = 0.0 where elem < 0 (a point that was not located)
 *   b_d == NULL (taper):  out = w * a
 *   otherwise (blend):    out = b if w == 0, a if w == 1, else (w * a) + ((1.0 - w) * b)
 * so a garbage or NaN a where w == 0 never leaks into a blend.  inner == outer is a hard cut.  out_d may be a_d or b_d.
 * Returns the number of nodes with w < 1.  MM_ERR_ARG (nothing is written) for a null ctx or array, a negative size,
 * ncomp >= 65536, radii that are not finite with 0 <= inner <= outer.  n == 0 and ncomp == 0 are valid.  Synchronises. */
int64_t mm_distance_taper(mm_context *ctx, const double *dist_d, int64_t n, double inner, double outer, int64_t ncomp,
                          const double *a_d, const double *b_d, const int64_t *elem_d, double *out_d, double *weight_out_d);

/* RESOLUTION: what a model asks of the mesh it sits on -- the time step the model forces and the shortest period the mesh
 * still resolves with it -- from the node spacing and the edge lengths of every element.  The reference has no counterpart
 * (it leaves this to Salvus).
 *   gll_points_d f64[nelem][P][dim], P = m^dim, m = order + 1, order 1, 2 or 4, dim 2 or 3, node p = i + m j + m^2 k; fields
 *   f64[C][nelem][P] (the layouts of mm_gll_mass).  Every difference, product, sum, root and quotient is rounded on its own
 *   (no fused multiply-add).  The distance of two nodes is sqrt((dx*dx + dy*dy) + dz*dz) with d = later - earlier (2-D:
 *   sqrt(dx*dx + dy*dy)).
 *   h[e][p]     = the least distance from node p to its tensor-line neighbours: the predecessor and the successor along
 *                 each of the dim directions, where they exist (a node at the end of a line has one neighbour along it)
 *   spacing[e]  = min_p h[e][p]
 *   edge_min[e], edge_max[e] = the least and greatest of the straight corner-to-corner edge lengths, 12 in 3-D and 4 in
 *                 2-D: corner c = i + 2 j + 4 k is node p = n i + m n j + m m n k (n = order), the edges join the corners
 *                 (c, c | 1 << d) with bit d of c clear.  On a curved element the edge is the CHORD, not the arc.
 *   With fast_d f64[nfast][nelem][P], nfast >= 1, and slow_d f64[nslow][nelem][P], nslow >= 0:
 *   vfast[e][p] = max_c fast[c][e][p];      step[e] = min_p (h[e][p] / vfast[e][p])
 *   vslow[e][p] = the least of the slow[c][e][p] that are > 0; if none is, min_c fast[c][e][p] (a fluid element, where
 *                 VS = 0, is resolved by its P wavelength)
 *   period[e]   = edge_max[e] / (min_p vslow[e][p])                      (one division per element)
 * A time step is courant * min_e step[e], a resolved period elements_per_wavelength * max_e period[e]: the two factors are
 * the caller's conventions, not part of this definition.  All minima and maxima are taken over exact values, so their order
 * cannot change a bit.  (The kernel takes them of the squared distances and then one root: a correctly rounded root is
 * monotone, so the bits are those of the statement.)
 * Validity.  An element is geometry-invalid when any of its coordinates is not finite; model-invalid when it is
 * geometry-invalid, when any of its fast or slow values is not finite, when any fast value is <= 0 or any slow value < 0.
 * A geometry-invalid element's entries of all five rows (and its row of node_h_d) are NaN; a model-invalid element's entries
 * of step and period are NaN.  Coincident nodes (h = 0) are valid and give step = 0.
 *   node_h_d f64[nelem][P] or NULL: h;  out_d f64[5][nelem]: spacing, edge_min, edge_max, step, period -- with nfast == 0
 *   rows 3 and 4 are not written (out_d may then be f64[3][nelem]) and slow_d must be NULL with nslow == 0;
 *   info_d int64[2]: the geometry-invalid and the model-invalid elements (equal with nfast == 0).
 * One streaming pass: 24 B read per node (8 more per node and velocity component), 24 or 40 B written per element.
 * MM_ERR_ARG (nothing is written) for a null ctx or array, another order or dim, a size out of range, nfast or nslow outside
 * [0, 1024], slow velocities without a fast one.  nelem == 0 is valid (info_d is zeroed).  Not synchronising: everything
 * stays on the device. */
int mm_gll_resolution(mm_context *ctx, int order, int dim, const double *gll_points_d, int64_t nelem, const double *fast_d,
                      int64_t nfast, const double *slow_d, int64_t nslow, double *node_h_d, double *out_d, int64_t *info_d);

/* The least (want_max == 0) or greatest (1) value of every row of values_d f64[nrows][n] that is not a NaN, and where it
 * stands: value_d f64[nrows], index_d int64[nrows], nvalid_d int64[nrows] (the values that are not NaN).  Among equal values
 * the LOWEST index wins; -0.0 and +0.0 compare equal; the value returned is the one stored at that index (so it may be
 * -0.0).  A row without a valid value gives NaN and -1.  In NumPy, per row:
 *   valid = np.flatnonzero(~np.isnan(row));  i = valid[np.argmax(row[valid])]   (np.argmin for the least)
 * Integer atomics only -- a 64-bit atomicMax on the order-preserving integer image of the double, then one on the complement
 * of the index of the values equal to it -- so the result is the same on every run.  No scratch, and nothing is read back:
 * not synchronising.  MM_ERR_ARG for a null ctx or array, nrows outside [0, 65536), n outside [0, 2^48), want_max other
 * than 0 or 1.  nrows == 0 and n == 0 are valid. */
int mm_arg_extreme(mm_context *ctx, const double *values_d, int64_t nrows, int64_t n, int want_max, double *value_d,
                   int64_t *index_d, int64_t *nvalid_d);

/* SCATTERED MODELS: the rows of a k-nearest-neighbour query turned into values -- a model that is only points with values
 * (no connectivity, no grid) onto any targets, by inverse-distance weights RELATIVE TO THE NEAREST SAMPLE.  The reference has
 * no counterpart (its users go through scipy.spatial.cKDTree and NumPy on the host).
 *   fields_d f64[ncomp][nsrc]; idx_d int64[npoints][k] and dist_d f64[npoints][k] exactly as mm_knn_query writes them (the
 *   statement is nonetheless defined for any contents); out_d f64[npoints][ncomp] when out_point_major, else
 *   f64[ncomp][npoints]; nearest_out_d f64[npoints] or NULL; nused_out_d int32[npoints] or NULL.
 * Per target i, every quotient, product and sum rounded on its own (no fused multiply-add):
 *   valid_j = (0 <= idx[i][j] < nsrc) and (dist[i][j] <= max_distance): a NaN distance is not valid, the padding index nsrc
 *     is not valid
 *   m = the number of valid j;  nused[i] = m
 *   m == 0: the target is OUTSIDE: outside == 0 writes fill_value to every component, outside == 2 leaves the target's
 *     entries of out_d as they are (1 is not defined here: the numbers are mm_sample_grid's); nearest[i] = +inf; the target
 *     is counted in the return value
 *   otherwise j0 = the lowest valid j, d0 = dist[i][j0], nearest[i] = d0, and
 *     exact hit: if a valid j has dist[i][j] == 0.0, with jz the lowest such j, out[c] = fields[c][idx[i][jz]], a copy of
 *       the bits; no weight is formed
 *     else, for j ascending:  r_j = d0 / dist[i][j];  q_j = r_j multiplied by r_j another (power - 1) times, left to right;
 *       w_j = q_j for a valid j and 0.0 otherwise;  s = 0.0, s = s + w_j;  per component num = 0.0,
 *       num = num + (w_j * v_j) with v_j = fields[c][idx[i][j]] for a valid j and 0.0 otherwise (an invalid entry's field is
 *       never read);  out[c] = num / s
 * The weights are relative to the nearest distance on purpose: 1 / d^p overflows for close samples and underflows to an
 * all-zero sum for far ones, while (d0 / d)^p lies in [0, 1] on sorted rows and the nearest sample always carries weight 1.
 * power is an integer in 1..8 (a fractional power would go through pow, whose bits cannot be pinned).  Nothing else is a
 * special case: a NaN field value under a weight of 0.0 gives NaN (under a cut neighbour it is not read); a target with a NaN
 * coordinate has NaN distances only and is outside; k == 1 is nearest neighbour, 0.0 + (1.0 * v) over 1.0: the sample's bits
 * (a -0.0 comes back as +0.0).
 * The outside count is an integer sum -- per workgroup, then one integer atomic each -- and there are no float atomics: every
 * output is the same on every run.  idx_d and dist_d are read 16 bytes at a time when k is even and both start on 16
 * bytes, 8 bytes at a time otherwise (same results).  Returns the number of outside targets, or a negative MM_ERR_*:
 * MM_ERR_ARG (nothing is written) for a null ctx or a null required array, a negative size, k outside 1..MM_KNN_MAX_K, power
 * outside 1..8, a max_distance that is a NaN or negative (+inf: no limit), outside not 0 or 2, ncomp >= 65536.
 * npoints == 0 is valid, and so is ncomp == 0 (with or without nearest_out_d / nused_out_d).  Synchronises. */
int64_t mm_idw_gather(mm_context *ctx, const double *fields_d, int64_t nsrc, int64_t ncomp, const int64_t *idx_d,
                      const double *dist_d, int64_t npoints, int64_t k, int power, double max_distance, int outside,
                      double fill_value, double *out_d, int out_point_major, double *nearest_out_d, int32_t *nused_out_d);

/* The streaming kernels of a preconditioned conjugate-gradient loop over ncomp independent systems of n unknowns each
 * (vectors f64[ncomp][n]), whose scalars never leave the device.  state_d f64[ncomp][8] holds, per system, the slots below:
 * the dots are written into MM_PCG_RZ, MM_PCG_PAP and MM_PCG_BB by mm_weighted_sum (one call per system with ncomp = 1).
 *   mm_pcg_combine:   out[c][i] = mass[i] * p[c][i] + tau * kp[c][i]; kp_d NULL: mass[i] * p[c][i]; mass_d NULL: tau * kp[c][i].
 *   mm_pcg_scalars:   MM_PCG_PHASE_START: every system active, RZ_OLD = ALPHA = BETA = 0.
 *                     MM_PCG_PHASE_BETA (after RZ = r^T z): an active system with sqrt(RZ) <= rtol * sqrt(BB) becomes inactive
 *                       for good; BETA = RZ / RZ_OLD (0 in the first iteration and for inactive systems); RZ_OLD = RZ.
 *                     MM_PCG_PHASE_ALPHA (after PAP = p^T A p): ALPHA = RZ_OLD / PAP (0 for inactive systems).
 *                     *nactive_d (nullable) = the number of active systems: the one number the host reads per iteration.
 *   mm_pcg_direction: p[c] = z[c] + BETA[c] * p[c] for active systems; the others are not touched.
 *   mm_pcg_advance:   x[c] = x[c] + ALPHA[c] * p[c] and r[c] = r[c] - ALPHA[c] * ap[c] for active systems.
 * MM_ERR_ARG (nothing is written) for a null ctx or array, a negative size, an unknown phase or a negative rtol.  Not
 * synchronising. */
#define MM_PCG_RZ 0
#define MM_PCG_RZ_OLD 1
#define MM_PCG_PAP 2
#define MM_PCG_BB 3
#define MM_PCG_ALPHA 4
#define MM_PCG_BETA 5
#define MM_PCG_ACTIVE 6
#define MM_PCG_PHASE_START 0
#define MM_PCG_PHASE_BETA 1
#define MM_PCG_PHASE_ALPHA 2
int mm_pcg_combine(mm_context *ctx, const double *mass_d, const double *p_d, double tau, const double *kp_d, int64_t n,
                   int64_t ncomp, double *out_d);
int mm_pcg_scalars(mm_context *ctx, double *state_d, int64_t ncomp, int phase, double rtol, int64_t *nactive_d);
int mm_pcg_direction(mm_context *ctx, const double *state_d, const double *z_d, int64_t n, int64_t ncomp, double *p_d);
int mm_pcg_advance(mm_context *ctx, const double *state_d, const double *p_d, const double *ap_d, int64_t n, int64_t ncomp,
                   double *x_d, double *r_d);

/* Unique points and the index array that rebuilds the input: np.unique(points, axis=0,
 * return_inverse=True) of reference utils.py:484-488 (get_unique_points, the pre-step of the GLL
 * target flows; scatter-back at components/interpolator.py:823).  points_d f64[npoints][dim];
 * unique_d f64[npoints][dim] (room for the worst case), rows in lexicographic (x, y, z) order;
 * inverse_d int64[npoints] with unique[inverse[i]] == points[i].  -0.0 equals +0.0 as in NumPy (the
 * row kept is the one with the smallest index); NaN coordinates are not supported.
 * Returns the number of unique rows, or a negative MM_ERR_*. */
int64_t mm_unique_points(mm_context *ctx, const double *points_d, int64_t npoints, int64_t dim,
                         double *unique_d, int64_t *inverse_d);

/* The same collapse WITHOUT NumPy's order, for callers that only scatter values back through the inverse -- which is all
 * the reference ever does with get_unique_points (components/interpolator.py:823, :1079-1081): the unique rows come in the
 * order of their first occurrence (unique[inverse[i]] == points[i] as above, -0.0 stored as +0.0; a row with a NaN
 * coordinate is a class of its own, as in np.unique(axis=0)).  A hash table instead of
 * a sort: 2-3x faster.  Returns the number of unique rows, or a negative MM_ERR_*. */
int64_t mm_unique_points_any_order(mm_context *ctx, const double *points_d, int64_t npoints, int64_t dim,
                                   double *unique_d, int64_t *inverse_d);

/* Layer-aware GLL drivers (reference components/interpolator.py:1047-1082): the scatter-back
 *     new_field[mask[layer]] = values[inverse].reshape(...)            (:1079-1081)
 * on the device.  values_d f64[nunique][ncomp] (what mm_interpolate_gll returns for the layer's unique target
 * points), inverse_d int64[nmasked * P] (mm_unique_points of the layer's element-nodal target points),
 * elem_ids_d int64[nmasked] (the layer's target elements); out_d f64[ncomp][nelem_out][P] receives
 * out[c][elem_ids[m]][p] = values[inverse[m * P + p]][c]; other rows are left alone. */
int mm_scatter_elements(mm_context *ctx, const double *values_d, int64_t nunique, int64_t ncomp,
                        const int64_t *inverse_d, const int64_t *elem_ids_d, int64_t nmasked, int64_t P,
                        int64_t nelem_out, double *out_d);

/* Earth meshes onto the sphere of their 1-D model (reference components/interpolator.py:1085-1144, make_spherical of
 * the drivers).  points_d f64[npoints][3]; rad_d = the z_node_1D values, f64[nrad].
 * mm_map_to_sphere: out = ((p * r_ref) * rad) / |p| per component, |p| = sqrt((x*x + y*y) + z*z), for every point with
 * |p| > 0; other points are copied unchanged.  Bit-identical to the reference's NumPy statements (r_ref = 6371000).
 * first_d == NULL: the element-nodal layout, rad_d[i] belongs to point i (nrad == npoints).  Otherwise the node
 * layout: point n takes rad_d[first_d[n]] (mm_first_occurrence); a point whose index is outside [0, nrad) is
 * copied unchanged.  out_d may be points_d (in place) but must not overlap it otherwise. */
int mm_map_to_sphere(mm_context *ctx, const double *points_d, int64_t npoints, const double *rad_d, int64_t nrad,
                     const int64_t *first_d, double r_ref, double *out_d);

/* np.unique(connectivity, return_index=True) as the node layout of map_to_sphere reads it: first_d int64[nnodes]
 * receives, for every node n, the smallest flat index i with connectivity_d[i] == n, or -1 when no entry names n.
 * connectivity_d int64[nentries] (the flattened [nelem][P] array).  Returns the number of unreferenced nodes
 * (>= 0; the map is only valid when it is 0), MM_ERR_ARG when an entry lies outside [0, nnodes), or another
 * negative MM_ERR_*.  Synchronises. */
int64_t mm_first_occurrence(mm_context *ctx, const int64_t *connectivity_d, int64_t nentries, int64_t nnodes,
                            int64_t *first_d);

/* map_to_ellipse's radial ratio (reference interpolator.py:1093-1097): ratio_d[i] = (|p_i| / r_ref) / rad, with rad
 * and first_d as in mm_map_to_sphere (a point without a valid radius index gets NaN). */
int mm_sphere_ratio(mm_context *ctx, const double *points_d, int64_t npoints, const double *rad_d, int64_t nrad,
                    const int64_t *first_d, double r_ref, double *ratio_d);

/* out = factor_d[i] * p_i per component (reference interpolator.py:1121); out_d may be points_d. */
int mm_scale_points(mm_context *ctx, const double *points_d, int64_t npoints, const double *factor_d, double *out_d);

/* find_gll_coeffs as query_model / gll_2_gll drive it (reference components/interpolator.py:113, :777): the tree is built
 * over ALL GLL points and the neighbour list of point indices becomes a list of element indices by
 * np.floor(index / P) -- in place on the device (idx_d int64[n]). */
int mm_points_to_elements(mm_context *ctx, int64_t *idx_d, int64_t n, int64_t P);

/* The fluid/solid fix-up of gll_2_gll (reference components/interpolator.py:829-841) on element data
 * values_d / previous_d f64[nelem][ncomp][P]: elements with solid_d[e] == 0 get their previous values back
 * ("values[~solid_elements] = new_values[~solid_elements]"), and so does a solid element whose parameter
 * vs_index is exactly 0.0 at any point.  Returns the number of SOLID elements restored, or a negative MM_ERR_*. */
int64_t mm_fluid_solid_fix(mm_context *ctx, double *values_d, const double *previous_d,
                           const unsigned char *solid_d, int64_t nelem, int64_t ncomp, int64_t P,
                           int64_t vs_index);

/* The whole hot path of reference scripts/cli.py:62-100 on resident arrays:
 * centroid -> search grid -> kNN -> locate -> gather.  connectivity_d is the mesh's own
 * (exodus-order) hex8 connectivity.  enc_d / w_d (nullable) receive the interpolation
 * operator (int64[N][8], f64[N][8]); out_d f64[N][ncomp] (nullable when only the operator is
 * wanted).  Non-finite coordinates (the same for mm_interpolate_hex8_on, _host and mm_interpolate_gll): the rows of
 * the finite targets are what they are without the others; a non-finite target's row is the locate stage's answer over
 * the list mm_knn_query gives for it; non-finite nodes reach the outputs only through the elements that own them.
 * Returns the number of failed points or a negative MM_ERR_*. */
int64_t mm_interpolate_hex8(mm_context *ctx, const double *nodes_d, int64_t nnodes,
                            const int64_t *connectivity_d, int64_t nelem, const double *points_d,
                            int64_t npoints, const double *fields_d, int64_t ncomp,
                            int64_t nelem_to_search, double *out_d, int64_t *enc_d, double *w_d);

/* A source mesh kept resident for repeated calls -- what the reference does when it builds its cKDTree once and queries it
 * for each of the 125 GLL points of the target elements or for every time step (scripts/cli.py:141-195):
 * mm_source_create computes the element centroids and the search grid ONCE; mm_interpolate_hex8_on is mm_interpolate_hex8
 * without those two stages (results identical, bit for bit).  nodes_d / connectivity_d are BORROWED: they must stay alive
 * and unchanged until mm_source_destroy. */
typedef struct mm_source mm_source;
int mm_source_create(mm_context *ctx, const double *nodes_d, int64_t nnodes, const int64_t *connectivity_d, int64_t nelem,
                     mm_source **out);
void mm_source_destroy(mm_context *ctx, mm_source *source);
int64_t mm_interpolate_hex8_on(mm_context *ctx, const mm_source *source, const double *points_d, int64_t npoints,
                               const double *fields_d, int64_t ncomp, int64_t nelem_to_search, double *out_d,
                               int64_t *enc_d, double *w_d);

/* The same path fed from HOST arrays -- what the reference's callers hold (NumPy arrays handed to
 * centroid / cKDTree / triLinearInterpolator / np.sum at scripts/cli.py:62-100): nodes f64[nnodes][3],
 * connectivity int64[nelem][8] (exodus order), points f64[npoints][3], fields f64[ncomp][nnodes], in place
 * results out_h f64[npoints][ncomp] and (both or neither) enc_h int64[npoints][8], w_h f64[npoints][8].
 * Uploads run on a second stream beside the kernels of the stage before (mesh -> centroids + grid |
 * targets -> kNN | fields -> locate); the device copies live in the context and are reused by later calls. */
int64_t mm_interpolate_hex8_host(mm_context *ctx, const double *nodes_h, int64_t nnodes,
                                 const int64_t *connectivity_h, int64_t nelem, const double *points_h,
                                 int64_t npoints, const double *fields_h, int64_t ncomp,
                                 int64_t nelem_to_search, double *out_h, int64_t *enc_h, double *w_h);

/* mm_interpolate_hex8 evaluates its candidate lists lazily (default on): the locate stage walks a
 * target's candidates in kNN order and stops at the first acceptance (1.6 candidates per target on
 * mesh-like inputs), so the pipeline first asks the kNN stage for the 8 nearest only and computes
 * the full nelem_to_search list just for the targets that exhaust those 8 (they then go through
 * the reference-order locate from candidate 0).  The k' nearest are the first k' of the k nearest,
 * so every output is bit-identical to the eager evaluation; on = 0 forces the eager one. */
int mm_set_lazy_lists(mm_context *ctx, int on);

/* Floating-point mode of the hex8 locate stage (mm_locate_hex8, mm_interpolate_hex8*, triLinearInterpolator).
 *   MM_FP_EXACT (default): the reference's arithmetic operation for operation (src/trilinearinterpolator.c:150-375)
 *     -- node ids, weights and interpolated values bit-identical to the reference.
 *   MM_FP_TOL: the Newton inversion runs in a cheaper arithmetic (polynomial form of the map, fused multiply-adds,
 *     Cramer's rule; csrc/mm_newton_hex8.h) that must CERTIFY every decision the reference makes -- each residual test
 *     against 1e-8 * scale, the final max|xi| against 1.025 -- with a margin two orders above the rounding differences
 *     between the two arithmetics; a solve it cannot certify is repeated in the reference's arithmetic.  Element / node
 *     ids and the failed count stay bit-identical; weights and values agree with the reference to
 *     max(1e-12, 64 eps |x| / h) (|x| / h: coordinate magnitude over element size; 1e-12 on the BASELINE meshes),
 *     relative to max|weight| = 1 resp. max|field|.  h is the element's shortest edge: on an element with a collapsed
 *     edge or face (h = 0) the bound is void, and it does not speak about elements that lost their orientation
 *     (mirrored, tangled); ids and the failed count are bit-identical there too.
 * The environment variable MM_FP_MODE=tol makes MM_FP_TOL the default of new contexts (how a user of the legacy
 * symbols opts in). */
#define MM_FP_EXACT 0
#define MM_FP_TOL 1
int mm_set_fp_mode(mm_context *ctx, int mode);
int mm_get_fp_mode(mm_context *ctx);
/* out4 = {solves of the last hex8 locate stage that MM_FP_TOL repeated in the reference's arithmetic, targets the first
 * pass left over (they go to the reference-order kernel, or with a long on-demand list to its second pass), targets that
 * second pass left over for the reference-order kernel, 0}.  Synchronises. */
int mm_last_locate_stats(mm_context *ctx, long long *out4);
/* The kNN kernels the last call launched, as a mask of MM_KNN_RAN_* (tests: which branch of the dispatcher ran).  A
 * list-mode launch is a pair of kernels, one wave or one lane per target, and the list's length picks the one that works. */
#define MM_KNN_RAN_LANE 1      /* knn_lane_kernel */
#define MM_KNN_RAN_STRIP 2     /* knn_strip_kernel */
#define MM_KNN_RAN_CELL 4      /* knn_cell_kernel */
#define MM_KNN_RAN_LIST 8      /* list mode: the stragglers, a forced list, a caller's list */
#define MM_KNN_RAN_GENERIC 16  /* k > 32: knn_query_kernel over one grid */
#define MM_KNN_RAN_LEVELS 32   /* k > 32: knn_query_levels_kernel over density levels */
#define MM_KNN_RAN_TREE 64     /* the density-adaptive tree */
#define MM_KNN_RAN_ONE_PASS 128 /* build: mm_interpolate_hex8 sorted the centroids as it computed them (centroid_sort_kernel) */
#define MM_KNN_RAN_TARGET_REPLAY 256 /* query: mm_interpolate_hex8 put the targets where the previous call's sort put them (target_replay_kernel) */
int mm_last_knn_kernels(mm_context *ctx, int *mask);

/* Stage timers (hipEvents on the context's stream).  With profiling on, every kernel
 * launched by the calls above is bracketed by events; mm_last_timings fills ms[stage] for
 * the stages of the LAST call (0 for stages that did not run) and returns the stage count. */
enum mm_stage {
    MM_STAGE_CENTROID = 0,
    MM_STAGE_KNN_BUILD = 1,
    MM_STAGE_KNN_QUERY = 2,    /* whole query: target sort + cell kernel + straggler kernel */
    MM_STAGE_LOCATE = 3,       /* whole locate: all launches + reference-order kernel (+ on-demand full lists) */
    MM_STAGE_GATHER = 4,
    MM_STAGE_KNN_CELL = 5,     /* the kNN cell kernel alone (inside MM_STAGE_KNN_QUERY) */
    MM_STAGE_LOCATE_PASS0 = 6, /* the first locate pass alone (inside MM_STAGE_LOCATE) */
    MM_STAGE_COUNT = 7
};
/* on: 0 no stage timers; 1 all stages; 2 only MM_STAGE_KNN_CELL and MM_STAGE_LOCATE_PASS0 (the two dominant
 * kernels: every timed stage costs the stream two events, ~5 us each between kernels) */
int mm_set_profiling(mm_context *ctx, int on);
int mm_last_timings(mm_context *ctx, double *ms, int n);

#ifdef __cplusplus
}
#endif
#endif /* MULTIMESH_HIP_H */
