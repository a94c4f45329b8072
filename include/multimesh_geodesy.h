/*
 * multimesh_geodesy.h -- an EXTENSION of the C ABI of multi_mesh_hip.so (multimesh_hip.h): GEOGRAPHIC (geodetic) coordinates
 * -- points seen on an ellipsoid of revolution, on arrays that stay in HBM.  Every model tool of the library reads a model at
 * a point's geocentric latitude, its longitude and the depth R - |p|.  The GEOGRAPHIC VIEW of a point p is the pseudo-point
 * p' with the geocentric latitude of p' = the geodetic latitude of p, the same longitude, and |p'| = R + h, h the height of p
 * above the ellipsoid: a tool that reads p' reads (geodetic latitude, longitude, depth below the ellipsoid) of p with no
 * change of its own.  The entry point lives in the same library; it is declared here and not in multimesh_hip.h because that
 * header's set of functions is pinned by the binding tests ("Geographic coordinates").  Bound by
 * multimesh_amd/geodesy.py.
 *
 * THE STATEMENT.  Every product, quotient, sum, difference and square root is an IEEE-754 binary64 operation rounded on its
 * own, as written and bracketed here, sums left to right; no fused multiply-add (the library is built with
 * -ffp-contract=off), no libm.  Nothing is special-cased beyond what is written: NaN, +-inf, -0.0 and denormals give what
 * IEEE arithmetic gives (the payload and sign of a NaN that an operation produces are the processor's).
 * tests/geodesy_cases.py is the NumPy form.
 *
 * THE ELLIPSOID: ell, a HOST array of eight doubles, copied into the kernel's arguments; the kernel derives nothing:
 *     ell[0] = a      the semi-major axis              ell[4] = 1 - f   (f the flattening)
 *     ell[1] = b      the semi-minor axis              ell[5] = ep2b = (a*a - b*b) / b
 *     ell[2] = e2     the first eccentricity squared   ell[6] = e2a  = e2 * a
 *     ell[3] = 1 - e2                                  ell[7] = R    the radius of the sphere the model tools measure depth from
 * That the eight agree with one another is the caller's business (multimesh_amd.geodesy.Ellipsoid forms them).
 *
 * DIRECTION 0, Cartesian (x, y, z) -> the geographic view:
 *     s = sqrt(x*x + y*y)
 *     cl = x / s and sl = y / s where s > 0, else cl = 1.0 and sl = 0.0   (cos and sin of the longitude; a point on the polar
 *                                                                          axis, or with a NaN s, takes longitude 0: the
 *                                                                          rule of mm_local_components)
 *   Bowring's iteration on normalised pairs (no tangent: the poles need no special case):
 *     u = b*s;  v = a*z
 *     THREE times:
 *         nb = sqrt(u*u + v*v);  cb = u / nb;  sb = v / nb
 *         zn = z + ep2b*((sb*sb)*sb);  sn = s - e2a*((cb*cb)*cb)
 *         u = sn;  v = (1-f)*zn
 *     nn = sqrt(sn*sn + zn*zn);  cphi = sn / nn;  sphi = zn / nn           (of the geodetic latitude)
 *     h = (s*cphi + z*sphi) - a*sqrt(1.0 - e2*(sphi*sphi))                 (the height above the ellipsoid)
 *     rho = R + h, or radius_d[i] when radius_d is given
 *     out = ((rho*cphi)*cl, (rho*cphi)*sl, rho*sphi);  height_out_d[i] = h when height_out_d is given
 *   The centre gives NaN through 0 / 0.  Three passes leave a latitude error of 1.7e-16 rad at |p| >= 1000 km and 4.3e-14 rad
 *   down to 200 km (DESIGN.md holds the measurement).  Within about 50 km of the centre -- inside the evolute of the
 *   meridian ellipse, whose cusps lie at e2*a on the equatorial plane and at ep2b on the axis -- a point has more than one
 *   normal to the ellipsoid and its geodetic latitude is NOT UNIQUE: there the result is whatever the statement gives.
 *
 * DIRECTION 1, a pseudo-point (x, y, z) -> Cartesian:
 *     r = sqrt((x*x + y*y) + z*z);  s, cl, sl as above
 *     sphi = z / r;  cphi = s / r;  h = r - R
 *     N = a / sqrt(1.0 - e2*(sphi*sphi))
 *     out = (((N + h)*cphi)*cl, ((N + h)*cphi)*sl, (N*(1-e2) + h)*sphi)
 *
 * ARRAYS, all on the device.  in_d and out_d are f64[n][3] -- also the flat form of element-nodal points [E][P][3].
 * out_d == in_d is allowed (a lane reads its point before it writes it); any other overlap of the two extents is refused.
 * radius_d and height_out_d are f64[n], optional (null: not given) and of direction 0 only.
 *
 * Runs on the context's stream and does not synchronise; one launch, one lane per point, no atomics.
 * MM_ERR_ARG, decided on the host with nothing written and before the device is touched:
 *   a null ctx; a negative n, or 3 * n at or past 2^48; a null ell, an ell that is not finite, a <= 0 or b <= 0; a direction
 *   outside {0, 1}; radius_d or height_out_d with direction 1; with n > 0: a null in_d or out_d, extents of in_d and out_d
 *   that overlap without out_d == in_d, radius_d or height_out_d overlapping out_d, height_out_d overlapping in_d or radius_d.
 *   n == 0 is valid.
 */
#ifndef MULTIMESH_GEODESY_H
#define MULTIMESH_GEODESY_H

#include "multimesh_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MM_GEODESY_TO_GEOGRAPHIC 0
#define MM_GEODESY_TO_CARTESIAN 1
#define MM_GEODESY_NCONST 8 /* the doubles of ell */

int mm_geographic_points(mm_context *ctx, int64_t n, const double *in_d, double *out_d, const double *ell, int direction,
                         const double *radius_d, double *height_out_d);

#ifdef __cplusplus
}
#endif
#endif /* MULTIMESH_GEODESY_H */
