// What the two spherical-harmonic kernels do to an element and to a node, stated once: mm_harmonic_model_apply
// (mm_harmonics.hip) and its transpose mm_harmonic_model_transpose (mm_harmonic_adjoint.hip).  The statement is published in
// include/multimesh_harmonics.h; tests/harmonic_cases.py is its NumPy form.  Every product, quotient, sum and square root is
// rounded on its own (-ffp-contract=off), no libm.
//   element_layer   the centre of an element picks its layer: the rows [a, b], or kDead (a NaN centre), kOutside (outside the
//                   table with extend off)
//   direction       ct, st, cp, sp of a node; the equator at the origin, longitude 0 on the axis
//   fourier_step    C_k, S_k from C_{k-1}, S_{k-1} by complex multiplication
//   sectoral_step   P_kk from P_{k-1,k-1}
//   legendre_second, legendre_next   P_{k+1,k} and P_lk, l >= k + 2
//   recurrence_tables, layer_starts_kernel: the tables d, a, b (host) and the first row of every layer (device)
#pragma once

#include <math.h>

#include <vector>

#include "mm_radial_table.h"

namespace mm_harmonic {

using mm_stream::kThreads;
constexpr int kDead = -1, kOutside = -2;   // an element's first row when it has none: a NaN centre, a centre outside the table

// ---- lstart from the radii, on the device (one workgroup; the host forms the same array for its check, and would have to
// wait for the stream a second time to hand it over).  lstart[0] = 0, then every row that repeats the radius before it, in
// ascending order, then m.  Writes at most m + 1 entries whatever the radii hold.
static __global__ __launch_bounds__(kThreads) void layer_starts_kernel(const double *__restrict__ R, int m,
                                                                       int *__restrict__ lstart)
{
    __shared__ int s_count[kThreads];
    const int tid = threadIdx.x;
    const int len = (m + kThreads - 1) / kThreads;
    const int lo = tid * len < 1 ? 1 : tid * len, hi = (tid + 1) * len < m ? (tid + 1) * len : m;
    int count = 0;
    for (int i = lo; i < hi; ++i) count += R[i] == R[i - 1];
    s_count[tid] = count;
    __syncthreads();
    int at = 1;
    for (int q = 0; q < tid; ++q) at += s_count[q];
    for (int i = lo; i < hi; ++i)
        if (R[i] == R[i - 1]) lstart[at++] = i;
    if (tid == 0) lstart[0] = 0;
    if (tid == kThreads - 1) lstart[at] = m;
}

// d[0 .. L], then a and b at idx(l, k): integer products (exact), one division, one square root.  Entries the recurrence
// never reads (a_kk, b_kk, b_{k+1,k}) are 0.
inline void recurrence_tables(int L, std::vector<double> &tab)
{
    const int nlm = (L + 1) * (L + 2) / 2;
    tab.assign((size_t)(L + 1) + 2 * (size_t)nlm, 0.0);
    double *d = tab.data(), *a = d + (L + 1), *b = a + nlm;
    for (int k = 1; k <= L; ++k) d[k] = k == 1 ? sqrt(3.0) : sqrt((double)(2 * k + 1) / (double)(2 * k));
    int base = 0;
    for (int k = 0; k <= L; ++k) {
        for (int l = k + 1; l <= L; ++l) {
            a[base + l - k] = sqrt((double)((2 * l + 1) * (2 * l - 1)) / (double)((l - k) * (l + k)));
            if (l >= k + 2) b[base + l - k] = sqrt((double)((l - 1 - k) * (l - 1 + k)) / (double)((2 * l - 1) * (2 * l - 3)));
        }
        base += L + 1 - k;
    }
}

// The rows [a, b] of the layer of the element whose P nodes are X[P][3]: c = (((X[0] + X[1]) + ...) + X[P-1]) / P per
// coordinate, rc = |c|; a = b = kDead for a NaN rc, a = kOutside for a centre outside the table with extend off.
__device__ __forceinline__ void element_layer(const double *X, int P, const double *R, int m, const int *lstart, int nlayers,
                                              int extend, int &a, int &b)
{
    const double rc = mm_radial_table::centre_radius(X, P);
    a = kDead, b = kDead;
    if (rc == rc) {
        if (!extend && (rc < R[0] || rc > R[m - 1])) a = kOutside;
        else mm_radial_table::layer_of(R, lstart, nlayers, rc, a, b);
    }
}

// r = |(x, y, z)| is the caller's (it also finds the node's interval)
__device__ __forceinline__ void direction(double x, double y, double z, double r, double &ct, double &st, double &cp,
                                          double &sp)
{
    const double rho = sqrt(x * x + y * y);
    ct = z / r, st = rho / r, cp = x / rho, sp = y / rho;
    if (r == 0.0) ct = 0.0, st = 1.0;
    if (rho == 0.0) cp = 1.0, sp = 0.0;
}

// C, S: C_{k-1}, S_{k-1} -> C_k, S_k, k >= 1
__device__ __forceinline__ void fourier_step(int k, double cp, double sp, double &C, double &S)
{
    if (k == 1) {
        C = cp;
        S = sp;
    } else {
        const double c = C * cp - S * sp;
        S = S * cp + C * sp;
        C = c;
    }
}

// P_{k-1,k-1} -> P_kk, k >= 1
__device__ __forceinline__ double sectoral_step(double dk, double st, double pkk) { return (dk * st) * pkk; }

// P_{k+1,k} from P_kk, and P_lk from P_{l-1,k} and P_{l-2,k} for l >= k + 2; a, b: the tables' entries at idx(l, k)
__device__ __forceinline__ double legendre_second(double a, double ct, double pkk) { return (a * ct) * pkk; }
__device__ __forceinline__ double legendre_next(double a, double b, double ct, double p1, double p2)
{
    return a * (ct * p1 - b * p2);
}

}  // namespace mm_harmonic
