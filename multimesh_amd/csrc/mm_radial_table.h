// The 1-D radial table with discontinuities, stated once for the kernels that read one: mm_radial_model_apply
// (mm_radial.hip) and mm_harmonic_model_apply (mm_harmonics.hip).  radius f64[m] ascending, a REPEATED radius marks a
// discontinuity; the layers are the maximal strictly ascending runs; lstart int32[nlayers + 1] holds the first row of every
// layer, then m.  The statement is published in include/multimesh_hip.h (mm_radial_model_apply): the layer of an element is
// decided once by its centre, a node's radius is clamped to the layer, bisected and turned into the lerp weight.
// Bit parity with NumPy (tests/radial_cases.py): the bisection is mm_upper_bound, the quotient is rounded once.
#pragma once

#include <vector>

#include "mm_stream.h"

// ---- the host's check of a table that was read back: MM_ERR_ARG on behalf of the entry point `who` for a radius that is
// not finite, a descending step or a layer of a single row; otherwise lstart = the first row of every layer, then m.
inline int mm_radial_table_layers(const char *who, const double *R, i64 m, std::vector<int> &lstart)
{
    lstart.clear();
    lstart.push_back(0);
    for (i64 i = 0; i < m; ++i) {
        MM_REQUIRE_AS(who, R[i] - R[i] == 0.0, "a radius of the table is not finite");
        if (i == 0) continue;
        MM_REQUIRE_AS(who, R[i] >= R[i - 1], "the radii of the table descend");
        if (R[i] == R[i - 1]) {
            MM_REQUIRE_AS(who, i - lstart.back() >= 2, "a layer of the table has a single row");
            lstart.push_back((int)i);
        }
    }
    MM_REQUIRE_AS(who, m - lstart.back() >= 2, "a layer of the table has a single row");
    lstart.push_back((int)m);
    return MM_OK;
}

struct mm_radial_table {
    // the first radius of every layer, as an axis to bisect
    struct LayerFloor {
        const double *R;
        const int *lstart;
        __device__ __forceinline__ double operator[](int k) const { return R[lstart[k]]; }
    };

    // rc of the element whose P nodes are X[P][3]: c = (((X[0] + X[1]) + ...) + X[P-1]) / P per coordinate, rc = |c|
    // (no libm: NumPy's bits).  Also what mm_layered_model_apply (mm_layered.hip) measures an element's depth by.
    static __device__ __forceinline__ double centre_radius(const double *X, int P)
    {
        double cx = X[0], cy = X[1], cz = X[2];
        for (int p = 1; p < P; ++p) {
            cx = cx + X[3 * p];
            cy = cy + X[3 * p + 1];
            cz = cz + X[3 * p + 2];
        }
        const double dp = (double)P;
        cx = cx / dp, cy = cy / dp, cz = cz / dp;
        return mm_norm3(cx, cy, cz);
    }

    // the rows [a, b] of the layer of an element whose centre has the radius rc (not a NaN): the last layer whose first
    // radius is <= rc, clipped: the layer with r_lo <= rc < r_hi, below the first layer the first, above the last the last
    static __device__ __forceinline__ void layer_of(const double *R, const int *lstart, int nlayers, double rc, int &a,
                                                    int &b)
    {
        int k = mm_upper_bound(LayerFloor{R, lstart}, 0, nlayers, rc) - 1;
        k = k < 0 ? 0 : k;
        a = lstart[k];
        b = lstart[k + 1] - 1;
    }

    // a node of radius r within the layer's rows [a, b]: r' = min(max(r, R[a]), R[b]), i = clip(upper_bound(R[a..b], r')
    // - 1, a, b - 1), t = (r' - R[i]) / (R[i + 1] - R[i])
    static __device__ __forceinline__ void interval_of(const double *R, int a, int b, double r, int &i, double &t)
    {
        r = r < R[a] ? R[a] : r;
        r = r > R[b] ? R[b] : r;
        i = mm_upper_bound(R, a, b + 1, r) - 1;
        i = i < a ? a : i;
        i = i > b - 1 ? b - 1 : i;
        t = (r - R[i]) / (R[i + 1] - R[i]);
    }
};
