// The column of a node in a COLUMN-MAJOR table over a latitude x longitude map (table[nlat][nlon][len]: the column of one map
// node is one contiguous run), stated once for the kernels that walk down such columns: mm_layered_model_apply (mm_layered.hip:
// bounds and values) and mm_radial_stretch (mm_topography.hip: shifts).  The cells come from mm_latlon.h's find_cell.
//   bilinear : entry q is lerp(ta, lerp(to, T[ja][io][q], T[ja][io1][q]), lerp(to, T[ja1][io][q], T[ja1][io1][q]))
//   cell     : the table is piecewise constant around its map nodes: per axis the column is t < 0.5 ? i : i1, entry q unchanged
// Every product and sum is rounded on its own (-ffp-contract=off): include/multimesh_layered.h, step 3, publishes the statement.
#pragma once

#include "mm_latlon.h"

namespace mm_column {

// Entry q of the column(s) of a node in a column-major table whose columns hold `len` doubles: the lerp over longitude, then
// latitude, of the four corner columns, or (cell mode) the entry of the nearest map node's column.
template <bool BILINEAR>
struct Column {
    const double *c00, *c01, *c10, *c11;   // [ja][io], [ja][io1], [ja1][io], [ja1][io1]
    double ta, to;

    __device__ __forceinline__ Column(const double *table, i64 len, int nlon, const mm_latlon::Cell &ca, const mm_latlon::Cell &co)
    {
        if (BILINEAR) {
            const i64 r0 = (i64)ca.i * nlon, r1 = (i64)ca.i1 * nlon;
            c00 = table + (r0 + co.i) * len;
            c01 = table + (r0 + co.i1) * len;
            c10 = table + (r1 + co.i) * len;
            c11 = table + (r1 + co.i1) * len;
            ta = ca.t, to = co.t;
        } else {
            const int ja = ca.t < 0.5 ? ca.i : ca.i1, io = co.t < 0.5 ? co.i : co.i1;
            c00 = c01 = c10 = c11 = table + ((i64)ja * nlon + io) * len;
            ta = to = 0.0;
        }
    }
    __device__ __forceinline__ double at(i64 q) const
    {
        if (BILINEAR) return mm_lerp(ta, mm_lerp(to, c00[q], c01[q]), mm_lerp(to, c10[q], c11[q]));
        return c00[q];
    }
};

}  // namespace mm_column
