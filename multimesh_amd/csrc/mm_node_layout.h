// The host-side checks of an array that is addressed by the ADDRESSING paragraph of include/multimesh_params.h --
// component c of node p of group e at base[e * group_stride + cols[c] * comp_stride + p] --, stated once: the refusals of
// one array, its extent, and the two relations an output may have to an input.  Nothing here touches the device.
// Users: mm_parametrisation, mm_frames.
#pragma once

#include <stdio.h>

#include "mm_common.h"

namespace mm_layout {

constexpr i64 kMaxExtent = (i64)1 << 48;

// the extent of an array in elements, or -1 when it is at or past 2^48
inline i64 extent_of(i64 ngroups, i64 P, i64 group_stride, i64 comp_stride, const int *cols, int ncomp)
{
    int maxcol = 0;
    for (int c = 0; c < ncomp; ++c) maxcol = cols[c] > maxcol ? cols[c] : maxcol;
    const unsigned __int128 ext = (unsigned __int128)(ngroups > 0 ? ngroups - 1 : 0) * (unsigned __int128)group_stride +
                                  (unsigned __int128)maxcol * (unsigned __int128)comp_stride + (unsigned __int128)P;
    return ext >= (unsigned __int128)kMaxExtent ? -1 : (i64)ext;
}

struct Span {
    const double *base;
    i64 group_stride, comp_stride, extent;
};

inline bool same_array(const Span &a, const Span &b)
{
    return a.base == b.base && a.group_stride == b.group_stride && a.comp_stride == b.comp_stride;
}

inline bool disjoint(const Span &a, const Span &b) { return a.base + a.extent <= b.base || b.base + b.extent <= a.base; }

// the checks of one array; who: the entry point, what: the array's name in its messages
inline int check_array(const char *who, const char *what, i64 ngroups, i64 P, const double *base, i64 group_stride,
                       i64 comp_stride, const int *cols, int ncomp, bool output, Span *span)
{
    char msg[160];
    auto fail = [&](const char *why) {
        snprintf(msg, sizeof msg, "%s: %s", what, why);
        return msg;
    };
    MM_REQUIRE_AS(who, cols != nullptr, fail("null cols"));
    MM_REQUIRE_AS(who, ngroups == 0 || base != nullptr, fail("null array"));
    MM_REQUIRE_AS(who, group_stride >= 0 && comp_stride >= 0, fail("negative stride"));
    for (int c = 0; c < ncomp; ++c) MM_REQUIRE_AS(who, cols[c] >= 0, fail("negative column"));
    const i64 extent = extent_of(ngroups, P, group_stride, comp_stride, cols, ncomp);
    MM_REQUIRE_AS(who, extent >= 0, fail("extent at or past 2^48 elements"));
    if (output) {
        for (int c = 0; c < ncomp; ++c)
            for (int b = 0; b < c; ++b) MM_REQUIRE_AS(who, cols[b] != cols[c], fail("two output columns are equal"));
    }
    if (output && ngroups > 0) {
        int maxcol = 0;
        for (int c = 0; c < ncomp; ++c) maxcol = cols[c] > maxcol ? cols[c] : maxcol;
        // planes (components outermost) or rows (groups outermost): otherwise two lanes could write one element
        const i64 groups_span = (ngroups > 0 ? ngroups - 1 : 0) * group_stride + P;
        const bool planes = (ngroups <= 1 || group_stride >= P) && comp_stride >= groups_span;
        const bool rows = comp_stride >= P && (ngroups <= 1 || group_stride >= (i64)maxcol * comp_stride + P);
        MM_REQUIRE_AS(who, planes || rows, fail("two nodes or components of the output share an element"));
    }
    *span = Span{base, group_stride, comp_stride, extent};
    return MM_OK;
}

}  // namespace mm_layout
