// Where a mesh ends: its boundary faces, which side of the domain each one is, their nodes, the distance of any point to
// the nearest of those nodes up to a cutoff, and a taper or blend of fields driven by that distance.
//
//   mm_boundary_faces     : the faces of a hexahedral mesh whose four sorted corner ids occur once among all 6 * nelem faces
//   mm_boundary_classify  : top / bottom / lateral side of every boundary face from its outward normal and the up direction
//   mm_boundary_nodes     : the (order + 1)^2 nodes of every selected face, face by face
//   mm_cutoff_distance    : d = min(cutoff, min over the sources of |x - s|), by a cell grid over the sources
//   mm_distance_taper     : w = smoothstep of d; out = w * a, or the blend (w * a) + ((1 - w) * b)
//
// Bit parity with the NumPy statements (tests/boundary_cases.py): every product, quotient and sum is rounded on its own
// (-ffp-contract=off); integer atomics only, and none of them reaches a result through its order: the hash table's claims
// decide which face stands for a class, never what the class is; the per-class counts, the histogram of the counting sort
// and the counts returned are integer sums; the order of the sources within a cell is free because a minimum has none.
//
// Conventions (include/multimesh_hip.h): corner c = i + 2 j + 4 k; local face f = 2 * axis + side; face code 6 e + f.
// mm_boundary_parts.h states the decoding of a code and the node of a face position once (face_of, face_node); a face's
// corners are its nodes at m = 2: (i, j) = (0,0), (1,0), (0,1), (1,1) in ascending order, (0,0), (1,0), (1,1), (0,1) in
// cyclic order.
//
// The faces.  A table of face indices with twice as many slots as faces (a power of two): a face hashes its sorted ids,
// claims an empty slot with one compare-and-swap or, where the slot is taken, compares its ids with the claimant's (read
// from the input, which nobody writes) and walks on when they differ -- mm_unique_hash.hip's pattern.  Every face adds one
// to its slot's count.  A face is a boundary face iff its slot's count is 1; flags, mm_exclusive_scan_int, emit: the codes
// come out ascending whatever the atomics did.
//
// The cutoff search and its margin (DESIGN.md section 5 has the derivation in full).  Cells of edge H > cutoff over the
// sources' bounding box -- the search grid, its fit to the caps and its bins are mm_surface.hip's too: mm_search_grid.h,
// mm_boundary_parts.h --, index floor(fl(fl(x - lo) * inv_h)) per axis with H = 1 / inv_h; a target looks at the 27 cells
// around its own.  Writing u = 2^-53: a source whose ROUNDED r is below cutoff has a true offset below cutoff * (1 + 4 u) on
// every axis (three roundings under the root, the root, the difference; with cutoff >= 2^-500 the squares' underflow is
// below 2^-73 of that).  The index argument v(x) = (x - lo) / H * (1 + delta), |delta| <= 2.01 u, is monotone in x, and
// for the targets that are not dismissed |x - lo| <= (dims + 1) H (1 + 3 u), so two points whose indices differ by two or
// more lie more than H * (1 - (2 dims + 2) * 2.01 u) apart.  With dims <= 1024 per axis that needs
// H >= cutoff * (1 + 4 u) / (1 - 2^-41); the edge is cutoff * (1 + 2^-30), about 2^11 times the need.  The index is formed
// from x - lo, one correctly rounded difference, so its error is relative to the offset within the box and NOT to |x|: a
// mesh at 6.3e6 m needs no absolute term.  Capping the cells only enlarges H.  A target whose index falls outside
// [-1, dims] on an axis -- or is a NaN -- is more than H from every source and keeps the cutoff at once.
#include "mm_boundary_parts.h"   // shared with mm_surface.hip: launch shape, counter words, faces, box, search grid
#include "mm_hash.h"

namespace {

constexpr unsigned kNoSlot = 0xffffffffu;  // slot_of of a face with an id out of range
constexpr double kEdgeMargin = 1.0 + 0x1p-30;

__device__ __forceinline__ void order2(unsigned &a, unsigned &b)
{
    const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo, b = hi;
}

// the four corner ids of face g = 6 e + f, sorted; false when one lies outside [0, nnodes) (nnodes < 2^31)
__device__ __forceinline__ bool face_key(const i64 *__restrict__ ids, i64 g, i64 nnodes, unsigned (&k)[4])
{
    const Face face = face_of(g, 2);
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const i64 id = ids[8 * face.e + face_node(face.a, face.fix, 2, c & 1, c >> 1)];
        ok = ok && (u64)id < (u64)nnodes;
        k[c] = (unsigned)id;
    }
    order2(k[0], k[1]), order2(k[2], k[3]), order2(k[0], k[2]), order2(k[1], k[3]), order2(k[1], k[2]);
    return ok;
}

// ------------------------------------------------------------------------------------------------ mm_boundary_faces
// table[s] = 1 + a face of the class that owns slot s (0: free, so that mm_zero_async clears table and counts in one
// launch); count[s] = the faces of that class; slot_of[g] = g's slot
__global__ __launch_bounds__(kThreads) void faces_insert_kernel(const i64 *__restrict__ ids, i64 nfaces, i64 nnodes,
                                                                int *__restrict__ table, unsigned mask, int *__restrict__ count,
                                                                unsigned *__restrict__ slot_of, u64 *bad)
{
    unsigned mine = 0;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x; g < nfaces; g += stride) {
        unsigned k[4];
        if (!face_key(ids, g, nnodes, k)) {
            ++mine;
            slot_of[g] = kNoSlot;
            continue;
        }
        unsigned s = (unsigned)mm_mix64(((u64)k[0] | ((u64)k[1] << 32)) ^ mm_mix64(((u64)k[2] | ((u64)k[3] << 32)) + 0x9e3779b97f4a7c15ull)) & mask;
        for (;;) {
            int cur = __atomic_load_n(&table[s], __ATOMIC_RELAXED);
            if (cur == 0) {
                const int old = atomicCAS(&table[s], 0, (int)g + 1);
                if (old == 0) break;   // claimed
                cur = old;
            }
            unsigned c[4];
            face_key(ids, (i64)cur - 1, nnodes, c);   // (a claimant's ids are in range)
            if (c[0] == k[0] && c[1] == k[1] && c[2] == k[2] && c[3] == k[3]) break;
            s = (s + 1) & mask;
        }
        atomicAdd(&count[s], 1);
        slot_of[g] = s;
    }
    mm_count_to(bad, mine);
}

// flag[g] = the face's key occurs once; counts: [0] such faces, [2] the faces whose key occurs more than twice
__global__ __launch_bounds__(kThreads) void faces_flag_kernel(const int *__restrict__ count, const unsigned *__restrict__ slot_of,
                                                              i64 nfaces, int *__restrict__ flag, u64 *counters)
{
    unsigned once = 0, many = 0;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x; g < nfaces; g += stride) {
        const unsigned s = slot_of[g];
        const int c = s == kNoSlot ? 0 : count[s];
        flag[g] = c == 1 ? 1 : 0;
        once += c == 1, many += c > 2;
    }
    mm_count_to(counters, once);
    mm_count_to(counters + 2, many);
}

// (a refused call writes nothing: *bad != 0)
__global__ __launch_bounds__(kThreads) void faces_emit_kernel(const int *__restrict__ flag, const int *__restrict__ rank,
                                                              i64 nfaces, i64 *__restrict__ faces, const u64 *__restrict__ counters,
                                                              i64 *__restrict__ info)
{
    if (counters[1] != 0) return;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x; g < nfaces; g += stride)
        if (flag[g]) faces[rank[g]] = g;
    if (info && blockIdx.x == 0 && threadIdx.x == 0) info[0] = (i64)counters[2];
}

// --------------------------------------------------------------------------------------------- mm_boundary_classify
struct ClassifyArgs {
    const double *corners;
    i64 nelem;
    const i64 *faces;
    i64 nb;
    int radial;
    double up[3], cos_min;
    int *side;
    u64 *bad;
};

// counts the codes outside [0, 6 nelem): their faces are not read
__global__ __launch_bounds__(kThreads) void codes_check_kernel(const i64 *__restrict__ faces, i64 nb, i64 nelem, u64 *bad)
{
    unsigned mine = 0;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 b = (i64)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += stride) mine += (u64)faces[b] >= (u64)(6 * nelem);
    mm_count_to(bad, mine);
}

__global__ __launch_bounds__(kThreads) void classify_kernel(const ClassifyArgs args)
{
    if (*args.bad != 0) return;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 b = (i64)blockIdx.x * blockDim.x + threadIdx.x; b < args.nb; b += stride) {
        const Face face = face_of(args.faces[b], 2);
        const double *X = args.corners + 24 * face.e;
        const int c0 = face_node(face.a, face.fix, 2, 0, 0), c1 = face_node(face.a, face.fix, 2, 1, 0);   // round the face
        const int c2 = face_node(face.a, face.fix, 2, 1, 1), c3 = face_node(face.a, face.fix, 2, 0, 1);
        double n[3], g[3], u[3], av[3], bv[3], fc[3], ec[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double q0 = X[3 * c0 + a], q1 = X[3 * c1 + a], q2 = X[3 * c2 + a], q3 = X[3 * c3 + a];
            av[a] = q2 - q0;
            bv[a] = q3 - q1;
            fc[a] = ((q0 + q1) + (q2 + q3)) * 0.25;
            double s = X[a] + X[3 + a];
#pragma unroll
            for (int c = 2; c < 8; ++c) s = s + X[3 * c + a];
            ec[a] = s * 0.125;
        }
        n[0] = av[1] * bv[2] - av[2] * bv[1];
        n[1] = av[2] * bv[0] - av[0] * bv[2];
        n[2] = av[0] * bv[1] - av[1] * bv[0];
#pragma unroll
        for (int a = 0; a < 3; ++a) g[a] = fc[a] - ec[a];
        if ((n[0] * g[0] + n[1] * g[1]) + n[2] * g[2] < 0.0) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
#pragma unroll
        for (int a = 0; a < 3; ++a) u[a] = args.radial ? fc[a] : args.up[a];
        const double t = (n[0] * u[0] + n[1] * u[1]) + n[2] * u[2];
        const double lim = args.cos_min * sqrt(((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) * ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]));
        args.side[b] = t >= lim ? 1 : (t <= -lim ? 2 : 0);   // (a NaN fails both tests)
    }
}

// ------------------------------------------------------------------------------------------------ mm_boundary_nodes
// (select_kernel, face_items_kernel and their driver: mm_boundary_parts.h)
// the (order + 1)^2 nodes of a face: k = lo + m * hi over the face's two free axes
struct NodeItems {
    static constexpr int kDoubles = 3;
    __host__ __device__ static int per_face(int m) { return m * m; }
    __device__ static void write(const double *__restrict__ X, int m, const Face &face, int k, double *__restrict__ dst)
    {
        const double *src = X + 3 * face_node(face.a, face.fix, m, k % m, k / m);
        dst[0] = src[0], dst[1] = src[1], dst[2] = src[2];
    }
};

// ----------------------------------------------------------------------------------------------- mm_cutoff_distance
// (sources_box_kernel, the search grid and its bins: mm_boundary_parts.h)
// a source is a record of its own in the one cell that holds it
struct PointBins {
    static constexpr int kDoubles = 3;
    __device__ static void cells(const Grid &g, const double *__restrict__ s, int (&c0)[3], int (&c1)[3])
    {
#pragma unroll
        for (int a = 0; a < 3; ++a) c0[a] = c1[a] = grid_cell(g, a, s[a]);
    }
};

// start == nullptr: no sources, every distance is the cutoff
__global__ __launch_bounds__(kThreads) void cutoff_query_kernel(const double *__restrict__ pts, i64 n, const double *__restrict__ sorted,
                                                                const int *__restrict__ start, const Grid g, double cutoff,
                                                                double *__restrict__ dist, u64 *count)
{
    unsigned mine = 0;
    const int dx = g.dims[0], dy = g.dims[1], dz = g.dims[2];
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        double d = cutoff;
        // the UNCLAMPED index, not grid_cell: the test against [-1, dims] below is the margin argument's own statement
        const double vx = floor(grid_coord(g, 0, x)), vy = floor(grid_coord(g, 1, y)), vz = floor(grid_coord(g, 2, z));
        // (a NaN fails the test: a point with a NaN coordinate keeps the cutoff)
        if (start && vx >= -1.0 && vx <= (double)dx && vy >= -1.0 && vy <= (double)dy && vz >= -1.0 && vz <= (double)dz) {
            const int cx = (int)vx, cy = (int)vy, cz = (int)vz;
            const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx + 1 < dx ? cx + 1 : dx - 1;
            const int y0 = cy > 0 ? cy - 1 : 0, y1 = cy + 1 < dy ? cy + 1 : dy - 1;
            const int z0 = cz > 0 ? cz - 1 : 0, z1 = cz + 1 < dz ? cz + 1 : dz - 1;
            for (int kz = z0; kz <= z1; ++kz)
                for (int ky = y0; ky <= y1; ++ky) {
                    const int row = grid_index(g, 0, ky, kz);   // (the row's cells x0 .. x1 are one run of sources)
                    const int b = start[row + x0], e = start[row + x1 + 1];
                    const double *s = sorted + 3 * (i64)b;   // (64-bit: 3 * K passes 2^31)
                    for (int j = b; j < e; ++j, s += 3) {
                        const double r = mm_norm3(x - s[0], y - s[1], z - s[2]);
                        if (r < d) d = r;
                    }
                }
        }
        dist[i] = d;
        mine += d < cutoff;
    }
    mm_count_to(count, mine);
}

// ------------------------------------------------------------------------------------------------ mm_distance_taper
// out may be a or b: no __restrict__ on the three, every lane reads its values before it writes one
__global__ __launch_bounds__(kThreads) void distance_taper_kernel(const double *__restrict__ dist, i64 n, double inner, double outer,
                                                                  int ncomp, const double *a, const double *b,
                                                                  const i64 *__restrict__ elem, double *out,
                                                                  double *__restrict__ weight, u64 *count)
{
    unsigned mine = 0;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double d = dist[i];
        double w;
        if (d <= inner) {
            w = 0.0;
        } else if (d >= outer) {
            w = 1.0;
        } else {
            const double s = (d - inner) / (outer - inner);
            w = (s * s) * (3.0 - 2.0 * s);
        }
        if (elem && elem[i] < 0) w = 0.0;
        mine += w < 1.0;
        if (weight) weight[i] = w;
        for (int c = 0; c < ncomp; ++c) {
            const double av = a[c * n + i];
            double o;
            if (b) {
                const double bv = b[c * n + i];
                o = w == 0.0 ? bv : (w == 1.0 ? av : (w * av) + ((1.0 - w) * bv));
            } else {
                o = w * av;
            }
            out[c * n + i] = o;
        }
    }
    mm_count_to(count, mine);
}

}  // namespace

extern "C" int64_t mm_boundary_faces(mm_context *ctx, const int64_t *corner_ids_d, int64_t nelem, int64_t nnodes,
                                     int64_t *faces_d, int64_t *info_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(nelem >= 0 && nelem < ((i64)1 << 27), "nelem must lie in [0, 2^27)");
    MM_REQUIRE(nnodes >= 0 && nnodes < ((i64)1 << 31), "nnodes must lie in [0, 2^31)");
    MM_REQUIRE(nelem == 0 || (corner_ids_d != nullptr && faces_d != nullptr), "null array");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    const i64 nfaces = 6 * nelem;
    u64 *counters = mm_counters_begin(ctx, kSlot, 3);   // [0] boundary faces, [1] ids out of range, [2] non-manifold faces
    if (!counters) return MM_ERR_HIP;
    if (nelem == 0) {
        if (info_d && mm_zero_async(ctx, info_d, sizeof(i64)) != MM_OK) return MM_ERR_HIP;
        return mm_counters_end(ctx, kSlot, 3) ? 0 : MM_ERR_HIP;
    }
    unsigned tsize = 1024;
    while ((u64)tsize < 2ull * (u64)nfaces) tsize <<= 1;
    int *table, *count, *flag, *rank, *tile_sums;
    unsigned *slot_of;
    mm_scratch_layout lay;
    lay.add(&table, 2 * (size_t)tsize);   // the table, then the counts
    lay.add(&slot_of, (size_t)nfaces);
    lay.add(&flag, (size_t)nfaces + 1);
    lay.add(&rank, (size_t)nfaces + 1);
    lay.add(&tile_sums, mm_scan_scratch_ints(nfaces));
    int rc = lay.commit(ctx, __func__);
    if (rc != MM_OK) return rc;
    count = table + tsize;
    if (mm_zero_async(ctx, table, 2 * (size_t)tsize * sizeof(int)) != MM_OK) return MM_ERR_HIP;
    const dim3 grid(stream_grid(nfaces)), block(kThreads);
    hipLaunchKernelGGL(faces_insert_kernel, grid, block, 0, ctx->stream, (const i64 *)corner_ids_d, nfaces, (i64)nnodes, table,
                       tsize - 1u, count, slot_of, counters + 1);
    hipLaunchKernelGGL(faces_flag_kernel, grid, block, 0, ctx->stream, (const int *)count, (const unsigned *)slot_of, nfaces, flag,
                       counters);
    MM_HIP_CHECK(hipGetLastError());
    rc = mm_exclusive_scan_int(ctx, flag, nfaces, rank, tile_sums);
    if (rc != MM_OK) return rc;
    hipLaunchKernelGGL(faces_emit_kernel, grid, block, 0, ctx->stream, (const int *)flag, (const int *)rank, nfaces, (i64 *)faces_d,
                       (const u64 *)counters, (i64 *)info_d);
    const i64 *got = mm_counters_end(ctx, kSlot, 3);
    if (!got) return MM_ERR_HIP;
    if (got[1] != 0) {
        mm_set_error(MM_ERR_ARG, "mm_boundary_faces: %lld faces have a corner id outside [0, %lld)", (long long)got[1],
                     (long long)nnodes);
        return MM_ERR_ARG;
    }
    return got[0];
}

extern "C" int mm_boundary_classify(mm_context *ctx, const double *corners_d, int64_t nelem, const int64_t *faces_d, int64_t nb,
                                    int radial, double upx, double upy, double upz, double cos_min, int *side_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(nelem >= 0 && nelem < ((i64)1 << 27), "nelem must lie in [0, 2^27)");
    MM_REQUIRE(nb >= 0 && nb <= 6 * nelem, "nb must lie in [0, 6 nelem]");
    MM_REQUIRE(radial == 0 || radial == 1, "radial must be 0 or 1");
    MM_REQUIRE(cos_min > 0.0 && cos_min <= 1.0, "cos_min must lie in (0, 1]");
    const double up2 = (upx * upx + upy * upy) + upz * upz;
    MM_REQUIRE(radial || (up2 > 0.0 && up2 < __builtin_inf()), "up must be finite and not zero");
    MM_REQUIRE(nb == 0 || (corners_d != nullptr && faces_d != nullptr && side_d != nullptr), "null array");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    if (nb == 0) return MM_OK;
    u64 *counters = mm_counters_begin(ctx, kSlot, 1);   // [0] codes out of range
    if (!counters) return MM_ERR_HIP;
    ClassifyArgs a;
    a.corners = corners_d;
    a.nelem = nelem;
    a.faces = (const i64 *)faces_d;
    a.nb = nb;
    a.radial = radial;
    a.up[0] = upx, a.up[1] = upy, a.up[2] = upz;
    a.cos_min = cos_min;
    a.side = side_d;
    a.bad = counters;
    hipLaunchKernelGGL(codes_check_kernel, dim3(stream_grid(nb)), dim3(kThreads), 0, ctx->stream, a.faces, (i64)nb, (i64)nelem, counters);
    hipLaunchKernelGGL(classify_kernel, dim3(stream_grid(nb)), dim3(kThreads), 0, ctx->stream, a);
    const i64 *got = mm_counters_end(ctx, kSlot, 1);
    if (!got) return MM_ERR_HIP;
    if (got[0] != 0) {
        mm_set_error(MM_ERR_ARG, "mm_boundary_classify: %lld face codes outside [0, %lld)", (long long)got[0], (long long)(6 * nelem));
        return MM_ERR_ARG;
    }
    return MM_OK;
}

extern "C" int64_t mm_boundary_nodes(mm_context *ctx, const double *points_d, int64_t nelem, int order, const int64_t *faces_d,
                                     const int *side_d, int64_t nb, int side_mask, double *out_d)
{
    return selected_face_items<NodeItems>(ctx, __func__, points_d, nelem, order, (const i64 *)faces_d, side_d, nb, side_mask, out_d);
}

extern "C" int64_t mm_cutoff_distance(mm_context *ctx, const double *points_d, int64_t n, const double *sources_d, int64_t K,
                                      double cutoff, double *dist_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(n >= 0 && n < ((i64)1 << 48), "n out of range");
    MM_REQUIRE(K >= 0 && K < ((i64)1 << 30), "K must lie in [0, 2^30)");
    MM_REQUIRE(cutoff > 0.0 && cutoff < __builtin_inf(), "cutoff must be positive and finite");
    MM_REQUIRE(cutoff >= kMinCutoff, "cutoff below 2^-500: the squares of the offsets would underflow under the margin");
    MM_REQUIRE(n == 0 || (points_d != nullptr && dist_d != nullptr), "null points or distances");
    MM_REQUIRE(K == 0 || sources_d != nullptr, "null sources");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    u64 *words = mm_counters_begin(ctx, kSlot, kWords);   // [0] points with d < cutoff, [1] bad sources, [2..7] the box
    if (!words) return MM_ERR_HIP;
    Grid g = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 1.0, 0.0, 0.0, {1, 1, 1}};
    double *sorted = nullptr;
    int *start = nullptr;
    if (K > 0) {
        hipLaunchKernelGGL(sources_box_kernel, dim3(stream_grid(K)), dim3(kThreads), 0, ctx->stream, sources_d, (i64)K, words);
        const i64 *got = mm_counters_end(ctx, kSlot, kWords);
        if (!got) return MM_ERR_HIP;
        if (got[1] != 0) {
            mm_set_error(MM_ERR_ARG, "mm_cutoff_distance: %lld sources are not finite", (long long)got[1]);
            return MM_ERR_ARG;
        }
        double extent[3];
        box_of_words(got, g.lo, g.hi);
        for (int a = 0; a < 3; ++a) {
            extent[a] = g.hi[a] - g.lo[a];
            MM_REQUIRE(extent[a] < __builtin_inf(), "the sources' extent overflows");
        }
        // the edge: above the cutoff by the margin, enlarged until the grid fits its caps (a larger edge keeps the search valid)
        mm_search_grid_fit(g, extent, cutoff * kEdgeMargin, 2);
        const int rc = bins_build<PointBins>(ctx, __func__, sources_d, K, K, g, sorted, start);
        if (rc != MM_OK) return rc;
    }
    if (n > 0)
        hipLaunchKernelGGL(cutoff_query_kernel, dim3(stream_grid(n)), dim3(kThreads), 0, ctx->stream, points_d, (i64)n,
                           (const double *)sorted, (const int *)start, g, cutoff, dist_d, words);
    const i64 *got = mm_counters_end(ctx, kSlot, 1);
    return got ? got[0] : MM_ERR_HIP;
}

extern "C" int64_t mm_distance_taper(mm_context *ctx, const double *dist_d, int64_t n, double inner, double outer, int64_t ncomp,
                                     const double *a_d, const double *b_d, const int64_t *elem_d, double *out_d,
                                     double *weight_out_d)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(n >= 0 && n < ((i64)1 << 48), "n out of range");
    MM_REQUIRE(ncomp >= 0 && ncomp < 65536, "ncomp out of range");
    MM_REQUIRE(inner >= 0.0 && outer >= inner && outer < __builtin_inf(), "the radii need 0 <= inner <= outer, both finite");
    MM_REQUIRE(n == 0 || dist_d != nullptr, "null distances");
    MM_REQUIRE(n == 0 || ncomp == 0 || (a_d != nullptr && out_d != nullptr), "null values");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    u64 *counters = mm_counters_begin(ctx, kSlot, 1);   // [0] nodes with w < 1
    if (!counters) return MM_ERR_HIP;
    if (n > 0)
        hipLaunchKernelGGL(distance_taper_kernel, dim3(stream_grid(n)), dim3(kThreads), 0, ctx->stream, dist_d, (i64)n, inner, outer,
                           (int)ncomp, a_d, b_d, (const i64 *)elem_d, out_d, weight_out_d, counters);
    const i64 *got = mm_counters_end(ctx, kSlot, 1);
    return got ? got[0] : MM_ERR_HIP;
}
