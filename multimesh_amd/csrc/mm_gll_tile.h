// The element tile of the GLL kernels that work node by node on the geometry of an element-nodal mesh, and the one copy
// of that geometry: J, det, G = J^-1, the unit radius, the reference gradient g and the physical gradient gr = G g.
// Who uses what: gll_mass_kernel (mm_mass.hip) and gll_gradient_kernel (mm_gradient.hip) use all of it; the stiffness
// kernel gll_diffusion_kernel (mm_diffusion.hip) uses the constants and the geometry functions and keeps its own lane
// set-up, loads and stores (see its header comment); gll_resolution_kernel (mm_resolution.hip) uses the tile, its fetch and
// the lanes' bookkeeping (Node) but no table and no Jacobian; mm_order.hip uses kThreads, kMaxBlocks, ipow and grid_size;
// radial_apply_kernel (mm_radial.hip), harmonic_apply_kernel (mm_harmonics.hip) and point_taper_kernel
// (mm_precondition.hip) use RunTile, the bookkeeping of the same tile for a P known only at run time.
// Every expression here is under a bit-parity contract with a NumPy statement (tests/mass_cases.py, diffusion_cases.py,
// gradient_cases.py) and its order of operations is published in include/multimesh_hip.h: every product is rounded on
// its own (-ffp-contract=off), every sum starts from its first term and adds in ascending a.
//
// The tile.  A 256-thread block takes a TILE of 256 / P whole elements (2 at P = 125, 9 at P = 27, 32 at P = 8), which
// are contiguous in memory: their coordinates go into LDS by coalesced 8-byte loads (LOADS = three per thread in 3-D), a
// component of u by one; lane t of the block is node t of the tile and reads its 3 m neighbours along the three tensor
// lines from LDS.  A lane is the same node (i, j, k) of every tile its block takes, so its rows of D (and, for those who
// ask, its weight product) live in registers for the whole kernel, read once from a copy of the tables in LDS.  At most
// kMaxBlocks blocks stride over the tiles; the last tile may hold fewer elements.  A kernel fetches a tile into
// registers one step ahead and copies it to LDS when its step comes: the LDS arrays, how many copies of them there are
// and where the barriers stand are each kernel's own.
//
// LDS layout.  Values indexed by the node of the tile are read along a tensor line with the strides 1, m, m^2 doubles;
// the 32 lanes of a half-wave (the conflict group of ds_read_b64, 32 banks of 8 bytes) read, along direction d, one
// address per line that crosses them: lanes that differ only in i_d read the same address (a broadcast), the others are
// consecutive nodes with i_d removed -- distinct addresses less than 32 doubles apart at m = 5 (i + 25 k, 0 <= i < 5,
// two values of k), so no two fall on one bank.  The coordinates keep the [node][dim] layout they have in memory:
// stride 3 doubles between nodes, odd, so the banks of 32 consecutive nodes are distinct as well.
#pragma once

#include "mm_stream.h"

namespace gll {

using mm_stream::kThreads;
using mm_stream::kMaxBlocks;   // blocks stride over the rest of the tiles

constexpr int ipow(int b, int e) { return e == 0 ? 1 : b * ipow(b, e - 1); }

// blocks of a launch over nelem elements, `tile` of them per block and step
inline unsigned grid_size(i64 nelem, int tile) { return mm_blocks(nelem, tile, kMaxBlocks); }

// The tile for a run-time P: 256 / P whole elements (groups of P points) per block and step.  Bookkeeping only -- as for
// the compile-time tile below, the load into LDS (a loop, or registers staged a step ahead) is each kernel's own.
struct RunTile {
    i64 ngroups;
    int P;
    int tile;     // whole elements per block and step
    int el;       // this lane's element of the tile: the same one in every tile
    i64 ntiles;

    __device__ __forceinline__ RunTile(i64 ngroups_, int P_)
        : ngroups(ngroups_), P(P_), tile(kThreads / P_), el((int)threadIdx.x / P_), ntiles((ngroups_ + tile - 1) / tile) {}
    // elements and nodes of tile t (the last one may hold fewer elements), its first node, its coordinates in points[.][3]
    __device__ __forceinline__ int nel(i64 t) const { return (int)(ngroups - t * tile < tile ? ngroups - t * tile : tile); }
    __device__ __forceinline__ int nnodes(i64 t) const { return nel(t) * P; }
    __device__ __forceinline__ i64 first_node(i64 t) const { return t * (i64)tile * P; }
    __device__ __forceinline__ const double *coords(const double *points, i64 t) const { return points + first_node(t) * 3; }
};

template <int ORDER, int DIM>
struct Tile {
    static constexpr int M = ORDER + 1;
    static constexpr int P = ipow(M, DIM);
    static constexpr int TILE = kThreads / P;            // elements per block and step
    static constexpr int TILE_NODES = TILE * P;          // <= 256
    static constexpr int TILE_DOUBLES = TILE_NODES * DIM;   // <= 768
    static constexpr int LOADS = (TILE_DOUBLES + kThreads - 1) / kThreads;
    static constexpr int TABLE = M * M;                  // doubles of D in the LDS table; the M weights follow it

    // ---- the tables: D f64[M][M] into tab[TABLE], or D and then the M weights into tab[TABLE + M]; ends with a barrier
    static __device__ __forceinline__ void load_tables(double *tab, const double *deriv)
    {
        const int tid = threadIdx.x;
        if (tid < TABLE) tab[tid] = deriv[tid];
        __syncthreads();
    }
    static __device__ __forceinline__ void load_tables(double *tab, const double *deriv,
                                                       const double *weights)
    {
        const int tid = threadIdx.x;
        if (tid < TABLE) tab[tid] = deriv[tid];
        else if (tid < TABLE + M) tab[tid] = weights[tid - TABLE];
        __syncthreads();
    }

    // ---- this lane's node of the tile: p = i[0] + M i[1] + M^2 i[2] of element el; direction d is the line of the
    // nodes that differ from it in i[d] alone, line[d] its first node (an offset in nodes of the tile), M^d its stride.
    // Node is the bookkeeping alone (mm_resolution.hip needs no table); Lane adds the lane's rows of D.
    struct Node {
        bool node_lane;   // 256 / P leaves lanes over: they hold no node (and are clamped to node 0)
        int el, p;        // the lane's element of the tile and its node of that element
        int i[DIM];
        int line[DIM];

        __device__ __forceinline__ Node()
        {
            const int tid = threadIdx.x;
            const bool has_node = tid < TILE_NODES;
            el = has_node ? tid / P : 0;
            p = has_node ? tid - el * P : 0;
            node_lane = has_node;
            const int pi = p % M, pj = (p / M) % M, pk = DIM == 3 ? p / (M * M) : 0;
            const int nbase = el * P;
            i[0] = pi, i[1] = pj;
            line[0] = nbase + (p - pi), line[1] = nbase + (p - pj * M);
            if constexpr (DIM == 3) i[2] = pk, line[2] = nbase + (p - pk * M * M);
        }
    };
    struct Lane : Node {
        double row[DIM][M];   // rows of D: D[i[d]][a]

        __device__ __forceinline__ explicit Lane(const double *tab) : Node()
        {
#pragma unroll
            for (int a = 0; a < M; ++a) {
                row[0][a] = tab[this->i[0] * M + a];
                row[1][a] = tab[this->i[1] * M + a];
                if constexpr (DIM == 3) row[2][a] = tab[this->i[2] * M + a];
            }
        }
        // (w_k * w_j) * w_i from the weights behind D in tab
        __device__ __forceinline__ double wprod(const double *tab) const
        {
            const double *w = tab + TABLE;
            if constexpr (DIM == 3) return (w[this->i[2]] * w[this->i[1]]) * w[this->i[0]];
            else return w[this->i[1]] * w[this->i[0]];
        }
    };

    // ---- tile bookkeeping
    // valid nodes of tile t: the last one may hold fewer elements
    static __device__ __forceinline__ int tile_nodes(i64 nelem, i64 t)
    {
        const i64 left = nelem - t * TILE;
        return (int)(left < TILE ? left : TILE) * P;
    }
    // the coordinates of tile t, coalesced, into registers (0.0 past the last element)
    static __device__ __forceinline__ void fetch_x(const double *gp, i64 nelem, i64 t, double (&stage)[LOADS])
    {
        const int tid = threadIdx.x;
        const int nd = tile_nodes(nelem, t) * DIM;
        const double *src = gp + t * (i64)TILE_DOUBLES;
#pragma unroll
        for (int r = 0; r < LOADS; ++r) {
            const int idx = r * kThreads + tid;
            stage[r] = idx < nd ? src[idx] : 0.0;
        }
    }
    // ... and from the registers into an LDS tile xs[TILE_DOUBLES]
    static __device__ __forceinline__ void store_x(double *xs, const double (&stage)[LOADS])
    {
        const int tid = threadIdx.x;
#pragma unroll
        for (int r = 0; r < LOADS; ++r) {
            const int idx = r * kThreads + tid;
            if (idx < TILE_DOUBLES) xs[idx] = stage[r];
        }
    }
    // this lane's value of component c of tile t (u f64[C][nelem][P])
    static __device__ __forceinline__ double fetch_u(const double *u, i64 nelem, i64 t, i64 c)
    {
        const int tid = threadIdx.x;
        const double *src = u + (c * (nelem * P) + t * (i64)TILE_NODES);
        return tid < tile_nodes(nelem, t) ? src[tid] : 0.0;
    }

    // ---- the geometry at this lane's node, from its rows of D (row[d][a] = D[i[d]][a]) and its line starts
    // J[d][c] = sum_a D[i[d]][a] * X[a along d][c] from the coordinate tile xs.  Each J[d][c] is its own ascending sum, so
    // the two forms give the same bits and differ in schedule alone: BY_DIRECTION forms J one tensor direction at a time
    // and keeps the scheduler from hoisting the next direction's LDS reads over this one's sums (all 3 m DIM values in
    // flight at once cost the order-4 3-D gradient kernel an occupancy step); otherwise the directions are interleaved.
    template <bool BY_DIRECTION>
    static __device__ __forceinline__ void jacobian(const double *xs, const double (&row)[DIM][M],
                                                    const int (&line)[DIM], double (&J)[3][3])
    {
        auto term = [&](int d, int a, int c) { return row[d][a] * xs[(line[d] + a * ipow(M, d)) * DIM + c]; };
        if constexpr (BY_DIRECTION) {
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
#pragma unroll
                for (int c = 0; c < DIM; ++c) J[d][c] = term(d, 0, c);
#pragma unroll
                for (int a = 1; a < M; ++a)
#pragma unroll
                    for (int c = 0; c < DIM; ++c) J[d][c] = J[d][c] + term(d, a, c);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int c = 0; c < DIM; ++c)
#pragma unroll
                for (int d = 0; d < DIM; ++d) J[d][c] = term(d, 0, c);
#pragma unroll
            for (int a = 1; a < M; ++a)
#pragma unroll
                for (int c = 0; c < DIM; ++c)
#pragma unroll
                    for (int d = 0; d < DIM; ++d) J[d][c] = J[d][c] + term(d, a, c);
        }
    }
    static __device__ __forceinline__ double det(const double (&J)[3][3])
    {
        if constexpr (DIM == 3)
            return (J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0])) +
                   J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
        else
            return J[0][0] * J[1][1] - J[0][1] * J[1][0];
    }
    // G = J^-1: the cofactors times 1 / det (the one division)
    static __device__ __forceinline__ void inverse(const double (&J)[3][3], double det, double (&G)[3][3])
    {
        const double rdet = 1.0 / det;
        if constexpr (DIM == 3) {
            G[0][0] = (J[1][1] * J[2][2] - J[1][2] * J[2][1]) * rdet;
            G[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * rdet;
            G[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * rdet;
            G[1][0] = (J[1][2] * J[2][0] - J[1][0] * J[2][2]) * rdet;
            G[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * rdet;
            G[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * rdet;
            G[2][0] = (J[1][0] * J[2][1] - J[1][1] * J[2][0]) * rdet;
            G[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * rdet;
            G[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * rdet;
        } else {
            G[0][0] = J[1][1] * rdet;
            G[0][1] = (-J[0][1]) * rdet;
            G[1][0] = (-J[1][0]) * rdet;
            G[1][1] = J[0][0] * rdet;
        }
    }
    // rh = x / |x| of this lane's node of the coordinate tile xs (3-D), 0 at the origin
    static __device__ __forceinline__ void unit_radius(const double *xs, double (&rh)[3])
    {
        const int tid = threadIdx.x;
        const double x0 = xs[tid * DIM], x1 = xs[tid * DIM + 1], x2 = xs[tid * DIM + 2];
        const double rn = mm_norm3(x0, x1, x2);
        const bool off_centre = rn > 0.0;
        rh[0] = off_centre ? x0 / rn : 0.0;
        rh[1] = off_centre ? x1 / rn : 0.0;
        rh[2] = off_centre ? x2 / rn : 0.0;
    }
    // the reference gradient g[d] = sum_a D[i[d]][a] * u[a along d] from the value tile us[TILE_NODES]
    static __device__ __forceinline__ void ref_gradient(const double *us, const double (&row)[DIM][M],
                                                        const int (&line)[DIM], double (&g)[3])
    {
#pragma unroll
        for (int d = 0; d < DIM; ++d) g[d] = row[d][0] * us[line[d]];
#pragma unroll
        for (int a = 1; a < M; ++a)
#pragma unroll
            for (int d = 0; d < DIM; ++d) g[d] = g[d] + row[d][a] * us[line[d] + a * ipow(M, d)];
    }
    // the physical gradient gr = G g
    static __device__ __forceinline__ void phys_gradient(const double (&G)[3][3], const double (&g)[3], double (&gr)[3])
    {
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            gr[c] = G[c][0] * g[0] + G[c][1] * g[1];
            if constexpr (DIM == 3) gr[c] = gr[c] + G[c][2] * g[2];
        }
    }
};

}  // namespace gll
