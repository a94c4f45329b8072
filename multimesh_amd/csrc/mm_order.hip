// A16 -- the polynomial order of element-nodal GLL values changed on the element they live on: per element, the tensor
// product of ONE rectangular 1-D table R f64[m_out][m_in] applied to the element's m_in^dim values.  With
// R[q][a] = l_a^in(g_q^out) that is the interpolation onto the GLL nodes of another order (up: exact for the polynomial the
// field is; down: the subsample on the coinciding nodes, whose rows of R are unit rows); with the transposed table and the
// orders swapped it is the transpose of that interpolation; with scale_in = the fine mass and div_out = the coarse mass it
// is the mass-weighted restriction M_c^-1 I^T M_f of a sensitivity kernel, in one pass.  No search, no Newton inversion.
//
//   mm_gll_tensor_apply  : out = (R (x) R (x) R) (in * scale_in) / div_out        per element and component
//   mm_element_deviation : max |a - b| and the largest bounding-box edge of b     per element (the check of gll_change_order)
//
// Bit parity with the NumPy statement (tests/order_cases.py): the table comes from the host, every product is rounded on
// its own (-ffp-contract=off), every sum starts from its first term and adds in ascending index, the division is one IEEE
// operation, nothing is special-cased (0 * NaN is NaN).  The order of the sweeps -- i, then j, then k -- is written out in
// include/multimesh_hip.h.
//
// The kernel follows gll_gradient_kernel: a 256-thread block takes a tile of 256 / max(P_in, P_out) whole elements and one
// component per step; the table goes into LDS once and each lane keeps, in registers, the row of R it needs in each sweep
// (a lane is the same entry of every step).  A step's input arrives through one load per lane (issued one step ahead and
// held in a register), is multiplied by scale_in and written to LDS; sweep 1 turns the TILE * m_in^dim values into
// TILE * m_out m_in^(dim-1), sweep 2 into TILE * m_out^2 m_in^(dim-2), sweep 3 (3-D) into the TILE * m_out^dim outputs: every
// one of these counts is at most 256, so each sweep is one entry per lane, a line of m_in reads from LDS, and a barrier
// separates a sweep from the next.  The last sweep's lane t is output value t of the step, so the stores are consecutive.
// No buffer is doubled: a buffer is written again one step later, behind at least one barrier that no lane reaches before
// it has finished reading this step's copy (vs: barriers 2 and 3; t1: barrier 3 and the next step's 1; t2: the next
// step's 1 and 2).
//
// Layouts (include/multimesh_hip.h).  0, [C][E][P]: a step is the contiguous run of one component of the tile.  2,
// [E][C][P]: the tile's data is ONE run of TILE * C items of P values; step c takes items c TILE .. (c + 1) TILE - 1 of it,
// again contiguous, and an item's element (for scale_in / div_out) is its index in the run divided by C.  1, [E][P][C]:
// step c reads component c of every node of the tile, addresses C doubles apart; the C steps of a tile follow each other
// in one block, so every cache line of the tile's run is fetched from HBM once and served from cache C - 1 times.
// scale_in / div_out stay in registers over the components of a tile in layouts 0 and 1 and are read per step in layout 2.
// HBM bytes per element and component: 8 (P_in + P_out), plus 8 per node and scale array.
#include "mm_common.h"
#include "mm_gll_tile.h"

namespace {

using gll::ipow;
using gll::kThreads;

template <int ORDER_IN, int ORDER_OUT, int DIM>
__global__ __launch_bounds__(kThreads) void gll_tensor_kernel(const double *__restrict__ table, int layout,
                                                              const double *__restrict__ in, double *__restrict__ out,
                                                              i64 nelem, i64 ncomp, const double *__restrict__ scale_in,
                                                              const double *__restrict__ div_out)
{
    constexpr int MI = ORDER_IN + 1, MO = ORDER_OUT + 1;
    constexpr int PI = ipow(MI, DIM), PO = ipow(MO, DIM);
    constexpr int TILE = kThreads / (PI > PO ? PI : PO);   // elements (items) per block and step
    constexpr int N1 = MO * ipow(MI, DIM - 1);             // values per item after sweep 1
    constexpr int N2 = MO * MO * ipow(MI, DIM - 2);        // ... after sweep 2 (2-D: the outputs)
    static_assert(TILE * PI <= kThreads && TILE * N1 <= kThreads && TILE * N2 <= kThreads && TILE * PO <= kThreads,
                  "one entry per lane in every sweep");
    __shared__ double vs[TILE * PI];
    __shared__ double t1s[TILE * N1];
    __shared__ double t2s[DIM == 3 ? TILE * N2 : 1];
    __shared__ double tab[MO * MI];

    const int tid = threadIdx.x;
    if (tid < MO * MI) tab[tid] = table[tid];
    __syncthreads();

    // what this lane is in the load, in each sweep and in the store (clamped to entry 0 where the lane has no part)
    const bool load_lane = tid < TILE * PI;
    const int item_l = load_lane ? tid / PI : 0;           // its item of the step
    const int node_l = load_lane ? tid - item_l * PI : 0;
    // sweep 1: entry r = qi + MO * rest of item, rest = b + MI * c  <-  v[a + MI * rest], a = 0 .. MI - 1
    const bool lane1 = tid < TILE * N1;
    const int it1 = lane1 ? tid / N1 : 0, r1 = lane1 ? tid - it1 * N1 : 0;
    const int src1 = it1 * PI + (r1 / MO) * MI;
    // sweep 2: entry r = qi + MO * (qj + MO * c)  <-  t1[qi + MO * (b + MI * c)], b = 0 .. MI - 1
    const bool lane2 = tid < TILE * N2;
    const int it2 = lane2 ? tid / N2 : 0, r2 = lane2 ? tid - it2 * N2 : 0;
    const int src2 = it2 * N1 + r2 % MO + MO * MI * (r2 / (MO * MO));
    // sweep 3: output q = qi + MO * (qj + MO * qk)  <-  t2[qi + MO * (qj + MO * c)], c = 0 .. MI - 1
    const bool store_lane = tid < TILE * PO;
    const int item_s = store_lane ? tid / PO : 0;
    const int node_s = store_lane ? tid - item_s * PO : 0;
    const int src3 = item_s * N2 + node_s % (MO * MO);
    double row1[MI], row2[MI], row3[MI];   // R[qi][.], R[qj][.], R[qk][.] of the three entries
#pragma unroll
    for (int a = 0; a < MI; ++a) {
        row1[a] = tab[(r1 % MO) * MI + a];
        row2[a] = tab[((r2 / MO) % MO) * MI + a];
        row3[a] = tab[(DIM == 3 ? node_s / (MO * MO) : 0) * MI + a];
    }

    const i64 ntiles = (nelem + TILE - 1) / TILE;
    auto tile_elems = [&](i64 t) -> i64 {   // valid elements of a tile: the last one may hold fewer
        const i64 left = nelem - t * TILE;
        return left < TILE ? left : TILE;
    };
    // item `item` of step c of a tile with nv elements: is it there, and which element of the tile is it
    auto item_ok = [&](i64 nv, i64 c, int item) -> bool {
        return layout == 2 ? c * TILE + item < nv * ncomp : item < nv;
    };
    auto item_elem = [&](i64 c, int item) -> i64 { return layout == 2 ? (c * TILE + item) / ncomp : item; };
    // offset of this lane's value of step c of the tile that starts at element e0, P values per item
    auto offset = [&](i64 e0, i64 c, i64 P) -> i64 {
        if (layout == 0) return (c * nelem + e0) * P + tid;
        if (layout == 2) return (e0 * ncomp + c * TILE) * P + tid;
        return (e0 * P + tid) * ncomp + c;
    };
    double stage = 0.0, sc = 1.0, dv = 1.0;
    auto fetch = [&](i64 t, i64 c) {
        const i64 e0 = t * TILE;
        stage = 0.0;
        if (load_lane && item_ok(tile_elems(t), c, item_l)) {
            const double x = in[offset(e0, c, PI)];
            if (scale_in != nullptr) {
                if (layout == 2 || c == 0) sc = scale_in[(e0 + item_elem(c, item_l)) * PI + node_l];
                stage = x * sc;
            } else {
                stage = x;
            }
        }
    };

    i64 tile = blockIdx.x;
    if (tile < ntiles) fetch(tile, 0);
    for (; tile < ntiles; tile += gridDim.x) {
        const i64 nv = tile_elems(tile);
        const i64 e0 = tile * TILE;
        for (i64 c = 0; c < ncomp; ++c) {
            if (load_lane) vs[tid] = stage;
            __syncthreads();
            // the next step's load
            if (c + 1 < ncomp) {
                fetch(tile, c + 1);
            } else if (tile + gridDim.x < ntiles) {
                fetch(tile + gridDim.x, 0);
            }
            if (lane1) {
                double acc = row1[0] * vs[src1];
#pragma unroll
                for (int a = 1; a < MI; ++a) acc = acc + row1[a] * vs[src1 + a];
                t1s[tid] = acc;
            }
            __syncthreads();
            double res = 0.0;
            if (lane2) {
                res = row2[0] * t1s[src2];
#pragma unroll
                for (int a = 1; a < MI; ++a) res = res + row2[a] * t1s[src2 + a * MO];
            }
            if constexpr (DIM == 3) {
                if (lane2) t2s[tid] = res;
                __syncthreads();
                if (store_lane) {
                    res = row3[0] * t2s[src3];
#pragma unroll
                    for (int a = 1; a < MI; ++a) res = res + row3[a] * t2s[src3 + a * MO * MO];
                }
            }
            if (store_lane && item_ok(nv, c, item_s)) {
                if (div_out != nullptr) {
                    if (layout == 2 || c == 0) dv = div_out[(e0 + item_elem(c, item_s)) * PO + node_s];
                    res = res / dv;
                }
                out[offset(e0, c, PO)] = res;
            }
        }
    }
}

template <int ORDER_IN, int ORDER_OUT, int DIM>
void launch_tensor(mm_context *ctx, const double *table, int layout, const double *in, double *out, i64 nelem, i64 ncomp,
                   const double *scale_in, const double *div_out)
{
    constexpr int PI = ipow(ORDER_IN + 1, DIM), PO = ipow(ORDER_OUT + 1, DIM);
    constexpr int TILE = kThreads / (PI > PO ? PI : PO);
    const dim3 grid(gll::grid_size(nelem, TILE));
    hipLaunchKernelGGL((gll_tensor_kernel<ORDER_IN, ORDER_OUT, DIM>), grid, dim3(kThreads), 0, ctx->stream, table, layout, in,
                       out, nelem, ncomp, scale_in, div_out);
}

// max |a - b| and the largest bounding-box edge of b, per element: what gll_change_order compares before it writes.  One
// wave per element, its lanes stride over the element's npts * DIM consecutive doubles (coalesced), a butterfly of
// shuffles ends it; the loop over elements is uniform within a wave, so every lane takes part in every shuffle.
constexpr int kWave = 64;

template <int DIM>
__global__ __launch_bounds__(kThreads) void element_deviation_kernel(const double *__restrict__ a, const double *__restrict__ b,
                                                                     i64 npts, i64 nelem, double *__restrict__ deviation,
                                                                     double *__restrict__ edge)
{
    constexpr int kWaves = kThreads / kWave;
    const int lane = threadIdx.x % kWave;
    const i64 n = npts * DIM;
    for (i64 e = (i64)blockIdx.x * kWaves + threadIdx.x / kWave; e < nelem; e += (i64)gridDim.x * kWaves) {
        const double *ae = a + e * n, *be = b + e * n;
        double dev = 0.0, lo[DIM], hi[DIM];
        int nan = 0;
#pragma unroll
        for (int d = 0; d < DIM; ++d) lo[d] = hi[d] = be[d];   // (node 0: fmin / fmax pass over a NaN unless all are)
        for (i64 i = lane; i < n; i += kWave) {
            const double x = be[i], diff = fabs(ae[i] - x);
            nan |= diff != diff;
            dev = fmax(dev, diff);
            const int axis = (int)(i % DIM);
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                if (d == axis) {
                    lo[d] = fmin(lo[d], x);
                    hi[d] = fmax(hi[d], x);
                }
            }
        }
        for (int s = kWave / 2; s > 0; s >>= 1) {
            dev = fmax(dev, __shfl_xor(dev, s));
            nan |= __shfl_xor(nan, s);
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                lo[d] = fmin(lo[d], __shfl_xor(lo[d], s));
                hi[d] = fmax(hi[d], __shfl_xor(hi[d], s));
            }
        }
        if (lane == 0) {
            double ed = hi[0] - lo[0];
#pragma unroll
            for (int d = 1; d < DIM; ++d) ed = fmax(ed, hi[d] - lo[d]);
            deviation[e] = nan ? __builtin_nan("") : dev;
            edge[e] = ed;
        }
    }
}

// [a, a + na) and [b, b + nb) share a byte
bool overlap(const double *a, i64 na, const double *b, i64 nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb * 8 && b0 < a0 + (uintptr_t)na * 8;
}

}  // namespace

extern "C" int mm_gll_tensor_apply(mm_context *ctx, int dim, int order_in, int order_out, const double *table_d, int layout,
                                   const double *in_d, double *out_d, int64_t nelem, int64_t ncomp, const double *scale_in_d,
                                   const double *div_out_d)
{
    // (what is wrong with the arguments is said before the context is looked at: none of these checks needs a device)
    MM_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
    MM_REQUIRE(order_in == 1 || order_in == 2 || order_in == 4, "order_in must be 1, 2 or 4");
    MM_REQUIRE(order_out == 1 || order_out == 2 || order_out == 4, "order_out must be 1, 2 or 4");
    MM_REQUIRE(order_in != order_out, "order_in equals order_out: nothing to resample (copy instead)");
    MM_REQUIRE(layout >= 0 && layout <= 2, "layout must be 0 ([C][E][P]), 1 ([E][P][C]) or 2 ([E][C][P])");
    MM_REQUIRE(nelem >= 0 && nelem < ((i64)1 << 48), "nelem out of range");
    MM_REQUIRE(ncomp >= 0 && ncomp < 65536, "ncomp out of range");
    MM_REQUIRE(nelem == 0 || ncomp < ((i64)1 << 55) / nelem, "nelem * ncomp out of range");   // offsets stay below 2^62
    MM_REQUIRE(table_d != nullptr, "null table");
    if (nelem > 0 && ncomp > 0) {
        MM_REQUIRE(in_d != nullptr && out_d != nullptr, "null array");
        i64 pin = order_in + 1, pout = order_out + 1;
        pin = dim == 3 ? pin * pin * pin : pin * pin;
        pout = dim == 3 ? pout * pout * pout : pout * pout;
        MM_REQUIRE(!overlap(in_d, ncomp * nelem * pin, out_d, ncomp * nelem * pout), "out_d must not overlap in_d");
        MM_REQUIRE(scale_in_d == nullptr || !overlap(scale_in_d, nelem * pin, out_d, ncomp * nelem * pout),
                   "out_d must not overlap scale_in_d");
        MM_REQUIRE(div_out_d == nullptr || !overlap(div_out_d, nelem * pout, out_d, ncomp * nelem * pout),
                   "out_d must not overlap div_out_d");
    }
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    if (nelem == 0 || ncomp == 0) return MM_OK;
    MM_HIP_CHECK(hipSetDevice(ctx->device));
#define MM_ORDER_CASE(I, O, D)                           \
    if (order_in == I && order_out == O && dim == D) \
    launch_tensor<I, O, D>(ctx, table_d, layout, in_d, out_d, nelem, ncomp, scale_in_d, div_out_d)
    MM_ORDER_CASE(1, 2, 2);
    MM_ORDER_CASE(1, 4, 2);
    MM_ORDER_CASE(2, 1, 2);
    MM_ORDER_CASE(2, 4, 2);
    MM_ORDER_CASE(4, 1, 2);
    MM_ORDER_CASE(4, 2, 2);
    MM_ORDER_CASE(1, 2, 3);
    MM_ORDER_CASE(1, 4, 3);
    MM_ORDER_CASE(2, 1, 3);
    MM_ORDER_CASE(2, 4, 3);
    MM_ORDER_CASE(4, 1, 3);
    MM_ORDER_CASE(4, 2, 3);
#undef MM_ORDER_CASE
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}

extern "C" int mm_element_deviation(mm_context *ctx, int dim, int64_t npts, const double *a_d, const double *b_d, int64_t nelem,
                                    double *deviation_d, double *edge_d)
{
    MM_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
    MM_REQUIRE(npts >= 1 && npts < ((i64)1 << 20), "npts out of range");
    MM_REQUIRE(nelem >= 0 && nelem < ((i64)1 << 40), "nelem out of range");   // offsets stay below 2^62
    if (nelem > 0) {
        MM_REQUIRE(a_d != nullptr && b_d != nullptr && deviation_d != nullptr && edge_d != nullptr, "null array");
        const i64 n = nelem * npts * dim;
        MM_REQUIRE(!overlap(a_d, n, deviation_d, nelem) && !overlap(b_d, n, deviation_d, nelem),
                   "deviation_d must not overlap an input");
        MM_REQUIRE(!overlap(a_d, n, edge_d, nelem) && !overlap(b_d, n, edge_d, nelem), "edge_d must not overlap an input");
        MM_REQUIRE(!overlap(deviation_d, nelem, edge_d, nelem), "edge_d must not overlap deviation_d");
    }
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    if (nelem == 0) return MM_OK;
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    const dim3 grid(gll::grid_size(nelem, kThreads / kWave));   // one wave per element
    if (dim == 2)
        hipLaunchKernelGGL(element_deviation_kernel<2>, grid, dim3(kThreads), 0, ctx->stream, a_d, b_d, npts, nelem, deviation_d,
                           edge_d);
    else
        hipLaunchKernelGGL(element_deviation_kernel<3>, grid, dim3(kThreads), 0, ctx->stream, a_d, b_d, npts, nelem, deviation_d,
                           edge_d);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}
