// The transpose of the spherical-harmonic evaluation (include/multimesh_harmonic_adjoint.h, which holds the statement;
// tests/harmonic_adjoint_cases.py is its NumPy form).
//
//   mm_harmonic_model_transpose : grad[c][j][plane][idx(l, k)] = sum over the nodes of (weight * value) * lerp weight *
//                                 {cos, sin}(k phi) * P_lk(cos theta), in a stated order
//
// Bit parity with the statement: what a node is comes from mm_harmonic_node.h, the device functions of the forward kernel;
// every product and sum is rounded on its own (-ffp-contract=off), no libm, no float atomics, no matrix instructions (their
// internal summation order cannot be stated).  The sums are sequential over the nodes of a segment by definition, so no term
// crosses lanes: a lane owns a sum and adds to it node after node.
//
// Shape.  A 256-lane workgroup owns a segment (16384 / P elements) and walks it in the forward kernel's tiles of 256 / P whole
// elements, in ascending order.  Per tile the lanes play two parts in turn.
//   lanes as NODES: lane t is node t of the tile (layer, interval i, weight t, direction, e0 and e1 of the pass's components,
//     as in the forward kernel).  Order by order it forms the factors a0, a1, b0, b1 of its node and, kLC degrees at a time,
//     P_lk, and puts both into LDS: fac[component, factor][node], pl[node][degree].  The (k, l) loops have wave-uniform trip
//     counts, the tables d, a, b come through scalar loads.
//   lanes as TERMS: lane (degree of the chunk, component, factor) keeps the running segment sum of its output value for the
//     current interval in a register and adds fac * pl of the tile's nodes in ascending order: two LDS reads, one product, one
//     sum per node.  The nodes' intervals sit in one register per 64 nodes and are read with readlane, so the walk is
//     wave-uniform: runs of nodes in one interval (normally the whole tile) are a loop without a branch; when the interval
//     changes, the sum goes to the segment's slab and the other interval's sum comes from it -- the same sequential sum
//     continued, not a new one.  At the end of a chunk the sum goes to the slab, at the start of the next tile it comes back:
//     the same lane wrote it.
//   A chunk has 16 x 4 x nc terms, nc <= 2 components per pass: 128 of the 256 lanes (64 with one component) are terms, the
//   chunks take the waves in turn.  LDS: 34 KiB of pl, 16 KiB of fac, 9 KiB of coordinates and rows: two workgroups per CU.
//   (More components per pass or longer chunks do not fit the 64 KiB a workgroup gets without asking; DESIGN.md section 5,
//   "Spherical-harmonic transpose", counts the cost.)
// The slabs start as +0.0 (one fill per pass).  A last kernel adds them in ascending segment and forms Lo_j + Hi_{j-1}.
// Passes: the host splits the components (two at a time) and the orders into passes whose slabs fit the scratch limit; a
// pass starts the recurrences over k at its first order.
#include "mm_gll_tile.h"
#include "mm_harmonic_node.h"

#include "multimesh_harmonic_adjoint.h"

namespace {

using namespace mm_stream;   // kThreads, kWave, kMaxBlocks
using namespace mm_harmonic;
constexpr i64 kMaxExtent = (i64)1 << 48;
constexpr int kPassComps = 2;                  // components per pass
constexpr int kLC = 16;                        // degrees per chunk
constexpr int kLCS = kLC + 1;                  // doubles between two nodes' rows of pl (odd: the lanes-as-nodes' stores spread)
constexpr int kFacStride = kThreads + 1;       // doubles between two factors' rows of fac (the lanes-as-terms' reads spread)
constexpr int kFactors = 4;                    // a0, a1, b0, b1 = plane * 2 + side: (cosine, sine) x (Lo, Hi)
typedef unsigned long long u64;

struct TransposeArgs {
    i64 ngroups, nseg;
    int P, Gs, m, nlayers, lmax, extend;
    i64 n;              // values per component
    int nc;             // components of this pass
    int k0, k1;         // its orders, both included
    int q0, nq;         // idx(k0, k0) and the number of (l, k) of the pass
    const double *weight, *values;   // (values: of the pass's first component)
    double *slab;       // f64[nseg][nc][m - 1][kFactors][nq]
    u64 *noutside;      // null in every pass but the first
};

__global__ __launch_bounds__(kThreads) void harmonic_transpose_kernel(const TransposeArgs args, const double *__restrict__ points,
                                                                      const double *__restrict__ R,
                                                                      const int *__restrict__ lstart,
                                                                      const double *__restrict__ td,
                                                                      const double *__restrict__ ta,
                                                                      const double *__restrict__ tb)
{
    __shared__ double pl[kThreads * kLCS];
    __shared__ double fac[kFactors * kPassComps * kFacStride];
    __shared__ double xs[3 * kThreads];
    __shared__ int s_a[kThreads], s_b[kThreads], s_i[kThreads];   // rows [a, b] per element; interval per node, -1: no part

    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int P = args.P, m = args.m, L = args.lmax, nc = args.nc, nq = args.nq;
    const int tile = kThreads / P, el = tid / P;
    const i64 n = args.n, interval = (i64)kFactors * nq;   // doubles of the slab per interval
    unsigned mine = 0;   // nodes of elements outside the table

    for (i64 s = blockIdx.x; s < args.nseg; s += gridDim.x) {
        const i64 g0 = s * args.Gs, g1 = g0 + args.Gs < args.ngroups ? g0 + args.Gs : args.ngroups;
        for (i64 e = g0; e < g1; e += tile) {
            const int nel = (int)(g1 - e < tile ? g1 - e : tile), nnodes = nel * P;
            const i64 first = e * P;
            const double *src = points + 3 * first;
            __syncthreads();   // (the previous tile's reads of LDS are done)
            for (int q = tid; q < 3 * nnodes; q += kThreads) xs[q] = src[q];
            __syncthreads();
            if (tid < nel) {
                int a, b;
                element_layer(xs + 3 * tid * P, P, R, m, lstart, args.nlayers, args.extend, a, b);
                s_a[tid] = a;
                s_b[tid] = b;
            }
            __syncthreads();
            // ---- this lane's node
            const bool node = tid < nnodes;
            const int a = node ? s_a[el] : kDead, b = node ? s_b[el] : kDead;
            const bool live = a >= 0;
            const double x = node ? xs[3 * tid] : 0.0, y = node ? xs[3 * tid + 1] : 0.0, z = node ? xs[3 * tid + 2] : 0.0;
            if (node && a == kOutside) ++mine;
            int i = 0;
            double t = 0.0;
            const double r = mm_norm3(x, y, z);
            if (live) mm_radial_table::interval_of(R, a, b, r, i, t);
            s_i[tid] = live ? i : -1;
            double ct, st, cp, sp;
            direction(x, y, z, r, ct, st, cp, sp);
            double e0[kPassComps], e1[kPassComps];
#pragma unroll
            for (int c = 0; c < kPassComps; ++c) {
                double g = 0.0;
                if (live && c < nc) {
                    g = args.values[c * n + first + tid];
                    if (args.weight) g = args.weight[first + tid] * g;
                }
                e0[c] = (1.0 - t) * g;
                e1[c] = t * g;
            }
            // the recurrences over k start at the pass's first order
            double C = 1.0, S = 0.0, pkk = 1.0;
            for (int k = 1; k < args.k0; ++k) {
                fourier_step(k, cp, sp, C, S);
                pkk = sectoral_step(td[k], st, pkk);
            }
            int base = args.q0;   // idx(k, k)
            int turn = 0;         // the chunks take the waves in turn (the same turn in every tile: a sum stays with its lane)
            for (int k = args.k0; k <= args.k1; ++k) {
                if (k >= 1) {
                    fourier_step(k, cp, sp, C, S);
                    pkk = sectoral_step(td[k], st, pkk);
                }
                __syncthreads();   // (the previous chunk's reads of fac and pl are done; s_i is written)
#pragma unroll
                for (int c = 0; c < kPassComps; ++c) {
                    double *f = fac + kFactors * c * kFacStride + tid;
                    f[0] = k ? e0[c] * C : e0[c];
                    f[kFacStride] = k ? e1[c] * C : e1[c];
                    f[2 * kFacStride] = e0[c] * S;   // (not read at k = 0)
                    f[3 * kFacStride] = e1[c] * S;
                }
                double p1 = pkk, p2 = pkk;
                for (int l0 = k; l0 <= L; l0 += kLC) {
                    const int lcn = L + 1 - l0 < kLC ? L + 1 - l0 : kLC;
                    if (l0 != k) __syncthreads();   // (the previous chunk's reads of pl are done)
                    for (int j = 0; j < lcn; ++j) {
                        const int l = l0 + j, q = base + (l - k);
                        double Plk = pkk;
                        if (l == k + 1) Plk = legendre_second(ta[q], ct, pkk);
                        if (l >= k + 2) Plk = legendre_next(ta[q], tb[q], ct, p1, p2);
                        if (l > k) p2 = p1, p1 = Plk;
                        pl[tid * kLCS + j] = Plk;
                    }
                    __syncthreads();
                    // ---- lanes as terms
                    const int tt = (tid + kWave * turn) & (kThreads - 1);
                    ++turn;
                    const int cf = tt / kLC, lc = tt % kLC;   // cf = component * 4 + factor
                    const bool active = cf < kFactors * nc && lc < lcn && (k > 0 || (cf & 2) == 0);
                    if (__ballot(active) == 0) continue;   // (the same for every lane of the wave)
                    const double *fr = fac + (active ? cf : 0) * kFacStride, *pr = pl + (active ? lc : 0);
                    double *sl = args.slab;
                    if (active)
                        sl += ((s * nc + (cf >> 2)) * (m - 1) * kFactors + (cf & 3)) * (i64)nq + (base - args.q0) + (l0 - k) + lc;
                    int cur = -1;
                    double sum = 0.0;
                    for (int blk = 0; blk < nnodes; blk += kWave) {
                        const int vi = s_i[blk + lane];
                        const u64 part = __ballot(vi >= 0);
                        int j = 0;
                        while (j < kWave && (part >> j) != 0) {
                            j += (int)__builtin_ctzll(part >> j);   // the next node that takes part
                            const int ij = __builtin_amdgcn_readlane(vi, j);
                            const u64 differ = ~(__ballot(vi == ij) >> j);   // (bit 0 is clear; the bits past 64 - j are set)
                            const int run = differ == 0 ? kWave : (int)__builtin_ctzll(differ);   // nodes in a row with this interval
                            if (ij != cur) {   // the running sum changes places with the slab's
                                if (active) {
                                    if (cur >= 0) sl[cur * interval] = sum;
                                    sum = sl[ij * interval];
                                }
                                cur = ij;
                            }
                            if (active) {
                                const double *f = fr + blk + j, *p = pr + (blk + j) * kLCS;
                                for (int w = 0; w < run; ++w) sum = sum + f[w] * p[w * kLCS];
                            }
                            j += run;
                        }
                    }
                    if (active && cur >= 0) sl[cur * interval] = sum;
                }
                base += L + 1 - k;
            }
        }
    }
    if (args.noutside) {   // one integer sum per workgroup, one atomic
        __shared__ unsigned s_count[kThreads / kWave];
        mine = wave_sum(mine);
        if (lane == 0) s_count[tid / kWave] = mine;
        __syncthreads();
        if (tid == 0) {
            unsigned total = 0;
#pragma unroll
            for (int wv = 0; wv < kThreads / kWave; ++wv) total += s_count[wv];
            if (total != 0) atomicAdd(args.noutside, (u64)total);
        }
    }
}

// grad[c][j][plane][q0 + ql] = Lo_j + Hi_{j-1} over the pass's components and (l, k): the slabs in ascending segment, each
// sum from +0.0.  One lane per output value.
__global__ __launch_bounds__(kThreads) void harmonic_gather_kernel(const double *__restrict__ slab, i64 nseg, int nc, int m,
                                                                   int q0, int nq, int nlm, double *__restrict__ grad)
{
    const i64 total = (i64)nc * m * 2 * nq;
    const i64 per_seg = (i64)nc * (m - 1) * kFactors * nq;
    for (i64 at = (i64)blockIdx.x * kThreads + threadIdx.x; at < total; at += (i64)gridDim.x * kThreads) {
        const int ql = (int)(at % nq), plane = (int)(at / nq % 2), j = (int)(at / (2 * (i64)nq) % m);
        const i64 c = at / (2 * (i64)nq * m);
        double lo = 0.0, hi = 0.0;
        if (j <= m - 2) {
            const double *p = slab + ((c * (m - 1) + j) * kFactors + plane * 2) * (i64)nq + ql;
            for (i64 s = 0; s < nseg; ++s) lo = lo + p[s * per_seg];
        }
        if (j >= 1) {
            const double *p = slab + ((c * (m - 1) + (j - 1)) * kFactors + plane * 2 + 1) * (i64)nq + ql;
            for (i64 s = 0; s < nseg; ++s) hi = hi + p[s * per_seg];
        }
        grad[((c * m + j) * 2 + plane) * nlm + q0 + ql] = lo + hi;
    }
}

struct Pass {
    i64 c0;
    int nc, k0, k1;
};

}  // namespace

extern "C" int mm_harmonic_model_transpose(mm_context *ctx, const double *points_d, int64_t ngroups, int64_t P,
                                           const double *radius_d, int64_t m, int lmax, const double *weight_d,
                                           const double *values_d, int64_t ncomp, int extend, double *grad_d,
                                           int64_t *noutside_d, int64_t scratch_limit)
{
    MM_REQUIRE(ctx != nullptr, "ctx is null");
    MM_REQUIRE(ngroups >= 0 && ngroups < kMaxExtent, "ngroups out of range");
    MM_REQUIRE(P >= 1 && P <= MM_HARMONIC_MAX_P, "P must lie in [1, 256]");
    MM_REQUIRE(m >= 2 && m < ((i64)1 << 24), "the table needs between 2 and 2^24 rows");
    MM_REQUIRE(lmax >= 0 && lmax <= MM_HARMONIC_MAX_LMAX, "lmax must lie in [0, 255]");
    MM_REQUIRE(ncomp >= 0 && ncomp < 65536, "ncomp out of range");
    MM_REQUIRE(extend == 0 || extend == 1, "extend must be 0 or 1");
    MM_REQUIRE(scratch_limit >= 0, "scratch_limit is negative");
    MM_REQUIRE(radius_d != nullptr, "null table");
    const i64 nlm = (i64)(lmax + 1) * (lmax + 2) / 2;
    const i64 n = ngroups * P;   // (< 2^56)
    MM_REQUIRE((unsigned __int128)ncomp * (unsigned __int128)n < (unsigned __int128)kMaxExtent,
               "values: extent at or past 2^48 elements");
    MM_REQUIRE((unsigned __int128)ncomp * (unsigned __int128)(m * 2 * nlm) < (unsigned __int128)kMaxExtent,
               "grad: extent at or past 2^48 elements");
    MM_REQUIRE(ncomp == 0 || grad_d != nullptr, "null grad_d");
    MM_REQUIRE(ngroups == 0 || ncomp == 0 || (points_d != nullptr && values_d != nullptr), "null array");
    MM_HIP_CHECK(hipSetDevice(ctx->device));
    // ---- the passes: the slabs of a pass hold, per segment, component, interval and factor, one double per (l, k) of its orders
    const int Gs = (int)(MM_HARMONIC_SEGMENT_NODES / P > 1 ? MM_HARMONIC_SEGMENT_NODES / P : 1);
    const i64 nseg = (ngroups + Gs - 1) / Gs;
    const unsigned __int128 limit = (unsigned __int128)(scratch_limit ? scratch_limit : MM_HARMONIC_ADJOINT_SCRATCH);
    const unsigned __int128 unit = (unsigned __int128)nseg * (unsigned __int128)((m - 1) * kFactors * (i64)sizeof(double));
    const bool fits = unit * (unsigned)(lmax + 1) <= limit;   // order 0 of one component, the largest
    std::vector<Pass> passes;
    size_t slab_doubles = 0;
    if (ncomp > 0 && fits) {
        for (i64 c0 = 0; c0 < ncomp;) {
            int nc = (int)(ncomp - c0 < kPassComps ? ncomp - c0 : kPassComps);
            if (unit * (unsigned)(nc * (lmax + 1)) > limit) nc = 1;
            for (int k0 = 0; k0 <= lmax;) {
                int k1 = k0;
                i64 nq = lmax + 1 - k0;
                while (k1 < lmax && unit * (unsigned __int128)(nc * (nq + lmax - k1)) <= limit) nq += lmax - k1, ++k1;
                passes.push_back(Pass{c0, nc, k0, k1});
                const size_t doubles = (size_t)(unit / sizeof(double)) * (size_t)(nc * nq);
                slab_doubles = doubles > slab_doubles ? doubles : slab_doubles;
                k0 = k1 + 1;
            }
            c0 += nc;
        }
    }
    // what the kernels need besides the caller's arrays is queued BEFORE the one wait: the recurrence tables from the host,
    // the layer starts from the radii on the device
    std::vector<double> tab;
    double *tab_d = nullptr, *slab_d = nullptr;
    int *lstart_d = nullptr;
    if (!passes.empty()) {
        recurrence_tables(lmax, tab);
        mm_scratch_layout lay;
        lay.add(&tab_d, tab.size());
        lay.add(&lstart_d, (size_t)m + 1);
        lay.add(&slab_d, slab_doubles);
        const int rc = lay.commit(ctx, __func__);
        if (rc != MM_OK) return rc;
        MM_HIP_CHECK(hipMemcpyAsync(tab_d, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(layer_starts_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, radius_d, (int)m, lstart_d);
    }
    // the table's radii, checked on the host
    std::vector<double> R((size_t)m);
    MM_HIP_CHECK(hipMemcpyAsync(R.data(), radius_d, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MM_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // (tab and R leave scope with this call)
    std::vector<int> lstart;
    const int table_rc = mm_radial_table_layers(__func__, R.data(), m, lstart);
    if (table_rc != MM_OK) return table_rc;
    if (ncomp == 0) return MM_OK;
    if (!fits) {
        mm_set_error(MM_ERR_UNSUPPORTED, "%s: the segment sums of order 0 of one component do not fit the scratch limit", __func__);
        return MM_ERR_UNSUPPORTED;
    }
    TransposeArgs a;
    a.ngroups = ngroups;
    a.nseg = nseg;
    a.P = (int)P;
    a.Gs = Gs;
    a.m = (int)m;
    a.nlayers = (int)lstart.size() - 1;
    a.lmax = lmax;
    a.extend = extend;
    a.n = n;
    a.weight = weight_d;
    a.slab = slab_d;
    const double *td = tab_d, *ta = tab_d + (lmax + 1), *tb = ta + nlm;
    bool counted = false;
    for (const Pass &p : passes) {
        a.nc = p.nc;
        a.k0 = p.k0;
        a.k1 = p.k1;
        a.q0 = p.k0 * (lmax + 1) - p.k0 * (p.k0 - 1) / 2;
        a.nq = (p.k1 + 1) * (lmax + 1) - (p.k1 + 1) * p.k1 / 2 - a.q0;
        a.values = values_d ? values_d + p.c0 * n : nullptr;
        a.noutside = counted ? nullptr : (u64 *)noutside_d;   // (every pass sees the same elements: counted once)
        counted = true;
        if (nseg > 0) {
            const size_t bytes = (size_t)nseg * p.nc * (size_t)(m - 1) * kFactors * (size_t)a.nq * sizeof(double);
            if (mm_zero_async(ctx, slab_d, bytes) != MM_OK) return MM_ERR_HIP;
            hipLaunchKernelGGL(harmonic_transpose_kernel, dim3(mm_blocks(nseg, 1, kMaxBlocks)), dim3(kThreads), 0, ctx->stream,
                               a, points_d, radius_d, lstart_d, td, ta, tb);
        }
        const i64 outputs = (i64)p.nc * m * 2 * a.nq;
        hipLaunchKernelGGL(harmonic_gather_kernel, dim3(mm_blocks(outputs, kThreads, 8192)), dim3(kThreads), 0, ctx->stream,
                           slab_d, nseg, p.nc, (int)m, a.q0, a.nq, (int)nlm, grad_d + p.c0 * (m * 2 * nlm));
    }
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
}
