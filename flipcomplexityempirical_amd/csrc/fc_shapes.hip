// Compactness series: replay of the FC_DIAG_SERIES flip logs against node areas,
// exterior lengths and shared edge lengths -- district areas, perimeters and Polsby-Popper scores,
// their time integrals and the score histograms over the yields of the series window, in exact
// integers.
//
// The mapping is the election series' (fc_votes.hip): one wavefront per chain, one 64-thread
// workgroup each, no global atomics, every output row has one owner.  Lanes are districts
// (k <= 32): lane d holds A[d], P[d] (int32: both totals are below 2^31), Q[d], their lazy time
// integrals and Q's histogram bin with the yield since which it has held it; the plan's least
// compact district (Qmin), its bin and its integral are wave-uniform.  Events are read 64 at a
// time, one per lane, two chunks ahead; a chunk's neighbour rows and node values are loaded into
// registers while the chunk before it is replayed and go to LDS when its turn comes.
//
// What differs from the election replay is the sequential phase.  A perimeter depends on the
// labels of the flipped node's neighbours at the time of the flip, so an event cannot resolve its
// districts by a compare over the chunk: per event, in log order, the neighbour slots are spread
// over lanes, each reads cur[w] of its neighbour from LDS, three 16-lane sums give the lengths to
// all neighbours, to those in the old district and to those in the target, and cur[v] = target is
// in LDS before the next event reads it.
#include <hip/hip_runtime.h>

#include "fc_replay_dev.h"
#include "fc_shapes.h"

namespace fc {
namespace {

using dev::min_lanes32;
using dev::rl32;
using dev::rl64;
using dev::row0_sum;

// searchsorted(edges, q, side="right"): the edges at or below q, lane l holding edge l
// (INT64_MAX past the end)
__device__ __forceinline__ int32_t score_bin(int64_t eq, int32_t q) { return __popcll(__ballot(eq <= (int64_t)q)); }

// W: slots per neighbour row (8 or 16)
template <int W>
__global__ __launch_bounds__(64) void shapes_kernel(const ShapesParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using NbrRows = replay::Rows<W>;
    constexpr int RV = NbrRows::RV;  // 16-byte pieces of a row
    const int lane = (int)threadIdx.x;
    const int32_t cl = (int32_t)blockIdx.x;
    const LogWindow &w = p.log;
    const int32_t c = w.c0 + cl;
    const int32_t k = w.k, n = w.n, n_edges = p.n_edges;
    const int32_t nb = n_edges + 1;
    int64_t *hist = (int64_t *)smem;                                   // [k + 1][nb], the last row Qmin's
    int32_t *tab = (int32_t *)(smem + shapes_hist_bytes(k, n_edges));  // [2][32] initial areas, perimeters
    int4 *stage4 = (int4 *)(tab + 64);                                 // [64][W] the chunk's neighbour rows
    int8_t *cur = (int8_t *)(stage4 + 64 * RV);                        // [npad]

    for (int i = lane; i < (k + 1) * nb; i += 64) hist[i] = 0;
    tab[lane] = 0;
    const int8_t *a = w.a0 + (size_t)c * w.npad;
    for (int u = lane; u < n; u += 64) cur[u] = (int8_t)((int)a[u] & 31);
    __syncthreads();
    // the window-start areas and perimeters by LDS adds: a node brings its exterior length and
    // the lengths to its neighbours in other districts, so a cut edge counts once from each end
    for (int u = lane; u < n; u += 64) {
        const int d = (int)cur[u];
        const ShapeNode nd = p.nodes[u];
        int32_t per = nd.ext;
        const int4 *row = (const int4 *)(p.rows + (size_t)u * W);
#pragma unroll
        for (int q = 0; q < RV; ++q) {
            const int4 r = row[q];
            if (r.x >= 0 && (int)cur[r.x] != d) per += r.y;
            if (r.z >= 0 && (int)cur[r.z] != d) per += r.w;
        }
        if (nd.area) atomicAdd(&tab[d], nd.area);
        if (per) atomicAdd(&tab[32 + d], per);
    }
    __syncthreads();

    const int64_t t0 = w.t0[cl];
    // lane d < k: district d
    int32_t A = lane < k ? tab[lane & 31] : 0;
    int32_t P = lane < k ? tab[32 + (lane & 31)] : 0;
    int32_t Q = (int32_t)shape_score(A, P);
    int64_t psum = 0, qsum = 0, t_last = t0, bin_t = t0;
    int32_t bin = 0;
    const int64_t eq = lane < n_edges ? p.edges[lane] : INT64_MAX;
    // wave-uniform: the least score, its bin, the yields since which they have held, the integral
    int32_t qmin = min_lanes32(lane < k ? Q : INT32_MAX), mbin = 0;
    int64_t qmin_t = t0, mbin_t = t0, min_sum = 0;
    if (n_edges > 0) {
        for (int d = 0; d < k; ++d) {
            const int32_t b = score_bin(eq, rl32(Q, d));
            if (lane == d) bin = b;
        }
        mbin = score_bin(eq, qmin);
    }

    const replay::Log log(w, cl);
    const int64_t ne = log.ne;
    // the next chunk's node values and rows (empty slots: length 0)
    auto load_row = [&](int v, int4 (&r)[RV], ShapeNode &nd) {
        nd = ShapeNode{0, 0};
        NbrRows::load(p.rows, v, 0, r);
        if (v >= 0) nd = p.nodes[v];
    };
    // the events of the next chunk and of the one after it, and the next chunk's rows
    replay::Prefetch<2> nx(log, lane);
    int v1, tg1;
    replay::decode(nx.e[0], lane < ne, n, k, v1, tg1);
    int4 r1[RV];
    ShapeNode nd1;
    load_row(v1, r1, nd1);
    for (int64_t base = 0; base < ne; base += 64) {
        const int64_t t = replay::ev_t(nx.e[0]);
        const int v = v1, tg = tg1;
        const int32_t area = nd1.area, ext = nd1.ext;
        NbrRows::stage(stage4, lane, r1);
        replay::decode(nx.e[1], base + 64 + lane < ne, n, k, v1, tg1);
        load_row(v1, r1, nd1);
        nx.advance(log, base, lane);
        __syncthreads();

        const int cnt = log.count(base);
        for (int i = 0; i < cnt; ++i) {
            const int vi = rl32(v, i);
            if (vi < 0) continue;
            const int64_t te = rl64(t, i);
            const int td = rl32(tg, i);
            const int32_t ar = rl32(area, i), ex = rl32(ext, i);
            // slot `lane` of the node's row: the neighbour's district now, and the shared length
            // (the row and cur[v] are read together: one LDS latency, then the neighbours')
            const RowSlot s = NbrRows::slot(stage4, i, lane, 0);
            const int cv = (int)cur[vi];
            const int dw = s.nbr >= 0 ? (int)cur[s.nbr] : -1;
            const int od = __builtin_amdgcn_readfirstlane(cv);
            const int32_t l_all = row0_sum(s.val);
            const int32_t l_old = row0_sum(dw == od ? s.val : 0);
            const int32_t l_tgt = row0_sum(dw == td ? s.val : 0);
            if (od != td) {
                if (lane == od || lane == td) {
                    const int64_t dt = te - t_last;
                    t_last = te;
                    psum += (int64_t)P * dt;
                    qsum += (int64_t)Q * dt;
                    // edges to the old district turn cut, edges to the target turn uncut, an edge
                    // to a third district moves from the old district's perimeter to the target's
                    if (lane == od) {
                        P += 2 * l_old - l_all - ex;
                        A -= ar;
                    } else {
                        P += l_all - 2 * l_tgt + ex;
                        A += ar;
                    }
                    Q = (int32_t)shape_score(A, P);
                }
                const int32_t qm = min_lanes32(lane < k ? Q : INT32_MAX);
                if (qm != qmin) {
                    min_sum += (int64_t)qmin * (te - qmin_t);
                    qmin_t = te;
                    qmin = qm;
                }
                if (n_edges > 0) {
                    const int32_t b_od = score_bin(eq, rl32(Q, od)), b_td = score_bin(eq, rl32(Q, td));
                    const int32_t b = lane == od ? b_od : (lane == td ? b_td : bin);
                    if (b != bin) {
                        hist[lane * nb + bin] += te - bin_t;
                        bin_t = te;
                        bin = b;
                    }
                    const int32_t mb = score_bin(eq, qmin);
                    if (mb != mbin) {
                        if (lane == 0) hist[k * nb + mbin] += te - mbin_t;
                        mbin_t = te;
                        mbin = mb;
                    }
                }
                if (lane == 0) cur[vi] = (int8_t)td;
            }
            __syncthreads();  // cur[v] is in LDS before the next event's lanes read their neighbours
        }
    }

    // the window's end: every integral takes its last segment
    const int64_t t1 = w.t_end[cl];
    psum += (int64_t)P * (t1 - t_last);
    qsum += (int64_t)Q * (t1 - t_last);
    min_sum += (int64_t)qmin * (t1 - qmin_t);
    if (n_edges > 0) {
        if (lane < k) hist[lane * nb + bin] += t1 - bin_t;
        if (lane == 0) hist[k * nb + mbin] += t1 - mbin_t;
    }
    __syncthreads();
    if (lane < k) {
        const size_t o = (size_t)cl * k + lane;
        p.area_now[o] = A;
        p.perim_now[o] = P;
        p.perim_sum[o] = psum;
        p.pp_now[o] = Q;
        p.pp_sum[o] = qsum;
    }
    if (lane == 0) p.pp_min_sum[cl] = min_sum;
    if (n_edges > 0) {
        for (int i = lane; i < k * nb; i += 64) p.pp_hist[(size_t)cl * k * nb + i] = hist[i];
        for (int i = lane; i < nb; i += 64) p.pp_min_hist[(size_t)cl * nb + i] = hist[k * nb + i];
    }
}

template <int W>
int launch_w(const ShapesParams &p, hipStream_t stream) {
    const size_t lds = shapes_lds_bytes(p.log.npad, p.log.k, p.n_edges, W);
    hipLaunchKernelGGL((shapes_kernel<W>), dim3((unsigned)p.log.nc), dim3(64), lds, stream, p);
    return (int)hipGetLastError();
}

}  // namespace

int launch_shapes(const ShapesParams &p, void *stream) {
    const LogWindow &w = p.log;
    if (w.nc <= 0) return (int)hipSuccess;
    if (w.k < 1 || w.k > 32 || p.n_edges < 0 || p.n_edges > kShapeMaxEdges || (p.width != 8 && p.width != 16) ||
        w.n > w.npad || !shapes_fit_lds(w.npad, w.k, p.n_edges, p.width))
        return (int)hipErrorInvalidValue;
    return p.width == 8 ? launch_w<8>(p, (hipStream_t)stream) : launch_w<16>(p, (hipStream_t)stream);
}

}  // namespace fc
