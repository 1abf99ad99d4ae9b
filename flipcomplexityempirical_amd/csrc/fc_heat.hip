// Heat-map series: replay of the FC_DIAG_SERIES event logs into the reference's
// heat maps over the yields of the series window -- the histograms of |cut| and |B|, per-edge cut
// times, per-node move counts and last moves, and the time each node spends in each district --
// in exact integers.
//
// One wavefront per chain, one 64-thread workgroup each, every output row has one owner, so no
// atomic crosses a workgroup (the mapping of fc_shapes.hip).  The current assignment is in LDS.
// Events are read 64 at a time, one per lane, two chunks ahead; a chunk's neighbour rows are
// loaded into registers while the chunk before it is replayed and go to LDS when its turn comes.
//
// The histograms are taken a chunk at a time: event j's |cut| and |B| hold from its t to the next
// event's, so its lane adds that difference (0 inside a burst) to their bins.  Everything else
// depends on the labels at the time of the event, so events are applied one at a time, in log
// order: the neighbour slots of the event's node are spread over lanes, each reads cur[w] of its
// neighbour, and an edge whose status the move toggles takes +t (turns uncut) or -t (turns cut);
// lanes past the row add the node's move, its last move and its two dwell terms, and store
// cur[v] = target.  The LDS operations of one wave execute in order, so the next event's reads
// see it.  No "since" time is kept per edge or node: the window's start (-t0) and end (+t_end)
// close the integrals of whatever is cut, and wherever a node is, at those two yields.
//
// Two accumulation forms, one kernel (template parameter LDS): the requested arrays privatised in
// LDS beside the assignment and written out once at the end, or the output rows in device memory
// as the accumulators.  Every accumulation is an add, LDS or global, whose result is not read back
// before the close, so neither form waits for one.  The host takes the global-rows form unless
// FC_HEAT_LDS_ROWS asks for the other: an LDS image leaves one wave per compute unit, and that
// measured 4.7 times slower on the C2 shape.
#include <hip/hip_runtime.h>

#include "fc_heat.h"
#include "fc_replay_dev.h"

namespace fc {
namespace {

using dev::rl32;
using dev::rl64;

typedef unsigned long long u64;

__device__ __forceinline__ void add(u64 *p, int64_t x) { (void)atomicAdd(p, (u64)x); }

// W: slots per neighbour row (8 or 16).  LDS: the accumulators are in LDS.
template <int W, bool LDS>
__global__ __launch_bounds__(64) void heat_kernel(const HeatParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using NbrRows = replay::Rows<W>;
    constexpr int RV = NbrRows::RV;  // 16-byte pieces of a row
    const int lane = (int)threadIdx.x;
    const int32_t cl = (int32_t)blockIdx.x;
    const LogWindow &w = p.log;
    const int32_t c = w.c0 + cl;
    const int32_t k = w.k, n = w.n, E = p.n_edges, nbw = p.nb_width;
    int4 *stage4 = (int4 *)smem;                 // [64][W] the chunk's neighbour rows
    int8_t *cur = (int8_t *)(stage4 + 64 * RV);  // [npad]
    const int nvec = (w.npad + 15) / 16;

    // the accumulators: LDS arrays in the entry point's order, or this chain's output rows
    size_t off = heat_base_bytes(w.npad, W);
    auto carve = [&](int a, int64_t *out) -> u64 * {
        const size_t len = heat_row_len(a, n, k, E, nbw);
        if constexpr (LDS) {
            u64 *q = (u64 *)(smem + off);
            if (out) off += (8 * len + 15) & ~(size_t)15;
            return q;
        } else {
            return (u64 *)out + (out ? (size_t)cl * len : 0);
        }
    };
    u64 *const cut_hist = carve(0, p.cut_hist);
    u64 *const nb_hist = carve(1, p.nb_hist);
    u64 *const ct = carve(2, p.cut_times);
    u64 *const moves = carve(3, p.moves);
    u64 *const last = carve(4, p.last_move);
    u64 *const dwell = carve(5, p.dwell);
    const bool h_cut = p.cut_hist, h_nb = p.nb_hist, h_ct = p.cut_times, h_mv = p.moves, h_last = p.last_move,
               h_dw = p.dwell;

    auto zero = [&](bool have, u64 *arr, int a) {
        if (!have) return;
        const int len = (int)heat_row_len(a, n, k, E, nbw);
        for (int i = lane; i < len; i += 64) arr[i] = 0;
    };
    zero(h_cut, cut_hist, 0);
    zero(h_nb, nb_hist, 1);
    zero(h_ct, ct, 2);
    zero(h_mv, moves, 3);
    zero(h_last, last, 4);
    zero(h_dw, dwell, 5);
    const uint4 *a4 = (const uint4 *)(w.a0 + (size_t)c * w.npad);
    for (int i = lane; i < nvec; i += 64) {
        uint4 x = a4[i];
        x.x &= 0x1f1f1f1fu;
        x.y &= 0x1f1f1f1fu;
        x.z &= 0x1f1f1f1fu;
        x.w &= 0x1f1f1f1fu;
        ((uint4 *)cur)[i] = x;
    }
    if constexpr (!LDS) __threadfence();  // the zeroes are in the rows before any add to them
    __syncthreads();

    const int64_t t0 = w.t0[cl], t_end = w.t_end[cl];
    // every node's district and every cut edge (from its lower end) with weight wt
    auto close = [&](int64_t wt) {
        if (!h_dw && !h_ct) return;
        for (int u = lane; u < n; u += 64) {
            const int d = (int)cur[u];
            if (h_dw && d < k) add(&dwell[(size_t)u * k + d], wt);
            if (!h_ct) continue;
            const int4 *row = (const int4 *)(p.rows + (size_t)u * W);
#pragma unroll
            for (int q = 0; q < RV; ++q) {
                const int4 r = row[q];
                if (r.x > u && (int)cur[r.x] != d) add(&ct[r.y], wt);
                if (r.z > u && (int)cur[r.z] != d) add(&ct[r.w], wt);
            }
        }
    };
    close(-t0);

    const replay::Log log(w, cl);
    const int64_t ne = log.ne;
    // the events of the next chunk and of the one after it, and the next chunk's rows (empty
    // slots: edge -1)
    replay::Prefetch<2> nx(log, lane);
    int v1, tg1;
    replay::decode(nx.e[0], lane < ne, n, k, v1, tg1);
    int4 r1[RV];
    NbrRows::load(p.rows, v1, -1, r1);
    // the window-start |cut| and |B| hold until the first event
    {
        const int64_t t_first = ne > 0 ? rl64(replay::ev_t(nx.e[0]), 0) : t_end;
        const int64_t c0v = p.cut0[cl], b0v = p.nb0[cl];
        if (lane == 0 && t_first > t0) {
            if (h_cut && c0v >= 0 && c0v <= E) add(&cut_hist[c0v], t_first - t0);
            if (h_nb && b0v >= 0 && b0v < nbw) add(&nb_hist[b0v], t_first - t0);
        }
    }

    for (int64_t base = 0; base < ne; base += 64) {
        const int64_t t = replay::ev_t(nx.e[0]);
        const int v = v1, tg = tg1;
        const int ecut = replay::ev_cut(nx.e[0]), enb = replay::ev_nb(nx.e[0]);
        const bool in = base + lane < ne;
        NbrRows::stage(stage4, lane, r1);
        replay::decode(nx.e[1], base + 64 + lane < ne, n, k, v1, tg1);
        NbrRows::load(p.rows, v1, -1, r1);
        nx.advance(log, base, lane);
        // the histograms: this event's |cut| and |B| hold until the next event's t
        int64_t t_next = (int64_t)__shfl_down((long long)t, 1);
        const int64_t t_chunk = rl64(replay::ev_t(nx.e[0]), 0);  // the next chunk's first t
        if (lane == 63) t_next = t_chunk;
        if (base + lane + 1 >= ne) t_next = t_end;
        if (in && t_next > t) {
            if (h_cut && ecut <= E) add(&cut_hist[ecut], t_next - t);
            if (h_nb && enb < nbw) add(&nb_hist[enb], t_next - t);
        }
        __syncthreads();

        const int cnt = log.count(base);
        for (int i = 0; i < cnt; ++i) {
            const int vi = rl32(v, i);
            if (vi < 0) continue;
            const int64_t te = rl64(t, i);
            const int td = rl32(tg, i);
            // slot `lane` of the node's row and the neighbour's district now (the row and cur[v]
            // are read together: one LDS latency, then the neighbours')
            const RowSlot s = NbrRows::slot(stage4, i, lane, -1);
            const int cv = (int)cur[vi];
            const int dw = s.nbr >= 0 ? (int)cur[s.nbr] : -1;
            const int od = __builtin_amdgcn_readfirstlane(cv);
            if (od != td) {
                // an edge to the old district turns cut (-t), one to the target turns uncut (+t)
                if (h_ct && s.nbr >= 0 && (dw == od || dw == td)) add(&ct[s.val], dw == td ? te : -te);
                if (h_dw && lane == 16 && od < k) add(&dwell[(size_t)vi * k + od], te);
                if (h_dw && lane == 17) add(&dwell[(size_t)vi * k + td], -te);
                if (lane == 18) cur[vi] = (int8_t)td;
            }
            if (h_mv && lane == 19) add(&moves[vi], 1);
            if (h_last && lane == 20) last[vi] = (u64)te;
            dev::compiler_fence();  // cur[v] is stored before the next event's lanes read their neighbours
        }
    }

    __syncthreads();
    close(t_end);
    if constexpr (LDS) {
        __syncthreads();
        auto flush = [&](u64 *arr, int64_t *out, int a) {
            if (!out) return;
            const size_t len = heat_row_len(a, n, k, E, nbw);
            u64 *row = (u64 *)out + (size_t)cl * len;
            for (size_t i = lane; i < len; i += 64) row[i] = arr[i];
        };
        flush(cut_hist, p.cut_hist, 0);
        flush(nb_hist, p.nb_hist, 1);
        flush(ct, p.cut_times, 2);
        flush(moves, p.moves, 3);
        flush(last, p.last_move, 4);
        flush(dwell, p.dwell, 5);
    }
}

template <int W>
int launch_w(const HeatParams &p, int32_t form, size_t lds, hipStream_t stream) {
    const dim3 grid((unsigned)p.log.nc), block(64);
    if (form == kHeatFormLds) launch_lds(heat_kernel<W, true>, grid, block, lds, stream, p);
    else launch_lds(heat_kernel<W, false>, grid, block, lds, stream, p);
    return (int)hipGetLastError();
}

}  // namespace

int launch_heat(const HeatParams &p, int32_t form, void *stream) {
    const LogWindow &w = p.log;
    if (w.nc <= 0) return (int)hipSuccess;
    if (w.k < 1 || w.k > 32 || w.n < 1 || w.n > w.npad || (w.npad & 15) || (p.width != 8 && p.width != 16) ||
        p.n_edges < 0 || p.nb_width < 1 || !p.rows || !p.cut0 || !p.nb0 ||
        (form != kHeatFormLds && form != kHeatFormGlobal))
        return (int)hipErrorInvalidValue;
    const uint32_t mask = (p.cut_hist ? kHeatCutHist : 0u) | (p.nb_hist ? kHeatNbHist : 0u) |
                          (p.cut_times ? kHeatCutTimes : 0u) | (p.moves ? kHeatMoves : 0u) |
                          (p.last_move ? kHeatLastMove : 0u) | (p.dwell ? kHeatDwell : 0u);
    const size_t lds = form == kHeatFormLds
                           ? heat_lds_bytes(w.npad, w.n, w.k, p.n_edges, p.nb_width, p.width, mask)
                           : heat_base_bytes(w.npad, p.width);
    return p.width == 8 ? launch_w<8>(p, form, lds, (hipStream_t)stream)
                        : launch_w<16>(p, form, lds, (hipStream_t)stream);
}

}  // namespace fc
