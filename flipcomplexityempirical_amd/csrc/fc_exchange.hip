// Replica exchange between the chains of one run (gfx950, MI355X).  DESIGN.md "Replica exchange".
//
// A ladder is an ordered list of chains; a chain's temperature is its row of the acceptance
// thresholds, which both flip kernels load at the start of every launch.  One launch of this
// kernel between two flip launches is one exchange round: it first attributes every ladder
// chain's streaming sums (and, with FC_LADDER_HIST, histogram rows) since the last round to the
// rung the chain held meanwhile, then tries the adjacent pairs of this round's parity and swaps
// the threshold rows of the accepted ones.  Replicas keep their state, draw counter and
// accumulators.
//
// Work is owned per item (fc_ladder.h LadderItem): the workgroup of pair (r, r + 1) attributes
// both of its replicas and then decides and applies the swap; a rung left unpaired by the parity
// is an item that only attributes.  Inside a ladder the rung map is a permutation, so every
// (ladder, rung) slot and every ladder chain has exactly one owner per round: no atomics, no
// synchronisation between workgroups, and the sums are reproducible.  The histogram deltas are
// the only real traffic: rows are streamed two bins per thread (16-byte accesses on the padded
// snapshot / slot rows), and rows whose bins did not move are only read.
#include <hip/hip_runtime.h>

#include "fc_internal.h"
#include "fc_ladder.h"

namespace fc {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxGrid = 2048;

static_assert(sizeof(fc_rung_stats) == (kRungFields + 2) * 8, "fc_rung_stats: 11 sums + 2 swap counters");

__device__ __forceinline__ int64_t sc_field(const ChainScalars &s, int f) {
    switch (f) {
        case 0: return s.steps;
        case 1: return s.proposals;
        case 2: return (int64_t)s.draw;
        case 3: return s.accepted;
        case 4: return s.inv_contig;
        case 5: return s.inv_pop;
        case 6: return s.sum_cut;
        case 7: return s.sum_nb;
        case 8: return s.sum_wait;
        case 9: return s.sum_cut2;
        default: return s.sum_nb2;
    }
}

// rung[i] += live[i] - snap[i]; snap[i] = live[i] over one histogram row of w bins.  snap and
// rung rows are 16-byte aligned and padded to an even width; the live row is 8-byte aligned.
__device__ __forceinline__ void attribute_row(const int64_t *live, int64_t *snap, int64_t *rung, int w, int t) {
    const int n2 = (w + 1) >> 1;
    const bool al = (((uintptr_t)live) & 15) == 0;
    for (int i = t; i < n2; i += kThreads) {
        const int e = 2 * i;
        longlong2 cur;
        if (al && e + 1 < w) {
            cur = *reinterpret_cast<const longlong2 *>(live + e);
        } else {
            cur.x = live[e];
            cur.y = e + 1 < w ? live[e + 1] : 0;
        }
        const longlong2 sn = *reinterpret_cast<const longlong2 *>(snap + e);
        if (cur.x == sn.x && cur.y == sn.y) continue;
        longlong2 rg = *reinterpret_cast<const longlong2 *>(rung + e);
        rg.x += cur.x - sn.x;
        rg.y += cur.y - sn.y;
        *reinterpret_cast<longlong2 *>(rung + e) = rg;
        *reinterpret_cast<longlong2 *>(snap + e) = cur;
    }
}

// chain c held slot s since the last attribution
__device__ __forceinline__ void attribute(const ExchangeParams &p, int c, int s, int t) {
    if (t < kRungFields) {
        const int64_t cur = sc_field(p.sc[c], t);
        int64_t *sn = p.snap + (size_t)c * kRungFields + t;
        reinterpret_cast<int64_t *>(p.rung + s)[t] += cur - *sn;
        *sn = cur;
    }
    if (p.cut_hist) {
        attribute_row(p.cut_hist + (size_t)c * p.cut_w, p.snap_cut + (size_t)c * p.cut_w2,
                      p.rung_cut + (size_t)s * p.cut_w2, p.cut_w, t);
        attribute_row(p.nb_hist + (size_t)c * p.nb_w, p.snap_nb + (size_t)c * p.nb_w2,
                      p.rung_nb + (size_t)s * p.nb_w2, p.nb_w, t);
    }
}

__global__ __launch_bounds__(kThreads) void exchange_kernel(ExchangeParams p) {
    __shared__ int s_acc;
    const int t = (int)threadIdx.x;
    for (int it = (int)blockIdx.x; it < p.n_items; it += (int)gridDim.x) {
        const LadderItem item = p.items[it];
        const int s = item.slot;
        const int c0 = p.chain_at[s];
        const int c1 = item.pair ? p.chain_at[s + 1] : -1;
        attribute(p, c0, s, t);
        if (c1 >= 0) attribute(p, c1, s + 1, t);
        if (!item.pair || !p.do_swap) continue;  // uniform over the workgroup
        if (t == 0) {
            const int32_t d = p.sc[c0].cut - p.sc[c1].cut;
            const uint64_t thr = ladder_threshold(p.pairs[s], d);
            const Words4 w = philox4x32_10(p.round, (uint32_t)p.slots[s].rung, p.slots[s].gid, 4u, p.seed_lo, p.seed_hi);
            const int acc = mant53(w.x0, w.x1) < thr ? 1 : 0;
            p.rung[s].swaps_tried += 1;
            p.rung[s].swaps_accepted += acc;
            s_acc = acc;
        }
        __syncthreads();
        if (s_acc) {
            if (t < p.tw) {  // the temperature: the two rows of acceptance thresholds
                uint64_t *r0 = p.thresh + (size_t)c0 * p.tw + t, *r1 = p.thresh + (size_t)c1 * p.tw + t;
                const uint64_t a = *r0, b = *r1;
                *r0 = b;
                *r1 = a;
            }
            if (t == 0) {
                p.slot_of[c0] = s + 1;
                p.slot_of[c1] = s;
                p.chain_at[s] = c1;
                p.chain_at[s + 1] = c0;
            }
        }
        __syncthreads();  // s_acc is reused by the next item
    }
}

}  // namespace

int launch_exchange(const ExchangeParams &p, void *stream) {
    const int grid = p.n_items < kMaxGrid ? p.n_items : kMaxGrid;
    if (grid <= 0) return (int)hipSuccess;
    hipLaunchKernelGGL(exchange_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

}  // namespace fc
