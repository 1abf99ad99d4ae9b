// Locality-splits series: replay of the FC_DIAG_SERIES flip logs against a node
// labelling (counties, municipalities) -- how many districts every locality meets, which
// localities are split, and the splits / excess histograms over the yields of the series window,
// in exact integers.
//
// One wavefront per chain, one 64-thread workgroup each, no global atomics, every output row has
// one owner (the mapping of fc_votes.hip).  The chain's image is in LDS: the cell table
// [n_loc][k] (uint16, two cells per 32-bit word), parts [n_loc], the integrals, the two histograms
// and the current assignment.
//
// The replay is chunk-parallel: 64 events, one per lane, are resolved together.  Every aggregate
// is a sum of per-event deltas, and an event's deltas depend only on the earlier events of the
// chunk on the same node, the same cells and the same locality.  A lane finds those as lane masks
// (match_mask: one ballot per key bit, so a dozen steps where a broadcast loop over the lanes
// takes 64) and counts them with popcounts:
//   1. old district: the target of the latest earlier event of the chunk on the same node, else
//      cur[v];
//   2. the sizes of the cells (c, old) and (c, target) just before the event: the chunk-start
//      table plus the net of the earlier events of the chunk on the same cell; split_rule then
//      gives the event's change of parts(c) and of sq, and the two zero-crossings;
//   3. parts(c) just before the event: the chunk-start value plus the earlier changes of the
//      chunk on c; with it the change of the split bit.
// A wave prefix sum of the (split, excess) changes gives both aggregates after every event, and
// each lane adds its run length (the yields up to the next event) to its two histogram bins.
// The time integrals need no order at all: a quantity that changes by delta at yield t and then
// holds adds delta * (t_end - t) to its sum over the window, on top of (its window-start value) *
// (the window's yields).  So split_sum, parts_sum, dlocs_sum and sq_sum are plain integer adds per
// event (LDS atomics for the shared rows, a register for sq), with nothing to flush at the end.
// The chunk is then applied to the table, parts and cur by LDS adds.
#include <hip/hip_runtime.h>

#include "fc_replay_dev.h"
#include "fc_splits.h"

namespace fc {
namespace {

using dev::rl32;
using dev::rl64;
using replay::bits_for;
using replay::match_mask;

__device__ __forceinline__ void lds_add64(int64_t *p, int64_t x) {
    atomicAdd((unsigned long long *)p, (unsigned long long)x);
}

__global__ __launch_bounds__(64) void splits_kernel(const SplitsParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = (int)threadIdx.x;
    const int32_t cl = (int32_t)blockIdx.x;
    const LogWindow &w = p.log;
    const int32_t ch = w.c0 + cl;
    const int32_t k = w.k, n = w.n, L = p.n_loc, X = p.x_top;
    const int32_t nck = L * k;
    const int bits_n = bits_for(n), bits_l = bits_for(L), bits_k = bits_for(k);
    int64_t *acc_split = (int64_t *)smem;                       // [L] sum_t split_t(c)
    int64_t *acc_parts = acc_split + L;                         // [L] sum_t parts_t(c)
    int64_t *hs = acc_parts + L;                                // [L + 1] splits histogram
    int64_t *he = hs + L + 1;                                   // [X + 1] excess histogram
    int64_t *dl = he + X + 1;                                   // [32] sum_t dlocs_t[d]
    int32_t *parts = (int32_t *)(dl + 32);                      // [L]
    uint32_t *tab = (uint32_t *)(parts + L);                    // [(nck + 1) / 2] cells, two per word
    int8_t *cur = (int8_t *)(tab + (nck + 1) / 2);              // [npad]
    auto cell = [&](int i) -> int32_t { return (int32_t)((tab[i >> 1] >> (16 * (i & 1))) & 0xffffu); };
    // +-1 on a cell: adds modulo 2^32 commute, so a half word that is below zero between two
    // adds of a chunk is exact again once all of them are in
    auto cell_add = [&](int i, int32_t d) { atomicAdd(&tab[i >> 1], (uint32_t)d << (16 * (i & 1))); };

    {
        uint32_t *z = (uint32_t *)smem;
        const int nz = (int)(((unsigned char *)cur - smem) / 4);
        for (int i = lane; i < nz; i += 64) z[i] = 0;
    }
    __syncthreads();
    // the window-start assignment into cur, and its table by LDS adds
    const int8_t *a = w.a0 + (size_t)ch * w.npad;
    for (int u = lane; u < n; u += 64) {
        int d = (int)a[u] & 31;
        d = d < k ? d : k - 1;
        cur[u] = (int8_t)d;
        cell_add(p.node_loc[u] * k + d, 1);
    }
    __syncthreads();
    const int64_t t0 = w.t0[cl], t1 = w.t_end[cl];
    const int64_t Y = t1 - t0;  // the window's yields
    // parts, the aggregates and the integrals' window-start terms
    int64_t s0 = 0, x0 = 0, q0 = 0;
    for (int c = lane; c < L; c += 64) {
        int32_t pc = 0;
        for (int d = 0; d < k; ++d) {
            const int64_t x = cell(c * k + d);
            if (x) {
                ++pc;
                q0 += x * x;
                lds_add64(&dl[d], Y);
            }
        }
        parts[c] = pc;
        acc_parts[c] = (int64_t)pc * Y;
        acc_split[c] = pc >= 2 ? Y : 0;
        s0 += pc >= 2 ? 1 : 0;
        x0 += pc - 1;
    }
    dev::wave_sum64_all(s0, x0, q0);
    int32_t splits = (int32_t)s0, excess = (int32_t)x0;  // wave-uniform: after the last event replayed
    int64_t sq_acc = 0;                                   // this lane's share of sum_t (sq_t - sq_t0)

    const replay::Log log(w, cl);
    const int64_t ne = log.ne;
    replay::Prefetch<1> nx(log, lane);  // this lane's event of the next chunk, loaded one chunk ahead
    // the yields before the first event
    if (lane == 0) {
        const int64_t head = (ne > 0 ? replay::ev_t(nx.e[0]) : t1) - t0;
        hs[min(max(splits, 0), L)] += head;
        he[min(max(excess, 0), X)] += head;
    }
    __syncthreads();

    for (int64_t base = 0; base < ne; base += 64) {
        const int64_t t = replay::ev_t(nx.e[0]);
        int v, tg;
        const bool valid = replay::decode(nx.e[0], base + lane < ne, n, k, v, tg);
        nx.advance(log, base, lane);
        const int cnt = log.count(base);
        // the first yield after this chunk's last run
        const int64_t t_next = base + 64 < ne ? rl64(replay::ev_t(nx.e[0]), 0) : t1;
        const int32_t loc = valid ? p.node_loc[v] : 0;
        // 1. the node's district before the event: the target of the latest earlier lane with the
        // same node, else cur[v]
        const uint64_t below = dev::bits_below(lane);
        const uint64_t same_v = match_mask((uint32_t)v, (uint32_t)v, bits_n, __ballot(valid));
        const uint64_t prev_v = same_v & below;
        const int t_prev = __shfl(tg, prev_v ? 63 - __builtin_clzll(prev_v) : lane);
        const int old = !valid ? 0 : (prev_v ? t_prev : (int)cur[v]);
        const bool last = (same_v & ~dev::bits_below(lane + 1)) == 0;
        const bool eff = valid && old != tg;
        // 2. the event's two cells, (loc, old) and (loc, tg), just before it: the chunk-start table
        // plus the net of the earlier moves of the chunk on the same cell -- the earlier lanes of
        // the same locality whose old or target district is this lane's
        const uint64_t earlier = match_mask((uint32_t)loc, (uint32_t)loc, bits_l, __ballot(eff)) & below;
        const uint64_t old_old = match_mask((uint32_t)old, (uint32_t)old, bits_k, earlier);
        const uint64_t tg_old = match_mask((uint32_t)old, (uint32_t)tg, bits_k, earlier);
        const uint64_t old_tg = match_mask((uint32_t)tg, (uint32_t)old, bits_k, earlier);
        const uint64_t tg_tg = match_mask((uint32_t)tg, (uint32_t)tg, bits_k, earlier);
        const int32_t ca = loc * k + old, cb = loc * k + tg;
        int32_t dpa = 0, dpb = 0, unused, xa = 1, xb = 0;
        int64_t dqa = 0, dqb = 0;
        if (eff) {
            xa = cell(ca) + __popcll(tg_old) - __popcll(old_old);
            xb = cell(cb) + __popcll(tg_tg) - __popcll(old_tg);
            split_rule(xa, -1, 0, dpa, unused, dqa);
            split_rule(xb, +1, 0, dpb, unused, dqb);
        }
        const int32_t dp = dpa + dpb;
        // 3. parts(c) before the event: the chunk-start value plus the earlier changes of the
        // chunk on c; with it the split bit's change over both moves
        const uint64_t up = __ballot(dp > 0), down = __ballot(dp < 0);
        int32_t ds = 0;
        if (eff) {
            const int32_t pc = parts[loc] + __popcll(earlier & up) - __popcll(earlier & down);
            int32_t d1, d2, s1, s2;
            int64_t q;
            split_rule(xa, -1, pc, d1, s1, q);
            split_rule(xb, +1, pc + d1, d2, s2, q);
            ds = s1 + s2;
        }
        // 4. splits and excess after every event of the chunk (one scan: both fit 16 bits)
        const int32_t sc = dev::wave_scan_incl(ds * 65536 + dp);
        const int32_t dx_i = (int32_t)(int16_t)(sc & 0xffff);
        const int32_t ds_i = (sc - dx_i) / 65536;
        const int32_t s_i = splits + ds_i, x_i = excess + dx_i;
        // (yields relative to the window start fit 32 bits: the window has fewer than 2^30)
        const int32_t tr = (int32_t)(t - t0);
        int32_t tr_after = __shfl_down(tr, 1);
        if (lane == cnt - 1) tr_after = (int32_t)(t_next - t0);
        if (lane < cnt) {
            const int64_t run = (int64_t)tr_after - tr;
            lds_add64(&hs[min(max(s_i, 0), L)], run);
            lds_add64(&he[min(max(x_i, 0), X)], run);
        }
        // 5., 6. the integrals: delta * (the yields from t to the window's end)
        const int64_t wr = t1 - t;
        sq_acc += (dqa + dqb) * wr;
        if (dp != 0) lds_add64(&acc_parts[loc], dp * wr);
        if (ds != 0) lds_add64(&acc_split[loc], ds * wr);
        if (dpa != 0) lds_add64(&dl[old], -wr);
        if (dpb != 0) lds_add64(&dl[tg], wr);
        splits += rl32(ds_i, 63);
        excess += rl32(dx_i, 63);
        __syncthreads();  // every lane has read cur, the table and parts
        // 7. the chunk into the table, parts and cur
        if (eff) {
            cell_add(ca, -1);
            cell_add(cb, 1);
            if (dp != 0) atomicAdd(&parts[loc], dp);
        }
        if (valid && last) cur[v] = (int8_t)tg;
        __syncthreads();
    }

    const int64_t sq_sum = q0 * Y + dev::wave_sum64(sq_acc);
    for (int i = lane; i < nck; i += 64) p.cells_now[(size_t)cl * nck + i] = cell(i);
    for (int c = lane; c < L; c += 64) {
        p.split_sum[(size_t)cl * L + c] = acc_split[c];
        p.parts_sum[(size_t)cl * L + c] = acc_parts[c];
    }
    if (lane < k) p.dlocs_sum[(size_t)cl * k + lane] = dl[lane];
    if (lane == 0) p.sq_sum[cl] = sq_sum;
    for (int i = lane; i <= L; i += 64) p.splits_hist[(size_t)cl * (L + 1) + i] = hs[i];
    for (int i = lane; i <= X; i += 64) p.excess_hist[(size_t)cl * (X + 1) + i] = he[i];
}

}  // namespace

int launch_splits(const SplitsParams &p, void *stream) {
    const LogWindow &w = p.log;
    if (w.nc <= 0) return (int)hipSuccess;
    if (w.k < 1 || w.k > 32 || w.n > w.npad || p.n_loc < 1 || p.n_loc > w.n || p.x_top < 0 ||
        p.x_top > kSplitMaxExcess || !p.node_loc || !splits_fit_lds(w.npad, w.k, p.n_loc, p.x_top))
        return (int)hipErrorInvalidValue;
    const size_t lds = splits_lds_bytes(w.npad, w.k, p.n_loc, p.x_top);
    hipLaunchKernelGGL(splits_kernel, dim3((unsigned)w.nc), dim3(64), lds, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

}  // namespace fc
