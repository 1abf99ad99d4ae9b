// Short bursts: replay of the FC_DIAG_SERIES event logs that scores every yield
// of the series window by a metric (fc_burst.h), keeps the latest yield with the best score, and
// rebuilds the plan held there -- into an output row and, for a rewind, into the run itself.
//
// One wavefront per chain, one 64-thread workgroup each, no global atomics, every output row has
// one owner (the mapping of fc_plans.hip).  The chain's image is in LDS: the current assignment,
// copied verbatim (padding included) from the chain's window-start row, and the start tallies.
//
// Phase 1, the score walk.  Lanes are districts (k <= 32): lane d holds a_d, b_d of the metric's
// two columns, its COUNT bit and its g in registers; their sums over the districts are kept
// wave-uniform and follow an event from the two lanes it changes (fc_votes.hip's scheme), so no
// event costs a wave reduction.  Events are read 64 at a time, one per lane, the next chunk loaded
// before the current one is used.  The chunk phase resolves each event's old district: cur[v],
// unless a lower lane of the chunk moves the same node (match_mask), then that lane's target; the
// highest lane of a node writes cur[v].  Events that share t are one yield (a ReCom burst): the
// score is taken after the last event of a t-group, which a lane knows from the t of the lane after
// it -- lane 0 of the chunk ahead for the chunk's last lane, so a group may straddle chunks.  A
// chunk in which many groups end (a flip log: every event is one) is then walked event by event, by
// readlane; one in which few end (ReCom bursts of hundreds of events) yield by yield, the lanes of a
// yield adding their node's columns to 32 x 2 LDS sums at once, from which lane d takes district
// d's change and the wave the new sums.  A state in force is held until the yield before the
// next group's t, or until the window's end: when a group ends while the state before it is the
// best, best_t first moves to t - 1 (the yields of rejected steps), and after the walk to steps.
//
// Phase 2, the best plan.  The window-start row again, then events [0, e_best) -- the events with
// t <= best_t -- chunk by chunk, the highest lane of a node writing cur[v] (fc_plans.hip's apply).
//
// A rewind writes, per chain: the d_assign row and the window-start row := the LDS row; and
// ChainScalars cut, nb, ser_cut0, ser_nb0 := those of best_t, ev_len := 0, ser_t0 := steps.  The
// window-start row is read only by its own workgroup, before the barrier that precedes the write.
#include <hip/hip_runtime.h>

#include "fc_burst.h"
#include "fc_replay_dev.h"

namespace fc {
namespace {

using dev::rl32;
using dev::rl64;
using replay::bits_for;
using replay::match_mask;

// A chunk with more t-groups ending in it than this is walked event by event, one with fewer yield
// by yield: a yield costs two barriers and a wave sum, an event a dozen readlanes
constexpr int kSegmentEnds = 16;

__global__ __launch_bounds__(64) void burst_kernel(const BurstParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = (int)threadIdx.x;
    const int32_t cl = (int32_t)blockIdx.x;
    const LogWindow &w = p.log;
    const int32_t ch = w.c0 + cl;
    const int32_t n = w.n, k = w.k;
    const int nvec = w.npad / 16;  // 16-byte vectors of a row
    const int bits_n = bits_for(n);
    const int32_t kind = p.kind, maximize = p.maximize;
    const bool votes = kind != FC_BURST_CUT;
    const int64_t num = p.num, den = p.den;
    int8_t *cur = (int8_t *)smem;                        // [npad]
    uint4 *cur4 = (uint4 *)smem;
    int32_t *tl = (int32_t *)(smem + (size_t)w.npad);    // [32][2] start tallies
    const uint4 *a4 = (const uint4 *)(w.a0 + (size_t)ch * w.npad);

    for (int i = lane; i < nvec; i += 64) cur4[i] = a4[i];
    tl[lane] = 0;
    __syncthreads();
    // the start tallies by LDS adds, one pass over the nodes
    if (votes)
        for (int u = lane; u < n; u += 64) {
            const int d = (int)cur[u] & 31;
            const int32_t xa = p.cols[(size_t)u * p.ncp + p.col_a], xb = p.cols[(size_t)u * p.ncp + p.col_b];
            if (xa) atomicAdd(&tl[2 * d], xa);
            if (xb) atomicAdd(&tl[2 * d + 1], xb);
        }
    __syncthreads();
    // lane d: district d's tallies, its COUNT bit and g; cnt and gsum: their sums, wave-uniform
    int64_t ta = 0, tb = 0, g = 0;
    int32_t bit = 0;
    int64_t cnt = 0, gsum = 0;
    // lane d takes the sums tl holds for district d (the start tallies, then a yield's changes)
    // and clears them, and every lane takes the new cnt and gsum
    auto take_tallies = [&]() {
        if (lane < 32) {
            ta += tl[2 * lane];
            tb += tl[2 * lane + 1];
            tl[2 * lane] = 0;
            tl[2 * lane + 1] = 0;
        }
        bit = 0;
        g = 0;
        if (lane < k) burst_district(ta, tb, num, den, bit, g);
        cnt = __popcll(__ballot(bit != 0));
        gsum = rl64(dev::wave_sum64(g), 0);
    };
    if (votes) take_tallies();

    const int64_t t0 = w.t0[cl], t_last = w.t_end[cl] - 1;
    int32_t cut_now = (int32_t)p.cut0[cl], nb_now = (int32_t)p.nb0[cl];  // wave-uniform
    const int64_t start_score = burst_score(kind, cnt, gsum, cut_now);
    int64_t score_now = start_score, best_score = start_score, best_t = t0, e_best = 0;
    int32_t best_cut = cut_now, best_nb = nb_now;
    bool held_best = true;  // the state in force has the best score

    const replay::Log log(w, cl);
    const int64_t ne = log.ne;
    replay::Prefetch<1> nx(log, lane);  // this lane's event of the next chunk, loaded one chunk ahead

    for (int64_t base = 0; base < ne; base += 64) {
        const replay::Event e = nx.e[0];
        const int64_t t = replay::ev_t(e);
        const int ecut = replay::ev_cut(e), enb = replay::ev_nb(e);
        const bool in = base + lane < ne;
        int v, tg;
        const bool valid = replay::decode(e, in, n, k, v, tg);
        const uint64_t ok = __ballot(valid);
        nx.advance(log, base, lane);
        const int cnt_ev = log.count(base);
        // the last event of its t-group: the lane after it (lane 0 of the chunk ahead) has another t
        int64_t t_after = __shfl_down((long long)t, 1);
        const int64_t t_ahead = base + 64 < ne ? rl64(replay::ev_t(nx.e[0]), 0) : INT64_MAX;
        if (lane == cnt_ev - 1) t_after = t_ahead;
        const uint64_t ends = __ballot(in && t_after != t);
        // the node's columns, and its district before the event
        int32_t xa = 0, xb = 0;
        if (votes && valid) {
            xa = p.cols[(size_t)v * p.ncp + p.col_a];
            xb = p.cols[(size_t)v * p.ncp + p.col_b];
        }
        int old = valid ? (int)cur[v] & 31 : 0;
        const uint64_t same = match_mask((uint32_t)v, (uint32_t)v, bits_n, ok);
        const uint64_t lower = same & ((1ull << lane) - 1ull);
        const int src = lower ? 63 - __builtin_clzll(lower) : lane;
        const int tg_src = __shfl(tg, src);
        if (valid && lower) old = tg_src;
        const bool last = valid && ((same >> lane) >> 1) == 0;
        __syncthreads();  // every lane has read cur before the chunk's last targets go in
        if (last) cur[v] = (int8_t)tg;
        __syncthreads();

        // yield te = the t of the chunk's event i is complete: its score against the best
        auto yield_done = [&](int i) {
            const int64_t te = rl64(t, i);
            if (held_best) best_t = te - 1;  // the state before it was held until then
            cut_now = rl32(ecut, i);
            nb_now = rl32(enb, i);
            score_now = burst_score(kind, cnt, gsum, cut_now);
            held_best = burst_takes(score_now, best_score, maximize);
            if (held_best) {
                best_score = score_now;
                best_t = te;
                e_best = base + i + 1;
                best_cut = cut_now;
                best_nb = nb_now;
            }
        };
        if (votes && __popcll(ends) > kSegmentEnds) {
            // many short yields (a flip log: one event each): event by event
            for (int i = 0; i < cnt_ev; ++i) {
                const int od = rl32(old, i), td = rl32(tg, i);
                if (od != td) {  // (an event that is no move has old = target = 0)
                    const int32_t ea = rl32(xa, i), eb = rl32(xb, i);
                    int32_t dbit = 0;
                    int64_t dg = 0;
                    if (lane == od || lane == td) {
                        const int32_t sgn = lane == td ? 1 : -1;
                        ta += sgn * ea;
                        tb += sgn * eb;
                        int32_t nbit;
                        int64_t ng;
                        burst_district(ta, tb, num, den, nbit, ng);
                        dbit = nbit - bit;
                        dg = ng - g;
                        bit = nbit;
                        g = ng;
                    }
                    cnt += rl32(dbit, od) + rl32(dbit, td);
                    gsum += rl64(dg, od) + rl64(dg, td);
                }
                if ((ends >> i) & 1ull) yield_done(i);
            }
        } else {
            // few long yields (ReCom bursts): yield by yield, the lanes of one adding their node's
            // columns to tl at once (int32 adds in any order: exact modulo 2^32, and the sums are
            // tallies' differences).  The lanes after the chunk's last end belong to a yield that
            // ends in a later chunk: their changes go in now.  (FC_BURST_CUT: the ends alone.)
            const bool moved = votes && old != tg;
            int lo = 0;
            for (uint64_t m = ends;; m &= m - 1) {
                const int i = m ? __builtin_ctzll(m) : 63;  // lanes lo .. i
                const bool mine = moved && lane >= lo && lane <= i;
                if (__ballot(mine)) {
                    if (mine) {
                        if (xa) {
                            atomicAdd(&tl[2 * old], -xa);
                            atomicAdd(&tl[2 * tg], xa);
                        }
                        if (xb) {
                            atomicAdd(&tl[2 * old + 1], -xb);
                            atomicAdd(&tl[2 * tg + 1], xb);
                        }
                    }
                    __syncthreads();
                    take_tallies();
                    __syncthreads();
                }
                if (!m) break;
                yield_done(i);
                lo = i + 1;
            }
        }
    }
    if (held_best) best_t = t_last;

    if (lane == 0) {
        if (p.best_score) p.best_score[cl] = best_score;
        if (p.best_t) p.best_t[cl] = best_t;
        if (p.start_score) p.start_score[cl] = start_score;
        if (p.end_score) p.end_score[cl] = score_now;
        if (p.best_cut) p.best_cut[cl] = best_cut;
        if (p.best_nb) p.best_nb[cl] = best_nb;
    }
    if (!p.best_plan && !p.rewind) return;

    // ---- phase 2: the plan at best_t ---------------------------------------------------------
    __syncthreads();
    for (int i = lane; i < nvec; i += 64) cur4[i] = a4[i];
    __syncthreads();
    for (int64_t base = 0; base < e_best; base += 64) {
        int v, tg;
        const bool in = base + lane < e_best;
        replay::Event e = {0ull, 0ull};
        if (in) e = log.ev[base + lane];
        const bool valid = replay::decode(e, in, n, k, v, tg);
        const uint64_t ok = __ballot(valid);
        const uint64_t same = match_mask((uint32_t)v, (uint32_t)v, bits_n, ok);
        if (valid && ((same >> lane) >> 1) == 0) cur[v] = (int8_t)tg;
        __syncthreads();
    }
    if (p.best_plan) {
        uint4 *row = (uint4 *)(p.best_plan + (size_t)cl * w.npad);
        for (int i = lane; i < nvec; i += 64) row[i] = cur4[i];
    }
    if (p.rewind) {
        uint4 *ga = (uint4 *)(p.assign + (size_t)ch * w.npad);
        uint4 *g0 = (uint4 *)(p.ser_a0 + (size_t)ch * w.npad);
        for (int i = lane; i < nvec; i += 64) {
            const uint4 c = cur4[i];
            ga[i] = c;
            g0[i] = c;
        }
        if (lane == 0) {
            ChainScalars *scp = p.sc + ch;
            scp->cut = best_cut;
            scp->nb = best_nb;
            scp->ev_len = 0;
            scp->ser_t0 = t_last;
            scp->ser_cut0 = best_cut;
            scp->ser_nb0 = best_nb;
        }
    }
}

}  // namespace

int launch_burst(const BurstParams &p, void *stream) {
    const LogWindow &w = p.log;
    if (w.nc <= 0) return (int)hipSuccess;
    const bool votes = burst_votes_kind(p.kind);
    if (w.k < 1 || w.k > 32 || w.n < 1 || w.n > w.npad || (w.npad & 15) || !burst_fits_lds(w.npad) || !p.cut0 ||
        !p.nb0 || (!votes && p.kind != FC_BURST_CUT) ||
        (votes && (!p.cols || p.col_a < 0 || p.col_a >= p.ncp || p.col_b < 0 || p.col_b >= p.ncp)) ||
        (p.rewind && (!p.assign || !p.ser_a0 || !p.sc)))
        return (int)hipErrorInvalidValue;
    launch_lds(burst_kernel, dim3((unsigned)w.nc), dim3(64), burst_lds_bytes(w.npad), (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

}  // namespace fc
