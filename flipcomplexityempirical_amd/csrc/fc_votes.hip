// Election series: replay of the FC_DIAG_SERIES flip logs against node vote
// columns -- district tallies, their time integrals, seats and efficiency-gap histograms over
// the yields of the series window, in exact integers.
//
// One wavefront per chain, one 64-thread workgroup each: no cross-workgroup synchronisation, no
// global atomics, every output row has one owner.  Lanes are districts (k <= 32): lane d holds
// S[d][.] (int32: column totals are below 2^31), its time integrals and, per election, its win
// bit and g value, all in registers (the column count is a template parameter so that the
// per-lane arrays are compile-time indexed).  Events are read 64 at a time, one per lane, the
// next chunk loaded before the current one is used; the chunk phase fetches each event's column
// row and resolves its node's old district (the target of the latest earlier event on the same
// node in the chunk, else cur[v]); the sequential phase then walks the chunk by readlane.  Only
// the lanes `old` and `target` change per event, and seats / gap follow from those two lanes' old
// and new values, so no event costs a wave reduction.  Every integral is lazy: a quantity adds
// value * (t - t_since) when it changes, and once more at the window's end.
#include <hip/hip_runtime.h>

#include "fc_replay_dev.h"
#include "fc_votes.h"

namespace fc {
namespace {

using dev::rl32;
using dev::rl64;

constexpr int kEdgeRegs = kVoteMaxEdges / 64;

// searchsorted(edges, gap, side="right"): the edges at or below gap, lane l holding edges
// l, 64 + l, ... (INT64_MAX past the end)
__device__ __forceinline__ int32_t gap_bin(const int64_t (&eq)[kEdgeRegs], int32_t n_edges, int64_t gap) {
    int32_t cnt = 0;
#pragma unroll
    for (int q = 0; q < kEdgeRegs; ++q)
        if (64 * q < n_edges) cnt += __popcll(__ballot(eq[q] <= gap));
    return cnt;
}

// NC: columns per row of p.cols; NEL: elections (compile time, so that a run with one election
// carries no code for four); GC: the current assignment in p.cur instead of LDS.
template <int NC, int NEL, bool GC>
__global__ __launch_bounds__(64) void votes_kernel(const VotesParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NE = NEL > 0 ? NEL : 1;  // array sizes
    constexpr int32_t n_el = NEL;
    constexpr int HE = kVoteMaxElections;  // histogram rows laid out in LDS (votes_hist_bytes)
    const int lane = (int)threadIdx.x;
    const int32_t cl = (int32_t)blockIdx.x;
    const LogWindow &w = p.log;
    const int32_t c = w.c0 + cl;
    const int32_t k = w.k, n = w.n, n_edges = p.n_edges;
    const int32_t nb = n_edges + 1;
    int64_t *hs = (int64_t *)smem;                  // [HE][k + 1] seats histograms
    int64_t *hg = hs + HE * (k + 1);                // [HE][nb] gap histograms
    int32_t *tl = (int32_t *)(hg + HE * nb);        // [32][kVoteMaxCols] initial tallies
    int8_t *lcur = (int8_t *)(tl + 32 * kVoteMaxCols);
    int8_t *gcur = p.cur + (size_t)cl * w.npad;
    auto cur_get = [&](int u) -> int { return GC ? (int)gcur[u] : (int)lcur[u]; };
    auto cur_set = [&](int u, int d) {
        if (GC) gcur[u] = (int8_t)d; else lcur[u] = (int8_t)d;
    };

    for (int i = lane; i < HE * (k + 1 + nb); i += 64) hs[i] = 0;  // hs and hg are contiguous
    for (int i = lane; i < 32 * kVoteMaxCols; i += 64) tl[i] = 0;
    __syncthreads();
    // the window-start assignment into cur, and its tallies by LDS adds
    const int8_t *a = w.a0 + (size_t)c * w.npad;
    for (int u = lane; u < n; u += 64) {
        const int d = (int)a[u] & 31;
        cur_set(u, d);
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int32_t x = p.cols[(size_t)u * NC + j];
            if (x) atomicAdd(&tl[d * NC + j], x);
        }
    }
    __syncthreads();

    const int64_t t0 = w.t0[cl];
    int32_t S[NC];
    int64_t ts[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        S[j] = lane < k ? tl[lane * NC + j] : 0;
        ts[j] = 0;
    }
    int64_t eq[kEdgeRegs];
#pragma unroll
    for (int q = 0; q < kEdgeRegs; ++q) eq[q] = 64 * q + lane < n_edges ? p.edges[64 * q + lane] : INT64_MAX;
    // lane d, per election: district d's tallies of the election's two columns (kept beside S:
    // S[col_a[e]] would be a runtime register index), its win bit, g and the time integral of
    // the win bit
    int32_t ea[NE], eb[NE], win[NE];
    int64_t g[NE], ws[NE];
    int64_t t_last = t0;
    // lane e < n_el also owns election e: seats, gap, its bin, the yields since which each has
    // held its value, and the gap integral
    int32_t seats = 0, bin = 0;
    int64_t gap = 0, gsum = 0, seats_t = t0, gap_t = t0, bin_t = t0;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        ea[e] = 0;
        eb[e] = 0;
        win[e] = 0;
        g[e] = 0;
        ws[e] = 0;
        if (e < n_el) {
            if (lane < k) {
                ea[e] = tl[lane * NC + p.col_a[e]];
                eb[e] = tl[lane * NC + p.col_b[e]];
            }
            election_rule(ea[e], eb[e], win[e], g[e]);
            const int32_t s0 = __popcll(__ballot(win[e] != 0));
            const int64_t g0 = rl64(dev::wave_sum64(g[e]), 0);  // wave-uniform
            const int32_t b0 = gap_bin(eq, n_edges, g0);
            if (lane == e) {
                seats = s0;
                gap = g0;
                bin = b0;
            }
        }
    }

    const replay::Log log(w, cl);
    const int64_t ne = log.ne;
    // this lane's event of the next chunk, loaded one chunk ahead.  (replay::Prefetch<1> and
    // replay::decode, spelt here: behind the calls the compiler no longer carries `valid` into the
    // loads below, and most instances' code, a dozen's registers, move)
    replay::Event nx = {0ull, 0ull};
    if (lane < ne) nx = log.ev[lane];
    for (int64_t base = 0; base < ne; base += 64) {
        const int64_t t = replay::ev_t(nx);
        int tg = replay::ev_target(nx);
        int v = replay::ev_node(nx);
        const bool valid = base + lane < ne && v < n && tg < k;
        if (!valid) { v = -1; tg = 0; }
        if (base + 64 + lane < ne) nx = log.ev[base + 64 + lane];
        // the node's column row, and per election its two columns (a memory index, not a register one)
        int32_t cr[NC], cra[NE], crb[NE];
#pragma unroll
        for (int j = 0; j < NC; ++j) cr[j] = valid ? p.cols[(size_t)v * NC + j] : 0;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            cra[e] = valid && e < n_el ? p.cols[(size_t)v * NC + p.col_a[e]] : 0;
            crb[e] = valid && e < n_el ? p.cols[(size_t)v * NC + p.col_b[e]] : 0;
        }
        int old = valid ? cur_get(v) : 0;
        bool last = true;
        const int cnt = log.count(base);
        for (int j = 0; j < cnt; ++j) {
            const int vj = rl32(v, j), tj = rl32(tg, j);
            if (vj == v) {
                if (j < lane) old = tj;
                if (j > lane) last = false;
            }
        }
        __syncthreads();  // every lane has read cur before the chunk's last targets go in
        if (valid && last) cur_set(v, tg);
        __syncthreads();

        for (int i = 0; i < cnt; ++i) {
            const int64_t te = rl64(t, i);
            const int od = rl32(old, i), td = rl32(tg, i);
            int32_t ce[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) ce[j] = rl32(cr[j], i);
            int32_t cea[NE], ceb[NE], dw[NE];
            int64_t dg[NE];
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                cea[e] = e < n_el ? rl32(cra[e], i) : 0;
                ceb[e] = e < n_el ? rl32(crb[e], i) : 0;
                dw[e] = 0;
                dg[e] = 0;
            }
            if (od != td && (lane == od || lane == td)) {
                const int64_t dt = te - t_last;
                t_last = te;
                const int32_t sgn = lane == td ? 1 : -1;
#pragma unroll
                for (int j = 0; j < NC; ++j) {
                    ts[j] += (int64_t)S[j] * dt;
                    S[j] += sgn * ce[j];
                }
#pragma unroll
                for (int e = 0; e < NE; ++e)
                    if (e < n_el) {
                        ws[e] += win[e] ? dt : 0;
                        ea[e] += sgn * cea[e];
                        eb[e] += sgn * ceb[e];
                        int32_t nw;
                        int64_t ng;
                        election_rule(ea[e], eb[e], nw, ng);
                        dw[e] = nw - win[e];
                        dg[e] = ng - g[e];
                        win[e] = nw;
                        g[e] = ng;
                    }
            }
            // the two lanes' changes go to the election's lane
            int32_t ds = 0, b2 = bin;
            int64_t dgp = 0;
#pragma unroll
            for (int e = 0; e < NE; ++e)
                if (e < n_el) {
                    const int32_t x = rl32(dw[e], od) + rl32(dw[e], td);
                    const int64_t y = rl64(dg[e], od) + rl64(dg[e], td);
                    int32_t b = 0;
                    if (y != 0 && n_edges > 0) b = gap_bin(eq, n_edges, rl64(gap, e) + y);
                    if (lane == e) {
                        ds = x;
                        dgp = y;
                        if (y != 0 && n_edges > 0) b2 = b;
                    }
                }
            if (ds != 0) {
                hs[lane * (k + 1) + seats] += te - seats_t;
                seats_t = te;
                seats += ds;
            }
            if (dgp != 0) {
                gsum += gap * (te - gap_t);
                gap_t = te;
                gap += dgp;
                if (b2 != bin) {
                    hg[lane * nb + bin] += te - bin_t;
                    bin_t = te;
                    bin = b2;
                }
            }
        }
    }

    // the window's end: every integral takes its last segment
    const int64_t t1 = w.t_end[cl];
    {
        const int64_t dt = t1 - t_last;
#pragma unroll
        for (int j = 0; j < NC; ++j) ts[j] += (int64_t)S[j] * dt;
#pragma unroll
        for (int e = 0; e < NE; ++e)
            if (e < n_el) ws[e] += win[e] ? dt : 0;
        if (lane < n_el) {
            gsum += gap * (t1 - gap_t);
            hs[lane * (k + 1) + seats] += t1 - seats_t;
            if (n_edges > 0) hg[lane * nb + bin] += t1 - bin_t;
        }
    }
    __syncthreads();
    const int32_t n_cols = p.n_cols;
    if (lane < k) {
        const size_t o = ((size_t)cl * k + lane) * n_cols;
#pragma unroll
        for (int j = 0; j < NC; ++j)
            if (j < n_cols) {
                p.tally_now[o + j] = S[j];
                p.tally_sum[o + j] = ts[j];
            }
    }
#pragma unroll
    for (int e = 0; e < NE; ++e)
        if (e < n_el && lane < k) p.wins_sum[((size_t)cl * n_el + e) * k + lane] = ws[e];
    if (lane < n_el) p.gap_sum[(size_t)cl * n_el + lane] = gsum;
    // the histogram rows of elections 0 .. n_el - 1 are contiguous in LDS and in the output
    for (int i = lane; i < n_el * (k + 1); i += 64) p.seats_hist[(size_t)cl * n_el * (k + 1) + i] = hs[i];
    if (n_edges > 0)
        for (int i = lane; i < n_el * nb; i += 64) p.gap_hist[(size_t)cl * n_el * nb + i] = hg[i];
}

template <int NC, int NEL>
int launch_nc_ne(const VotesParams &p, bool global_cur, hipStream_t stream) {
    const size_t hist = votes_hist_bytes(p.log.k, p.n_edges);
    const dim3 grid((unsigned)p.log.nc), block(64);
    if (global_cur)
        hipLaunchKernelGGL((votes_kernel<NC, NEL, true>), grid, block, hist, stream, p);
    else
        hipLaunchKernelGGL((votes_kernel<NC, NEL, false>), grid, block, hist + (((size_t)p.log.npad + 15) & ~(size_t)15),
                           stream, p);
    return (int)hipGetLastError();
}

template <int NC>
int launch_nc(const VotesParams &p, bool global_cur, hipStream_t stream) {
    static_assert(kVoteMaxElections == 4, "one instance per election count");
    switch (p.n_el) {
    case 0: return launch_nc_ne<NC, 0>(p, global_cur, stream);
    case 1: return launch_nc_ne<NC, 1>(p, global_cur, stream);
    case 2: return launch_nc_ne<NC, 2>(p, global_cur, stream);
    case 3: return launch_nc_ne<NC, 3>(p, global_cur, stream);
    default: return launch_nc_ne<NC, 4>(p, global_cur, stream);
    }
}

}  // namespace

int votes_padded_cols(int32_t n_cols) { return n_cols <= 2 ? 2 : n_cols <= 4 ? 4 : 8; }

int launch_votes(const VotesParams &p, bool global_cur, void *stream) {
    const LogWindow &w = p.log;
    if (w.nc <= 0) return (int)hipSuccess;
    if (w.k < 1 || w.k > 32 || p.n_cols < 1 || p.n_cols > kVoteMaxCols || p.n_el < 0 || p.n_el > kVoteMaxElections ||
        p.n_edges < 0 || p.n_edges > kVoteMaxEdges || (global_cur && !p.cur) ||
        (!global_cur && !votes_cur_in_lds(w.npad, w.k, p.n_edges)))
        return (int)hipErrorInvalidValue;
    switch (votes_padded_cols(p.n_cols)) {
    case 2: return launch_nc<2>(p, global_cur, (hipStream_t)stream);
    case 4: return launch_nc<4>(p, global_cur, (hipStream_t)stream);
    default: return launch_nc<8>(p, global_cur, (hipStream_t)stream);
    }
}

}  // namespace fc
