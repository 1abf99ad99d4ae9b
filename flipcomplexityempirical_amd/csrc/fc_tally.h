// The k = 2 tally log (DESIGN.md §4 "Batch (k = 2)"): what one entry means and how it is applied.
// flip2_kernel (fc_flip2.hip) writes the entries, or applies them itself when a chain's log is
// full; tally_reduce_kernel (fc_tally.hip) applies a launch's logs after it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fc_internal.h"

namespace fc {

// The per-yield tallies of the reference's loop body (grid_chain_sec11.py:367-400) for one
// accepted state and its run (kind 0: a flushed queue entry -- yield t of the flip, `run` yields,
// node u | old-district ring bits << 16, |cut| | target << 31, |B|) or for the yields a batch's
// start state adds right after a flush (kind 1: yields steps0 + 1 .. steps0 + r0 of the state
// the last flip created; node last_flip | its district << 16, 0xffff: none).  Every update
// commutes (sums and maxima), so where and in which order they are applied leaves the results
// bit-identical: inside the flip kernel (a full log) or by tally_reduce after the launch.
template <int RMAX>
__device__ __forceinline__ void tally_apply(const KParams &p, int c, int64_t t, int run, uint32_t qv, uint32_t qc,
                                            uint32_t nbk, int64_t lab0, int64_t lab1) {
    const int n = p.n;
    const int cq = (int)(qc & 0x7fffffffu), nbq = (int)(nbk & 0x7fffffffu);
    if (p.diag & FC_DIAG_HIST) {
        atomicAdd((unsigned long long *)&p.cut_hist[(size_t)c * (p.n_edges + 1) + cq], (unsigned long long)run);
        atomicAdd((unsigned long long *)&p.nb_hist[(size_t)c * (n + 1) + nbq], (unsigned long long)run);
    }
    const int u = (int)(qv & 0xffffu);
    if (nbk >> 31) {  // kind 1: the start state's further yields (the per-batch form in flip2_kernel)
        if ((p.diag & FC_DIAG_FLIPS) && u != 0xffff) {
            const size_t o = (size_t)c * n + u;
            atomicMax((unsigned long long *)(p.last_flipped + o), (unsigned long long)(t + run));
            atomicAdd((unsigned long long *)(p.part_sum + o), (unsigned long long)(((qv >> 16) & 1u ? lab0 - lab1 : lab1 - lab0) * run));
            atomicAdd((unsigned long long *)(p.num_flips + o), (unsigned long long)run);
        }
        return;
    }
    const int tg = (int)(qc >> 31);
    const int64_t lab_t = tg ? lab1 : lab0, lab_o = tg ? lab0 : lab1;
    const uint32_t up = qv >> 16;  // neighbours in the old district: their edges turn cut
    if (p.diag & FC_DIAG_FLIPS) {  // the run's share (fc_run_read_flips closes the last run)
        const size_t o = (size_t)c * n + u;
        const int64_t t_last = t + run - 1;
        atomicMax((unsigned long long *)(p.last_flipped + o), (unsigned long long)t_last);
        atomicAdd((unsigned long long *)(p.part_sum + o), (unsigned long long)((lab_o - lab_t) * t_last));
        atomicAdd((unsigned long long *)(p.num_flips + o), (unsigned long long)run);
    }
    if (p.diag & FC_DIAG_FLIPS_EXACT) {
        const size_t o = (size_t)c * n + u;
        atomicAdd((unsigned long long *)(p.flip_count + o), 1ull);
        atomicAdd((unsigned long long *)(p.occ_acc + o), (unsigned long long)(-(lab_t - lab_o) * t));
        atomicMax((unsigned long long *)(p.last_accept + o), (unsigned long long)t);
    }
    if (p.diag & FC_DIAG_EDGES) {
        const int4 *er = (const int4 *)(p.ring_eid + (size_t)u * RMAX);
        int eid[RMAX];
#pragma unroll
        for (int j = 0; j < RMAX / 4; ++j) {
            const int4 e4 = er[j];
            eid[4 * j] = e4.x;
            eid[4 * j + 1] = e4.y;
            eid[4 * j + 2] = e4.z;
            eid[4 * j + 3] = e4.w;
        }
        int64_t *ea = p.edge_acc + (size_t)c * p.n_edges;
#pragma unroll
        for (int i = 0; i < RMAX; ++i)
            if (eid[i] >= 0) atomicAdd((unsigned long long *)(ea + eid[i]), (unsigned long long)(((up >> i) & 1u) ? -t : t));
    }
}

// One tally-log entry in 16 B (one coalesced store per lane): dt = t - t0 (< 2^24: launches
// with the log are at most 2^23 steps), run (< 2^24), |B| (< 2^16), node | ring bits << 16,
// |cut| (< 2^24), target, kind (0: a queue entry, 1: a start state's further yields).
__device__ __forceinline__ uint4 tally_pack(int64_t dt, int run, uint32_t qv, uint32_t qc, uint32_t nbk) {
    const uint32_t r = (uint32_t)run, kind = nbk >> 31;
    return make_uint4(((uint32_t)dt & 0xffffffu) | (r << 24), (r >> 8) | ((nbk & 0xffffu) << 16), qv,
                      (qc & 0xffffffu) | ((qc >> 31) << 24) | (kind << 25));
}

}  // namespace fc
