// Plan samples: replay of the FC_DIAG_SERIES flip logs up to a list of yields --
// the assignment each chain holds at every one of them, with |cut|, |B|, the Hamming distance to
// the window-start plan and the district populations, in exact integers.
//
// One wavefront per chain, one 64-thread workgroup each, no global atomics, every output row has
// one owner (the mapping of fc_splits.hip).  The chain's image is in LDS: the current assignment,
// copied verbatim (padding included) from the chain's window-start row, and 32 district
// populations of the sample being written.
//
// The walk reads the log in chunks of 64 events, one per lane, the next chunk loaded before the
// current one is used, and keeps a wave-uniform sample cursor j.  While times[j] is below the next
// chunk's first t (or the log has ended), the lanes of the chunk not yet applied with t <= times[j]
// are applied, |cut| and |B| are taken from the highest lane with t <= times[j], and sample j is
// written; then the rest of the chunk is applied.  The walk stops at j = n_times.
//
// The one ordering hazard is several events on one node in one apply step (a flip chain flips the
// same boundary node back and forth): of the step's lanes with the same node, the highest writes
// cur[v].  A lane finds those lanes with match_mask (fc_replay_dev.h), one ballot per bit of the
// node id; a step of one lane needs no mask.
#include <hip/hip_runtime.h>

#include "fc_plans.h"
#include "fc_replay_dev.h"

namespace fc {
namespace {

using dev::rl32;
using dev::rl64;
using replay::bits_for;
using replay::match_mask;

// the bytes of x that are not 0
__device__ __forceinline__ int nonzero_bytes(uint32_t x) {
    return __popc((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u);
}

__global__ __launch_bounds__(64) void plans_kernel(const PlansParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = (int)threadIdx.x;
    const int32_t cl = (int32_t)blockIdx.x;
    const LogWindow &w = p.log;
    const int32_t ch = w.c0 + cl;
    const int32_t n = w.n, k = w.k, nT = p.n_times;
    const int nvec = w.npad / 16;  // 16-byte vectors of a row
    const int bits_n = bits_for(n);
    int8_t *cur = (int8_t *)smem;                        // [npad]
    uint4 *cur4 = (uint4 *)smem;
    int64_t *popk = (int64_t *)(smem + (size_t)w.npad);  // [32]
    const uint4 *a4 = (const uint4 *)(w.a0 + (size_t)ch * w.npad);
    for (int i = lane; i < nvec; i += 64) cur4[i] = a4[i];
    __syncthreads();

    // sample j: the row, dist0 and pops in one pass over cur, 16 nodes per lane and step
    auto emit = [&](int32_t j, int32_t cut_now, int32_t nb_now) {
        const size_t s = (size_t)cl * nT + j;
        uint4 *row = p.plans ? (uint4 *)(p.plans + s * (size_t)w.npad) : nullptr;
        const bool by_node = p.pops && k != 2;  // per-node adds into popk; k = 2: two wave sums
        if (by_node) {
            if (lane < 32) popk[lane] = 0;
            __syncthreads();
        }
        int64_t dist = 0, p0 = 0, p1 = 0;
        for (int i = lane; i < nvec; i += 64) {
            const uint4 c = cur4[i];
            if (row) row[i] = c;
            if (p.dist0) {  // (padding bytes are equal by construction)
                const uint4 a = a4[i];
                dist += nonzero_bytes(c.x ^ a.x) + nonzero_bytes(c.y ^ a.y) + nonzero_bytes(c.z ^ a.z) +
                        nonzero_bytes(c.w ^ a.w);
            }
            if (p.pops) {
                const uint32_t cw[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int4 pp = ((const int4 *)p.node_pop)[4 * i + q];
                    const int32_t pv[4] = {pp.x, pp.y, pp.z, pp.w};
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int d = (int)(cw[q] >> (8 * b)) & 31;
                        if (k == 2) {
                            p0 += d ? 0 : pv[b];
                            p1 += d ? pv[b] : 0;
                        } else if (pv[b]) {
                            atomicAdd((unsigned long long *)&popk[d], (unsigned long long)(int64_t)pv[b]);
                        }
                    }
                }
            }
        }
        if (p.dist0) {
            dist = dev::wave_sum64(dist);
            if (lane == 0) p.dist0[s] = dist;
        }
        if (p.pops && k == 2) {
            dev::wave_sum64_all(p0, p1);
            if (lane == 0) {
                p.pops[s * 2] = p0;
                p.pops[s * 2 + 1] = p1;
            }
        }
        if (by_node) {
            __syncthreads();
            if (lane < k) p.pops[s * (size_t)k + lane] = popk[lane];
        }
        if (lane == 0) {
            if (p.cut) p.cut[s] = cut_now;
            if (p.nb) p.nb[s] = nb_now;
        }
        __syncthreads();  // every lane has read cur and popk
    };

    const replay::Log log(w, cl);
    const int64_t ne = log.ne;
    replay::Prefetch<1> nx(log, lane);  // this lane's event of the next chunk, loaded one chunk ahead
    int32_t cut_now = (int32_t)p.cut0[cl], nb_now = (int32_t)p.nb0[cl];  // wave-uniform
    int32_t j = 0;

    for (int64_t base = 0; j < nT; base += 64) {
        const replay::Event e = nx.e[0];
        const int64_t t = replay::ev_t(e);
        const int v = replay::ev_node(e), tg = replay::ev_target(e);
        const int ecut = replay::ev_cut(e), enb = replay::ev_nb(e);
        const bool in = base + lane < ne;
        const uint64_t inm = __ballot(in);
        const uint64_t ok = __ballot(in && v < n && tg < k);  // the lanes that may write cur
        nx.advance(log, base, lane);
        // the next chunk's first t: samples from it on wait for that chunk
        const int64_t t_next = base + 64 < ne ? rl64(replay::ev_t(nx.e[0]), 0) : INT64_MAX;
        // lanes m (wave-uniform, all of them in `ok`) into cur: of the lanes with one node, the highest
        auto apply = [&](uint64_t m) {
            if (!m) return;
            const bool mine = (m >> lane) & 1ull;
            if (__popcll(m) == 1) {
                if (mine) cur[v] = (int8_t)tg;
                return;
            }
            const uint64_t same = match_mask((uint32_t)v, (uint32_t)v, bits_n, m);
            if (mine && ((same >> lane) >> 1) == 0) cur[v] = (int8_t)tg;
        };
        uint64_t done = 0;  // the chunk's lanes applied so far
        while (j < nT) {
            const int64_t T = p.times[j];
            if (T >= t_next) break;
            const uint64_t le = __ballot(in && t <= T);
            apply(le & ~done & ok);
            done |= le;
            if (le) {
                const int hi = 63 - __builtin_clzll(le);
                cut_now = rl32(ecut, hi);
                nb_now = rl32(enb, hi);
            }
            __syncthreads();
            emit(j, cut_now, nb_now);
            ++j;
        }
        if (j >= nT) break;  // events after the last sample are not applied
        apply(inm & ~done & ok);
        if (inm) {
            const int hi = 63 - __builtin_clzll(inm);
            cut_now = rl32(ecut, hi);
            nb_now = rl32(enb, hi);
        }
        __syncthreads();
    }
}

}  // namespace

int launch_plans(const PlansParams &p, void *stream) {
    const LogWindow &w = p.log;
    if (w.nc <= 0 || p.n_times <= 0) return (int)hipSuccess;
    if (w.k < 1 || w.k > 32 || w.n < 1 || w.n > w.npad || (w.npad & 15) || !p.times || !p.cut0 || !p.nb0 ||
        (p.pops && !p.node_pop))
        return (int)hipErrorInvalidValue;
    launch_lds(plans_kernel, dim3((unsigned)w.nc), dim3(64), plans_lds_bytes(w.npad), (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

}  // namespace fc
