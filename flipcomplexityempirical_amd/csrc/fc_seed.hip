// Seed plans for gfx950: random k-district start plans by recursive tree bipartition,
// gerrychain 0.2's recursive_tree_part [gc-0.2] restated with an integer population rule
// (include/flipchain.h fc_graph_seed_plans).
//
// One plan per wavefront; the plan's assignment and the spanning-tree working set live in LDS,
// in the ReCom kernel's layout (fc_lds.h recom_lds).  Attempt r of a plan labels every node k - 1
// (the remainder M) and cuts one district off M per level i = 0 .. k - 2: the ReCom proposal's
// bipartition_tree on M -- fc_bipartition.h, the text the ReCom kernels include -- with the cut
// rule  lo <= s <= hi  and  m lo <= pop(M) - s <= m hi  (m = k - 1 - i more districts must fit the
// remainder), then subtree(child) -> district i.  Removing a subtree from a tree leaves a tree, so
// every remainder and with it the last district is connected.  A level without a cut after
// max_attempts attempts ends the attempt; attempt r + 1 starts from scratch, up to max_restarts.
// The draws are Philox calls at draw index 0xFFFFFFFF00000000 | r << 8 | i, which no run's draw
// counter reaches, with the plan's global id as the chain word: a plan does not depend on the
// launch it is computed in.
// Subtree populations are int32 with bit 31 as the subset mark, as in fc_recom.hip: the host
// refuses a population total above INT32_MAX (fc_plan.cpp check_seed).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <type_traits>

#include "fc_device.h"
#include "fc_internal.h"
#include "fc_philox.h"
#include "fc_tree_dev.h"

// the seed kernel keeps no phase counters (the diagnostic builds profile the ReCom run)
#undef FC_STAMP
#undef FC_PROF
#define FC_STAMP(t)
#define FC_PROF(i, x)

namespace fc {

using namespace dev;

namespace {

template <int RMAX>
__global__ __launch_bounds__(256) void seed_kernel(SeedParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = (int)(threadIdx.x & 63u);
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c = (int)blockIdx.x * (int)(blockDim.x >> 6) + wv;
    if (c >= p.n_plans) return;
    const int n = p.n, k = p.k;
    const int npad = (n + 15) & ~15;
    const auto lds = recom_lds(smem + (size_t)wv * p.chain_lds_bytes, npad, RMAX);  // the plan's arrays (fc_lds.h)
    using TAdj = typename std::conditional<RMAX == 8, uint8_t, uint16_t>::type;
    uint64_t *best = (uint64_t *)lds.keys;
    int32_t *spop = (int32_t *)lds.keys;
    int16_t *par = (int16_t *)lds.par, *comp = (int16_t *)lds.comp, *order = (int16_t *)lds.order;
    TAdj *tadj = (TAdj *)lds.tadj;
    int8_t *a = (int8_t *)lds.a;
    auto tadj_or = [&](int x, uint32_t bits) {
        constexpr int kPer = 4 / (int)sizeof(TAdj);
        atomicOr((uint32_t *)tadj + x / kPer, bits << (8 * (int)sizeof(TAdj) * (x % kPer)));
    };
    const NodeRec<RMAX> *__restrict__ G = (const NodeRec<RMAX> *)p.graph;
    constexpr int kScanU = RMAX == 8 ? kScanU8 : 2;
    const uint4 *__restrict__ NB = (const uint4 *)p.nbe;
    const int nq = p.nb_d >> 2;

    const uint32_t gid = p.plan_id_offset + (uint32_t)c;
    const int8_t rest = (int8_t)(k - 1);  // the remainder's label
    auto inM = [&](int x) { return a[x] == rest; };
    int64_t attempts_tot = 0, trees_tot = 0;
    int restarts = 0, ok = 0;
    for (int r = 0; r <= p.max_restarts && !ok; ++r) {
        restarts = r;
        {
            const uint32_t w4 = 0x01010101u * (uint32_t)(uint8_t)rest;
            for (int i = lane; i < npad / 16; i += kWave) ((uint4 *)a)[i] = make_uint4(w4, w4, w4, w4);
        }
        wave_sync();
        int64_t popM = p.pop_total;
        int level = 0;
        for (; level < k - 1; ++level) {
            const int64_t m = k - 1 - level;  // districts the remainder must still hold
            const int64_t rem_lo = m * p.pop_lo, rem_hi = m * p.pop_hi;
            const uint64_t d = 0xFFFFFFFF00000000ull | ((uint64_t)(uint32_t)r << 8) | (uint64_t)level;
            auto cut_pop = [&](int32_t s) {
                const int64_t s64 = s, left = popM - s64;
                return s64 >= p.pop_lo && s64 <= p.pop_hi && left >= rem_lo && left <= rem_hi;
            };
#include "fc_bipartition.h"
            attempts_tot += attempts;
            if (child < 0) break;
            // subtree(child) -> district `level` (spop is defined on M only)
            for (int x = lane; x < n; x += kWave)
                if (inM(x) && spop[x] < 0) a[x] = (int8_t)level;
            popM -= p0;
            wave_sync();
        }
        ok = level == k - 1 ? 1 : 0;
    }

    // |cut| and |B| of the plan: one pass over the nodes' neighbour rows (every cut edge seen from
    // both ends), as the ReCom body's step 5 counts them
    int cut = 0, nb = 0;
    if (ok) {
        int cc = 0, bb = 0;
        for (int x0 = lane; x0 < n; x0 += kJumpU * kWave) {
            uint4 nw[kJumpU][RMAX / 4];
#pragma unroll
            for (int u = 0; u < kJumpU; ++u) {
                const int xc = x0 + u * kWave < n ? x0 + u * kWave : x0;
#pragma unroll
                for (int q = 0; q < RMAX / 4; ++q)
                    nw[u][q] = q < nq ? NB[(size_t)xc * nq + q] : make_uint4(~0u, ~0u, ~0u, ~0u);
            }
#pragma unroll
            for (int u = 0; u < kJumpU; ++u) {
                if (x0 + u * kWave >= n) break;
                const int ax = a[x0 + u * kWave];
                int dn = 0;
#pragma unroll
                for (int j = 0; j < RMAX; ++j) {
                    const uint32_t y = word4(nw[u][j >> 2], j & 3) & 0xffffu;
                    dn += (y != 0xffffu && a[y] != ax) ? 1 : 0;
                }
                cc += dn;
                bb += dn > 0 ? 1 : 0;
            }
        }
        cut = (int)(wave_sum64(cc) / 2);
        nb = (int)wave_sum64(bb);
    } else {
        for (int i = lane; i < npad / 16; i += kWave) ((uint4 *)a)[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
    }
    wave_sync();

    // ---- write back: the row (padded, 16 bytes per store) and the plan's record ----------------
    {
        uint4 *ga = (uint4 *)(p.assign + (size_t)c * npad);
        for (int i = lane; i < npad / 16; i += kWave) ga[i] = ((const uint4 *)a)[i];
    }
    if (lane == 0) {
        fc_seed_stats st;
        st.attempts = attempts_tot;
        st.trees = trees_tot;
        st.restarts = restarts;
        st.ok = ok;
        st.cut = cut;
        st.nb = nb;
        p.stats[c] = st;
    }
}

}  // namespace

int launch_seed(const SeedParams &p, int ring_max, void *stream, char *name, size_t name_cap) {
    const int wpb = waves_per_block(p.chain_lds_bytes);
    const int blocks = (p.n_plans + wpb - 1) / wpb;
    const size_t lds = (size_t)p.chain_lds_bytes * wpb;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(blocks), block(kWave * wpb);
    if (ring_max != 8 && ring_max != 16) return (int)hipErrorInvalidValue;
    if (name) snprintf(name, name_cap, "fc::seed_kernel<%d>", ring_max);
    if (ring_max == 8) launch_lds(seed_kernel<8>, grid, block, lds, s, p);
    else launch_lds(seed_kernel<16>, grid, block, lds, s, p);
    return (int)hipGetLastError();
}

}  // namespace fc
