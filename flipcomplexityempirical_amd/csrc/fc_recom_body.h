    // The body of both ReCom kernel instances: included, as text, inside recom_kernel<RMAX> and
    // recom_log_kernel<RMAX> (fc_recom.hip), and nowhere else; steps 2-4 of a proposal are
    // fc_bipartition.h, included below.  In scope there:
    //   RMAX, p          the kernel's template parameter and its RecomParams argument;
    //   LOG              constexpr bool: the run keeps a move log.  An accepted step then appends one
    //                    fc_event per node that changes district, all with the new state's yield
    //                    index, |cut| and |B| (a burst; DESIGN.md "ReCom move log");
    //   events, ev_cap   the log, [n_chains * ev_cap] (read with LOG only).
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = (int)(threadIdx.x & 63u);
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c = (int)blockIdx.x * (int)(blockDim.x >> 6) + wv;
    if (c >= p.n_chains) return;
    const int n = p.n, E = p.n_edges;
    const int npad = (n + 15) & ~15;
    unsigned char *base = smem + (size_t)wv * p.chain_lds_bytes;
    const auto lds = recom_lds(base, npad, RMAX);  // the chain's arrays (fc_lds.h)
    using TAdj = typename std::conditional<RMAX == 8, uint8_t, uint16_t>::type;
    uint64_t *best = (uint64_t *)lds.keys;
    int32_t *spop = (int32_t *)lds.keys;
    int16_t *par = (int16_t *)lds.par, *comp = (int16_t *)lds.comp, *order = (int16_t *)lds.order;
    TAdj *tadj = (TAdj *)lds.tadj;
    int8_t *a = (int8_t *)lds.a;
    // tree-edge bits by 32-bit LDS atomics on the word holding the node's entry
    auto tadj_or = [&](int x, uint32_t bits) {
        constexpr int kPer = 4 / (int)sizeof(TAdj);
        atomicOr((uint32_t *)tadj + x / kPer, bits << (8 * (int)sizeof(TAdj) * (x % kPer)));
    };
    const NodeRec<RMAX> *__restrict__ G = (const NodeRec<RMAX> *)p.graph;
    constexpr int kScanU = RMAX == 8 ? kScanU8 : 2;
    const uint4 *__restrict__ NB = (const uint4 *)p.nbe;  // neighbour rows, nq vectors each
    const int nq = p.nb_d >> 2;

    {
        const uint4 *ga = (const uint4 *)(p.assign + (size_t)c * npad);
        for (int i = lane; i < npad / 16; i += kWave) ((uint4 *)a)[i] = ga[i];
    }
    ChainScalars *scp = p.sc + c;
    uint64_t draw = scp->draw;
    const uint64_t draw_cap = draw + (uint64_t)p.max_draws;
    int64_t steps = scp->steps, proposals = scp->proposals, accepted = scp->accepted, inv_pop = scp->inv_pop;
    int64_t sum_cut = scp->sum_cut, sum_nb = scp->sum_nb, attempts_tot = scp->bfs_calls, trees_tot = scp->bfs_levels;
    int64_t trace_len = scp->trace_len;
    [[maybe_unused]] int64_t ev_len = 0;
    if constexpr (LOG) ev_len = scp->ev_len;
    int cut = scp->cut, nb = scp->nb;
    const int pop_lo = scp->pop_lo, pop_hi = scp->pop_hi;  // this chain's bounds (chain_pop_bounds)
    int stuck = 0;
    const uint32_t gid = p.chain_id_offset + (uint32_t)c;
    const bool trace_on = p.trace && c < p.trace_chains;
    int64_t rem = p.n_steps;
#ifdef FC_PHASE_PROF
    // phase cycles (diagnostic build; tools/prof_recom_report.py): 0 loop, 1 edge + popM,
    // 2 spanning trees, 3 Boruvka scans, 4 hooks, 5 pointer jumps, 6 root choice, 7 BFS order,
    // 8 subtree sums, 9 cut choice, 10 subset marks, 11 step 5; counts: 12 Boruvka rounds,
    // 13 BFS levels, 14 trees, 15 pointer-jump passes, 16 proposals, 17 attempts
    int64_t *prof_acc = (int64_t *)(base + p.chain_lds_bytes - kProfSlots * 8);
    if (lane < kProfSlots) prof_acc[lane] = 0;
#endif
    wave_sync();
    FC_STAMP(t_loop0);

    while (rem > 0) {
        if (draw >= draw_cap) {
            stuck = 1;
            break;
        }
        const uint64_t d = draw++;
        FC_STAMP(t_s0);
        FC_PROF(16, 1);
        const Words4 w = philox4x32_10((uint32_t)d, (uint32_t)(d >> 32), gid, 0u, p.seed_lo, p.seed_hi);
        // ---- 1. recom: edge = random.choice(tuple(partition["cut_edges"])) ----------------
        int tot = 0;
        const int e_sel = kth_item(E, lane, mulhi64(((uint64_t)w.x3 << 32) | w.x0, (uint64_t)cut),
                                   [&](int e) { return a[p.eu[e]] != a[p.ev[e]]; }, tot);
        const int d0 = a[p.eu[e_sel]], d1 = a[p.ev[e_sel]];
        auto inM = [&](int x) { return a[x] == d0 || a[x] == d1; };
        int64_t pm = 0;
        for (int x = lane; x < n; x += kWave) pm += inM(x) ? G[x].pop : 0;
        const int64_t popM = wave_sum64(pm);
        ++proposals;
        FC_STAMP(t_s1);
        FC_PROF(1, t_s1 - t_s0);
        // ---- 2-4. bipartition_tree (fc_bipartition.h, shared as text with fc_seed.hip) -------
        // cuts: |pop(subtree(x)) - ideal| < epsilon * ideal (has_ideal_population)
        auto cut_pop = [&](int32_t s) { return fabs((double)s - p.pop_target) < p.epsilon * p.pop_target; };
#include "fc_bipartition.h"
        attempts_tot += attempts;
        if (child < 0) {
            stuck = 1;
            break;
        }
        // ---- 5. the proposed state: subtree(child) -> parts[0], rest of M -> parts[1] --------
        FC_STAMP(t_5a);
        auto na = [&](int x) -> int { return inM(x) ? (spop[x] < 0 ? d0 : d1) : a[x]; };
        const int64_t p1 = popM - p0;
        int flags;
        if (p0 < pop_lo || p0 > pop_hi || p1 < pop_lo || p1 > pop_hi) {
            ++inv_pop;
            flags = 8;
        } else {
            ++steps;
            --rem;
            flags = 1;
            // one pass over the nodes' neighbour rows: |cut'| (every cut edge seen from both
            // ends) and |B'| (nodes with a neighbour in another district)
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
                    const int ax = na(x0 + u * kWave);
                    int dn = 0;
#pragma unroll
                    for (int j = 0; j < RMAX; ++j) {
                        const uint32_t y = word4(nw[u][j >> 2], j & 3) & 0xffffu;
                        dn += (y != 0xffffu && na((int)y) != ax) ? 1 : 0;
                    }
                    cc += dn;
                    bb += dn > 0 ? 1 : 0;
                }
            }
            const int cut_new = (int)(wave_sum64(cc) / 2);
            // cut_accept: random() < base ** (cut - cut'), table over cut - cut' in [-E, E]
            if (mant53(w.x1, w.x2) < p.accept_thresh[cut - cut_new + E]) {
                flags |= 2;
                ++accepted;
                nb = (int)wave_sum64(bb);
                wave_sync();
                if constexpr (LOG) {
                    // the burst: the moved nodes in ascending id, compacted 64 nodes at a time --
                    // consecutive lanes' 16-byte stores fill consecutive slots.  Slots at or past
                    // ev_cap are counted, not written (a lane reads and writes its own a[x] only)
                    const uint64_t tail = ((uint64_t)(uint16_t)cut_new << 16) | ((uint64_t)(uint16_t)nb << 32);
                    ulong2 *const ev = (ulong2 *)events + (size_t)c * (size_t)ev_cap;
                    for (int x0 = 0; x0 < n; x0 += kWave) {
                        const int x = x0 + lane;
                        const int tg = x < n ? na(x) : 0;
                        const bool moved = x < n && tg != a[x];
                        const int incl = wave_scan_incl(moved ? 1 : 0);
                        const int64_t idx = ev_len + incl - 1;
                        if (moved && idx < ev_cap)
                            ev[idx] = make_ulong2((unsigned long)steps,
                                                  (unsigned long)((uint64_t)(uint16_t)x | tail | ((uint64_t)(uint8_t)tg << 48)));
                        if (moved) a[x] = (int8_t)tg;
                        ev_len += __builtin_amdgcn_readlane(incl, kWave - 1);
                    }
                } else {
                    for (int x = lane; x < n; x += kWave) a[x] = (int8_t)na(x);
                }
                cut = cut_new;
            }
            sum_cut += cut;
            sum_nb += nb;
        }
        wave_sync();
        if (trace_on && lane == 0 && trace_len < p.trace_cap) {
            fc_recom_record &rr = p.trace[(size_t)c * p.trace_cap + trace_len];
            rr.draw = (int64_t)d;
            rr.edge = e_sel;
            rr.root = root;
            rr.child = child;
            rr.attempts = attempts;
            rr.flags = flags;
            rr.cut = cut;
        }
        if (trace_on) ++trace_len;
        wave_sync();
        FC_STAMP(t_5b);
        FC_PROF(11, t_5b - t_5a);
    }
    FC_STAMP(t_loop1);
    FC_PROF(0, t_loop1 - t_loop0);
#ifdef FC_PHASE_PROF
    wave_sync();
    if (lane == 0)
        for (int i = 0; i < kProfSlots; ++i) p.prof[(size_t)c * kProfSlots + i] = prof_acc[i];
#endif

    // ---- write back ---------------------------------------------------------------------
    {
        uint4 *ga = (uint4 *)(p.assign + (size_t)c * npad);
        for (int i = lane; i < npad / 16; i += kWave) ga[i] = ((const uint4 *)a)[i];
    }
    if (lane == 0) {
        scp->draw = draw;
        scp->steps = steps;
        scp->proposals = proposals;
        scp->accepted = accepted;
        scp->inv_pop = inv_pop;
        scp->sum_cut = sum_cut;
        scp->sum_nb = sum_nb;
        scp->bfs_calls = attempts_tot;
        scp->bfs_levels = trees_tot;
        scp->trace_len = trace_len;
        if constexpr (LOG) scp->ev_len = ev_len;
        scp->cut = cut;
        scp->nb = nb;
        scp->stuck = stuck;
    }
