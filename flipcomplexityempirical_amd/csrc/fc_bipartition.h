        // bipartition_tree of a node subset M, as text: included inside the ReCom kernels' proposal
        // loop (fc_recom_body.h) and the seed-plan kernel's level loop (fc_seed.hip), and nowhere
        // else.  Text, not a device function, for the reason fc_recom.hip gives for its body.
        // The includer supplies, in scope:
        //   inM(x)           the membership test of M (x < n);
        //   cut_pop(s)       the cut test of a subtree population s (int32_t), x != root being the block's;
        //   d, gid           the Philox draw index (uint64_t) and chain word (uint32_t);
        //   p                .max_attempts, .node_repeats, .seed_lo, .seed_hi, .eu, .ev, .eslot;
        //   trees_tot        the spanning-tree counter (int64_t, incremented per tree);
        //   RMAX, lane, n, npad, G, NB, nq, kScanU and the LDS arrays best, spop, par, comp, order,
        //   tadj with tadj_or, laid out by fc_lds.h's recom_lds.
        // It leaves: attempts made, tree (the last tree's index), root and child (-1: no cut within
        // p.max_attempts), p0 = pop(subtree(child)), and with a child the sign bit of spop[x] set
        // on subtree(child) -- spop[x] is defined for the nodes of M only.
        int tree = -1, root = -1, child = -1, attempts = 0;
        int64_t p0 = 0;  // subtree(child)'s population
        for (int t = 0; t < p.max_attempts; ++t) {
            ++attempts;
            FC_PROF(17, 1);
            if (t / p.node_repeats != tree) {
                tree = t / p.node_repeats;
                ++trees_tot;
                FC_STAMP(t_tr0);
                FC_PROF(14, 1);
                const Words4 kw = philox4x32_10((uint32_t)d, (uint32_t)(d >> 32), gid, 0x80000000u | (uint32_t)tree,
                                                p.seed_lo, p.seed_hi);
                const uint64_t key = ((uint64_t)kw.x1 << 32) | kw.x0;
                // Boruvka maximum spanning tree of M (weights with edge-id tie break).  A root's
                // hook target goes to the high half of its key word (the low half, ~edge id, still
                // tells a mutual hook); order[] holds the active nodes -- those with a neighbour in
                // another component at the last scan (components only merge, so a node without one
                // never has one again), kept in node order
                auto tgt = [&](int x) -> int { return ((const int32_t *)best)[2 * x + 1]; };
                auto set_tgt = [&](int x, int r) { ((int32_t *)best)[2 * x + 1] = r; };
                int m_act = 0;
                for (int x0 = 0; x0 < npad; x0 += kWave) {
                    const int x = x0 + lane;
                    const bool in = x < n && inM(x);
                    if (x < npad) {  // (npad is a multiple of 16 only)
                        comp[x] = in ? (int16_t)x : (int16_t)-1;
                        tadj[x] = 0;
                    }
                    const int incl = wave_scan_incl(in ? 1 : 0);
                    if (in) order[m_act + incl - 1] = (int16_t)x;
                    m_act += __builtin_amdgcn_readlane(incl, kWave - 1);
                }
                wave_sync();
                for (;;) {
                    FC_STAMP(t_b0);
                    FC_PROF(12, 1);
                    for (int x = lane; x < n; x += kWave) best[x] = 0;
                    wave_sync();
                    // kScanU active nodes per lane at a time: their neighbour rows (nb_d / 4
                    // vector loads: ids and edge ids) and the neighbours' components, every read
                    // issued before the first use; the keys are then formed by selects, without a
                    // branch per neighbour (a row holds the neighbours only: a ring's other cells
                    // cost no weight); the nodes still active are written back in order
                    int m_next = 0;
                    for (int i0 = 0; i0 < m_act; i0 += kScanU * kWave) {
                        int xs[kScanU], cxs[kScanU];
                        uint4 nw[kScanU][RMAX / 4];
#pragma unroll
                        for (int u = 0; u < kScanU; ++u) {
                            const int i = i0 + u * kWave + lane;
                            xs[u] = i < m_act ? (int)order[i] : -1;
                        }
#pragma unroll
                        for (int u = 0; u < kScanU; ++u) {
                            const int xc = xs[u] >= 0 ? xs[u] : 0;
                            cxs[u] = xs[u] >= 0 ? (int)comp[xc] : -1;
#pragma unroll
                            for (int q = 0; q < RMAX / 4; ++q)
                                nw[u][q] = q < nq ? NB[(size_t)xc * nq + q] : make_uint4(~0u, ~0u, ~0u, ~0u);
                        }
                        int cyv[kScanU][RMAX];
#pragma unroll
                        for (int u = 0; u < kScanU; ++u)
#pragma unroll
                            for (int j = 0; j < RMAX; ++j) {
                                const uint32_t nb = word4(nw[u][j >> 2], j & 3) & 0xffffu;
                                cyv[u][j] = nb != 0xffffu ? (int)comp[nb] : -1;
                            }
#pragma unroll
                        for (int u = 0; u < kScanU; ++u)
#pragma unroll
                            for (int j = 0; j < RMAX; ++j) asm volatile("" : "+v"(cyv[u][j]));
#pragma unroll
                        for (int u = 0; u < kScanU; ++u) {
                            const int cx = cxs[u];
                            uint64_t bk = 0;
                            bool any = false;
#pragma unroll
                            for (int q = 0; q < RMAX / 4; ++q) {
                                if (q >= nq) break;
#pragma unroll
                                for (int t4 = 0; t4 < 4; ++t4) {
                                    const int j = 4 * q + t4;
                                    const uint32_t e = word4(nw[u][q], t4) >> 16;
                                    const bool use = cx >= 0 && cyv[u][j] >= 0 && cyv[u][j] != cx;
                                    any |= use;
                                    const uint64_t kk = ((splitmix64(key + (uint64_t)e) >> 32) << 32) | (0xffffffffu - e);
                                    bk = (use && kk > bk) ? kk : bk;
                                }
                            }
                            if (bk) atomicMax((unsigned long long *)&best[cx], (unsigned long long)bk);
                            // (positions <= the entries this iteration read: in-place is safe)
                            const int incl = wave_scan_incl(any ? 1 : 0);
                            if (any) order[m_next + incl - 1] = (int16_t)xs[u];
                            m_next += __builtin_amdgcn_readlane(incl, kWave - 1);
                        }
                    }
                    m_act = m_next;
                    wave_sync();
                    FC_STAMP(t_b1);
                    FC_PROF(3, t_b1 - t_b0);
                    bool hooked = false;
                    for (int x0 = lane; x0 < n; x0 += kJumpU * kWave) {  // kJumpU roots' reads in flight
                        bool rt[kJumpU];
                        uint64_t bxs[kJumpU];
                        int es[kJumpU], us[kJumpU], vs[kJumpU];
                        uint32_t kss[kJumpU];
#pragma unroll
                        for (int u = 0; u < kJumpU; ++u) {
                            const int x = x0 + u * kWave;
                            rt[u] = x < n && comp[x] == x;
                        }
#pragma unroll
                        for (int u = 0; u < kJumpU; ++u) bxs[u] = rt[u] ? best[x0 + u * kWave] : 0ull;
#pragma unroll
                        for (int u = 0; u < kJumpU; ++u) {
                            es[u] = bxs[u] ? (int)(0xffffffffu - (uint32_t)bxs[u]) : 0;
                            us[u] = p.eu[es[u]];
                            vs[u] = p.ev[es[u]];
                            kss[u] = p.eslot[es[u]];
                        }
#pragma unroll
                        for (int u = 0; u < kJumpU; ++u) {
                            if (!rt[u]) continue;
                            const int x = x0 + u * kWave;
                            if (bxs[u] == 0) {  // no edge out (M's last component)
                                set_tgt(x, x);
                                continue;
                            }
                            const int other = comp[us[u]] == x ? comp[vs[u]] : comp[us[u]];
                            // hook (both roots chose this edge: the smaller id stays a root)
                            set_tgt(x, ((uint32_t)best[other] == (uint32_t)bxs[u] && x < other) ? x : other);
                            hooked = true;
                            // record the tree edge on both endpoints (the other end's index in the row)
                            tadj_or(us[u], 1u << (kss[u] & 0xffu));
                            tadj_or(vs[u], 1u << (kss[u] >> 8));
                        }
                    }
                    wave_sync();
                    FC_STAMP(t_b2);
                    FC_PROF(4, t_b2 - t_b1);
                    if (!__any(hooked)) break;
                    // the new roots: every old root follows its hook targets to the one hooked onto
                    // itself (distinct keys: the only cycles are mutual hooks, broken by id), then
                    // every node takes its old root's new root -- two passes, where pointer jumping
                    // over all nodes took about four per round
                    FC_PROF(15, 1);
                    for (int x0 = lane; x0 < n; x0 += kJumpU * kWave) {
                        bool rt[kJumpU];
                        int rs[kJumpU];
#pragma unroll
                        for (int u = 0; u < kJumpU; ++u) rt[u] = x0 + u * kWave < n && comp[x0 + u * kWave] == x0 + u * kWave;
#pragma unroll
                        for (int u = 0; u < kJumpU; ++u) rs[u] = rt[u] ? tgt(x0 + u * kWave) : 0;
#pragma unroll
                        for (int u = 0; u < kJumpU; ++u) {
                            if (!rt[u]) continue;
                            int r = rs[u];
                            for (int r2 = tgt(r); r2 != r; r2 = tgt(r)) r = r2;
                            set_tgt(x0 + u * kWave, r);
                        }
                    }
                    wave_sync();
                    for (int x0 = lane; x0 < n; x0 += kJumpU * kWave) {  // kJumpU reads in flight
                        int cxs[kJumpU], rts[kJumpU];
#pragma unroll
                        for (int u = 0; u < kJumpU; ++u) cxs[u] = x0 + u * kWave < n ? (int)comp[x0 + u * kWave] : -1;
#pragma unroll
                        for (int u = 0; u < kJumpU; ++u) rts[u] = cxs[u] >= 0 ? tgt(cxs[u]) : -1;
#pragma unroll
                        for (int u = 0; u < kJumpU; ++u)
                            if (rts[u] != cxs[u]) comp[x0 + u * kWave] = (int16_t)rts[u];
                    }
                    wave_sync();
                    FC_STAMP(t_b3);
                    FC_PROF(5, t_b3 - t_b2);
                }
                FC_STAMP(t_tr1);
                FC_PROF(2, t_tr1 - t_tr0);
            }
            FC_STAMP(t_r0);
            const Words4 cw = philox4x32_10((uint32_t)d, (uint32_t)(d >> 32), gid, 0x40000000u | (uint32_t)t,
                                            p.seed_lo, p.seed_hi);
            // root = choice([x for x in h if h.degree(x) > 1]), ascending node id
            int nroot = 0;
            auto is_inner = [&](int x) { return inM(x) && __popc((uint32_t)tadj[x]) > 1; };
            int nr_tot = 0;
            {
                // count first (the choice multiplies by the count)
                const int chunk = (n + kWave - 1) / kWave;
                const int lo = min(n, lane * chunk), hi = min(n, lo + chunk);
                int cc = 0;
                for (int i = lo; i < hi; ++i) cc += is_inner(i) ? 1 : 0;
                nr_tot = __builtin_amdgcn_readlane(wave_scan_incl(cc), kWave - 1);
            }
            if (nr_tot == 0) continue;
            root = kth_item(n, lane, mulhi64(((uint64_t)cw.x1 << 32) | cw.x0, (uint64_t)nr_tot), is_inner, nroot);
            FC_STAMP(t_r1);
            FC_PROF(6, t_r1 - t_r0);
            // the tree's adjacency as a CSR in the Boruvka keys' space (dead until the subtree sums):
            // offsets by a wave scan of the tree degrees, neighbour ids from the ring slots
            int16_t *toff = (int16_t *)best;       // [n + 1]
            int16_t *tnb = toff + recom_csr_first(n);  // [2 (|M| - 1)]
            {
                int ob = 0;
                for (int x0 = 0; x0 < n; x0 += kWave) {
                    const int x = x0 + lane;
                    const int dg = x < n ? __popc((uint32_t)tadj[x]) : 0;
                    const int incl = wave_scan_incl(dg);
                    if (x < n) toff[x] = (int16_t)(ob + incl - dg);
                    ob += __builtin_amdgcn_readlane(incl, kWave - 1);
                }
                if (lane == 0) toff[n] = (int16_t)ob;
                for (int x0 = lane; x0 < n; x0 += kScanU * kWave) {
                    uint32_t tbs[kScanU];
                    int os[kScanU];
                    uint4 nw[kScanU][RMAX / 4];
#pragma unroll
                    for (int u = 0; u < kScanU; ++u) {
                        const int x = x0 + u * kWave;
                        const int xc = x < n ? x : x0;
                        tbs[u] = x < n ? (uint32_t)tadj[x] : 0u;
                        os[u] = toff[xc];
#pragma unroll
                        for (int q = 0; q < RMAX / 4; ++q)
                            nw[u][q] = q < nq ? NB[(size_t)xc * nq + q] : make_uint4(~0u, ~0u, ~0u, ~0u);
                    }
#pragma unroll
                    for (int u = 0; u < kScanU; ++u) {
                        int o = os[u];
#pragma unroll
                        for (int j = 0; j < RMAX; ++j)
                            if ((tbs[u] >> j) & 1u) tnb[o++] = (int16_t)(word4(nw[u][j >> 2], j & 3) & 0xffffu);
                    }
                }
            }
            wave_sync();
            // BFS order over the tree, a level at a time; children placed by a wave scan of the
            // child counts; level starts in comp[]
            if (lane == 0) {
                order[0] = (int16_t)root;
                par[root] = -1;
                comp[0] = 0;
            }
            wave_sync();
            int L = 0;
            {
                int ls = 0, le = 1;
                while (ls < le) {
                    // level L = order[ls, le) holds a node: its end is the next level's start.  The
                    // root has two children or more, so L + 1 <= |M| - 1 < npad always (the test
                    // never fails; comp[npad] would be order[0]).  Written again after the level
                    if (lane == 0 && L + 1 < npad) comp[L + 1] = (int16_t)le;
                    int nb_end = le;
                    for (int i0 = ls; i0 < le; i0 += kWave) {
                        const int i = i0 + lane;
                        int x = 0, o0 = 0, o1 = 0, px = -1;
                        if (i < le) {
                            x = order[i];
                            o0 = toff[x];
                            o1 = toff[x + 1];
                            px = par[x];
                        }
                        const int nch = o1 - o0 - (px >= 0 ? 1 : 0);
                        const int incl = wave_scan_incl(nch);
                        int pos = nb_end + incl - nch;
                        nb_end += __builtin_amdgcn_readlane(incl, kWave - 1);
                        // every child read issued at once.  The written entries end before par;
                        // the up to RMAX - 1 read past o1 run into par where npad - n < 3 (RMAX =
                        // 16: 5) and always end before comp, in the chain's own slice; their
                        // values are discarded (tests/native/lds_layout_check.cpp)
                        int yv[RMAX];
#pragma unroll
                        for (int j = 0; j < RMAX; ++j) yv[j] = tnb[o0 + j];
#pragma unroll
                        for (int j = 0; j < RMAX; ++j) asm volatile("" : "+v"(yv[j]));
#pragma unroll
                        for (int j = 0; j < RMAX; ++j) {
                            if (o0 + j >= o1 || yv[j] == px) continue;
                            order[pos++] = (int16_t)yv[j];
                            par[yv[j]] = (int16_t)x;
                        }
                    }
                    wave_sync();
                    ++L;
                    ls = le;
                    le = nb_end;
                    // (an empty level ends the walk and its end is never read: nM = comp[L]; a
                    // path of npad nodes rooted next to an end would put it at comp[npad] = order[0])
                    if (lane == 0 && ls < le && L + 1 < npad) comp[L + 1] = (int16_t)le;
                }
            }
            wave_sync();
            FC_STAMP(t_r2);
            FC_PROF(7, t_r2 - t_r1);
            FC_PROF(13, L);
            // subtree populations, leaves upward
            const int nM = comp[L];
            for (int i = lane; i < nM; i += kWave) {
                const int x = order[i];
                spop[x] = G[x].pop;
            }
            wave_sync();
            for (int l = L - 1; l >= 1; --l) {
                for (int i = comp[l] + lane; i < comp[l + 1]; i += kWave) {
                    const int x = order[i];
                    atomicAdd(&spop[par[x]], spop[x]);
                }
                wave_sync();
            }
            FC_STAMP(t_r3);
            FC_PROF(8, t_r3 - t_r2);
            // cuts: the non-root nodes of M whose subtree population passes the includer's test
            auto is_cut = [&](int x) { return inM(x) && x != root && cut_pop(spop[x]); };
            int ncut = 0;
            {
                const int chunk = (n + kWave - 1) / kWave;
                const int lo = min(n, lane * chunk), hi = min(n, lo + chunk);
                int cc = 0;
                for (int i = lo; i < hi; ++i) cc += is_cut(i) ? 1 : 0;
                ncut = __builtin_amdgcn_readlane(wave_scan_incl(cc), kWave - 1);
            }
            if (ncut == 0) continue;
            int dummy = 0;
            child = kth_item(n, lane, mulhi64(((uint64_t)cw.x3 << 32) | cw.x2, (uint64_t)ncut), is_cut, dummy);
            FC_STAMP(t_r4);
            FC_PROF(9, t_r4 - t_r3);
            // subset = subtree(child): marks flow down the BFS levels
            p0 = spop[child];
            if (lane == 0) spop[child] |= (int32_t)0x80000000u;
            wave_sync();
            for (int l = 1; l < L; ++l) {
                for (int i = comp[l] + lane; i < comp[l + 1]; i += kWave) {
                    const int x = order[i];
                    if (spop[par[x]] < 0) spop[x] |= (int32_t)0x80000000u;
                }
                wave_sync();
            }
            FC_STAMP(t_r5);
            FC_PROF(10, t_r5 - t_r4);
            break;
        }
