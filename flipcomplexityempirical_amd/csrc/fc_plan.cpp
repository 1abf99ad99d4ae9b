// The host half of fc_run_create (fc_plan.h): parameter checks, LDS layout and residency
// arithmetic, launch tuning, each chain's validated initial state, the parameter hash and the
// ReCom tables.  Plain C++ (no HIP).
#include "fc_plan.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "fc_philox.h"
#include "fc_ring_table.h"

namespace fc {
namespace {

int bad(std::string &err, int code, const std::string &msg) {
    err = msg;
    return code;
}

// U53 acceptance threshold of a probability bound x: random() < x as mant53 < threshold
uint64_t u53_threshold(double x) {
    if (!(x < 1.0)) return 1ull << 53;  // always accepted
    if (!(x > 0.0)) return 0;
    return (uint64_t)std::ceil(x * 9007199254740992.0);
}

bool district_contiguous(const HostGraph &g, const int8_t *a, int k, std::vector<int32_t> &q,
                         std::vector<uint8_t> &seen) {
    std::fill(seen.begin(), seen.end(), 0);
    for (int d = 0; d < k; ++d) {
        int32_t start = -1, size = 0;
        for (int32_t u = 0; u < g.n; ++u)
            if (a[u] == d) { if (start < 0) start = u; ++size; }
        if (start < 0) continue;
        q.clear();
        q.push_back(start);
        seen[start] = 1;
        for (size_t h = 0; h < q.size(); ++h) {
            const int32_t u = q[h];
            for (int32_t j = g.row_ptr[u]; j < g.row_ptr[u + 1]; ++j) {
                const int32_t w = g.col_idx[j];
                if (a[w] == d && !seen[w]) { seen[w] = 1; q.push_back(w); }
            }
        }
        if ((int32_t)q.size() != size) return false;
    }
    return true;
}

// the device node records as bytes, the run's frozen nodes marked (FC_CON_FIXED)
template <int RMAX>
std::vector<unsigned char> pack_records(const HostGraph &g, const int32_t *frozen, int32_t n_frozen) {
    std::vector<NodeRec<RMAX>> recs(g.n);
    for (int32_t v = 0; v < g.n; ++v) {
        auto &r = recs[v];
        std::memset(&r, 0, sizeof r);
        r.meta = g.meta[v];
        r.pop = g.pop[v];
        r.deg = g.row_ptr[v + 1] - g.row_ptr[v];
        for (int j = 0; j < RMAX; ++j) {
            const uint32_t x = (uint32_t)g.ring[(size_t)v * g.ring_max + j] & 0xffffu;
            r.ring[j >> 1] |= x << (16 * (j & 1));
        }
    }
    for (int32_t i = 0; i < n_frozen; ++i) recs[frozen[i]].meta |= kMetaFrozen;
    const unsigned char *b = (const unsigned char *)recs.data();
    return std::vector<unsigned char>(b, b + recs.size() * sizeof(NodeRec<RMAX>));
}

bool is_variant(const fc_params &p) {
    return p.accept != FC_ACCEPT_CUT || p.con_valid != 0 || p.con_accept != 0 || p.n_frozen > 0;
}

int check_params(const HostGraph &g, const fc_params *p, int32_t n_chains, const double *bases, std::string &err) {
    // the caller's fc_params layout must be this library's: nothing past struct_size is read
    if (p->struct_size != sizeof(fc_params) || p->abi_version != FC_ABI_VERSION)
        return bad(err, FC_ERR_ARG, "fc_run_create: fc_params.struct_size " + std::to_string(p->struct_size) +
                                    " / abi_version " + std::to_string(p->abi_version) + " do not match this library (" +
                                    std::to_string(sizeof(fc_params)) + " / " + std::to_string(FC_ABI_VERSION) +
                                    "): set them with fc_params_init or sizeof / FC_ABI_VERSION of the same flipchain.h");
    if (p->k < 2 || p->k > kMaxKGeneral)
        return bad(err, FC_ERR_UNSUPPORTED, "fc_run_create: k must be in [2, 32]");
    if (p->proposal == FC_PROPOSE_BI_SIGN && p->k != 2)
        return bad(err, FC_ERR_ARG, "fc_run_create: slow_reversible_propose_bi flips between two districts (k == 2)");
    if (p->proposal != FC_PROPOSE_BI_SIGN && p->proposal != FC_PROPOSE_PAIR && p->proposal != FC_PROPOSE_RECOM)
        return bad(err, FC_ERR_UNSUPPORTED, "fc_run_create: unsupported proposal");
    const bool recom = p->proposal == FC_PROPOSE_RECOM;
    if (p->stream != FC_STREAM_NODE && p->stream != FC_STREAM_BAND)
        return bad(err, FC_ERR_ARG, "fc_run_create: stream must be FC_STREAM_NODE or FC_STREAM_BAND");
    if (p->stream == FC_STREAM_BAND && (p->k != 2 || recom || g.n > 4096))
        return bad(err, FC_ERR_UNSUPPORTED, "fc_run_create: the band stream is for k = 2 flip runs on n <= 4096 nodes");
    if (recom) {
        if (p->accept != FC_ACCEPT_CUT || p->con_valid != 0 || p->con_accept != 0 || p->n_frozen > 0)
            return bad(err, FC_ERR_UNSUPPORTED, "fc_run_create: recom runs with the population Validator and cut_accept");
        if (!(p->recom_epsilon >= 0.0) || !(p->recom_pop_target > 0.0))
            return bad(err, FC_ERR_ARG, "fc_run_create: recom needs pop_target > 0 and epsilon >= 0");
        if (g.n > 8000)
            return bad(err, FC_ERR_UNSUPPORTED, "fc_run_create: recom keeps a chain's spanning tree in LDS (n <= 8000)");
        // fc_recom.hip sums subtree populations in int32 and marks the subset in bit 31
        int64_t pop_total = 0;
        for (int32_t u = 0; u < g.n; ++u) pop_total += g.pop[u];
        if (pop_total > INT32_MAX)
            return bad(err, FC_ERR_UNSUPPORTED, "fc_run_create: recom sums subtree populations in 31 bits (population total " +
                                                std::to_string(pop_total) + " exceeds INT32_MAX = 2147483647)");
        if (bases)
            for (int32_t c = 1; c < n_chains; ++c)
                if (bases[c] != bases[0]) return bad(err, FC_ERR_UNSUPPORTED, "fc_run_create: recom takes one base");
    }
    const int32_t n = g.n, k = p->k;
    // accept / constraint variants (uniform_accept, annealing_cut_accept_backwards,
    // boundary_condition, fixed_endpoints: grid_chain_sec11.py:39-52,81-110,159-165)
    const uint32_t con_valid = p->con_valid ? p->con_valid : (FC_CON_CONTIG | FC_CON_POP);
    const uint32_t con_all = FC_CON_CONTIG | FC_CON_POP | FC_CON_BOUNDARY | FC_CON_FIXED | FC_CON_EMPTY;
    if (is_variant(*p)) {
        if (k != 2) return bad(err, FC_ERR_UNSUPPORTED, "fc_run_create: accept / constraint variants need k == 2");
        if (p->accept < FC_ACCEPT_CUT || p->accept > FC_ACCEPT_ANNEAL)
            return bad(err, FC_ERR_ARG, "fc_run_create: unknown accept kind");
        if ((con_valid | p->con_accept) & ~con_all) return bad(err, FC_ERR_ARG, "fc_run_create: unknown constraint bits");
        if (!((con_valid | p->con_accept) & FC_CON_CONTIG))
            return bad(err, FC_ERR_UNSUPPORTED, "fc_run_create: single_flip_contiguous must be a Validator or accept "
                                            "constraint (the device keeps districts connected)");
        if (((con_valid | p->con_accept) & FC_CON_BOUNDARY) && g.n_gamma == 0)
            return bad(err, FC_ERR_UNSUPPORTED, "fc_run_create: boundary_condition needs a planar graph with a simple "
                                            "outer face (its nodes are the boundary set)");
        if (p->n_frozen < 0 || (p->n_frozen > 0 && !p->frozen)) return bad(err, FC_ERR_ARG, "fc_run_create: frozen nodes");
        for (int32_t i = 0; i < p->n_frozen; ++i)
            if (p->frozen[i] < 0 || p->frozen[i] >= n) return bad(err, FC_ERR_ARG, "fc_run_create: frozen node out of range");
    }
    return FC_OK;
}

// population bounds per chain, the district ids' range, labels, the |B| width and its
// log(1 - p) table, the bases
int plan_tables(const HostGraph &g, const fc_params *p, int32_t n_chains, const int8_t *init_assign,
                const double *bases, RunPlan &r, std::string &err) {
    const int32_t n = g.n, k = p->k;
    const bool recom = p->proposal == FC_PROPOSE_RECOM;
    // population bounds per chain (fc_params.chain_pop_bounds, else pop_lo / pop_hi for all)
    std::vector<int64_t> &pop_bounds = r.pop_bounds;
    pop_bounds.resize(2 * (size_t)n_chains);
    for (int32_t c = 0; c < n_chains; ++c) {
        pop_bounds[2 * (size_t)c] = p->chain_pop_bounds ? p->chain_pop_bounds[2 * (size_t)c] : p->pop_lo;
        pop_bounds[2 * (size_t)c + 1] = p->chain_pop_bounds ? p->chain_pop_bounds[2 * (size_t)c + 1] : p->pop_hi;
        for (int j = 0; j < 2; ++j)
            if (pop_bounds[2 * (size_t)c + j] > INT32_MAX || pop_bounds[2 * (size_t)c + j] < INT32_MIN)
                return bad(err, FC_ERR_UNSUPPORTED, "fc_run_create: population bounds must fit int32");
    }
    for (int64_t i = 0; i < (int64_t)n_chains * n; ++i)
        if (init_assign[i] < 0 || init_assign[i] >= k) return bad(err, FC_ERR_ARG, "fc_run_create: district id out of range");

    r.p = *p;
    r.labels.resize(k);
    for (int i = 0; i < k; ++i) r.labels[i] = p->labels ? p->labels[i] : i;
    r.p.labels = nullptr;
    // |b_nodes| as the driver's len(partition["b_nodes"]) counts it: nodes (b_nodes_bi, :155-156),
    // or with FC_FLAG_NB_PAIRS the (node, district) pairs of the pair updater b_nodes (:151-153)
    // a k > 2 driver registers for slow_reversible_propose (:117-130) -- at most
    // sum_u min(deg u, k - 1).  With k = 2 both counts are the same.
    const bool nb_pairs = (p->flags & FC_FLAG_NB_PAIRS) && k > 2;
    if ((p->flags & FC_FLAG_NB_PAIRS) && recom)
        return bad(err, FC_ERR_UNSUPPORTED, "fc_run_create: FC_FLAG_NB_PAIRS is for flip proposals");
    r.nb_w = n + 1;
    if (nb_pairs) {
        int64_t mx = 0;
        for (int32_t u = 0; u < n; ++u) mx += std::min<int64_t>(g.row_ptr[u + 1] - g.row_ptr[u], k - 1);
        if (mx > 65535)  // fc_event.nb is 16 bits
            return bad(err, FC_ERR_UNSUPPORTED, "fc_run_create: FC_FLAG_NB_PAIRS: more than 65535 possible pairs");
        r.nb_w = (int32_t)mx + 1;
    }
    const int32_t nbw = r.nb_w;
    r.log1mp.resize(nbw);
    if (p->log1mp) {
        std::copy(p->log1mp, p->log1mp + nbw, r.log1mp.begin());
    } else {
        const double denom = std::pow((double)n, (double)k) - 1.0;
        for (int32_t b = 0; b < nbw; ++b) r.log1mp[b] = std::log(1.0 - (double)b / denom);
    }
    r.p.log1mp = nullptr;
    r.p.frozen = nullptr;
    r.p.chain_pop_bounds = nullptr;
    r.p.con_valid = p->con_valid ? p->con_valid : (FC_CON_CONTIG | FC_CON_POP);
    r.variant = is_variant(*p);
    r.n_chains = n_chains;
    r.bases0.resize(n_chains);
    for (int32_t c = 0; c < n_chains; ++c) r.bases0[c] = bases ? bases[c] : p->base;
    return FC_OK;
}

// npad, words, the district-graph rule's use, the multi-flip marks, the PAIR slot bound and one
// chain's LDS bytes
int plan_lds(const HostGraph &g, const fc_params *p, RunPlan &r, std::string &err) {
    const int32_t n = g.n, R = g.ring_max, k = p->k;
    const bool recom = p->proposal == FC_PROPOSE_RECOM;
    const bool nb_pairs = (p->flags & FC_FLAG_NB_PAIRS) && k > 2;
    r.npad = (n + 15) & ~15;
    r.words = (n + 63) / 64;
    if (g.max_degree > 16)  // dev::wave_bfs labels each old neighbour with a 4-bit id
        return bad(err, FC_ERR_UNSUPPORTED, "fc_run_create: node degree above 16");
    if (recom)   // fc_recom.hip takes its pointers from the same layout (fc_lds.h)
        r.chain_lds_bytes = (int32_t)recom_lds<size_t>(0, r.npad, R).end;
    else if (k == 2)  // fc_flip2.hip: a, fcnt, thresholds, 3 BFS bitmaps, slots, commit marks (2 npad + 16),
                      // wait / tally queue (24 B per entry), launch start time, pace, first queued yield,
                      // tally-log length, launch's first yield (40) (sec11: 10,016 B, so 16 chains still
                      // fill a CU's 160 KB at the 1280-B allocation granule)
        r.chain_lds_bytes = 4 * r.npad + (2 * R + 2) * 8 + 24 * r.words + 5 * 64 * 4 + 16 + kWaitQ * 24 + 40 +
                            (p->stream == FC_STREAM_BAND ? 8 * r.words : 0);  // the band bitmap (sec11: 200 B)
    // k > 2: with every node's ring exact (all bounded faces triangles / quadrilaterals, so the
    // rings list every face-adjacent cell) contiguity is decided by the district-graph rule
    // (fc_kernels.hip district_rule) instead of the device search, whose scratch is then not
    // allocated; FC_FLAG_FORCE_BFS keeps the search (cross-check)
    r.dgraph = !recom && k > 2 && k <= kMaxKDistrictRule && g.n_exact == n && g.planar && g.outer_simple &&
               !(p->flags & FC_FLAG_FORCE_BFS);
    if (!recom && k > 2)  // fc_kernels.hip: a, fcnt (one packed byte per node with the district-graph
                          // rule), thresholds, [BFS scratch | district tables], slots, district
                          // populations, wait queue; the multi-flip commit's hashed marks (last)
                          // only when it is on, so an "off" run keeps its residency
    {
        const int base_b = (r.dgraph ? 1 : 2) * r.npad + (2 * R + 2) * 8 +
                           (r.dgraph ? dgraph_lds_bytes(k) : bfs_bytes(n)) + 5 * 64 * 4 +
                           kMaxKGeneral * 4 + kNfh * 4 + kWaitQK * 16;
        // chains per CU the LDS holds (granule 1280 B per one-wave workgroup, measured: DESIGN.md
        // §4), capped by the 16 waves the k > 2 instances' registers allow
        auto per_cu = [](int b) { return std::min(16, 160 * 1024 / (((b + 15) / 16 * 16 + 1279) / 1280 * 1280)); };
        const int mf = p->tune_multi_flip;
        r.mf_marks = 0;
        // FC_FLAG_NB_PAIRS runs take the one-flip-at-a-time commit: the multi-flip pass counts
        // |B| as nodes only (its pair count would cost the C5 instance the register that keeps
        // three waves per SIMD)
        if (r.dgraph && mf != -1 && !nb_pairs) {
            // exact marks (a byte per node) when they cost no residency, else the hashed set
            const bool fits = per_cu(base_b + r.npad) >= per_cu(base_b + hb_bytes(R));
            r.mf_marks = mf == 2 ? 1 : mf == 3 ? 2 : (fits ? 2 : 1);
        }
        r.chain_lds_bytes = base_b + (r.mf_marks == 2 ? r.npad : r.mf_marks == 1 ? hb_bytes(R) : 0);
    }
    // PAIR slot bound: fc_params.wmax > 0 fixes it; otherwise the canonical stream's bound is
    // the state's largest foreign-district count (kept on the device, wmax = 0)
    r.wmax = 1;
    if (k > 2) r.wmax = p->wmax > 0 ? p->wmax : 0;
    if (k > 2 && p->wmax > 0 && p->wmax < std::min(g.max_degree, k - 1))  // would skew the proposal
        return bad(err, FC_ERR_ARG, "fc_run_create: a fixed PAIR slot bound (wmax) must be >= min(max degree, k - 1) = " +
                                    std::to_string(std::min(g.max_degree, k - 1)) + " (<= 0: the canonical dynamic bound)");
#ifdef FC_PHASE_PROF
    r.chain_lds_bytes += kProfSlots * 8;  // phase-cycle accumulators (diagnostic build)
#endif
    r.chain_lds_bytes = (r.chain_lds_bytes + 15) & ~15;
    if ((size_t)r.chain_lds_bytes * waves_per_block(r.chain_lds_bytes) > 160 * 1024)
        return bad(err, FC_ERR_UNSUPPORTED, "fc_run_create: graph too large for the wave-per-chain LDS layout");
    return FC_OK;
}

// ---- launch tuning (scheduling only; 0 = default) --------------------------------------
// k = 2 node stream: a window of up to 64 * nsub = 256 draws per batch (the four node words
// of one Philox call per lane), closed by the 64th boundary hit -- no round cut-off (the band
// stream keeps rounds of 64 with the hit_stop cut-off).  Before round 4, C2 sweeps on one MI355X, ms per launch: before stale slots were re-evaluated
// in place, 2 rounds / 32 hits 10.7, 4 / 12 10.3 (4 / 8 10.55, 4 / 24 10.8); with the
// re-evaluation, 4 / 12 9.33, 4 / 20..64 8.9-9.0, 2 / 32 10.3, 8 / 32..64 9.45-9.55
int plan_tune(const HostGraph &g, const fc_params *p, RunPlan &r, std::string &err) {
    const int32_t k = p->k;
    const bool recom = p->proposal == FC_PROPOSE_RECOM;
    auto &t = r.tune;
    // k > 2 (one MI355X, 2000-step launches): C3 (wmax 3) 1.80 / 2.14 / 2.09e9 proposals/s with
    // 1 / 2 / 4 rounds, C4 (wmax 6) 6.6 / 7.9 / 7.6e8, C5 (wmax 16, ~39 draws per
    // proposal) 3.0 / 4.1 / 4.8e8
    const int wmax_k = k > 2 ? (p->wmax > 0 ? p->wmax : std::max(1, std::min(g.max_degree, k - 1))) : 1;
    t.nsub = p->tune_nsub ? p->tune_nsub : (k == 2 ? 4 : wmax_k > 8 ? 4 : 2);
    if (!recom && !(t.nsub == 1 || t.nsub == 2 || t.nsub == 4))
        return bad(err, FC_ERR_ARG, std::string("fc_run_create: tune_nsub must be 1, 2 or 4 for the ") +
                                    (k == 2 ? "k = 2" : "k > 2") + " kernel (got " + std::to_string(t.nsub) + ")");
    // the round cut-off applies to the k > 2 rounds and the k = 2 band stream; the k = 2 node
    // stream takes a window of 64 * nsub draws (four node words per lane's Philox call)
    // closed by the 64th hit, so a cut-off there would silently change nothing
    if (k == 2 && !recom && p->stream == FC_STREAM_NODE && p->tune_hit_stop != 0)
        return bad(err, FC_ERR_ARG, "fc_run_create: tune_hit_stop has no effect on the k = 2 node stream (its batch window "
                                "is 64 * tune_nsub draws, closed by the 64th boundary hit); leave it 0");
    t.hit_stop = p->tune_hit_stop ? p->tune_hit_stop : 32;
    if (t.hit_stop < 1) return bad(err, FC_ERR_ARG, "fc_run_create: tune_hit_stop must be >= 1");
    t.par_min = p->tune_par_min ? p->tune_par_min : 3;
    if (t.par_min < 1) return bad(err, FC_ERR_ARG, "fc_run_create: tune_par_min must be >= 1");
    // k > 2 with the district-graph rule: commit several independent flips per pass (64 /
    // RMAX of them).  Auto (0) = on (C4 +32 %, C3 +3.5 %)
    if (p->tune_multi_flip < -1 || p->tune_multi_flip > 3)
        return bad(err, FC_ERR_ARG, "fc_run_create: tune_multi_flip must be 0 (auto), 1 (on), -1 (off), 2 (on, hashed "
                                "marks) or 3 (on, exact marks)");
    t.multi = p->tune_multi_flip != -1;
    const int qmax = k == 2 ? kWaitQ : kWaitQK;
    t.wait_q = p->tune_wait_queue ? p->tune_wait_queue : qmax;
    if (t.wait_q < 1 || t.wait_q > qmax)
        return bad(err, FC_ERR_ARG, "fc_run_create: tune_wait_queue must be in [1, " + std::to_string(qmax) + "]");
    t.wpb = p->tune_chains_per_block ? p->tune_chains_per_block : 1;
    if (t.wpb != 1 && t.wpb != 2 && t.wpb != 4)
        return bad(err, FC_ERR_ARG, "fc_run_create: tune_chains_per_block must be 1, 2 or 4");
    t.wpb = std::min(t.wpb, waves_per_block(r.chain_lds_bytes));
    // k = 2, 8-cell rings: the ring verdicts from a table of (ring class, ring bits) when the graph
    // has at most this many classes (fc_ring_table.h; 256 entries of 2 B per class).  0: no table
    // (fc_params_init sets the default, 64 classes = 32 KB: the hot rows stay in the vector L1)
    t.ring_table = p->tune_ring_table;
    if (t.ring_table < 0 || t.ring_table > kRingTableMaxClasses)
        return bad(err, FC_ERR_ARG, "fc_run_create: tune_ring_table must be in [0, " + std::to_string(kRingTableMaxClasses) +
                                    "] (0: no table)");
    // large k > 2 chains that need the search: 4 = one chain per 256-thread workgroup,
    // searched by all of it.  Default 1: the workgroup's helper waves carry the kernel's
    // VGPR count, so a chain then holds four waves' registers and fewer chains are
    // resident, and these searches are short (≈ 2 levels from the C4 / C5 start plans):
    // C4 forced search 5.7 ms (1 wave) against 7.3 ms (workgroup), C5 7.9 against 16.8,
    // C5 without positions 11.7 against 28.1 (1024 chains x 1000 steps, one MI355X)
    const int sw = p->tune_search_waves ? p->tune_search_waves : 1;
    if (sw != 1 && sw != 4) return bad(err, FC_ERR_ARG, "fc_run_create: tune_search_waves must be 1 or 4");
    t.coop = !recom && k > 2 && !r.dgraph && r.chain_lds_bytes > kBigChainLds && sw == 4;
    if (t.coop) r.chain_lds_bytes += 32 * 4;  // control words of the cooperative search
    // k = 2: chains with a short boundary need many draws per proposal and set the launch
    // time; they get the SIMD's issue priority over the chains sharing it (s_setprio 1/2/3
    // below |B| = n/2, n/5, n/10); once a chain has taken 1/16 of its steps, its projected
    // finish against the previous launch's slowest chain sets the priority instead
    const bool div_default = !p->tune_prio_div[0] && !p->tune_prio_div[1] && !p->tune_prio_div[2];
    for (int i = 0; i < 3; ++i) t.prio_div[i] = div_default ? (i == 0 ? 2 : i == 1 ? 5 : 10) : p->tune_prio_div[i];
    if (t.prio_div[0] > 0 && (t.prio_div[1] <= 0 || t.prio_div[2] <= 0))
        return bad(err, FC_ERR_ARG, "fc_run_create: tune_prio_div needs three positive divisors (or [0] < 0: off)");
    // k = 2: deal chains to SIMDs by the previous launch's draws (fc_deal.hip).  Off by
    // default: C2's dispatch order already gives every SIMD one or two of its slow chains
    // (chain dealing)
    t.deal = p->tune_deal ? p->tune_deal : -1;
    if (t.deal != 1 && t.deal != -1) return bad(err, FC_ERR_ARG, "fc_run_create: tune_deal must be 1 or -1");
    t.deal = t.deal > 0 && k == 2 && !recom;
    const bool th_default = p->tune_prio_th[0] == 0.0f && p->tune_prio_th[1] == 0.0f && p->tune_prio_th[2] == 0.0f;
    const float th0[3] = {0.95f, 1.0f, 1.05f};  // tools/archive/gpu_knobs_r04.sh: 55.3 against 55.8 ms at {0.9, 1.0, 1.1}
    for (int i = 0; i < 3; ++i) t.prio_th[i] = th_default ? th0[i] : p->tune_prio_th[i];
    return FC_OK;
}

// the upload vectors, sized and zeroed (init_chain fills chain c's part of each)
void size_state(const HostGraph &g, const fc_params *p, RunPlan &r) {
    const int32_t n = g.n, E = g.n_edges, R = g.ring_max, k = p->k;
    const size_t C = (size_t)r.n_chains;
    const bool recom = p->proposal == FC_PROPOSE_RECOM;
    r.assign.assign(C * r.npad, 0);
    r.fcnt.assign(C * r.npad, 0);
    r.sc.resize(C);
    r.popk.assign(C * kMaxKGeneral, 0);
    r.nfh.assign(k > 2 && !recom ? C * kNfh : 0, 0);
    r.sbits.assign(p->stream == FC_STREAM_BAND ? C * r.words : 0, 0);
    r.mcnt.assign(r.dgraph ? C * k * k : 0, 0);
    r.ngk.assign(r.dgraph ? C * 32 : 0, 0);
    r.thresh.resize(C * (2 * R + 1));
    if (p->diag_mask & FC_DIAG_HIST) { r.cut_hist.assign(C * (E + 1), 0); r.nb_hist.assign(C * r.nb_w, 0); }
    if (p->diag_mask & FC_DIAG_FLIPS) r.part_sum.assign(C * n, 0);
}

// ---- host-side initial state (validated like MarkovChain.__init__ [gc-0.2]) ---------
// chain c's part of every upload vector; q / seen: the contiguity search's scratch
int init_chain(const HostGraph &g, const fc_params *p, int32_t c, const int8_t *a, double base, RunPlan &r,
               std::vector<int32_t> &q, std::vector<uint8_t> &seen, std::string &err) {
    const int32_t n = g.n, E = g.n_edges, R = g.ring_max, k = p->k, nbw = r.nb_w;
    const bool recom = p->proposal == FC_PROPOSE_RECOM, band = p->stream == FC_STREAM_BAND;
    const bool nb_pairs = (p->flags & FC_FLAG_NB_PAIRS) && k > 2;
    const bool want_hist = p->diag_mask & FC_DIAG_HIST, want_flips = p->diag_mask & FC_DIAG_FLIPS;
    const uint32_t con_valid = r.p.con_valid;
    const std::vector<int64_t> &pop_bounds = r.pop_bounds;
    std::memcpy(&r.assign[(size_t)c * r.npad], a, n);
    int64_t pops[kMaxKGeneral] = {0};
    int32_t ng[kMaxKGeneral] = {0};
    for (int32_t u = 0; u < n; ++u) {
        if (a[u] < 0 || a[u] >= k)
            return bad(err, FC_ERR_ARG, "chain " + std::to_string(c) + ": district id out of range [0, k)");
        pops[a[u]] += g.pop[u];
        if (g.meta[u] & kMetaGamma) ng[a[u]] += 1;
    }
    if (con_valid & FC_CON_POP)
        for (int d = 0; d < k; ++d)
            if (pops[d] < pop_bounds[2 * (size_t)c] || pops[d] > pop_bounds[2 * (size_t)c + 1])
                return bad(err, FC_ERR_INVALID_STATE, "chain " + std::to_string(c) +
                                                      ": The given initial_state is not valid according is_valid (population).");
    if ((con_valid & FC_CON_BOUNDARY) && (ng[0] == 0 || ng[1] == 0))
        return bad(err, FC_ERR_INVALID_STATE, "chain " + std::to_string(c) +
                                              ": The given initial_state is not valid according is_valid (boundary_condition).");
    if (!district_contiguous(g, a, k, q, seen))
        return bad(err, FC_ERR_INVALID_STATE, "chain " + std::to_string(c) +
                                              ": The given initial_state is not valid according is_valid (contiguity).");
    int32_t cut = 0, nb = 0;
    for (int32_t e = 0; e < E; ++e) cut += a[g.eu[e]] != a[g.ev[e]];
    for (int32_t u = 0; u < n; ++u) {
        // k = 2: foreign neighbours; k > 2: foreign districts nf(u) (the PAIR slot count)
        int32_t f = 0;
        uint32_t dm = 0;
        for (int32_t j = g.row_ptr[u]; j < g.row_ptr[u + 1]; ++j) {
            f += a[g.col_idx[j]] != a[u];
            if (a[g.col_idx[j]] != a[u]) dm |= 1u << a[g.col_idx[j]];
        }
        if (k > 2 && !recom) {
            f = __builtin_popcount(dm);
            r.nfh[(size_t)c * kNfh + f] += 1;
        }
        r.fcnt[(size_t)c * r.npad + u] = (uint8_t)f;
        nb += nb_pairs ? f : f > 0;
    }
    if (band) {  // the band S of the initial state: b_nodes and their neighbours
        uint64_t *sb = &r.sbits[(size_t)c * r.words];
        for (int32_t u = 0; u < n; ++u) {
            if (!r.fcnt[(size_t)c * r.npad + u]) continue;
            sb[u >> 6] |= 1ull << (u & 63);
            for (int32_t j = g.row_ptr[u]; j < g.row_ptr[u + 1]; ++j) sb[g.col_idx[j] >> 6] |= 1ull << (g.col_idx[j] & 63);
        }
    }
    ChainScalars &s = r.sc[c];
    std::memset(&s, 0, sizeof s);
    s.cut = cut;
    s.nb = nb;
    s.pops[0] = (int32_t)pops[0];
    s.pops[1] = (int32_t)pops[1];
    for (int d = 0; d < kMaxKGeneral; ++d) r.popk[(size_t)c * kMaxKGeneral + d] = (int32_t)pops[d];
    if (r.dgraph) {
        // face-adjacent cell pairs {u, w} (w in ring(u), counted once: u < w) per district pair
        int32_t *mc = &r.mcnt[(size_t)c * k * k];
        for (int32_t u = 0; u < n; ++u) {
            const int32_t L = (int32_t)(g.meta[u] & kMetaLenMask);
            for (int32_t j = 0; j < L; ++j) {
                const int32_t w = g.ring[(size_t)u * R + j];
                if (w <= u || a[w] == a[u]) continue;
                const int32_t X = std::min(a[u], a[w]), Y = std::max(a[u], a[w]);
                ++mc[X * k + Y];
            }
        }
        for (int d = 0; d < k; ++d) r.ngk[(size_t)c * 32 + d] = ng[d];
    }
    s.ngamma[0] = ng[0];
    s.ngamma[1] = ng[1];
    s.last_flip = -1;
    s.pop_lo = (int32_t)pop_bounds[2 * (size_t)c];
    s.pop_hi = (int32_t)pop_bounds[2 * (size_t)c + 1];
    int64_t wait0 = 0;
    if (p->diag_mask & FC_DIAG_WAIT) {
        const uint32_t gid = p->chain_id_offset + (uint32_t)c;
        Words4 w = philox4x32_10(0u, 0u, gid, 2u, (uint32_t)p->seed, (uint32_t)(p->seed >> 32));
        wait0 = geom_from(u53(w.x0, w.x1), r.log1mp[nb]);
    }
    s.wait_cur = wait0;
    s.hit_time = (cut >= p->hit_lo && cut <= p->hit_hi) ? 0 : -1;
    s.ser_t0 = 0;
    s.ser_cut0 = cut;
    s.ser_nb0 = nb;
    // yield #0 (the initial state) enters every per-yield sum
    s.sum_cut = cut;
    s.sum_nb = nb;
    s.sum_cut2 = (int64_t)cut * cut;
    s.sum_nb2 = (int64_t)nb * nb;
    s.sum_wait = wait0;
    if (want_hist) {
        r.cut_hist[(size_t)c * (E + 1) + cut] = 1;
        r.nb_hist[(size_t)c * nbw + nb] = 1;
    }
    if (want_flips)
        for (int32_t u = 0; u < n; ++u) r.part_sum[(size_t)c * n + u] = r.labels[a[u]];  // :219
    for (int dd = -R; dd <= R; ++dd) {
        if (p->accept == FC_ACCEPT_ANNEAL) {
            // annealing_cut_accept_backwards, :99: base ** (beta * (-(cut' - cut))); the
            // |B'| / |B| factor is applied on the device (the table holds the double)
            const double bw = std::pow(base, p->beta * (double)(-dd));
            uint64_t t;
            std::memcpy(&t, &bw, 8);
            r.thresh[(size_t)c * (2 * R + 1) + (dd + R)] = t;
            continue;
        }
        // cut_accept: random() < base ** (-(cut' - cut)), grid_chain_sec11.py:175,179
        r.thresh[(size_t)c * (2 * R + 1) + (dd + R)] = u53_threshold(std::pow(base, (double)(-dd)));
    }
    return FC_OK;
}

// every parameter a trajectory depends on besides seed / chain ids, for fc_run_restore
uint64_t hash_params(const fc_params *p, const double *bases, const RunPlan &r) {
    uint64_t h = kFnvBasis;
    h = fnv1a(h, r.thresh.data(), r.thresh.size() * 8);
    h = fnv1a(h, r.pop_bounds.data(), r.pop_bounds.size() * 8);
    h = fnv1a(h, r.labels.data(), r.labels.size() * 4);
    h = fnv1a(h, r.log1mp.data(), r.log1mp.size() * 8);
    const int64_t scal[] = {p->k, p->proposal, p->accept, (int64_t)r.p.con_valid, (int64_t)p->con_accept, p->flags,
                            r.wmax, p->hit_lo, p->hit_hi, p->recom_node_repeats, p->recom_max_attempts,
                            p->stream};
    h = fnv1a(h, scal, sizeof scal);
    const double dscal[] = {p->beta, p->recom_pop_target, p->recom_epsilon, bases ? bases[0] : p->base};
    h = fnv1a(h, dscal, sizeof dscal);
    if (p->n_frozen > 0) h = fnv1a(h, p->frozen, (size_t)p->n_frozen * 4);
    return h;
}

void recom_tables(const HostGraph &g, double base, RunPlan &r) {
    const int32_t E = g.n_edges;
    neighbour_rows(g, r.nb_d, r.nbe, r.eslot);
    // cut_accept: random() < base ** (cut - cut'), cut - cut' in [-E, E]
    r.recom_thresh.resize(2 * (size_t)E + 1);
    for (int32_t dd = -E; dd <= E; ++dd) r.recom_thresh[dd + E] = u53_threshold(std::pow(base, (double)dd));
}

}  // namespace

void neighbour_rows(const HostGraph &g, int32_t &nb_d, std::vector<uint32_t> &nbe, std::vector<uint32_t> &eslot) {
    const int32_t n = g.n, E = g.n_edges;
    // the neighbours of each node in ring order with their edge ids (node ids and edge ids
    // < 65535: n <= 8000, degree <= 16), and each edge end's index in the other end's row:
    // the spanning-tree scan reads one row per node instead of its ring and ring edge ids
    const int R = g.ring_max;
    nb_d = std::max(4, (g.max_degree + 3) / 4 * 4);
    nbe.assign((size_t)n * nb_d, ~0u);
    eslot.assign((size_t)std::max(E, 1), 0u);
    for (int32_t x = 0; x < n; ++x) {
        int k = 0;
        for (int j = 0; j < R; ++j) {
            const int32_t e = g.ring_eid[(size_t)x * R + j];
            if (e < 0) continue;
            nbe[(size_t)x * nb_d + k] = (uint32_t)g.ring[(size_t)x * R + j] | ((uint32_t)e << 16);
            eslot[e] |= (uint32_t)k << (g.eu[e] == x ? 0 : 8);
            ++k;
        }
    }
}

int plan_seed(const HostGraph &g, const fc_seed_params &p, int32_t n_plans, SeedPlan &s, std::string &err) {
    const std::string w = "fc_graph_seed_plans: ";
    if (p.struct_size != sizeof(fc_seed_params) || p.abi_version != FC_ABI_VERSION)
        return bad(err, FC_ERR_ARG, w + "fc_seed_params.struct_size " + std::to_string(p.struct_size) + " / abi_version " +
                                    std::to_string(p.abi_version) + " do not match this library (" +
                                    std::to_string(sizeof(fc_seed_params)) + " / " + std::to_string(FC_ABI_VERSION) +
                                    "): set them with fc_seed_params_init");
    if (n_plans < 0) return bad(err, FC_ERR_ARG, w + "n_plans must be >= 0");
    if (p.k < 2 || p.k > kMaxKGeneral) return bad(err, FC_ERR_ARG, w + "k must be in [2, 32]");
    if (p.pop_lo > p.pop_hi)
        return bad(err, FC_ERR_ARG, w + "pop_lo " + std::to_string(p.pop_lo) + " > pop_hi " + std::to_string(p.pop_hi));
    if (p.node_repeats < 0 || p.max_attempts < 0 || p.max_restarts < 0)
        return bad(err, FC_ERR_ARG, w + "node_repeats, max_attempts and max_restarts must be >= 0 (0: the default)");
    if (p.max_restarts >= (1 << 24))  // the attempt is bits 8..31 of the draw index
        return bad(err, FC_ERR_ARG, w + "max_restarts must be below 2^24");
    if (g.n > 8000)
        return bad(err, FC_ERR_UNSUPPORTED, w + "seed plans keep a plan's spanning tree in LDS (n <= 8000)");
    int64_t total = 0;
    for (int32_t u = 0; u < g.n; ++u) {
        if (g.pop[u] < 0) return bad(err, FC_ERR_UNSUPPORTED, w + "node populations must be >= 0");
        total += g.pop[u];
    }
    // fc_seed.hip sums subtree populations in int32 and marks the subset in bit 31, as fc_recom.hip does
    if (total > INT32_MAX)
        return bad(err, FC_ERR_UNSUPPORTED, w + "seed plans sum subtree populations in 31 bits (population total " +
                                            std::to_string(total) + " exceeds INT32_MAX = 2147483647)");
    if (g.max_degree > 16) return bad(err, FC_ERR_UNSUPPORTED, w + "node degree above 16");
    if (!g.connected) return bad(err, FC_ERR_UNSUPPORTED, w + "the graph must be connected");
    // k districts inside [lo, hi] must be able to hold the total (bounds beyond the total are
    // clipped first, so that the products stay in int64)
    const int64_t lo = std::max<int64_t>(p.pop_lo, -1), hi = std::min<int64_t>(p.pop_hi, total);
    if (lo > total || (int64_t)p.k * lo > total)
        return bad(err, FC_ERR_ARG, w + "k * pop_lo = " + std::to_string(p.k) + " * " + std::to_string(p.pop_lo) +
                                    " exceeds the population total " + std::to_string(total));
    if (hi < 0 || (int64_t)p.k * hi < total)
        return bad(err, FC_ERR_ARG, w + "k * pop_hi = " + std::to_string(p.k) + " * " + std::to_string(p.pop_hi) +
                                    " is below the population total " + std::to_string(total));
    s.p = p;
    // (a bound outside [0, total] admits what the clipped one admits: populations are in [0, total])
    s.p.pop_lo = std::max<int64_t>(p.pop_lo, 0);
    s.p.pop_hi = hi;
    s.p.node_repeats = p.node_repeats > 0 ? p.node_repeats : 1;
    s.p.max_attempts = p.max_attempts > 0 ? p.max_attempts : 256;
    s.p.max_restarts = p.max_restarts > 0 ? p.max_restarts : 16;
    s.pop_total = total;
    s.npad = (g.n + 15) & ~15;
    s.chain_lds_bytes = ((int32_t)recom_lds<size_t>(0, s.npad, g.ring_max).end + 15) & ~15;
    s.node_recs = g.ring_max == 8 ? pack_records<8>(g, nullptr, 0) : pack_records<16>(g, nullptr, 0);
    neighbour_rows(g, s.nb_d, s.nbe, s.eslot);
    return FC_OK;
}

int plan_run(const HostGraph &g, const fc_params &params, int32_t n_chains, const int8_t *init_assign,
             const double *bases, RunPlan &plan, std::string &err) {
    const fc_params *p = &params;
    plan = RunPlan{};
    if (int rc = check_params(g, p, n_chains, bases, err)) return rc;
    if (int rc = plan_tables(g, p, n_chains, init_assign, bases, plan, err)) return rc;
    if (int rc = plan_lds(g, p, plan, err)) return rc;
    if (int rc = plan_tune(g, p, plan, err)) return rc;
    size_state(g, p, plan);
    std::vector<int32_t> q;
    std::vector<uint8_t> seen(g.n);
    for (int32_t c = 0; c < n_chains; ++c)
        if (int rc = init_chain(g, p, c, init_assign + (size_t)c * g.n, bases ? bases[c] : p->base, plan, q, seen, err))
            return rc;
    plan.param_hash = hash_params(p, bases, plan);
    plan.node_recs = g.ring_max == 8 ? pack_records<8>(g, p->frozen, p->n_frozen) : pack_records<16>(g, p->frozen, p->n_frozen);
    plan.nbr4 = true;
    for (uint64_t m : g.meta) plan.nbr4 = plan.nbr4 && __builtin_popcount((uint32_t)(m >> kMetaNbrShift) & 0xffffu) <= 4;
    // k = 2 flips on 8-cell rings: the ring verdicts as a table per class of node (fc_ring_table.h).  A
    // function of the graph alone; the records of such a run carry each node's class above its degree
    // (only the k > 2 kernel reads the degree, and its runs get the plain records)
    if (p->k == 2 && p->proposal != FC_PROPOSE_RECOM && g.ring_max == kRingTableRmax) {
        std::vector<uint16_t> cls;
        // (the kernel reads the table in its neighbour-list body only: none for a graph that takes the other)
        plan.ring_classes = build_ring_table(g.meta.data(), g.n, plan.nbr4 ? plan.tune.ring_table : 0, cls, plan.ring_table);
        plan.ring_table_on = !plan.ring_table.empty();
        if (plan.ring_table_on) {
            for (int32_t v = 0; v < g.n; ++v) {
                unsigned char *at = plan.node_recs.data() + (size_t)v * sizeof(NodeRec<8>) + offsetof(NodeRec<8>, deg);
                int32_t deg;
                std::memcpy(&deg, at, sizeof deg);
                deg |= (int32_t)cls[v] << 16;
                std::memcpy(at, &deg, sizeof deg);
            }
        }
    }
    if (p->proposal == FC_PROPOSE_RECOM) recom_tables(g, bases ? bases[0] : p->base, plan);
    // the event log (FC_DIAG_SERIES with a capacity) and the traced chains
    if ((p->diag_mask & FC_DIAG_SERIES) && p->event_cap > 0)
        plan.ev_cap = p->event_cap;
    else
        plan.p.diag_mask &= ~FC_DIAG_SERIES;
    plan.p.trace_chains = p->trace_chains > 0 && p->trace_cap > 0 ? std::min(p->trace_chains, n_chains) : 0;
    return FC_OK;
}

InstanceFacts instance_facts(const HostGraph &g, const RunShape &r, bool tape, bool trace) {
    // (line for line with the struct)
    return {r.p.proposal == FC_PROPOSE_RECOM ? Family::kRecom : r.p.k == 2 ? Family::kFlip2 : Family::kFlipK,
            g.ring_max, r.tune.nsub,
            tape, trace, r.p.hit_lo <= r.p.hit_hi,
            r.p.diag_mask, r.p.flags,
            r.variant, g.n_exact == g.n, r.p.stream == FC_STREAM_BAND,
            r.tune.coop != 0, r.dgraph, r.tune.multi != 0,
            r.mf_marks,
            r.ev_cap > 0};
}

}  // namespace fc
