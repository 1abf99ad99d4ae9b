// Host-side planning of a run (fc_plan.cpp): everything fc_run_create decides before it touches
// the device -- parameter checks, the LDS layout, launch tuning, every chain's validated initial
// state and the tables that are then uploaded.  Plain C++: no HIP header here or in fc_plan.cpp,
// so the host sanitizer harness (tests/sanitize/) drives it without a GPU.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "fc_internal.h"

namespace fc {

// FNV-1a over a byte range (checkpoint parameter hash, ladder layout, frame tables)
inline uint64_t fnv1a(uint64_t h, const void *data, size_t bytes) {
    const unsigned char *b = (const unsigned char *)data;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}
constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull;

// fc_params.tune_* with the defaults filled in
struct RunTune {
    int32_t nsub, hit_stop, par_min, wait_q, wpb, coop, deal, multi;
    int32_t ring_table;      // k = 2: most ring classes a lookup table is built for (0: none)
    int32_t prio_div[3];     // prio_div[0] <= 0: priorities off
    float prio_th[3];
};

// What a run keeps of its plan for its lifetime (struct fc_run derives from it).
struct RunShape {
    fc_params p{};      // the caller's, with its pointers nulled, con_valid resolved, FC_DIAG_SERIES
                        // cleared when no event log is kept and trace_chains clipped to n_chains
    std::vector<int32_t> labels;
    std::vector<double> log1mp;
    int32_t nb_w = 0;   // entries of the |B| histogram / log(1 - p) table: n + 1, or with
                        // FC_FLAG_NB_PAIRS (k > 2) the largest pair count + 1
    int32_t n_chains = 0;
    int32_t npad = 0;
    int32_t words = 0;
    int32_t chain_lds_bytes = 0;
    bool dgraph = false;
    int32_t mf_marks = 0;        // k > 2 multi-flip commit: 0 off, 1 hashed neighbour marks, 2 exact marks
    int32_t wmax = 1;
    int32_t nb_d = 4;            // recom: nbe row length
    int64_t ev_cap = 0;          // FC_DIAG_SERIES: events kept per chain (0: no event log)
    uint64_t param_hash = 0;     // FNV-1a of every trajectory-determining parameter (checkpoint check)
    bool variant = false;        // accept / constraint variants (FULL k = 2 instance)
    bool nbr4 = false;           // no node has more than four neighbours (kFlagNbr4), from the records
    int32_t ring_classes = 0;    // k = 2 flips, 8-cell rings: distinct (length, neighbours, links) of the nodes' rings
    bool ring_table_on = false;  // ... and a verdict table was built for them (kFlagRingTable, fc_ring_table.h)
    RunTune tune{};
    std::vector<double> bases0;        // [n_chains] the base each chain was created with
    std::vector<int64_t> pop_bounds;   // [2 * n_chains]
};

// The plan: the shape plus the host vectors fc_run_create uploads (an empty one: no such buffer).
struct RunPlan : RunShape {
    std::vector<unsigned char> node_recs;  // NodeRec<ring_max>[n], frozen nodes marked; with a ring table, each
                                           // node's class in the upper half of NodeRec::deg
    std::vector<uint16_t> ring_table;      // [ring_classes * 256] RingEntry (fc_ring_table.h); empty: none
    std::vector<int8_t> assign;            // [n_chains * npad]
    std::vector<uint8_t> fcnt;             // [n_chains * npad]
    std::vector<ChainScalars> sc;          // [n_chains]
    std::vector<int32_t> popk;             // [n_chains * kMaxKGeneral]
    std::vector<int32_t> nfh;              // k > 2 flips: [n_chains * kNfh]
    std::vector<uint64_t> sbits;           // band stream: [n_chains * words]
    std::vector<int32_t> mcnt, ngk;        // district-graph rule: [n_chains * k * k], [n_chains * 32]
    std::vector<uint64_t> thresh;          // [n_chains * (2 ring_max + 1)]
    std::vector<int64_t> cut_hist, nb_hist;  // FC_DIAG_HIST: yield #0 counted
    std::vector<int64_t> part_sum;         // FC_DIAG_FLIPS
    std::vector<uint32_t> nbe, eslot;      // recom: neighbour rows, edge ends' row indices
    std::vector<uint64_t> recom_thresh;    // recom: [2E + 1]
};

// Checks `p`, `init_assign` ([n_chains * n] district ids) and `bases` ([n_chains] or null: p.base)
// against `g` and fills `plan`.  Returns FC_OK, or an FC_ERR_* code with its message in `err`.
// `p`, `init_assign` non-null and n_chains > 0 are the caller's to check.
int plan_run(const HostGraph &g, const fc_params &p, int32_t n_chains, const int8_t *init_assign,
             const double *bases, RunPlan &plan, std::string &err);

// What choose_instance (fc_instance.h) reads of a run.  A tape can be set and cleared after creation,
// so fc_run_steps asks at each call: `tape` / `trace`: a replay tape / a trace buffer is set now.
InstanceFacts instance_facts(const HostGraph &g, const RunShape &r, bool tape, bool trace);

// The tables of the spanning-tree kernels (RecomParams / SeedParams nbe, eslot): each node's
// neighbours in ring order with their edge ids, nb_d entries per row, and each edge end's index in
// the other end's row.  A function of the graph: the ReCom plan and the seed plans share it.
void neighbour_rows(const HostGraph &g, int32_t &nb_d, std::vector<uint32_t> &nbe, std::vector<uint32_t> &eslot);

// The host half of fc_graph_seed_plans: the argument checks (FC_OK, or an FC_ERR_* code with its
// message in `err`), the defaults filled in and the bounds clipped to [0, total], the LDS bytes of
// a plan and the tables that are then uploaded.
struct SeedPlan {
    fc_seed_params p{};
    int64_t pop_total = 0;
    int32_t npad = 0, chain_lds_bytes = 0, nb_d = 4;
    std::vector<unsigned char> node_recs;
    std::vector<uint32_t> nbe, eslot;
};
int plan_seed(const HostGraph &g, const fc_seed_params &p, int32_t n_plans, SeedPlan &s, std::string &err);

}  // namespace fc
