// Which kernel instance a run launches, stated once: the template arguments of the three chain
// kernel families as data, the rule that picks them from what a run holds, and the name rocprofv3
// reports for each.  The split exists so that each hot loop keeps its registers; the
// launchers (fc_flip2.hip, fc_kernels.hip, fc_recom.hip) only map the value chosen here to its
// template instance, and tests/native/instance_check.cpp executes the rule on the CPU.  No HIP.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/flipchain.h"

namespace fc {

struct Flip2Instance { int ring, nsub; bool full, search, xtra, band; };  // flip2_kernel<RMAX, NSUB, FULL, SEARCH, XTRA, BAND>
struct FlipKInstance { int ring, nsub, km; bool full; int mf; };          // flip_kernel<RMAX, NSUB, KM, FULL, MF>
struct RecomInstance { int ring; bool log; };                             // recom_kernel<RMAX> / recom_log_kernel<RMAX>
inline bool operator==(const Flip2Instance &a, const Flip2Instance &b) {
    return a.ring == b.ring && a.nsub == b.nsub && a.full == b.full && a.search == b.search && a.xtra == b.xtra &&
           a.band == b.band;
}
inline bool operator==(const FlipKInstance &a, const FlipKInstance &b) {
    return a.ring == b.ring && a.nsub == b.nsub && a.km == b.km && a.full == b.full && a.mf == b.mf;
}
inline bool operator==(const RecomInstance &a, const RecomInstance &b) { return a.ring == b.ring && a.log == b.log; }

enum class Family { kFlip2, kFlipK, kRecom };  // k = 2 flips, k > 2 flips, tree proposals

// What the choice reads of a run (fc_plan.h instance_facts derives it)
struct InstanceFacts {
    Family family;
    int ring, nsub;                 // the graph's ring width; fc_params.tune_nsub resolved
    bool tape, trace, hit_window;   // a replay tape / a trace buffer is set; hit_lo <= hit_hi
    uint32_t diag, flags;           // FC_DIAG_*, FC_FLAG_*
    bool variant, all_exact, band;  // accept / constraint variants or frozen nodes; the run rule decides every
                                    // node's contiguity; the run has a band bitmap (FC_STREAM_BAND)
    bool coop, dgraph, multi;       // k > 2: workgroup-cooperative search; district-graph rule; tune.multi
    int mf_marks;                   // k > 2: RunShape.mf_marks
    bool log;                       // ReCom: the run keeps a move log (ev_cap > 0)
};
struct Instance { Family family; Flip2Instance flip2; FlipKInstance flipk; RecomInstance recom; };  // family's member is set

// The rule.  False for a ring width other than 8 / 16 or (flip kernels) an nsub other than 1 / 2 / 4.
inline bool choose_instance(const InstanceFacts &f, Instance &out) {
    out = Instance{f.family, {}, {}, {}};
    if (f.ring != 8 && f.ring != 16) return false;
    if (f.family == Family::kRecom) {
        out.recom = {f.ring, f.log};
        return true;
    }
    if (f.nsub != 1 && f.nsub != 2 && f.nsub != 4) return false;
    // FULL: replay tapes, traces, event logs, histograms, per-node/per-edge tallies or a
    // hitting-time window; the lean instance (proposals, steps, sums, waits) keeps its register
    // budget for the hot loop.
    const bool full = f.tape || f.trace || (f.diag & ~(uint32_t)FC_DIAG_WAIT) || f.hit_window;
    if (f.family == Family::kFlip2) {
        // XTRA: replay tapes, traces, accept / constraint variants, frozen nodes (and so FULL)
        const bool xtra = f.tape || f.trace || f.variant;
        // no search code when the run rule decides every proposal (all nodes exact, no forced search)
        const bool search = !f.all_exact || (f.flags & FC_FLAG_FORCE_BFS);
        out.flip2 = {f.ring, f.nsub, full || f.variant, search, xtra, f.band};
        return true;
    }
    // k > 2.  `full` has no variant term: variants are k = 2 only (fc_run_create refuses them
    // otherwise).  KM: 1 cooperative search, 3 district-graph rule (off under FC_FLAG_FORCE_BFS,
    // and coop needs it off), 0 the one-wave search.  MF, the multi-flip commit of the district-rule
    // instance when the run asks for it: 1 hashed marks, 2 exact marks (room for a byte per node)
    const int km = f.coop ? 1 : f.dgraph ? 3 : 0;
    out.flipk = {f.ring, f.nsub, km, full, km == 3 && f.multi ? f.mf_marks : 0};
    return true;
}

// The instance spelled as rocprofv3 reports it
inline void format_instance(const Flip2Instance &i, char *name, size_t cap) {
    auto b = [](bool x) { return x ? "true" : "false"; };
    std::snprintf(name, cap, "fc::flip2_kernel<%d, %d, %s, %s, %s, %s>", i.ring, i.nsub, b(i.full), b(i.search), b(i.xtra),
                  b(i.band));
}
inline void format_instance(const FlipKInstance &i, char *name, size_t cap) {
    std::snprintf(name, cap, "fc::flip_kernel<%d, %d, %d, %s, %d>", i.ring, i.nsub, i.km, i.full ? "true" : "false", i.mf);
}
inline void format_instance(const RecomInstance &i, char *name, size_t cap) {
    std::snprintf(name, cap, i.log ? "fc::recom_log_kernel<%d>" : "fc::recom_kernel<%d>", i.ring);
}

}  // namespace fc
