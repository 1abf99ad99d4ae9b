// ReCom tree proposal for gfx950: the step the reference builds beside its flip chain
// (grid_chain_sec11.py:328-335, partial(recom, pop_col="population",
// pop_target=ideal_population, epsilon=0.05, node_repeats=1)) under gerrychain 0.2's
// MarkovChain loop [gc-0.2] (Validator re-draws, cut_accept-style acceptance).
//
// One chain per wavefront; the chain's assignment and the spanning-tree working set live
// in LDS.  A proposal:
//   1. picks a cut edge (k-th cut edge in edge-id order: per-lane edge chunks + a wave scan)
//      and merges its two districts M;
//   2. draws a random spanning tree of M: edge weights splitmix64(key + e) >> 32, maximum
//      spanning tree by Boruvka (per-component best edge by LDS atomicMax on
//      weight << 32 | ~e, hooking, pointer jumping);
//   3. roots it at the k-th node of tree degree > 1, orders it by a level-synchronous BFS
//      over the tree and sums subtree populations level by level from the leaves;
//   4. picks the k-th balanced cut (|pop(subtree) - pop_target| < epsilon * pop_target),
//      trying new roots / trees while there is none (node_repeats roots per tree);
//   5. relabels subtree(child) -> parts[0], the rest of M -> parts[1], evaluates the
//      population Validator and the cut_accept test, and applies the accepted state.
// The canonical random stream (recomref.h) makes the trajectory bit-identical to the CPU
// restatement in oracle/recomref.c.
// Subtree populations are int32 with bit 31 as the subset mark (spop): fc_run_create refuses
// a ReCom run on a graph whose population total exceeds INT32_MAX (fc_plan.cpp).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "fc_device.h"
#include "fc_internal.h"
#include "fc_philox.h"
#include "fc_tree_dev.h"

namespace fc {

using namespace dev;

namespace {

// The lean instance (runs without a move log) and the logging one (a run with FC_DIAG_SERIES and
// an event_cap): two entry points over one body, so that a profiler shows which ran and the lean
// one's code does not carry the log.  The log's buffer and capacity are arguments of the logging
// instance alone, after RecomParams: the lean instance's argument layout is what it was.
// The body is text (fc_recom_body.h), not a device function: handing RecomParams to a shared
// function makes the compiler read every field at entry instead of where it is used, which moved
// the lean instance's registers (DESIGN.md "ReCom move log").
template <int RMAX>
__global__ __launch_bounds__(256) void recom_kernel(RecomParams p) {
    constexpr bool LOG = false;
    [[maybe_unused]] fc_event *const events = nullptr;
    [[maybe_unused]] constexpr int64_t ev_cap = 0;
#include "fc_recom_body.h"
}
template <int RMAX>
__global__ __launch_bounds__(256) void recom_log_kernel(RecomParams p, fc_event *events, int64_t ev_cap) {
    constexpr bool LOG = true;
#include "fc_recom_body.h"
}

}  // namespace

int launch_recom(const RecomParams &p, fc_event *events, int64_t ev_cap, const RecomInstance &inst, void *stream,
                 char *name, size_t name_cap) {
    const int wpb = waves_per_block(p.chain_lds_bytes);
    const int blocks = (p.n_chains + wpb - 1) / wpb;
    const size_t lds = (size_t)p.chain_lds_bytes * wpb;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(blocks), block(kWave * wpb);
    const bool ok = with_value<16, 8>(inst.ring, [&](auto r) {  // (the lists' order: fc_device.h with_value)
        return with_value<0, 1>(inst.log, [&](auto l) {
            constexpr int R = decltype(r)::value;
            constexpr bool LOG = decltype(l)::value;
            const RecomInstance built{R, LOG};  // what is launched is what is named
            if (!(built == inst)) return false;
            if (name) format_instance(built, name, name_cap);
            if constexpr (LOG) launch_lds(recom_log_kernel<R>, grid, block, lds, s, p, events, ev_cap);
            else launch_lds(recom_kernel<R>, grid, block, lds, s, p);
            return true;
        });
    });
    if (!ok) return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

}  // namespace fc
