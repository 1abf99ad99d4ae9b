// The series window of a replay of the FC_DIAG_SERIES event logs (DESIGN.md §4 "Series window"):
// what every pass over the logs of chains [c0, c0 + nc) needs.
//
// One convention: the per-chain arrays hold [nc] entries and are indexed by the call-local chain
// cl = c - c0; a0 and events are the run's and are indexed by the global chain c = c0 + cl.  A pass
// replays min(ev_len, ev_cap) events of a chain.
//
// Two passes (fc_shapes.hip, fc_heat.hip) also walk host-built neighbour rows: RowSlot, row_width
// and build_rows below are theirs.  The device side of a replay is in fc_replay_dev.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/flipchain.h"

namespace fc {

struct LogWindow {
    const int8_t *a0;         // [n_chains * npad] assignment at the series window start
    int32_t npad, n, k;
    const fc_event *events;   // [n_chains * ev_cap]
    int64_t ev_cap;
    const int64_t *ev_len;    // [nc] events of chain c0 + cl
    const int64_t *t0;        // [nc] first yield of the window
    const int64_t *t_end;     // [nc] last yield of the window + 1
    int32_t c0, nc;
};

// A slot of a node's neighbour row: the neighbour's id (-1: empty) and the pass's value of the
// edge to it (the length shared, the edge's canonical id)
struct alignas(8) RowSlot {
    int32_t nbr, val;
};

// Slots per neighbour row for a graph of this maximum degree (the kernels' instances), 0: none
inline int32_t row_width(int32_t max_degree) { return max_degree <= 8 ? 8 : max_degree <= 16 ? 16 : 0; }

// The neighbour rows: every canonical edge e = (eu[e], ev[e]) in the rows of both its ends, in
// edge order, with the value edge_val[e] (null: e itself); an empty slot holds `empty`.
// width >= the maximum degree.  HIP-free host code.
inline void build_rows(int32_t n, int32_t n_edges, const int32_t *eu, const int32_t *ev, int32_t width,
                       const int32_t *edge_val, int32_t empty, std::vector<RowSlot> &rows) {
    rows.assign((size_t)n * width, RowSlot{-1, empty});
    std::vector<int32_t> fill((size_t)n, 0);
    for (int32_t e = 0; e < n_edges; ++e) {
        const int32_t u = eu[e], w = ev[e], x = edge_val ? edge_val[e] : e;
        rows[(size_t)u * width + fill[u]++] = RowSlot{w, x};
        rows[(size_t)w * width + fill[w]++] = RowSlot{u, x};
    }
}

}  // namespace fc
