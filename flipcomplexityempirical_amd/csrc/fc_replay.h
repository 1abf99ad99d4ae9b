// The series window of a replay of the FC_DIAG_SERIES event logs (DESIGN.md §4 "Series window"):
// what every pass over the logs of chains [c0, c0 + nc) needs.
//
// One convention: the per-chain arrays hold [nc] entries and are indexed by the call-local chain
// cl = c - c0; a0 and events are the run's and are indexed by the global chain c = c0 + cl.  A pass
// replays min(ev_len, ev_cap) events of a chain.
#pragma once
#include <stdint.h>

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

}  // namespace fc
