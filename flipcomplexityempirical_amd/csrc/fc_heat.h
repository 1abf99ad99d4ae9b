// Heat-map series: the parameters of the kernel that replays the FC_DIAG_SERIES
// event logs into the reference's heat maps over the series window (fc_heat.hip) -- the |cut| and
// |B| histograms, per-edge cut times, per-node move counts, last moves and district dwell times --
// and the layout of a chain's image.  The neighbour / edge rows the kernel walks are fc_replay.h's
// (build_rows with the edge's canonical id as the value, -1 in an empty slot).
//
// a_t is the window-start assignment with every logged event of t_e <= t applied in log order.
// Every per-edge and per-node integral is kept lazily (DESIGN.md §4 "cut_times"): an event at
// yield t that turns edge e uncut adds +t, one that turns it cut adds -t, and the close adds
// t_end for an edge cut at the end and -t0 for one cut at the start; dwell[u][d] takes +t when u
// leaves d and -t when it enters.  The toggles inside a burst (events of one t) cancel.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fc_philox.h"  // FC_HD
#include "fc_replay.h"

namespace fc {

// The outputs of a call, as bits of the mask heat_lds_bytes takes, in the entry point's order
enum : uint32_t { kHeatCutHist = 1u, kHeatNbHist = 2u, kHeatCutTimes = 4u, kHeatMoves = 8u, kHeatLastMove = 16u,
                  kHeatDwell = 32u };
constexpr int kHeatArrays = 6;
// The accumulation forms (fc_run_heat_series_info)
constexpr int32_t kHeatFormLds = 0, kHeatFormGlobal = 1;

// Kernel parameters (passed by value).  Output rows are per chain of the call, [nc] rows each; a
// null output is skipped.
struct HeatParams {
    LogWindow log;             // the chains read and their window (fc_replay.h)
    const RowSlot *rows;       // [n * width] neighbour rows: the edge's canonical id, -1 in an empty slot
    int32_t width;             // slots per row: 8 or 16
    int32_t n_edges;           // E
    int32_t nb_width;          // entries of an |B| histogram row
    const int64_t *cut0, *nb0; // [nc] |cut| and |B| at the window start
    int64_t *cut_hist;         // [nc * (E + 1)]
    int64_t *nb_hist;          // [nc * nb_width]
    int64_t *cut_times;        // [nc * E]
    int64_t *moves, *last_move; // [nc * n]
    int64_t *dwell;            // [nc * n * k]
};

// int64 entries of output `a` (0 .. 5) per chain
FC_HD size_t heat_row_len(int a, int32_t n, int32_t k, int32_t n_edges, int32_t nb_width) {
    return a == 0 ? (size_t)n_edges + 1 : a == 1 ? (size_t)nb_width : a == 2 ? (size_t)n_edges
         : a == 5 ? (size_t)n * (size_t)k : (size_t)n;
}

// LDS bytes of the part both forms keep: the chunk's neighbour rows [64][width] and the current
// assignment (npad is a multiple of 16)
FC_HD size_t heat_base_bytes(int32_t npad, int32_t width) {
    return sizeof(RowSlot) * 64 * (size_t)width + (((size_t)npad + 15) & ~(size_t)15);
}
// LDS bytes of a chain's image in the LDS form: the base, then every requested array (mask) in
// the entry point's order, each padded to 16 bytes
FC_HD size_t heat_lds_bytes(int32_t npad, int32_t n, int32_t k, int32_t n_edges, int32_t nb_width, int32_t width,
                            uint32_t mask) {
    size_t b = heat_base_bytes(npad, width);
    for (int a = 0; a < kHeatArrays; ++a)
        if ((mask >> a) & 1u) b += (8 * heat_row_len(a, n, k, n_edges, nb_width) + 15) & ~(size_t)15;
    return b;
}

// One 64-thread workgroup per chain of [c0, c0 + nc); `form` kHeatFormLds needs
// heat_lds_bytes(...) of dynamic LDS, kHeatFormGlobal heat_base_bytes(...).  Returns a hipError_t
// as int.
int launch_heat(const HeatParams &p, int32_t form, void *stream);

}  // namespace fc
