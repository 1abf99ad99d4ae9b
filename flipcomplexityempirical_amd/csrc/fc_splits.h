// Locality-splits series: the rule by which one node's move changes a locality's
// district count, its split bit and the sum of squared cell sizes, shared by the host entry point
// fc_splits_eval and the replay kernel (fc_splits.hip), and the parameters of that kernel.
//
// A cell (c, d) holds the nodes of locality c that district d has; parts(c) is the number of
// occupied cells of c, c is split iff parts(c) >= 2, and sq is the sum of the squared cell sizes.
// A flip of a node of locality c from district `old` to `target` is two moves: the node leaves
// the cell (c, old) and enters the cell (c, target).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fc_philox.h"  // FC_HD
#include "fc_replay.h"

namespace fc {

constexpr int32_t kSplitMaxExcess = 1023;  // excess_hist's top bin: it collects every larger excess
constexpr int32_t kSplitCellMax = 65535;   // a cell is a uint16 (FC_DIAG_SERIES bounds n by 65,535)

// One move of one node: it enters (dir > 0) or leaves (dir < 0) a cell that holds `count` nodes
// before the move (count >= 1 for a leave), in a locality that meets `parts` districts before it.
// dparts, dsplit: the change of that number and of the locality's split bit; dsq: the change of
// the cell's squared size.
FC_HD void split_rule(int32_t count, int32_t dir, int32_t parts, int32_t &dparts, int32_t &dsplit, int64_t &dsq) {
    dparts = dir > 0 ? (count == 0 ? 1 : 0) : (count == 1 ? -1 : 0);
    dsplit = (parts + dparts >= 2 ? 1 : 0) - (parts >= 2 ? 1 : 0);
    dsq = dir > 0 ? 2 * (int64_t)count + 1 : 1 - 2 * (int64_t)count;
}

// Kernel parameters (passed by value).  Output rows are per chain of the call, [nc] rows each.
struct SplitsParams {
    LogWindow log;            // the chains read and their window (fc_replay.h)
    const int32_t *node_loc;  // [n] labels in [0, n_loc)
    int32_t n_loc;
    int32_t x_top;            // X = min(x_max, kSplitMaxExcess): excess_hist has X + 1 bins
    int64_t *cells_now;       // [nc * n_loc * k]
    int64_t *split_sum, *parts_sum;  // [nc * n_loc]
    int64_t *dlocs_sum;       // [nc * k]
    int64_t *sq_sum;          // [nc]
    int64_t *splits_hist;     // [nc * (n_loc + 1)]
    int64_t *excess_hist;     // [nc * (x_top + 1)]
};

// LDS bytes of the kernel's int64 rows: the two per-locality integrals, the two histograms and
// the districts' integrals
FC_HD size_t splits_acc_bytes(int32_t n_loc, int32_t x_top) {
    return 8 * (2 * (size_t)n_loc + ((size_t)n_loc + 1) + ((size_t)x_top + 1) + 32);
}
// LDS bytes of the kernel: those rows, parts [n_loc] (int32), the uint16 table [n_loc][k] (two
// cells per 32-bit word) and the current assignment (int8, padded to 16 bytes)
inline size_t splits_lds_bytes(int32_t npad, int32_t k, int32_t n_loc, int32_t x_top) {
    return splits_acc_bytes(n_loc, x_top) + 4 * (size_t)n_loc + 4 * (((size_t)n_loc * (size_t)k + 1) / 2) +
           (((size_t)npad + 15) & ~(size_t)15);
}
// Whether a chain's image fits the default dynamic LDS limit
inline bool splits_fit_lds(int32_t npad, int32_t k, int32_t n_loc, int32_t x_top) {
    return splits_lds_bytes(npad, k, n_loc, x_top) <= 48 * 1024;
}

// One wavefront per chain of [c0, c0 + nc).  Returns a hipError_t as int.
int launch_splits(const SplitsParams &p, void *stream);

}  // namespace fc
