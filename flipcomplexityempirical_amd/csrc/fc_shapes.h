// Compactness series: the per-yield score of one district, shared by the host
// entry point fc_shape_score and the replay kernel (fc_shapes.hip), and the parameters of that
// kernel.
//
// With A the district's area and P its perimeter (both 0 .. 2^31 - 1), the score is
//   Q(A, P) = min(floor(2^20 A / P^2), 2^31 - 1),   0 when P = 0:
// the Polsby-Popper score 4 pi A / P^2 in units of 4 pi / 2^20.  2^20 A < 2^51 and P^2 < 2^62, so
// one unsigned 64-bit division is exact.
#pragma once
#include <stdint.h>

#include "fc_philox.h"  // FC_HD
#include "fc_replay.h"

namespace fc {

constexpr int kShapeMaxEdges = 64;    // Polsby-Popper histogram edges (65 bins): one per lane
constexpr int kShapeScoreBits = 20;   // Q's fixed point
constexpr int64_t kShapeScoreMax = 0x7fffffff;

// One district of one yield.  0 <= area, perim <= 2^31 - 1.
FC_HD int64_t shape_score(int64_t area, int64_t perim) {
    if (perim <= 0) return 0;
    const uint64_t q = ((uint64_t)area << kShapeScoreBits) / ((uint64_t)perim * (uint64_t)perim);
    return q > (uint64_t)kShapeScoreMax ? kShapeScoreMax : (int64_t)q;
}

// A node's own values (its neighbour rows are RowSlots of the length shared, 0 in an empty slot)
struct alignas(8) ShapeNode {
    int32_t area, ext;
};

// Kernel parameters (passed by value).  Output rows are per chain of the call, [nc] rows each.
struct ShapesParams {
    LogWindow log;            // the chains read and their window (fc_replay.h)
    const RowSlot *rows;      // [n * width] neighbour rows
    const ShapeNode *nodes;   // [n]
    int32_t width;            // slots per row: 8 or 16
    int32_t n_edges;
    const int64_t *edges;     // [n_edges] ascending
    int64_t *area_now, *perim_now, *perim_sum, *pp_now, *pp_sum;  // [nc * k]
    int64_t *pp_min_sum;      // [nc]
    int64_t *pp_hist;         // [nc * k * (n_edges + 1)]
    int64_t *pp_min_hist;     // [nc * (n_edges + 1)]
};

// LDS bytes of the kernel's histograms: (k + 1) rows, the last one Qmin's (padded to 16 bytes)
FC_HD size_t shapes_hist_bytes(int32_t k, int32_t n_edges) {
    return (8 * (size_t)(k + 1) * (size_t)(n_edges + 1) + 15) & ~(size_t)15;
}
// LDS bytes of the kernel: the histograms, the initial area / perimeter table [2][32], the
// chunk's neighbour rows and the current assignment
inline size_t shapes_lds_bytes(int32_t npad, int32_t k, int32_t n_edges, int32_t width) {
    return shapes_hist_bytes(k, n_edges) + 4 * 2 * 32 + sizeof(RowSlot) * 64 * (size_t)width +
           (((size_t)npad + 15) & ~(size_t)15);
}
// Whether a chain's image fits the default dynamic LDS limit
inline bool shapes_fit_lds(int32_t npad, int32_t k, int32_t n_edges, int32_t width) {
    return shapes_lds_bytes(npad, k, n_edges, width) <= 48 * 1024;
}

// One wavefront per chain of [c0, c0 + nc).  Returns a hipError_t as int.
int launch_shapes(const ShapesParams &p, void *stream);

}  // namespace fc
