// Plan samples: the parameters of the kernel that replays the FC_DIAG_SERIES flip
// logs up to chosen yields and writes the assignment held at each of them (fc_plans.hip).
//
// a_t is the window-start assignment with every logged event of t_e <= t applied in log order;
// sample j of a chain is a_{times[j]}, with |cut| and |B| at that yield, the Hamming distance to
// the window-start plan and the district populations.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fc_replay.h"

namespace fc {

// Kernel parameters (passed by value).  Output rows are per chain of the call and sample,
// [nc * n_times] rows each; a null output is skipped.
struct PlansParams {
    LogWindow log;             // the chains read and their window (fc_replay.h); t_end is not read
    int32_t n_times;
    const int64_t *times;      // [n_times] absolute yields, strictly increasing, inside every chain's window
    const int64_t *cut0, *nb0; // [nc] |cut| and |B| at the window start
    const int32_t *node_pop;   // [npad] node populations, 0 beyond n (read for pops only)
    int8_t *plans;             // [nc * n_times * npad] staged rows, 16-byte aligned each
    int64_t *cut, *nb, *dist0; // [nc * n_times]
    int64_t *pops;             // [nc * n_times * k]
};

// LDS bytes of the kernel: the current assignment (npad is a multiple of 16) and the district
// populations of the sample being written
inline size_t plans_lds_bytes(int32_t npad) { return (size_t)npad + 32 * 8; }

// One wavefront per chain of [c0, c0 + nc).  Returns a hipError_t as int.
int launch_plans(const PlansParams &p, void *stream);

}  // namespace fc
