// The pass plan of the k = 2 tally reduce (fc_tally.hip), stated once as data: which of the nine
// per-chain arrays a run keeps, their bytes, and how launch_tally_reduce packs them into LDS
// passes of at most the device's dynamic-LDS limit (first fit, in array order; an array above the
// limit takes global atomics).  The launcher queries the limit, calls plan_tally_reduce and
// launches what it returns; tests/native/tally_plan_check.cpp executes the rule on the CPU.  No HIP.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/flipchain.h"

namespace fc {

// the arrays, in the order tally_reduce_kernel lays them out in LDS
enum : uint32_t { TR_CUT = 1, TR_NB = 2, TR_EDGE = 4, TR_NF = 8, TR_PS = 16, TR_LF = 32, TR_FC = 64, TR_OCC = 128, TR_LA = 256 };
constexpr int kTrArrays = 9;

// One plan: passes [0, n_passes) with the arrays of lmask[i] privatised in bytes[i] of LDS, and the
// arrays of gmask under global atomics (applied by pass 0).  n_passes >= 1 for a planned reduce
// (one pass with lmask 0 when nothing fits); 0: no reduce planned yet.
struct TallyPlan {
    int64_t limit = 0;  // the LDS bytes per workgroup the plan was made for
    int32_t n_passes = 0;
    uint32_t gmask = 0;
    uint32_t lmask[kTrArrays] = {0};
    int64_t bytes[kTrArrays] = {0};
};
inline bool operator==(const TallyPlan &a, const TallyPlan &b) {
    if (a.limit != b.limit || a.n_passes != b.n_passes || a.gmask != b.gmask) return false;
    for (int i = 0; i < a.n_passes; ++i)
        if (a.lmask[i] != b.lmask[i] || a.bytes[i] != b.bytes[i]) return false;
    return true;
}

// the arrays a run with these diagnostics keeps
inline uint32_t tally_arrays(uint32_t diag) {
    uint32_t have = 0;
    if (diag & FC_DIAG_HIST) have |= TR_CUT | TR_NB;
    if (diag & FC_DIAG_EDGES) have |= TR_EDGE;
    if (diag & FC_DIAG_FLIPS) have |= TR_NF | TR_PS | TR_LF;
    if (diag & FC_DIAG_FLIPS_EXACT) have |= TR_FC | TR_OCC | TR_LA;
    return have;
}

// per-chain bytes of array a (tally_reduce_kernel's tr_len, 8 B per entry)
inline size_t tally_array_bytes(int a, int32_t n, int32_t n_edges) {
    return 8 * (size_t)(a == 0 ? n_edges + 1 : a == 1 ? n + 1 : a == 2 ? n_edges : n);
}

// The arrays the run keeps, packed greedily into passes of at most `limit` bytes of LDS (sec11
// with every tally on gfx950: one pass of 139 KiB, one 1024-thread workgroup per CU: the log is
// read once); an array above the limit goes to global atomics.
inline TallyPlan plan_tally_reduce(uint32_t diag, int32_t n, int32_t n_edges, size_t limit) {
    TallyPlan pl;
    pl.limit = (int64_t)limit;
    const uint32_t have = tally_arrays(diag);
    for (int a = 0; a < kTrArrays; ++a) {
        if (!((have >> a) & 1u)) continue;
        const size_t b = tally_array_bytes(a, n, n_edges);
        if (b > limit) {
            pl.gmask |= 1u << a;
            continue;
        }
        bool put = false;
        for (int i = 0; i < pl.n_passes && !put; ++i)
            if ((size_t)pl.bytes[i] + b <= std::max(limit, b)) {
                pl.lmask[i] |= 1u << a;
                pl.bytes[i] += (int64_t)b;
                put = true;
            }
        if (!put) {
            pl.lmask[pl.n_passes] = 1u << a;
            pl.bytes[pl.n_passes] = (int64_t)b;
            ++pl.n_passes;
        }
    }
    if (pl.n_passes == 0) pl.n_passes = 1;  // nothing in LDS: one launch, lmask 0
    return pl;
}

}  // namespace fc
