// Device helpers of the spanning-tree bipartition (fc_bipartition.h), shared by the kernels that
// include it: the ReCom kernels (fc_recom.hip) and the seed-plan kernel (fc_seed.hip).
// In an anonymous namespace, as they were inside fc_recom.hip: every including file gets copies
// with internal linkage, so the compiler's inlining of them into the ReCom kernels is what it was.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fc_device.h"

namespace fc {
namespace {

using namespace dev;

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t mulhi64(uint64_t r, uint64_t n) { return __umul64hi(r, n); }

__device__ __forceinline__ uint32_t word4(const uint4 &w, int t) { return t == 0 ? w.x : t == 1 ? w.y : t == 2 ? w.z : w.w; }

// Index of the k-th set flag over items [0, count) split into per-lane contiguous chunks:
// `flag(i)` is evaluated twice per item of the owning lane (count, then locate).
template <typename F>
__device__ int kth_item(int count, int lane, uint64_t k, F flag, int &total) {
    const int chunk = (count + kWave - 1) / kWave;
    const int lo = min(count, lane * chunk), hi = min(count, lo + chunk);
    int c = 0;
    for (int i = lo; i < hi; ++i) c += flag(i) ? 1 : 0;
    const int incl = wave_scan_incl(c);
    total = __builtin_amdgcn_readlane(incl, kWave - 1);
    const int excl = incl - c;
    int found = -1;
    if ((uint64_t)excl <= k && k < (uint64_t)incl) {
        int r = (int)(k - (uint64_t)excl);
        for (int i = lo; i < hi; ++i)
            if (flag(i)) {
                if (r == 0) { found = i; break; }
                --r;
            }
    }
    const uint64_t own = __ballot(found >= 0);
    return own ? __builtin_amdgcn_readlane(found, __builtin_ctzll(own)) : -1;
}

#ifndef FC_RECOM_SCAN_U
#define FC_RECOM_SCAN_U 2
#endif
#ifndef FC_RECOM_JUMP_U
#define FC_RECOM_JUMP_U 4
#endif
constexpr int kScanU8 = FC_RECOM_SCAN_U;  // Boruvka scan: nodes per lane in flight (RMAX = 8; 2 for 16)
constexpr int kJumpU = FC_RECOM_JUMP_U;  // pointer jumping: nodes per lane in flight

}  // namespace
}  // namespace fc
