// Wave-uniform lane masks of the k = 2 flip kernel's lean instances, shared by the kernel and the
// host-side check (tests/native/lane_mask_check.cpp compares every form with its definition).
//
// A mask is 64 bits, bit l for lane l.  The forms are plain C++ without a shift by 64.  Where the
// argument may be 64 the shift is made in two halves of at most 32 (a shift right, a subtract and
// two 64-bit scalar shifts on a wave-uniform argument); a select of two 64-bit values instead compiles
// to a compare and two 32-bit selects, which is what fc_device.h's bits_below costs beside its shift
// and 64-bit subtract (the other kernels keep it).  Where the call site has the argument below 64,
// or an upper bound of at least 1, one shift.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define FC_LANE_HD __host__ __device__ __forceinline__
#else
#define FC_LANE_HD inline
#endif

namespace fc {

// lanes n and up (bit l set iff l >= n), n in [0, 64]
FC_LANE_HD uint64_t lanes_from(int n) { return (~0ull << (n >> 1)) << (n - (n >> 1)); }
// ... where the call site has n < 64
FC_LANE_HD uint64_t lanes_from_lt64(int n) { return ~0ull << n; }
// lanes above n (bit l set iff l > n), n in [0, 63]: the second shift takes the place of n + 1 = 64
FC_LANE_HD uint64_t lanes_above_lt64(int n) { return (~0ull << n) << 1; }

// lanes below n (bit l set iff l < n), n in [0, 64]
FC_LANE_HD uint64_t lanes_below(int n) { return ~lanes_from(n); }
// ... where the call site has n >= 1 (n in [1, 64]): one shift right
FC_LANE_HD uint64_t lanes_below_ge1(int n) { return ~0ull >> (64 - n); }
// lanes up to and including n, n in [0, 63]
FC_LANE_HD uint64_t lanes_upto_lt64(int n) { return ~lanes_above_lt64(n); }

// lanes lo .. hi - 1 (bit l set iff lo <= l < hi), 0 <= lo, hi <= 64; empty when hi <= lo
FC_LANE_HD uint64_t lanes_in(int lo, int hi) { return lanes_from(lo) & ~lanes_from(hi); }
// ... where the call site has lo < 64
FC_LANE_HD uint64_t lanes_in_lo_lt64(int lo, int hi) { return lanes_from_lt64(lo) & ~lanes_from(hi); }
// ... and hi >= 1
FC_LANE_HD uint64_t lanes_in_lo_lt64_hi_ge1(int lo, int hi) { return lanes_from_lt64(lo) & lanes_below_ge1(hi); }
// lanes lo + 1 .. hi - 1, lo in [0, 63]
FC_LANE_HD uint64_t lanes_after_lt64(int lo, int hi) { return lanes_above_lt64(lo) & ~lanes_from(hi); }
// ... and hi >= 1
FC_LANE_HD uint64_t lanes_after_lt64_hi_ge1(int lo, int hi) { return lanes_above_lt64(lo) & lanes_below_ge1(hi); }

}  // namespace fc
