// Host check of csrc/fc_lane_mask.h, the lane-range masks of the k = 2 flip kernel's lean instances,
// against their definition (tests/test_lane_masks.py builds and runs it, plain and under the address
// and undefined-behaviour sanitizers: a shift by 64 would be reported there): bit l set iff
// lo <= l < hi, for every n in [0, 64] and every pair 0 <= lo, hi <= 64 (hi < lo: empty), each form on
// the domain its name promises.
#include <stdint.h>
#include <stdio.h>

#include "fc_lane_mask.h"

using namespace fc;

static long checked = 0, bad = 0;

static void expect(bool ok, const char *what, long a, long b, long c) {
    ++checked;
    if (!ok && ++bad <= 20) printf("BAD %s (%ld, %ld, %ld)\n", what, a, b, c);
}

// the definition: bit l set iff lo <= l < hi
static uint64_t range_def(int lo, int hi) {
    uint64_t m = 0;
    for (int l = 0; l < 64; ++l)
        if (lo <= l && l < hi) m |= 1ull << l;
    return m;
}

int main() {
    for (int n = 0; n <= 64; ++n) {
        expect(lanes_below(n) == range_def(0, n), "lanes_below", n, 0, 0);
        expect(lanes_from(n) == range_def(n, 64), "lanes_from", n, 0, 0);
        if (n >= 1) expect(lanes_below_ge1(n) == range_def(0, n), "lanes_below_ge1", n, 0, 0);
        if (n < 64) {
            expect(lanes_from_lt64(n) == range_def(n, 64), "lanes_from_lt64", n, 0, 0);
            expect(lanes_above_lt64(n) == range_def(n + 1, 64), "lanes_above_lt64", n, 0, 0);
            expect(lanes_upto_lt64(n) == range_def(0, n + 1), "lanes_upto_lt64", n, 0, 0);
        }
    }
    for (int lo = 0; lo <= 64; ++lo)
        for (int hi = 0; hi <= 64; ++hi) {  // (hi < lo: empty, as the kernel's ranges may be)
            const uint64_t def = range_def(lo, hi);
            expect(lanes_in(lo, hi) == def, "lanes_in", lo, hi, 0);
            if (lo < 64) {
                expect(lanes_in_lo_lt64(lo, hi) == def, "lanes_in_lo_lt64", lo, hi, 0);
                expect(lanes_after_lt64(lo, hi) == range_def(lo + 1, hi), "lanes_after_lt64", lo, hi, 0);
                if (hi >= 1) {
                    expect(lanes_in_lo_lt64_hi_ge1(lo, hi) == def, "lanes_in_lo_lt64_hi_ge1", lo, hi, 0);
                    expect(lanes_after_lt64_hi_ge1(lo, hi) == range_def(lo + 1, hi), "lanes_after_lt64_hi_ge1", lo, hi, 0);
                }
            }
        }
    printf("checked %ld bad %ld\n", checked, bad);
    return bad ? 1 : 0;
}
