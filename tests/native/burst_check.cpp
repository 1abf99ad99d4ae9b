// The HIP-free checks of csrc/fc_burst.h at their edges (tests/test_burst.py reads the lines).
#include <cstdio>
#include <cstring>
#include "fc_burst.h"
int main() {
    fc_burst_metric m;
    std::memset(&m, 0, sizeof m);
    m.struct_size = sizeof m; m.kind = FC_BURST_COUNT; m.col_a = 0; m.col_b = 1; m.num = 1; m.den = 2; m.maximize = 1;
    const int64_t tot[8] = {100, 200, 300, 0, 0, 0, 0, 0};
    auto say = [&](const char *what) { const char *e = fc::burst_metric_error(m, 3, tot); std::printf("%s=%s\n", what, e ? e : "ok"); };
    say("good");
    m.col_b = 3; say("col_b_is_n_cols");
    m.col_b = 2; say("col_b_last");
    m.col_a = 2; say("same_columns");
    m.col_a = -1; say("negative_column");
    m.col_a = 0; m.kind = FC_BURST_CUT; m.col_b = 9; say("cut_ignores_columns");
    m.kind = 3; say("unknown_kind");
    m.kind = FC_BURST_GAP; m.col_b = 1; m.den = (int64_t(1) << 20); m.num = m.den - 1;
    const int64_t big[8] = {(int64_t(1) << 42) - 7, 6, 7, 0, 0, 0, 0, 0};
    { const char *e = fc::burst_metric_error(m, 3, big); std::printf("below_bound=%s\n", e ? e : "ok"); }
    m.col_b = 2;
    { const char *e = fc::burst_metric_error(m, 3, big); std::printf("at_bound=%s\n", e ? e : "ok"); }
    const int top = 48 * 1024 - 256;
    std::printf("fit=%d%d%d bytes=%zu\n", (int)fc::burst_fits_lds(top), (int)fc::burst_fits_lds(top + 16),
                (int)fc::burst_fits_lds(16), fc::burst_lds_bytes(top));
    return 0;
}
