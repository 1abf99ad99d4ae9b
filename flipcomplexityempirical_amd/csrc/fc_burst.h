// Short bursts: the score of every yield of a series window, the best of them, and
// the rewind of a ReCom chain to the plan it held there.  The metric rule shared by the host entry
// point fc_burst_eval and the replay kernel (fc_burst.hip), the host checks of a metric, and the
// parameters of that kernel.  HIP-free.
//
// A metric maps the state at one yield to an int64 score.  With a_d, b_d district d's tallies of
// the metric's two vote columns:
//   FC_BURST_COUNT  the districts with den * a_d > num * (a_d + b_d) (num / den = 1 / 2: the seats
//                   of A as election_rule counts them; equality is not counted);
//   FC_BURST_GAP    |sum_d g(a_d, b_d)|, g of election_rule (fc_votes.h) in its doubled units;
//   FC_BURST_CUT    |cut| of the yield.
// The best yield of a window is the LATEST yield whose score is best (gerrychain's >=): a
// candidate replaces the best when it is at least as good, and the yields a state is held for
// (rejected steps write no event) count as yields of that state.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fc_internal.h"
#include "fc_votes.h"

namespace fc {

constexpr int64_t kBurstMaxDen = int64_t(1) << 20;
constexpr int64_t kBurstProductBound = int64_t(1) << 62;  // den * (a column's total) stays below this

// 1 when district (a, b) is above the share num / den.  a, b >= 0.
FC_HD int32_t burst_counts(int64_t a, int64_t b, int64_t num, int64_t den) { return den * a > num * (a + b) ? 1 : 0; }

// One district's share of both vote scores: its COUNT bit and its g.
FC_HD void burst_district(int64_t a, int64_t b, int64_t num, int64_t den, int32_t &cnt, int64_t &g) {
    int32_t win;
    election_rule(a, b, win, g);
    cnt = burst_counts(a, b, num, den);
}

// The score of a yield from its districts' sums (cnt, gsum) and its |cut|.
FC_HD int64_t burst_score(int32_t kind, int64_t cnt, int64_t gsum, int64_t cut) {
    if (kind == FC_BURST_COUNT) return cnt;
    if (kind == FC_BURST_GAP) return gsum < 0 ? -gsum : gsum;
    return cut < 0 ? -cut : cut;
}

// Whether a later yield of score s replaces a best of score `best`: at least as good.
FC_HD bool burst_takes(int64_t s, int64_t best, int32_t maximize) { return maximize ? s >= best : s <= best; }

inline bool burst_votes_kind(int32_t kind) { return kind == FC_BURST_COUNT || kind == FC_BURST_GAP; }

// Whether den * total < 2^62 (0 < den, 0 <= total), without forming the product: every den * a_d,
// num * (a_d + b_d) and sum of g is then below 2^63
inline bool burst_product_ok(int64_t den, int64_t total) { return total < (kBurstProductBound + den - 1) / den; }

// The host checks of a metric against a run's vote columns (n_cols 0: none set; col_total[j] the
// sum of column j).  Returns nullptr or what is wrong.  A vote kind with n_cols = 0 passes: the
// caller reports the missing setter.
inline const char *burst_metric_error(const fc_burst_metric &m, int32_t n_cols, const int64_t *col_total) {
    if (m.struct_size != sizeof(fc_burst_metric)) return "struct_size is not sizeof(fc_burst_metric)";
    if (m.kind != FC_BURST_COUNT && m.kind != FC_BURST_GAP && m.kind != FC_BURST_CUT) return "unknown kind";
    if (m.maximize != 0 && m.maximize != 1) return "maximize must be 0 or 1";
    if (!(0 < m.num && m.num < m.den && m.den <= kBurstMaxDen)) return "needs 0 < num < den <= 2^20";
    if (!burst_votes_kind(m.kind) || n_cols == 0) return nullptr;
    if (m.col_a < 0 || m.col_a >= n_cols || m.col_b < 0 || m.col_b >= n_cols || m.col_a == m.col_b)
        return "needs two different columns below n_cols";
    if (!burst_product_ok(m.den, col_total[m.col_a] + col_total[m.col_b]))
        return "den * (the columns' totals) reaches 2^62";
    return nullptr;
}

// Kernel parameters (passed by value).  Output rows are per chain of the call, [nc] each; a null
// output is skipped.
struct BurstParams {
    LogWindow log;             // the chains read and their window (fc_replay.h)
    const int64_t *cut0, *nb0; // [nc] |cut| and |B| at the window start
    int32_t kind, maximize;
    int64_t num, den;
    const int32_t *cols;       // [n * ncp] node columns (vote kinds), rows of ncp entries
    int32_t ncp, col_a, col_b;
    int32_t rewind;            // FC_BURST_REWIND: the best plan goes into the run
    int64_t *best_score, *best_t, *start_score, *end_score, *best_cut, *best_nb;
    int8_t *best_plan;         // [nc * npad] staged rows, 16-byte aligned each
    // rewind only: the run's rows and scalars, indexed by the global chain
    int8_t *assign;            // [n_chains * npad]
    int8_t *ser_a0;            // [n_chains * npad] (log.a0, writable)
    ChainScalars *sc;          // [n_chains]
};

// LDS bytes of the kernel: the current assignment (npad is a multiple of 16) and the start tallies
// of 32 districts' two columns
inline size_t burst_lds_bytes(int32_t npad) { return (size_t)npad + 32 * 2 * 4; }
// Whether a chain's image fits the default dynamic LDS limit (votes_cur_in_lds' 48 KB)
inline bool burst_fits_lds(int32_t npad) { return burst_lds_bytes(npad) <= 48 * 1024; }

// One wavefront per chain of [c0, c0 + nc).  Returns a hipError_t as int.
int launch_burst(const BurstParams &p, void *stream);

}  // namespace fc
