// Election series: the per-yield rule of one district of a two-party election,
// shared by the host entry point fc_election_eval and the replay kernel (fc_votes.hip), and the
// parameters of that kernel.
//
// An election is a pair of node columns (A, B).  With a, b the district's tallies of the two
// columns, A wins the district iff a > b (a tie is won by neither), and the district's share of
// the efficiency gap, in doubled integer units, is
//   g(a, b) = 3b - a  (a > b),   b - 3a  (a < b),   0  (a == b):
// the winner wastes a - (a + b) / 2 votes and the loser all of theirs, so the sum of g over the
// districts divided by twice the election's votes is (wasted_B - wasted_A) / total.
#pragma once
#include <stdint.h>

#include "fc_philox.h"  // FC_HD
#include "fc_replay.h"

namespace fc {

constexpr int kVoteMaxCols = 8;       // node columns per run
constexpr int kVoteMaxElections = 4;  // (A, B) column pairs
constexpr int kVoteMaxEdges = 256;    // efficiency-gap histogram edges (257 bins)

// One district of one yield: the win bit of A and g(a, b).  a, b >= 0.
FC_HD void election_rule(int64_t a, int64_t b, int32_t &win, int64_t &g) {
    win = a > b ? 1 : 0;
    g = a > b ? 3 * b - a : (a < b ? b - 3 * a : 0);
}

// Kernel parameters (passed by value).  Output rows are per chain of the call, [nc] rows each.
struct VotesParams {
    LogWindow log;            // the chains read and their window (fc_replay.h)
    const int32_t *cols;      // [n * NC] node columns, rows padded to the kernel's NC
    int32_t n_cols;
    int32_t n_el;
    int32_t col_a[kVoteMaxElections], col_b[kVoteMaxElections];
    int32_t n_edges;
    const int64_t *edges;     // [n_edges] ascending
    int8_t *cur;              // [nc * npad] the current assignment when it is not kept in LDS
    int64_t *tally_now, *tally_sum;  // [nc * k * n_cols]
    int64_t *seats_hist;             // [nc * n_el * (k + 1)]
    int64_t *wins_sum;               // [nc * n_el * k]
    int64_t *gap_sum;                // [nc * n_el]
    int64_t *gap_hist;               // [nc * n_el * (n_edges + 1)]
};

// LDS bytes of the kernel's histograms and tally scratch (its current assignment comes after)
inline size_t votes_hist_bytes(int32_t k, int32_t n_edges) {
    return 8 * (size_t)kVoteMaxElections * ((size_t)(k + 1) + (size_t)(n_edges + 1)) + 4 * 32 * kVoteMaxCols;
}
// Whether a chain's current assignment fits the default dynamic LDS limit beside them
inline bool votes_cur_in_lds(int32_t npad, int32_t k, int32_t n_edges) {
    return votes_hist_bytes(k, n_edges) + (size_t)npad + 16 <= 48 * 1024;
}

// Row length of the uploaded column table for n_cols columns (the kernel's instances: 2, 4, 8)
int votes_padded_cols(int32_t n_cols);
// One wavefront per chain of [c0, c0 + nc); global_cur: the current assignment in p.cur.
// Returns a hipError_t as int.
int launch_votes(const VotesParams &p, bool global_cur, void *stream);

}  // namespace fc
