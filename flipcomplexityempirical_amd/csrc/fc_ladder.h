// Replica exchange (parallel tempering): the swap decision shared by the host and the exchange
// kernel (fc_exchange.hip), and the parameters of that kernel.  DESIGN.md "Replica exchange".
//
// Replica x at rung r (base b_r) and y at rung r + 1 trade temperatures with probability
// min(1, (b_r / b_{r+1}) ** (cut_x - cut_y)).  The decision must be the same bits on both sides, so
// neither calls pow / exp / log: the host prepares, per adjacent pair, qq = min(b) / max(b) and
// T[j] = pow(qq, 2^j), and ladder_threshold multiplies the entries of |d|'s set bits.
#pragma once
#include <stdint.h>

#include <cmath>

#include "../../include/flipchain.h"
#include "fc_philox.h"

namespace fc {

constexpr int kLadderBits = 17;       // |d| <= E < 2^17 (fc_run_set_ladders refuses larger graphs)
constexpr int kRungFields = 11;       // attributed ChainScalars fields (fc_rung_stats order)

struct LadderPair {
    double T[kLadderBits];  // qq ** (2 ** j); entries below 2^-200 are stored as 0
    int32_t unfav;          // sign of d = cut_x - cut_y for which the ratio is below 1 (0: equal bases)
    int32_t pad;
};

// Host only: the table of the pair (rung r, rung r + 1).
inline LadderPair ladder_pair(double b_lo_rung, double b_hi_rung) {
    LadderPair t{};
    t.unfav = b_lo_rung < b_hi_rung ? 1 : b_lo_rung > b_hi_rung ? -1 : 0;
    const double qq = t.unfav > 0 ? b_lo_rung / b_hi_rung : b_hi_rung / b_lo_rung;
    for (int j = 0; j < kLadderBits; ++j) {
        const double v = std::pow(qq, std::ldexp(1.0, j));
        t.T[j] = v < 0x1p-200 ? 0.0 : v;
    }
    return t;
}

// U53 threshold of the swap: accept iff mant53 < threshold.  Multiplications and compares only.
FC_HD uint64_t ladder_threshold(const LadderPair &t, int32_t d) {
    if (d == 0 || t.unfav == 0 || (d > 0) != (t.unfav > 0)) return 1ull << 53;  // ratio ** d >= 1
    const uint32_t a = (uint32_t)(d < 0 ? -d : d);
    double p = 1.0;
    for (int j = 0; j < kLadderBits; ++j) {
        if (!((a >> j) & 1u)) continue;
        p *= t.T[j];
        if (p < 0x1p-64) { p = 0.0; break; }  // no denormal is ever formed
    }
    return (uint64_t)ceil(p * 9007199254740992.0);
}

// One work item of an exchange round: the pair (slot, slot + 1), or a rung left unpaired by this
// parity (attributed only).  Slots are flat: ladder l's rung r is slot ladder_off[l] + r.
struct LadderItem {
    int32_t slot;
    int32_t pair;   // 1: (slot, slot + 1) is tried after both are attributed
};

struct LadderSlot {
    int32_t rung;   // within its ladder
    uint32_t gid;   // global chain id of the chain listed first in the ladder (the stream's G)
};

struct ChainScalars;

struct ExchangeParams {
    const LadderItem *items;
    int32_t n_items;
    int32_t do_swap;              // 0: attribute only (fc_run_read_rung_stats)
    uint32_t round;               // the run's round counter (Philox ctr word 0)
    uint32_t seed_lo, seed_hi;
    const LadderSlot *slots;      // [M]
    const LadderPair *pairs;      // [M], by lower slot
    int32_t *slot_of;             // [n_chains] flat slot held, -1: in no ladder
    int32_t *chain_at;            // [M]
    const ChainScalars *sc;       // [n_chains]
    uint64_t *thresh;             // [n_chains * tw]
    int32_t tw;                   // 2 * RMAX + 1
    int64_t *snap;                // [n_chains * kRungFields] streaming sums at the last attribution
    fc_rung_stats *rung;          // [M]
    // FC_LADDER_HIST (all null / 0 otherwise): the run's histograms, their snapshots and the
    // per-slot histograms; snapshot and slot rows are padded to an even width (16-byte rows)
    const int64_t *cut_hist, *nb_hist;
    int64_t *snap_cut, *snap_nb, *rung_cut, *rung_nb;
    int32_t cut_w, nb_w;          // E + 1, nb_w
    int32_t cut_w2, nb_w2;        // padded widths
};

int launch_exchange(const ExchangeParams &p, void *stream);

}  // namespace fc
