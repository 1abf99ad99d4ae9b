// The k = 2 slot evaluation as a lookup: the ring verdicts of a node are a pure function of its
// ring's district bits (8 of them with an 8-cell ring) and three constants of the node -- ring
// length, neighbour mask and link mask -- and a lattice has only a few distinct triples (interior,
// sides, corners, the nodes beside a removed corner).  One 16-bit entry per (class, ring bits)
// holds what the evaluation derives from the bits; the kernel's list body (fc_flip2.hip) fetches it
// instead of running the arithmetic.  The arithmetic (ring_runs, ring_entry_of) is stated here for
// the builder, its check and the ring body of the kernel instances that carry the table (their
// fall-back without one).  The other flip2_kernel instances keep their own copy of ring_runs'
// expressions, so that they compile to what they were: nothing but reading ties that copy to this
// statement (the GPU test of the table against ring_table=0 compares the lean instances only).
// So an edit to ring_runs is made by hand a second and a third time in fc_flip2.hip: in phase 2's
// ring branch and in reeval, each under `if constexpr (kTwoBody) ... else`.
//
// HIP-free: the host builds the table (fc_plan.cpp), tests/native/ring_table_check.cpp compares
// every entry with the arithmetic.  The k > 2 kernel's one_run sites could read the same table.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <array>
#include <vector>

#include "fc_internal.h"
#include "fc_ring.h"

namespace fc {

// The two run-rule verdicts of a ring: s_lin with the ring open between its last and first cell,
// s_cyc with the closing step (cell Ln-1 to cell 0) counted as a link when both ends are in A.
// inA: the ring's old-district bits, none at Ln and up; full = 2^Ln - 1.
// (Two written-out copies of this body live in fc_flip2.hip: change all three together.)
FC_RING_HD void ring_runs(uint32_t inA, uint32_t nbrA, uint32_t link, uint32_t Ln, uint32_t full, bool &s_lin,
                          bool &s_cyc) {
    const uint32_t rot = Ln ? (((inA >> 1) | (inA << (Ln - 1))) & full) : 0u;
    const uint32_t lk = inA & rot & link;
    s_lin = one_run_flat(nbrA, full & ~lk, full);
    // the ring's closing step (cell Ln-1 to cell 0), when both ends are in A
    const uint32_t vlink = (Ln >= 2) ? ((inA & (inA >> (Ln - 1)) & 1u) << (Ln - 1)) : 0u;
    s_cyc = one_run_flat(nbrA, full & ~(lk | vlink), full);
}

// ---- the entry -------------------------------------------------------------------------------
// bits 0-4: delta + 8 (delta = cut(S') - cut(S), in [-8, 8]); bits 12-15: nA, the old-district
// neighbours; the verdict bits sit where the kernel's status word has them (LF_HIT, LF_SLIN,
// LF_SCYC of fc_device.h: fc_flip2.hip asserts the equality), so one mask moves all three.
typedef uint16_t RingEntry;
constexpr int kRingTableRmax = 8;             // ring cells indexed: 256 entries per class
constexpr int kRingTableRow = 1 << kRingTableRmax;
constexpr uint32_t kReDeltaMask = 0x1fu;
constexpr uint32_t kReHit = 1u << 8;          // tmask != 0: a boundary node, the draw is a proposal
constexpr uint32_t kReSlin = 1u << 10;
constexpr uint32_t kReScyc = 1u << 11;
constexpr uint32_t kReVerdicts = kReHit | kReSlin | kReScyc;
constexpr int kReNaShift = 12;
constexpr int kRingTableMaxClasses = 255;     // class ids share NodeRec::deg's upper half with nothing else

// The entry of ring bits `bits` for a node of ring length Ln (<= 8), neighbour mask nbr and link
// mask link.  Bits at Ln and up are ignored (a padded ring cell holds the node itself, so the
// kernel's index has them set or clear with the node's own district): every entry is computed
// from bits & full, and the kernel indexes with the unmasked byte.
FC_RING_HD RingEntry ring_entry_of(uint32_t bits, uint32_t Ln, uint32_t nbr, uint32_t link) {
    const uint32_t full = (1u << Ln) - 1u;
    const uint32_t inA = bits & full;
    const uint32_t nbrA = inA & nbr;   // old-district neighbours
    const uint32_t tmask = nbr & ~inA;  // target-district neighbours
    const int nA = __builtin_popcount(nbrA);
    const int delta = nA - __builtin_popcount(tmask);
    bool s_lin, s_cyc;
    ring_runs(inA, nbrA, link, Ln, full, s_lin, s_cyc);
    return (RingEntry)((uint32_t)(delta + kRingTableRmax) | (tmask != 0u ? kReHit : 0u) | (s_lin ? kReSlin : 0u) |
                       (s_cyc ? kReScyc : 0u) | ((uint32_t)nA << kReNaShift));
}
FC_RING_HD int ring_entry_delta(uint32_t e) { return (int)(e & kReDeltaMask) - kRingTableRmax; }
FC_RING_HD int ring_entry_na(uint32_t e) { return (int)(e >> kReNaShift); }

// ---- the builder (host) ----------------------------------------------------------------------
// A node's class: (Ln, nbr, link) of its meta word (fc_internal.h).
typedef std::array<uint32_t, 3> RingClassKey;
inline RingClassKey ring_class_key(uint64_t meta) {
    return {(uint32_t)(meta & kMetaLenMask), (uint32_t)(meta >> kMetaNbrShift) & 0xffffu,
            (uint32_t)(meta >> kMetaLinkShift) & 0xffffu};
}

// Groups the n nodes of meta[] by class.  Class ids are dense (0 .. count - 1) and follow the keys'
// order, not the nodes': a renumbered graph gives every key the id it had.  Returns the class count.
// With count <= cap (and count <= kRingTableMaxClasses, every ring of at most 8 cells), cls[v] is
// node v's class and table[cls << 8 | bits] its entry for every byte `bits`; otherwise both come
// back empty: no table, the caller keeps the arithmetic.
inline int build_ring_table(const uint64_t *meta, int n, int cap, std::vector<uint16_t> &cls,
                            std::vector<RingEntry> &table) {
    cls.clear();
    table.clear();
    std::vector<RingClassKey> keys(n);
    bool fits = true;
    for (int v = 0; v < n; ++v) {
        keys[v] = ring_class_key(meta[v]);
        fits = fits && keys[v][0] <= (uint32_t)kRingTableRmax;
    }
    std::vector<RingClassKey> uniq(keys);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    const int count = (int)uniq.size();
    if (!fits || count > cap || count > kRingTableMaxClasses) return count;
    cls.resize(n);
    for (int v = 0; v < n; ++v)
        cls[v] = (uint16_t)(std::lower_bound(uniq.begin(), uniq.end(), keys[v]) - uniq.begin());
    table.resize((size_t)count * kRingTableRow);
    for (int c = 0; c < count; ++c)
        for (uint32_t bits = 0; bits < (uint32_t)kRingTableRow; ++bits)
            table[(size_t)c * kRingTableRow + bits] = ring_entry_of(bits, uniq[c][0], uniq[c][1], uniq[c][2]);
    return count;
}

}  // namespace fc
