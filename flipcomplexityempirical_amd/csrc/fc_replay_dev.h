// The device side of a replay of the FC_DIAG_SERIES event logs (DESIGN.md §4 "Series window"),
// shared by fc_votes.hip, fc_shapes.hip, fc_splits.hip, fc_plans.hip and fc_heat.hip: the fc_event
// bit layout, a chain's log, the chunk prefetch, the neighbour-row staging and match_mask.  All of
// them take one wavefront per chain and read the log 64 events at a time, one per lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "fc_device.h"
#include "fc_replay.h"

namespace fc {
namespace replay {

// ---- an fc_event as one 16-byte load: x is t, y the packed fields -----------------------------
typedef ulonglong2 Event;
static_assert(sizeof(fc_event) == 16 && offsetof(fc_event, t) == 0 && offsetof(fc_event, v) == 8,
              "an event is one ulonglong2: t in x, v in the low bits of y");
constexpr int kCutShift = 8 * ((int)offsetof(fc_event, cut) - 8);
constexpr int kNbShift = 8 * ((int)offsetof(fc_event, nb) - 8);
constexpr int kTargetShift = 8 * ((int)offsetof(fc_event, target) - 8);
static_assert(kCutShift == 16 && kNbShift == 32 && kTargetShift == 48, "v, cut, nb: 16 bits each; target: 8");

__device__ __forceinline__ int64_t ev_t(const Event &e) { return (int64_t)e.x; }
__device__ __forceinline__ int ev_node(const Event &e) { return (int)(e.y & 0xffffu); }
__device__ __forceinline__ int ev_cut(const Event &e) { return (int)((e.y >> kCutShift) & 0xffffu); }
__device__ __forceinline__ int ev_nb(const Event &e) { return (int)((e.y >> kNbShift) & 0xffffu); }
__device__ __forceinline__ int ev_target(const Event &e) { return (int)((e.y >> kTargetShift) & 0xffu); }

// This lane's event as a move: its node and target, v = -1 and tg = 0 for an event past the log
// (!in_range) or out of range of the graph or the districts.  Returns whether it is a move.
__device__ __forceinline__ bool decode(const Event &e, bool in_range, int32_t n, int32_t k, int &v, int &tg) {
    v = ev_node(e);
    tg = ev_target(e);
    const bool valid = in_range && v < n && tg < k;
    if (!valid) {
        v = -1;
        tg = 0;
    }
    return valid;
}

// ---- the log of chain c0 + cl -----------------------------------------------------------------
struct Log {
    const Event *ev;
    int64_t ne;  // events replayed: min(ev_len, ev_cap)

    // (w by value: a reference would take the address of the kernel's parameter block, and a
    // kernel that takes it nowhere else reads its arguments in another order after that)
    __device__ __forceinline__ Log(const LogWindow w, int32_t cl)
        : ev((const Event *)(w.events + (size_t)(w.c0 + cl) * w.ev_cap)),
          ne(w.ev_len[cl] < w.ev_cap ? w.ev_len[cl] : w.ev_cap) {}
    // events of the chunk that starts at base
    __device__ __forceinline__ int count(int64_t base) const { return (int)(ne - base < 64 ? ne - base : 64); }
};

// This lane's events of the next DEPTH chunks, loaded ahead of their use: e[0] is the chunk about
// to be replayed (a two-ahead pass also decodes e[1], to start the next chunk's row loads).
template <int DEPTH>
struct Prefetch {
    Event e[DEPTH];

    __device__ __forceinline__ Prefetch(const Log &log, int lane) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            e[d] = Event{0ull, 0ull};
            if (64 * d + lane < log.ne) e[d] = log.ev[64 * d + lane];
        }
    }
    // base: the chunk e[0] holds.  Every slot moves up one and the chunk DEPTH ahead is loaded;
    // past the log's end the last slot is zeroed (with one slot it keeps its event instead, which
    // a pass rejects by its index: the form each kernel had)
    __device__ __forceinline__ void advance(const Log &log, int64_t base, int lane) {
#pragma unroll
        for (int d = 0; d + 1 < DEPTH; ++d) e[d] = e[d + 1];
        if (DEPTH > 1) e[DEPTH - 1] = Event{0ull, 0ull};
        if (base + 64 * DEPTH + lane < log.ne) e[DEPTH - 1] = log.ev[base + 64 * DEPTH + lane];
    }
};

// ---- neighbour rows (RowSlot, fc_replay.h), W slots each: RV 16-byte pieces ---------------------
// A chunk's rows are loaded into registers while the chunk before it is replayed, go to LDS
// ([64][W] at stage4) when its turn comes, and are read per event with one slot per lane.
template <int W>
struct Rows {
    static constexpr int RV = W / 2;

    // node v's row, or W empty slots of value `empty` for v < 0
    static __device__ __forceinline__ void load(const RowSlot *rows, int v, int32_t empty, int4 (&r)[RV]) {
#pragma unroll
        for (int q = 0; q < RV; ++q) r[q] = make_int4(-1, empty, -1, empty);
        if (v >= 0) {
            const int4 *row = (const int4 *)(rows + (size_t)v * W);
#pragma unroll
            for (int q = 0; q < RV; ++q) r[q] = row[q];
        }
    }
    static __device__ __forceinline__ void stage(int4 *stage4, int lane, const int4 (&r)[RV]) {
#pragma unroll
        for (int q = 0; q < RV; ++q) stage4[lane * RV + q] = r[q];
    }
    // slot `lane` of the row of the chunk's event i (an empty slot for the lanes past the row)
    static __device__ __forceinline__ RowSlot slot(const int4 *stage4, int i, int lane, int32_t empty) {
        RowSlot s = RowSlot{-1, empty};
        if (lane < W) s = ((const RowSlot *)stage4)[i * W + lane];
        return s;
    }
};

// ---- lane masks --------------------------------------------------------------------------------
// The lanes of `on` whose key `theirs` equals this lane's key `mine` (both below 2^bits, bits
// wave-uniform): per key bit one ballot of the lanes that have it set, of which a lane keeps those
// that agree with its own bit.  Call with the whole wave active.
__device__ __forceinline__ uint64_t match_mask(uint32_t mine, uint32_t theirs, int bits, uint64_t on) {
    uint64_t differ = 0;
    for (int b = 0; b < bits; ++b) {
        const uint64_t has = __ballot((theirs >> b) & 1u);
        differ |= ((mine >> b) & 1u) ? ~has : has;
    }
    return ~differ & on;
}
// bits that hold every value below x (x >= 1)
__device__ __forceinline__ int bits_for(int32_t x) { return x <= 1 ? 0 : 32 - __builtin_clz((uint32_t)(x - 1)); }

}  // namespace replay
}  // namespace fc
