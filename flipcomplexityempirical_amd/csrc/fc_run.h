// Internal to the C-ABI layer (fc_capi.cpp, fc_ckpt.cpp, fc_tempering.cpp, fc_readout.cpp):
// struct fc_run, the owning device buffer its members are, error reporting and shared helpers.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "fc_burst.h"
#include "fc_heat.h"
#include "fc_internal.h"
#include "fc_ladder.h"
#include "fc_plan.h"
#include "fc_plans.h"
#include "fc_shapes.h"
#include "fc_splits.h"
#include "fc_votes.h"

namespace fc {

// Sets the calling thread's fc_last_error() message and returns `code`.
int fail(int code, const std::string &msg);

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return fc::fail(FC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// Device memory owned by its holder: move-only, freed by the destructor.  The int results are
// FC_OK or fail()'s code.
template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            std::swap(p_, o.p_);
            std::swap(cap_, o.cap_);
        }
        return *this;
    }
    ~DevBuf() { release(); }

    operator T *() const { return p_; }
    T *get() const { return p_; }
    size_t capacity() const { return cap_; }  // elements held

    void release() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // `count` elements, uninitialised (what was held is released; 0 leaves the buffer null)
    int alloc(size_t count) {
        release();
        if (count == 0) return FC_OK;
        hipError_t e = hipMalloc((void **)&p_, count * sizeof(T));
        if (e != hipSuccess) {
            p_ = nullptr;
            return fail(FC_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        }
        cap_ = count;
        return FC_OK;
    }
    int alloc_zero(size_t count) {
        if (int rc = alloc(count)) return rc;
        if (count) HIP_TRY(hipMemset(p_, 0, count * sizeof(T)));
        return FC_OK;
    }
    int upload(const T *src, size_t count) {
        if (int rc = alloc(count)) return rc;
        if (count) HIP_TRY(hipMemcpy(p_, src, count * sizeof(T), hipMemcpyHostToDevice));
        return FC_OK;
    }
    int upload(const std::vector<T> &v) { return upload(v.data(), v.size()); }
    // at least `count` elements: reallocates (contents lost) only when that exceeds capacity()
    int grow(size_t count) { return count > cap_ ? alloc(count) : FC_OK; }

private:
    T *p_ = nullptr;
    size_t cap_ = 0;
};

// N HIP events recorded along the last call of an entry point, for its elapsed-time read-out:
// each created by its first mark(), destroyed with their holder (an fc_run: never copied).
template <int N>
struct EventMarks {
    hipEvent_t ev[N] = {};

    ~EventMarks() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int mark(int i, hipStream_t stream) {
        if (!ev[i]) HIP_TRY(hipEventCreate(&ev[i]));
        HIP_TRY(hipEventRecord(ev[i], stream));
        return FC_OK;
    }
    int elapsed(int i, int j, float *ms) const {  // milliseconds from event i to event j
        HIP_TRY(hipEventElapsedTime(ms, ev[i], ev[j]));
        return FC_OK;
    }
};

// Whether `bytes` more of device memory fit a tenth of what is free (fc_readout.cpp).
int fits_free_tenth(size_t bytes, bool &fits);

constexpr size_t kMaxLaunchEvents = 4096;  // per-launch HIP event pairs kept (fc_run_timings)

}  // namespace fc

using fc::DevBuf;
using fc::fail;
using fc::fits_free_tenth;
using fc::fnv1a;

struct fc_run : fc::RunShape {
    fc::HostGraph g;  // host copy (sizes, edges, rings for readouts)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // the last launch's pair (of launch_events)
    bool timed = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> launch_events;  // pool
    size_t n_launch_events = 0;                                      // recorded since last read
    size_t ev_head = 0;          // launch_events: oldest recorded pair (ring of kMaxLaunchEvents)
    // device buffers
    DevBuf<unsigned char> d_graph;  // NodeRec<ring_max>[n]
    DevBuf<int32_t> d_ring_eid;
    DevBuf<int8_t> d_assign;
    DevBuf<uint8_t> d_fcnt;
    DevBuf<fc::ChainScalars> d_sc;
    DevBuf<uint64_t> d_thresh;
    DevBuf<double> d_log1mp;
    DevBuf<uint32_t> d_pkeys;  // the seed's Philox round keys (k = 2 flip kernel)
    DevBuf<uint16_t> d_ring_table;  // [ring_classes * 256] ring verdicts by class and ring bits (k = 2; null: none)
    DevBuf<int32_t> d_labels;
    DevBuf<int64_t> d_cut_hist, d_nb_hist;
    DevBuf<int64_t> d_edge_acc;
    // k = 2 full diagnostics: the per-chain tally log (KParams tl_*), grown by fc_run_steps; its
    // capacity is n_chains * 4 words per granted entry
    DevBuf<uint32_t> d_tl;
    DevBuf<int64_t> d_tl_len, d_tl_t0;
    int64_t tl_want = 0;           // entries per chain the last launch asked for
    fc::TallyPlan tl_plan;         // the pass plan the last tally reduce launched (fc_run_tally_plan)
    int32_t series_staged = -1;    // last fc_run_frame_series_changes: 1 one staged pass, 0 two passes
    DevBuf<int64_t> d_num_flips, d_part_sum, d_last_flipped;
    DevBuf<int64_t> d_flip_count, d_occ_acc, d_last_accept;  // FC_DIAG_FLIPS_EXACT
    DevBuf<int32_t> d_popk;
    DevBuf<int32_t> d_nfh;     // k > 2: per chain, nodes per foreign-district count (PAIR slot bound)
    DevBuf<uint64_t> d_sbits;  // k = 2 band stream: per chain, the band S as a bitmap (words u64)
    DevBuf<int32_t> d_mcnt, d_ngk;  // k > 2 district-graph rule tables
    DevBuf<fc_event> d_events;
    DevBuf<fc_record> d_trace;
    DevBuf<uint32_t> d_tape;
    int64_t tape_draws = 0;
    DevBuf<int64_t> d_prof;   // FC_PHASE_PROF builds
    DevBuf<uint32_t> d_eta;   // k = 2: per-launch pace of the slowest chain (issue priorities)
    DevBuf<uint32_t> d_deal, d_order, d_ctime;  // k = 2 chain dealing (fc_deal.hip)
    bool deal_timed = false;    // d_ctime holds a launch's per-chain durations
    int64_t n_flip_launches = 0;
    DevBuf<int32_t> d_eu, d_ev;       // recom: canonical edge list
    DevBuf<uint32_t> d_nbe, d_eslot;  // recom: neighbour rows, edge ends' row indices
    DevBuf<uint64_t> d_recom_thresh;  // recom: [2E+1] acceptance thresholds
    DevBuf<int8_t> d_ser_a0;   // FC_DIAG_SERIES: assignment at the series window start
    // The series calls (fc_readout.cpp open_window / OutPack) share two buffers, grown on demand.
    // Every call fills what it reads of them and synchronises before it returns, so nothing is
    // carried from one call to the next
    DevBuf<int64_t> d_ser_meta;  // per call: ev_len, t0, t_end (LogWindow), then |cut| and |B| at the window
                                 // start, of the chains read, [nc] each
    DevBuf<int64_t> d_ser_out;   // per call: the int64 outputs of the election / compactness series,
                                 // one after the other
    DevBuf<double> d_fs_out;   // fc_run_frame_series output (slope, angle), grown on demand
    DevBuf<int32_t> d_fs_cnt;  // ... frame-cut counts
    // fc_run_frame_series_changes, kept across calls (one call per launch in the driver loop):
    // the frame tables (fc_run_frame_series' too; re-uploaded only when the frame changes), per-chain counts / offsets
    // (sized for every chain of the run), and the (t, slope, angle) outputs, grown on demand
    uint64_t fc_frame_hash = 0;
    int32_t fc_rows = 0;  // rows of d_fc_tog
    DevBuf<int64_t> d_fc_wcnt;  // change points per chain and frame-series wave
    DevBuf<int64_t> d_st_t;     // one-pass change points: per-wave staging ranges (t; slope, angle)
    DevBuf<double> d_st_sa;     // [2 * staged entries]
    DevBuf<int32_t> d_fc_fuv, d_fc_tidx;
    DevBuf<uint64_t> d_fc_tog;
    DevBuf<double> d_fc_mid;
    DevBuf<int64_t> d_fc_cnt, d_fc_off;
    DevBuf<int64_t> d_fc_t;
    DevBuf<double> d_fc_sa;     // [2 * change points the outputs hold]
    // election series (fc_run_set_elections; fc_votes.h, fc_votes.hip).  el_n_cols 0: not set
    int32_t el_n_cols = 0, el_n_el = 0, el_n_edges = 0;
    int32_t el_col_a[fc::kVoteMaxElections] = {0}, el_col_b[fc::kVoteMaxElections] = {0};
    int64_t el_col_total[fc::kVoteMaxCols] = {0};  // the columns' sums (fc_run_burst_select's overflow bound)
    DevBuf<int32_t> d_el_cols;    // [n * votes_padded_cols(el_n_cols)]
    DevBuf<int64_t> d_el_edges;   // [el_n_edges]
    DevBuf<int8_t> d_el_cur;      // per call: current-assignment rows when they are not kept in LDS
    // compactness series (fc_run_set_shapes; fc_shapes.h, fc_shapes.hip).  sh_width 0: not set
    int32_t sh_width = 0, sh_n_edges = 0;
    DevBuf<fc::RowSlot> d_sh_rows;     // [n * sh_width] neighbour rows
    DevBuf<fc::ShapeNode> d_sh_nodes;  // [n]
    DevBuf<int64_t> d_sh_edges;   // [sh_n_edges]
    // locality-splits series (fc_run_set_localities; fc_splits.h, fc_splits.hip).  sp_n_loc 0: not set
    int32_t sp_n_loc = 0, sp_x_max = 0;
    DevBuf<int32_t> d_sp_loc;     // [n] node labels
    // plan samples (fc_run_sample_plans; fc_plans.h, fc_plans.hip): no setter, nothing kept but buffers
    DevBuf<int8_t> d_pl_rows;     // per call: the staged plan rows, npad bytes each, grown on demand
    DevBuf<int64_t> d_pl_in;      // per call: times [n_times]
    DevBuf<int32_t> d_pl_pop;     // [npad] node populations, 0 beyond n (uploaded by the first call with pops)
    fc::EventMarks<3> pl_ev;      // last call: before the kernel, after it, after the row copy
    bool pl_timed = false, pl_copied = false;           // (fc_run_sample_plans_ms)
    // heat-map series (fc_run_heat_series; fc_heat.h, fc_heat.hip): no setter; the neighbour / edge rows
    // are built and uploaded by the first call and kept, like the frame tables.  ht_width 0: not yet
    int32_t ht_width = 0;
    int32_t ht_optin = 0;         // the device's opt-in dynamic LDS limit, queried by the first call
    DevBuf<fc::RowSlot> d_ht_rows;   // [n * ht_width]
    fc::EventMarks<2> ht_ev;      // last call: before the kernel, after it
    int32_t ht_form = -1;         // last call that launched: fc::kHeatFormLds / kHeatFormGlobal (-1: none yet)
    int64_t ht_lds = 0;           // ... and the dynamic LDS bytes of its workgroups
    // short bursts (fc_run_burst_select; fc_burst.h, fc_burst.hip): no setter (the vote columns are the
    // election series'); the staged best-plan rows share d_pl_rows
    fc::EventMarks<2> bs_ev;      // last call: before the kernel, after it
    bool bs_timed = false;        // (fc_run_burst_select_ms)
    char kname[96] = {0};       // last launched flip-kernel instance
    // replica exchange (fc_run_set_ladders; fc_ladder.h, fc_exchange.hip).  Slots are flat: ladder
    // l's rung r is slot lad_off[l] + r
    std::vector<int32_t> lad_off, lad_members, lad_slot_ladder;  // [L + 1], [M], [M]
    uint32_t lad_hash = 0;             // hash of the layout, the checkpoint header's word (0: no ladders)
    uint64_t ex_round = 0;             // exchange rounds so far
    int32_t lad_n_items[3] = {0, 0, 0};  // work items of parity 0 / 1 and of the attribute-only pass
    DevBuf<fc::LadderItem> d_lad_items[3];
    DevBuf<fc::LadderSlot> d_lad_slots;
    DevBuf<fc::LadderPair> d_lad_pairs;
    DevBuf<int32_t> d_slot_of, d_chain_at;
    DevBuf<int64_t> d_lad_snap;     // [n_chains * kRungFields]
    DevBuf<fc_rung_stats> d_rung;   // [M]
    DevBuf<int64_t> d_snap_cut, d_snap_nb, d_rung_cut, d_rung_nb;

    // The caller selects the run's device first (fc_run_destroy); the buffers free themselves.
    ~fc_run() {
        for (auto &pr : launch_events) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
        if (stream) (void)hipStreamDestroy(stream);
    }

    // entries per chain the tally log holds (fc_run_diag_paths' "granted")
    int64_t tl_cap() const { return n_chains > 0 ? (int64_t)(d_tl.capacity() / ((size_t)n_chains * 4)) : 0; }
};

// fc_run_sync, then the ChainScalars of chains [c0, c0 + nc) into sc
int download_scalars(fc_run *r, int32_t c0, int32_t nc, std::vector<fc::ChainScalars> &sc);
