// Readouts of a run and the series drivers (fc_series.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "fc_run.h"

// Whether `bytes` more of device memory fit a tenth of what is free: the bound on a buffer that a
// run keeps and a single call sizes (fc_run.h).
int fc::fits_free_tenth(size_t bytes, bool &fits) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    fits = bytes <= free_b / 10;
    return FC_OK;
}

namespace {

// a chain whose event log ran past event_cap has no series to evaluate
int check_event_overflow(const fc_run *r, const char *who, int32_t chain, const fc::ChainScalars &s) {
    if (s.ev_len > r->ev_cap)
        return fail(FC_ERR_ARG, std::string(who) + ": chain " + std::to_string(chain) +
                                    " overflowed event_cap; reset the series window more often");
    return FC_OK;
}

// ---- the driver the series calls share (DESIGN.md §4 "Series window") -------------------------

// what a ReCom run without a move log is told (it has no event buffer: fc_run_create makes one
// for FC_DIAG_SERIES with an event_cap, and the logging kernel instance fills it)
int no_move_log(const std::string &who, const char *pass) {
    return fail(FC_ERR_UNSUPPORTED, who + ": " + pass + " replays the event log, and this ReCom run keeps none; create "
                                        "the run with FC_DIAG_SERIES and an event_cap to log its moves");
}

struct CallRules {
    const char *log_pass = nullptr;   // the pass's name, for a ReCom run without a move log (no_move_log)
    const char *unset = nullptr;      // the setter the pass needs and the run has not had, or null
    const char *k2_only = nullptr;    // the pass follows k = 2 flips: what to say of another run
    const char *flips_only = nullptr; // the pass has an output per flip: what to say of a ReCom run
};

// The checks every series call `who` over chains [c0, c0 + nc) makes of the run and the range,
// before any device work.
int check_series_call(const fc_run *r, const char *who, int32_t c0, int32_t nc, const CallRules &rules) {
    const std::string w(who);
    const bool recom = r->p.proposal == FC_PROPOSE_RECOM;
    if (rules.flips_only && recom) return fail(FC_ERR_UNSUPPORTED, w + ": " + rules.flips_only);
    if (rules.log_pass && recom && !r->d_events) return no_move_log(w, rules.log_pass);
    if (!r->d_events) return fail(FC_ERR_ARG, w + ": FC_DIAG_SERIES not enabled");
    if (rules.unset) return fail(FC_ERR_ARG, w + ": call " + rules.unset + " first");
    if (rules.k2_only && r->p.k != 2) return fail(FC_ERR_UNSUPPORTED, w + ": " + rules.k2_only);
    if (c0 < 0 || nc < 0 || c0 + nc > r->n_chains) return fail(FC_ERR_ARG, w + ": chain range");
    return FC_OK;
}

struct SeriesCall {
    fc::LogWindow log{};
    std::vector<fc::ChainScalars> sc;  // the scalars of chains [c0, c0 + nc)
    const int64_t *cut0 = nullptr, *nb0 = nullptr;  // device, [nc]: |cut| and |B| at the window start
};

// The window of a checked call: the chains' scalars, the per-chain overflow check (and, with
// bound_yields, a window below 2^30 yields), and ev_len, t0, t_end, ser_cut0, ser_nb0, indexed by
// the call-local chain, in r->d_ser_meta.  download_scalars leaves the run idle, so the upload is
// a blocking copy of pageable memory: the window is on the device when this returns.
int open_window(fc_run *r, const char *who, int32_t c0, int32_t nc, bool bound_yields, SeriesCall &s) {
    const std::string w(who);
    s.log = fc::LogWindow{};
    s.log.a0 = r->d_ser_a0;
    s.log.npad = r->npad;
    s.log.n = r->g.n;
    s.log.k = r->p.k;
    s.log.events = r->d_events;
    s.log.ev_cap = r->ev_cap;
    s.log.c0 = c0;
    s.log.nc = nc;
    if (int rc = download_scalars(r, c0, nc, s.sc)) return rc;
    std::vector<int64_t> meta((size_t)5 * nc);
    for (int32_t i = 0; i < nc; ++i) {
        const fc::ChainScalars &x = s.sc[i];
        if (int rc = check_event_overflow(r, who, c0 + i, x)) return rc;
        if (bound_yields && x.steps - x.ser_t0 + 1 >= (int64_t(1) << 30))
            return fail(FC_ERR_ARG, w + ": chain " + std::to_string(c0 + i) +
                                        "'s window has 2^30 yields or more; reset the series window more often");
        meta[i] = x.ev_len;
        meta[(size_t)nc + i] = x.ser_t0;
        meta[(size_t)2 * nc + i] = x.steps + 1;
        meta[(size_t)3 * nc + i] = x.ser_cut0;
        meta[(size_t)4 * nc + i] = x.ser_nb0;
    }
    if (int rc = r->d_ser_meta.grow(meta.size())) return rc;
    HIP_TRY(hipMemcpy(r->d_ser_meta, meta.data(), meta.size() * 8, hipMemcpyHostToDevice));
    s.log.ev_len = r->d_ser_meta;
    s.log.t0 = r->d_ser_meta + nc;
    s.log.t_end = r->d_ser_meta + 2 * (size_t)nc;
    s.cut0 = r->d_ser_meta + 3 * (size_t)nc;
    s.nb0 = r->d_ser_meta + 4 * (size_t)nc;
    return FC_OK;
}

// The int64 outputs of a series call, one after the other in r->d_ser_out.
struct OutPack {
    std::vector<size_t> off;  // [outputs + 1]
    int64_t *dev = nullptr;

    int reserve(fc_run *r, std::initializer_list<size_t> sizes) {
        off.assign(1, 0);
        for (size_t sz : sizes) off.push_back(off.back() + sz);
        if (int rc = r->d_ser_out.grow(off.back())) return rc;
        dev = r->d_ser_out;
        return FC_OK;
    }
    int64_t *at(size_t i) const { return dev + off[i]; }
    // the outputs the caller asked for (a host pointer, a size), then the stream synchronised
    int fetch(fc_run *r, std::initializer_list<int64_t *> host) const {
        size_t i = 0;
        for (int64_t *h : host) {
            if (h && off[i + 1] > off[i])
                HIP_TRY(hipMemcpyAsync(h, at(i), (off[i + 1] - off[i]) * 8, hipMemcpyDeviceToHost, r->stream));
            ++i;
        }
        HIP_TRY(hipStreamSynchronize(r->stream));
        return FC_OK;
    }
};

// histogram edges as fc_run_set_elections / fc_run_set_shapes take them
int check_hist_edges(const char *who, const char *name, int32_t n, int32_t max, const int64_t *edges) {
    const std::string w(who);
    if (n < 0 || n > max) return fail(FC_ERR_ARG, w + ": n_" + name + " must be 0.." + std::to_string(max));
    if (n > 0 && !edges) return fail(FC_ERR_ARG, w + ": null " + name);
    for (int32_t i = 1; i < n; ++i)
        if (edges[i] <= edges[i - 1]) return fail(FC_ERR_ARG, w + ": " + name + " must be strictly ascending");
    return FC_OK;
}

int check_frame_edges(const char *who, int32_t n, int32_t n_frame, const int32_t *frame_u, const int32_t *frame_v) {
    for (int32_t j = 0; j < n_frame; ++j)
        if (frame_u[j] < 0 || frame_u[j] >= n || frame_v[j] < 0 || frame_v[j] >= n || frame_u[j] == frame_v[j])
            return fail(FC_ERR_ARG, std::string(who) + ": frame edge " + std::to_string(j) + " out of range");
    return FC_OK;
}

// the frame kernels' toggle tables: tog_idx[node] is the node's row in tog[.][4] (a 256-bit mask
// of the frame edges incident to it) or -1
void build_toggles(int32_t n, int32_t n_frame, const int32_t *frame_u, const int32_t *frame_v,
                   std::vector<int32_t> &tog_idx, std::vector<uint64_t> &tog) {
    tog_idx.assign(n, -1);
    tog.clear();
    for (int32_t j = 0; j < n_frame; ++j) {
        const int32_t ends[2] = {frame_u[j], frame_v[j]};
        for (int32_t x : ends) {
            if (tog_idx[x] < 0) {
                tog_idx[x] = (int32_t)(tog.size() / 4);
                tog.insert(tog.end(), 4, 0);
            }
            tog[(size_t)tog_idx[x] * 4 + (j >> 6)] |= uint64_t(1) << (j & 63);
        }
    }
}

// The inputs of a frame launch over `log`.  The frame tables are kept by the run and uploaded
// when the frame differs from the last call's (either frame entry point's).
int frame_inputs(fc_run *r, const fc::LogWindow &log, int32_t n_frame, const int32_t *frame_u,
                 const int32_t *frame_v, const double *mid_xy, double cx, double cy, fc::FrameParams &fp) {
    const int32_t n = r->g.n;
    uint64_t h = fnv1a(fc::kFnvBasis, &n_frame, sizeof n_frame);
    h = fnv1a(h, frame_u, (size_t)n_frame * 4);
    h = fnv1a(h, frame_v, (size_t)n_frame * 4);
    h = fnv1a(h, mid_xy, (size_t)n_frame * 16);
    if (!r->d_fc_fuv || h != r->fc_frame_hash) {
        std::vector<int32_t> tog_idx;
        std::vector<uint64_t> tog;
        build_toggles(n, n_frame, frame_u, frame_v, tog_idx, tog);
        int q;
        if ((q = r->d_fc_fuv.alloc((size_t)2 * 256))) return q;
        if ((q = r->d_fc_tidx.alloc((size_t)n))) return q;
        if ((q = r->d_fc_tog.alloc((size_t)4 * 512))) return q;
        if ((q = r->d_fc_mid.alloc((size_t)2 * 256))) return q;
        if (n_frame) {
            HIP_TRY(hipMemcpy(r->d_fc_fuv, frame_u, (size_t)n_frame * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(r->d_fc_fuv + n_frame, frame_v, (size_t)n_frame * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(r->d_fc_mid, mid_xy, (size_t)n_frame * 16, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(r->d_fc_tog, tog.data(), tog.size() * 8, hipMemcpyHostToDevice));
        }
        HIP_TRY(hipMemcpy(r->d_fc_tidx, tog_idx.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        r->fc_frame_hash = h;
        r->fc_rows = (int32_t)(tog.size() / 4);
    }
    fp = fc::FrameParams{};
    fp.log = log;
    fp.n_frame = n_frame;
    fp.fu = r->d_fc_fuv;
    fp.fv = r->d_fc_fuv + n_frame;
    fp.mid = r->d_fc_mid;
    fp.cx = cx;
    fp.cy = cy;
    fp.tog_idx = r->d_fc_tidx;
    fp.tog_mask = r->d_fc_tog;
    fp.n_rows = r->fc_rows;
    return FC_OK;
}

}  // namespace

extern "C" {

int fc_run_read_stats(fc_run *r, fc_chain_stats *out) {
    if (!r || !out) return fail(FC_ERR_ARG, "fc_run_read_stats: null argument");
    std::vector<fc::ChainScalars> sc;
    if (int rc = download_scalars(r, 0, r->n_chains, sc)) return rc;
    for (int32_t c = 0; c < r->n_chains; ++c) {
        const fc::ChainScalars &s = sc[c];
        fc_chain_stats &o = out[c];
        o.steps = s.steps;
        o.proposals = s.proposals;
        o.draws = (int64_t)s.draw;
        o.accepted = s.accepted;
        o.inv_contig = s.inv_contig;
        o.inv_pop = s.inv_pop;
        o.sum_cut = s.sum_cut;
        o.sum_nb = s.sum_nb;
        o.sum_wait = s.sum_wait;
        o.sum_cut2 = s.sum_cut2;
        o.sum_nb2 = s.sum_nb2;
        o.wait_cur = s.wait_cur;
        o.bfs_calls = s.bfs_calls;
        o.bfs_levels = s.bfs_levels;
        o.cut = s.cut;
        o.nb = s.nb;
        o.last_flip = s.last_flip;
        o.stuck = s.stuck;
        o.hit_time = s.hit_time;
        o.events = s.ev_len;
        o.series_t0 = s.ser_t0;
        o.series_cut0 = s.ser_cut0;
        o.series_nb0 = s.ser_nb0;
    }
    return FC_OK;
}

int fc_run_read_state(fc_run *r, int8_t *assign_out) {
    if (!r || !assign_out) return fail(FC_ERR_ARG, "fc_run_read_state: null argument");
    if (int rc = fc_run_sync(r)) return rc;
    std::vector<int8_t> a((size_t)r->n_chains * r->npad);
    HIP_TRY(hipMemcpy(a.data(), r->d_assign, a.size(), hipMemcpyDeviceToHost));
    for (int32_t c = 0; c < r->n_chains; ++c)
        std::memcpy(assign_out + (size_t)c * r->g.n, &a[(size_t)c * r->npad], r->g.n);
    return FC_OK;
}

int fc_run_read_pops(fc_run *r, int64_t *pops_out) {
    if (!r || !pops_out) return fail(FC_ERR_ARG, "fc_run_read_pops: null argument");
    const int k = r->p.k;
    if (k == 2) {
        std::vector<fc::ChainScalars> sc;
        if (int rc = download_scalars(r, 0, r->n_chains, sc)) return rc;
        for (int32_t c = 0; c < r->n_chains; ++c) {
            pops_out[2 * c] = sc[c].pops[0];
            pops_out[2 * c + 1] = sc[c].pops[1];
        }
    } else {
        if (int rc = fc_run_sync(r)) return rc;
        std::vector<int32_t> pk((size_t)r->n_chains * fc::kMaxKGeneral);
        HIP_TRY(hipMemcpy(pk.data(), r->d_popk, pk.size() * 4, hipMemcpyDeviceToHost));
        for (int32_t c = 0; c < r->n_chains; ++c)
            for (int d = 0; d < k; ++d) pops_out[(size_t)c * k + d] = pk[(size_t)c * fc::kMaxKGeneral + d];
    }
    return FC_OK;
}

int fc_run_read_trace(fc_run *r, int32_t chain, fc_record *out, int64_t cap, int64_t *len) {
    if (!r || !out || !len) return fail(FC_ERR_ARG, "fc_run_read_trace: null argument");
    if (chain < 0 || chain >= r->p.trace_chains) return fail(FC_ERR_ARG, "fc_run_read_trace: chain is not traced");
    std::vector<fc::ChainScalars> sc;
    if (int rc = download_scalars(r, chain, 1, sc)) return rc;
    const fc::ChainScalars &s = sc[0];
    const int64_t n = std::min<int64_t>({s.trace_len, r->p.trace_cap, cap});
    HIP_TRY(hipMemcpy(out, r->d_trace + (size_t)chain * r->p.trace_cap, (size_t)n * sizeof(fc_record),
                      hipMemcpyDeviceToHost));
    *len = s.trace_len;
    return FC_OK;
}

int fc_run_read_recom_trace(fc_run *r, int32_t chain, fc_recom_record *out, int64_t cap, int64_t *len) {
    if (!r || !out || !len) return fail(FC_ERR_ARG, "fc_run_read_recom_trace: null argument");
    if (r->p.proposal != FC_PROPOSE_RECOM) return fail(FC_ERR_ARG, "fc_run_read_recom_trace: not a recom run");
    if (chain < 0 || chain >= r->p.trace_chains) return fail(FC_ERR_ARG, "fc_run_read_recom_trace: chain is not traced");
    std::vector<fc::ChainScalars> sc;
    if (int rc = download_scalars(r, chain, 1, sc)) return rc;
    const fc::ChainScalars &s = sc[0];
    const int64_t n = std::min<int64_t>({s.trace_len, r->p.trace_cap, cap});
    static_assert(sizeof(fc_recom_record) == sizeof(fc_record), "trace slots are shared");
    HIP_TRY(hipMemcpy(out, (const fc_recom_record *)r->d_trace.get() + (size_t)chain * r->p.trace_cap,
                      (size_t)n * sizeof(fc_recom_record), hipMemcpyDeviceToHost));
    *len = s.trace_len;
    return FC_OK;
}

int fc_run_trace_reset(fc_run *r) {
    if (!r) return fail(FC_ERR_ARG, "fc_run_trace_reset: null run");
    std::vector<fc::ChainScalars> sc;
    if (int rc = download_scalars(r, 0, r->n_chains, sc)) return rc;
    for (auto &s : sc) s.trace_len = 0;
    HIP_TRY(hipMemcpy(r->d_sc, sc.data(), sc.size() * sizeof(sc[0]), hipMemcpyHostToDevice));
    return FC_OK;
}

int fc_run_read_events(fc_run *r, int32_t chain, fc_event *out, int64_t cap, int64_t *len) {
    if (!r || !len || (cap > 0 && !out)) return fail(FC_ERR_ARG, "fc_run_read_events: null argument");
    if (!r->d_events) return fail(FC_ERR_ARG, "fc_run_read_events: FC_DIAG_SERIES not enabled");
    if (chain < 0 || chain >= r->n_chains) return fail(FC_ERR_ARG, "fc_run_read_events: chain out of range");
    std::vector<fc::ChainScalars> sc;
    if (int rc = download_scalars(r, chain, 1, sc)) return rc;
    const fc::ChainScalars &s = sc[0];
    const int64_t n = std::min<int64_t>({s.ev_len, r->ev_cap, cap});
    if (n > 0)
        HIP_TRY(hipMemcpy(out, r->d_events + (size_t)chain * r->ev_cap, (size_t)n * sizeof(fc_event),
                          hipMemcpyDeviceToHost));
    *len = s.ev_len;
    return FC_OK;
}

int fc_run_series_reset(fc_run *r) {
    if (!r) return fail(FC_ERR_ARG, "fc_run_series_reset: null run");
    std::vector<fc::ChainScalars> sc;
    if (int rc = download_scalars(r, 0, r->n_chains, sc)) return rc;
    for (auto &s : sc) {
        s.ev_len = 0;
        s.ser_t0 = s.steps;
        s.ser_cut0 = s.cut;
        s.ser_nb0 = s.nb;
    }
    HIP_TRY(hipMemcpy(r->d_sc, sc.data(), sc.size() * sizeof(sc[0]), hipMemcpyHostToDevice));
    if (r->d_ser_a0)
        HIP_TRY(hipMemcpy(r->d_ser_a0, r->d_assign, (size_t)r->n_chains * r->npad, hipMemcpyDeviceToDevice));
    return FC_OK;
}

int fc_run_autocorr(fc_run *r, const int32_t *lags, int32_t nlags, int64_t *lag_sums, double *acf) {
    if (!r || !lags || nlags <= 0 || !lag_sums) return fail(FC_ERR_ARG, "fc_run_autocorr: null argument");
    const int32_t C = r->n_chains;
    if (int rc = check_series_call(r, "fc_run_autocorr", 0, C, {})) return rc;
    for (int32_t j = 0; j < nlags; ++j)
        if (lags[j] < 0) return fail(FC_ERR_ARG, "fc_run_autocorr: negative lag");
    SeriesCall s;
    if (int rc = open_window(r, "fc_run_autocorr", 0, C, false, s)) return rc;
    const fc::LogWindow &w = s.log;
    std::vector<int64_t> len(C);
    std::vector<int32_t> cut0(C);
    int64_t max_len = 0;
    for (int32_t c = 0; c < C; ++c) {
        cut0[c] = s.sc[c].ser_cut0;
        len[c] = s.sc[c].steps - s.sc[c].ser_t0 + 1;  // yields t0 .. steps
        max_len = std::max(max_len, len[c]);
    }
    // lag 0 is always evaluated first: it yields the window totals Sx = H_0 and Sxx = P_0
    std::vector<int32_t> lg(nlags + 1);
    lg[0] = 0;
    std::copy(lags, lags + nlags, lg.begin() + 1);
    const int32_t nl = nlags + 1;
    // device scratch: metadata + dense series for a batch of chains (<= 1 GiB)
    const int64_t stride = (max_len + 7) & ~int64_t(7);
    const int32_t batch = (int32_t)std::max<int64_t>(1, std::min<int64_t>({C, 65535, (int64_t(1) << 29) / stride}));
    DevBuf<int64_t> d_len;
    DevBuf<int32_t> d_cut0, d_lags;
    DevBuf<uint16_t> d_x;
    DevBuf<unsigned long long> d_sums;
    int q;
    if ((q = d_len.upload(len))) return q;
    if ((q = d_cut0.upload(cut0))) return q;
    if ((q = d_lags.upload(lg))) return q;
    if ((q = d_x.alloc((size_t)batch * stride))) return q;
    if ((q = d_sums.alloc((size_t)C * nl * 3))) return q;
    HIP_TRY(hipMemsetAsync(d_sums, 0, (size_t)C * nl * 3 * 8, r->stream));
    for (int32_t c0 = 0; c0 < C; c0 += batch) {
        // the window's per-chain arrays from the batch's first chain on: the kernels index them
        // by the chain within the batch
        const int32_t nc = std::min(batch, C - c0);
        int e = fc::launch_series_expand(w.events, w.ev_cap, w.ev_len + c0, w.t0 + c0, d_cut0 + c0, d_len + c0, c0,
                                         nc, stride, max_len, d_x, r->stream);
        if (e) return fail(FC_ERR_HIP, std::string("series expand: ") + hipGetErrorString((hipError_t)e));
        e = fc::launch_series_lagsums(d_x, d_len + c0, c0, nc, stride, max_len, d_lags, nl, d_sums,
                                      r->stream);
        if (e) return fail(FC_ERR_HIP, std::string("series lag sums: ") + hipGetErrorString((hipError_t)e));
    }
    std::vector<int64_t> sums((size_t)C * nl * 3);
    HIP_TRY(hipMemcpyAsync(sums.data(), d_sums, sums.size() * 8, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    for (int32_t c = 0; c < C; ++c) {
        const int64_t *s0 = &sums[(size_t)c * nl * 3];
        const __int128 Sxx = s0[0], Sx = s0[1], T = len[c];
        for (int32_t j = 0; j < nlags; ++j) {
            const int64_t *s = s0 + 3 * (j + 1);
            lag_sums[(size_t)c * nlags + j] = s[0];
            if (!acf) continue;
            const __int128 L = lags[j];
            double v = 0.0;
            if (L < T) {
                // T^2 * sum_{t < T-L} (x_t - m)(x_{t+L} - m), m = Sx / T, in exact integers
                const __int128 num = T * T * (__int128)s[0] - T * Sx * ((__int128)s[1] + s[2]) + (T - L) * Sx * Sx;
                const __int128 den = T * (T * Sxx - Sx * Sx);
                if (den != 0) v = (double)num / (double)den;
            }
            acf[(size_t)c * nlags + j] = v;
        }
    }
    return FC_OK;
}

int fc_run_frame_series(fc_run *r, int32_t c0, int32_t nc, int32_t n_frame, const int32_t *frame_u,
                        const int32_t *frame_v, const double *mid_xy, double cx, double cy, int64_t cap,
                        double *slope, double *angle, int32_t *n_cut, int64_t *len) {
    if (!r || !frame_u || !frame_v || !mid_xy || !slope || !angle || !n_cut || !len)
        return fail(FC_ERR_ARG, "fc_run_frame_series: null argument");
    CallRules rules;
    rules.k2_only = "the frame series follows k = 2 flips (the reference computes boundary_slope only in its "
                    "two-district drivers)";
    rules.flips_only = "a ReCom step moves many nodes at once (a burst of events with one t), and the "
                       "frame series has an entry per event: it follows flip runs only";
    if (int rc = check_series_call(r, "fc_run_frame_series", c0, nc, rules)) return rc;
    if (n_frame < 0 || n_frame > 256) return fail(FC_ERR_UNSUPPORTED, "fc_run_frame_series: at most 256 frame edges");
    const int32_t n = r->g.n;
    if (int rc = check_frame_edges("fc_run_frame_series", n, n_frame, frame_u, frame_v)) return rc;
    if (nc == 0) return FC_OK;
    SeriesCall s;
    if (int rc = open_window(r, "fc_run_frame_series", c0, nc, false, s)) return rc;
    for (int32_t i = 0; i < nc; ++i) {
        if (s.sc[i].ev_len + 1 > cap)
            return fail(FC_ERR_ARG, "fc_run_frame_series: cap < events + 1 for chain " + std::to_string(c0 + i));
        len[i] = s.sc[i].ev_len + 1;
    }
    int q;
    const size_t outn = (size_t)nc * cap;
    // the large outputs are kept by the run (chunked callers ask for similar sizes)
    if ((q = r->d_fs_out.grow(2 * outn))) return q;
    if ((q = r->d_fs_cnt.grow(outn))) return q;
    double *const d_out = r->d_fs_out;
    int32_t *const d_cnt = r->d_fs_cnt;
    fc::FrameParams fp;
    if ((q = frame_inputs(r, s.log, n_frame, frame_u, frame_v, mid_xy, cx, cy, fp))) return q;
    fp.cap = cap;
    fp.slope = d_out;
    fp.angle = d_out + outn;
    fp.n_cut = d_cnt;
    const int e = fc::launch_frame(fp, fc::kFrameEvents, r->stream);
    if (e) return fail(FC_ERR_HIP, std::string("frame series: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipStreamSynchronize(r->stream));
    HIP_TRY(hipMemcpy(slope, d_out, outn * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(angle, d_out + outn, outn * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(n_cut, d_cnt, outn * 4, hipMemcpyDeviceToHost));
    return FC_OK;
}

int fc_run_frame_series_changes(fc_run *r, int32_t c0, int32_t nc, int32_t n_frame, const int32_t *frame_u,
                                const int32_t *frame_v, const double *mid_xy, double cx, double cy, int64_t cap,
                                int64_t *offsets, int64_t *t, double *slope, double *angle) {
    if (!r || !frame_u || !frame_v || !mid_xy || !offsets)
        return fail(FC_ERR_ARG, "fc_run_frame_series_changes: null argument");
    const bool query = !t && !slope && !angle;
    if (!query && (!t || !slope || !angle)) return fail(FC_ERR_ARG, "fc_run_frame_series_changes: null output");
    CallRules rules;
    rules.k2_only = "k = 2 runs only";
    rules.flips_only = "a ReCom step moves many nodes at once (a burst of events with one t), and the "
                       "frame series has an entry per event: it follows flip runs only";
    if (int rc = check_series_call(r, "fc_run_frame_series_changes", c0, nc, rules)) return rc;
    if (n_frame < 0 || n_frame > 256)
        return fail(FC_ERR_UNSUPPORTED, "fc_run_frame_series_changes: at most 256 frame edges");
    const int32_t n = r->g.n;
    if (int rc = check_frame_edges("fc_run_frame_series_changes", n, n_frame, frame_u, frame_v)) return rc;
    offsets[0] = 0;
    if (nc == 0) return FC_OK;
    SeriesCall s;
    if (int rc = open_window(r, "fc_run_frame_series_changes", c0, nc, false, s)) return rc;
    int q;
    if (!r->d_fc_cnt) {
        const size_t C = (size_t)r->n_chains;
        if ((q = r->d_fc_cnt.alloc(C))) return q;
        if ((q = r->d_fc_off.alloc(C))) return q;
        if ((q = r->d_fc_wcnt.alloc(C * fc::kFrameWaves))) return q;
    }
    fc::FrameParams fp;
    if ((q = frame_inputs(r, s.log, n_frame, frame_u, frame_v, mid_xy, cx, cy, fp))) return q;
    fp.cp_cnt = r->d_fc_cnt;
    fp.wcnt = r->d_fc_wcnt;
    // one pass (count and write together) into per-wave staging ranges when they fit a tenth of
    // the free device memory: sized by event_cap, kept by the run
    const int64_t nk = (r->ev_cap + 63) / 64;
    const int64_t sub = 64 * ((nk + fc::kFrameWaves - 1) / fc::kFrameWaves) + 1;
    const int64_t stage_cap = sub * fc::kFrameWaves;
    bool staged = false;
    if (!query && !(r->p.flags & FC_FLAG_SERIES_TWO_PASS)) {
        const size_t want = (size_t)r->n_chains * (size_t)stage_cap;
        if (2 * want > r->d_st_sa.capacity()) {  // (d_st_sa is allocated last: it vouches for d_st_t)
            bool fits = false;
            if ((q = fits_free_tenth(want * 24, fits))) return q;
            if (fits) {
                r->d_st_t.release();  // both go before either comes back
                r->d_st_sa.release();
                if ((q = r->d_st_t.grow(want))) return q;
                if ((q = r->d_st_sa.grow(2 * want))) return q;
            }
        }
        staged = 2 * want <= r->d_st_sa.capacity();
    }
    if (!query) r->series_staged = staged ? 1 : 0;
    const size_t stn = r->d_st_sa.capacity() / 2;  // staging: slope at d_st_sa, angle at d_st_sa + stn
    if (staged) {
        fp.cap = stage_cap;
        fp.t_out = r->d_st_t;
        fp.slope = r->d_st_sa;
        fp.angle = r->d_st_sa + stn;
    }
    // (two passes: the first counts the change points per chain -> offsets)
    int e = fc::launch_frame(fp, staged ? fc::kFrameStage : fc::kFrameCount, r->stream);
    if (e) return fail(FC_ERR_HIP, std::string(staged ? "frame changes (stage): " : "frame changes (count): ") +
                                       hipGetErrorString((hipError_t)e));
    std::vector<int64_t> cnt(nc);
    HIP_TRY(hipMemcpyAsync(cnt.data(), r->d_fc_cnt, (size_t)nc * 8, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    for (int32_t i = 0; i < nc; ++i) offsets[i + 1] = offsets[i] + cnt[i];
    const int64_t total = offsets[nc];
    if (query) return FC_OK;
    if (cap < total)  // offsets are filled: the caller can size its buffers and call again
        return fail(FC_ERR_ARG, "fc_run_frame_series_changes: cap " + std::to_string(cap) + " < " +
                                    std::to_string(total) + " change points (offsets[nc])");
    if (2 * (size_t)total > r->d_fc_sa.capacity()) {  // (d_fc_sa is allocated last: it vouches for d_fc_t)
        const size_t want = (size_t)total + (size_t)total / 4 + 1024;  // headroom: one allocation per run
        r->d_fc_t.release();  // both go before either comes back
        r->d_fc_sa.release();
        if ((q = r->d_fc_t.grow(want))) return q;
        if ((q = r->d_fc_sa.grow(2 * want))) return q;
    }
    // pass 2: (t, slope, angle) at the offsets, then one copy per array
    HIP_TRY(hipMemcpyAsync(r->d_fc_off, offsets, (size_t)nc * 8, hipMemcpyHostToDevice, r->stream));
    double *const d_sl = r->d_fc_sa, *const d_an = r->d_fc_sa + r->d_fc_sa.capacity() / 2;
    if (staged) {  // the staged ranges packed at the offsets
        e = fc::launch_frame_compact(nc, stage_cap, r->d_st_t, r->d_st_sa, r->d_st_sa + stn, r->d_fc_wcnt, r->d_fc_off,
                                     r->d_fc_t, d_sl, d_an, r->stream);
    } else {
        fp.cp_off = r->d_fc_off;
        fp.t_out = r->d_fc_t;
        fp.slope = d_sl;
        fp.angle = d_an;
        e = fc::launch_frame(fp, fc::kFrameWrite, r->stream);
    }
    if (e) return fail(FC_ERR_HIP, std::string("frame changes (write): ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipMemcpyAsync(t, r->d_fc_t, (size_t)total * 8, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipMemcpyAsync(slope, d_sl, (size_t)total * 8, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipMemcpyAsync(angle, d_an, (size_t)total * 8, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return FC_OK;
}

// ---- election series (fc_votes.h, fc_votes.hip) -------------------------------

int fc_election_eval(int32_t k, const int64_t *a, const int64_t *b, int32_t *seats, int64_t *gap) {
    if (!a || !b) return fail(FC_ERR_ARG, "fc_election_eval: null argument");
    if (k < 1 || k > fc::kMaxKGeneral) return fail(FC_ERR_ARG, "fc_election_eval: k must be 1..32");
    int32_t s = 0;
    int64_t gsum = 0;
    for (int32_t d = 0; d < k; ++d) {
        if (a[d] < 0 || b[d] < 0 || a[d] > INT32_MAX || b[d] > INT32_MAX)
            return fail(FC_ERR_ARG, "fc_election_eval: tallies must be in 0 .. 2^31 - 1");
        int32_t w;
        int64_t g;
        fc::election_rule(a[d], b[d], w, g);
        s += w;
        gsum += g;
    }
    if (seats) *seats = s;
    if (gap) *gap = gsum;
    return FC_OK;
}

int fc_run_set_elections(fc_run *r, int32_t n_cols, const int32_t *node_cols, int32_t n_elections,
                         const int32_t *col_a, const int32_t *col_b, int32_t n_gap_edges, const int64_t *gap_edges) {
    if (!r || !node_cols) return fail(FC_ERR_ARG, "fc_run_set_elections: null argument");
    if (r->p.proposal == FC_PROPOSE_RECOM && !r->d_events) return no_move_log("fc_run_set_elections", "the election series");
    if (!r->d_events) return fail(FC_ERR_ARG, "fc_run_set_elections: FC_DIAG_SERIES not enabled");
    if (n_cols < 1 || n_cols > fc::kVoteMaxCols) return fail(FC_ERR_ARG, "fc_run_set_elections: n_cols must be 1..8");
    if (n_elections < 0 || n_elections > fc::kVoteMaxElections)
        return fail(FC_ERR_ARG, "fc_run_set_elections: n_elections must be 0..4");
    if (n_elections > 0 && (!col_a || !col_b)) return fail(FC_ERR_ARG, "fc_run_set_elections: null election columns");
    if (int rc = check_hist_edges("fc_run_set_elections", "gap_edges", n_gap_edges, fc::kVoteMaxEdges, gap_edges))
        return rc;
    const int32_t n = r->g.n;
    int64_t col_total[fc::kVoteMaxCols] = {0};
    for (int32_t j = 0; j < n_cols; ++j) {
        int64_t tot = 0;
        for (int32_t u = 0; u < n; ++u) {
            const int32_t x = node_cols[(size_t)u * n_cols + j];
            if (x < 0)
                return fail(FC_ERR_ARG, "fc_run_set_elections: negative value in column " + std::to_string(j));
            tot += x;
        }
        if (tot > INT32_MAX)
            return fail(FC_ERR_ARG, "fc_run_set_elections: column " + std::to_string(j) + " totals over 2^31 - 1");
        col_total[j] = tot;
    }
    for (int32_t e = 0; e < n_elections; ++e)
        if (col_a[e] < 0 || col_a[e] >= n_cols || col_b[e] < 0 || col_b[e] >= n_cols || col_a[e] == col_b[e])
            return fail(FC_ERR_ARG, "fc_run_set_elections: election " + std::to_string(e) +
                                        " needs two different columns below n_cols");
    // rows padded to the kernel instance's column count
    const int32_t ncp = fc::votes_padded_cols(n_cols);
    std::vector<int32_t> cols((size_t)n * ncp, 0);
    for (int32_t u = 0; u < n; ++u)
        std::copy(node_cols + (size_t)u * n_cols, node_cols + (size_t)(u + 1) * n_cols, cols.begin() + (size_t)u * ncp);
    if (int rc = fc_run_sync(r)) return rc;  // a reader of the previous tables may still run
    r->el_n_cols = 0;
    if (int rc = r->d_el_cols.upload(cols)) return rc;
    if (int rc = r->d_el_edges.upload(gap_edges, (size_t)n_gap_edges)) return rc;
    for (int32_t e = 0; e < fc::kVoteMaxElections; ++e) {
        r->el_col_a[e] = e < n_elections ? col_a[e] : 0;
        r->el_col_b[e] = e < n_elections ? col_b[e] : 0;
    }
    std::copy(col_total, col_total + fc::kVoteMaxCols, r->el_col_total);
    r->el_n_el = n_elections;
    r->el_n_edges = n_gap_edges;
    r->el_n_cols = n_cols;
    return FC_OK;
}

int fc_run_election_series(fc_run *r, int32_t c0, int32_t nc, int64_t *tally_now, int64_t *tally_sum,
                           int64_t *seats_hist, int64_t *wins_sum, int64_t *gap_sum, int64_t *gap_hist) {
    if (!r) return fail(FC_ERR_ARG, "fc_run_election_series: null run");
    if (int rc = check_series_call(r, "fc_run_election_series", c0, nc,
                                   {"the election series", r->el_n_cols ? nullptr : "fc_run_set_elections"}))
        return rc;
    if (gap_hist && r->el_n_edges == 0)
        return fail(FC_ERR_ARG, "fc_run_election_series: gap_hist needs gap_edges (fc_run_set_elections)");
    if (nc == 0) return FC_OK;
    SeriesCall s;
    if (int rc = open_window(r, "fc_run_election_series", c0, nc, true, s)) return rc;
    const int32_t k = r->p.k, n_cols = r->el_n_cols, n_el = r->el_n_el, n_edges = r->el_n_edges;
    OutPack out;
    int q;
    if ((q = out.reserve(r, {(size_t)nc * k * n_cols, (size_t)nc * k * n_cols, (size_t)nc * n_el * (k + 1),
                             (size_t)nc * n_el * k, (size_t)nc * n_el, (size_t)nc * n_el * (n_edges + 1)})))
        return q;
    const bool global_cur = (r->p.flags & FC_FLAG_VOTES_GLOBAL_CUR) || !fc::votes_cur_in_lds(r->npad, k, n_edges);
    if (global_cur && (q = r->d_el_cur.grow((size_t)nc * r->npad))) return q;
    fc::VotesParams vp{};
    vp.log = s.log;
    vp.cols = r->d_el_cols;
    vp.n_cols = n_cols;
    vp.n_el = n_el;
    for (int e = 0; e < fc::kVoteMaxElections; ++e) {
        vp.col_a[e] = r->el_col_a[e];
        vp.col_b[e] = r->el_col_b[e];
    }
    vp.n_edges = n_edges;
    vp.edges = r->d_el_edges;
    vp.cur = global_cur ? r->d_el_cur.get() : nullptr;
    vp.tally_now = out.at(0);
    vp.tally_sum = out.at(1);
    vp.seats_hist = out.at(2);
    vp.wins_sum = out.at(3);
    vp.gap_sum = out.at(4);
    vp.gap_hist = out.at(5);
    const int e = fc::launch_votes(vp, global_cur, r->stream);
    if (e) return fail(FC_ERR_HIP, std::string("election series: ") + hipGetErrorString((hipError_t)e));
    return out.fetch(r, {tally_now, tally_sum, seats_hist, wins_sum, gap_sum, gap_hist});
}

// ---- compactness series (fc_shapes.h, fc_shapes.hip) ---------------------------

int fc_shape_score(int64_t area, int64_t perim, int64_t *q) {
    if (!q) return fail(FC_ERR_ARG, "fc_shape_score: null argument");
    if (area < 0 || perim < 0 || area > INT32_MAX || perim > INT32_MAX)
        return fail(FC_ERR_ARG, "fc_shape_score: area and perim must be in 0 .. 2^31 - 1");
    *q = fc::shape_score(area, perim);
    return FC_OK;
}

int fc_run_set_shapes(fc_run *r, const int32_t *node_area, const int32_t *node_ext, const int32_t *edge_len,
                      int32_t n_pp_edges, const int64_t *pp_edges) {
    if (!r || !node_area) return fail(FC_ERR_ARG, "fc_run_set_shapes: null argument");
    if (r->p.proposal == FC_PROPOSE_RECOM && !r->d_events) return no_move_log("fc_run_set_shapes", "the compactness series");
    if (!r->d_events) return fail(FC_ERR_ARG, "fc_run_set_shapes: FC_DIAG_SERIES not enabled");
    const int32_t n = r->g.n, E = r->g.n_edges;
    if (E > 0 && !edge_len) return fail(FC_ERR_ARG, "fc_run_set_shapes: null edge_len");
    if (int rc = check_hist_edges("fc_run_set_shapes", "pp_edges", n_pp_edges, fc::kShapeMaxEdges, pp_edges)) return rc;
    int64_t area = 0, perim = 0;
    for (int32_t u = 0; u < n; ++u) {
        if (node_area[u] < 0 || (node_ext && node_ext[u] < 0))
            return fail(FC_ERR_ARG, "fc_run_set_shapes: negative area or exterior length at node " + std::to_string(u));
        area += node_area[u];
        perim += node_ext ? node_ext[u] : 0;
    }
    for (int32_t e = 0; e < E; ++e) {
        if (edge_len[e] < 0) return fail(FC_ERR_ARG, "fc_run_set_shapes: negative length at edge " + std::to_string(e));
        perim += edge_len[e];
    }
    if (area > INT32_MAX) return fail(FC_ERR_ARG, "fc_run_set_shapes: node_area totals over 2^31 - 1");
    if (perim > INT32_MAX)
        return fail(FC_ERR_ARG, "fc_run_set_shapes: node_ext and edge_len together total over 2^31 - 1");
    const int32_t W = fc::row_width(r->g.max_degree);
    if (W == 0) return fail(FC_ERR_UNSUPPORTED, "fc_run_set_shapes: node degree above 16");
    if (!fc::shapes_fit_lds(r->npad, r->p.k, n_pp_edges, W))
        return fail(FC_ERR_UNSUPPORTED,
                    "fc_run_set_shapes: a chain's image (" +
                        std::to_string(fc::shapes_lds_bytes(r->npad, r->p.k, n_pp_edges, W)) +
                        " bytes: assignment, histograms, neighbour rows) does not fit 48 KB of LDS");
    // the neighbour rows: every canonical edge, with its length, in the rows of both its ends
    std::vector<fc::RowSlot> rows;
    fc::build_rows(n, E, r->g.eu.data(), r->g.ev.data(), W, edge_len, 0, rows);
    std::vector<fc::ShapeNode> nodes(n);
    for (int32_t u = 0; u < n; ++u) nodes[u] = fc::ShapeNode{node_area[u], node_ext ? node_ext[u] : 0};
    if (int rc = fc_run_sync(r)) return rc;  // a reader of the previous tables may still run
    r->sh_width = 0;
    if (int rc = r->d_sh_rows.upload(rows)) return rc;
    if (int rc = r->d_sh_nodes.upload(nodes)) return rc;
    if (int rc = r->d_sh_edges.upload(pp_edges, (size_t)n_pp_edges)) return rc;
    r->sh_n_edges = n_pp_edges;
    r->sh_width = W;
    return FC_OK;
}

int fc_run_shape_series(fc_run *r, int32_t c0, int32_t nc, int64_t *area_now, int64_t *perim_now, int64_t *perim_sum,
                        int64_t *pp_now, int64_t *pp_sum, int64_t *pp_min_sum, int64_t *pp_hist,
                        int64_t *pp_min_hist) {
    if (!r) return fail(FC_ERR_ARG, "fc_run_shape_series: null run");
    if (int rc = check_series_call(r, "fc_run_shape_series", c0, nc,
                                   {"the compactness series", r->sh_width ? nullptr : "fc_run_set_shapes"}))
        return rc;
    if ((pp_hist || pp_min_hist) && r->sh_n_edges == 0)
        return fail(FC_ERR_ARG, "fc_run_shape_series: the histograms need pp_edges (fc_run_set_shapes)");
    if (nc == 0) return FC_OK;
    SeriesCall s;
    if (int rc = open_window(r, "fc_run_shape_series", c0, nc, true, s)) return rc;
    const int32_t k = r->p.k, n_edges = r->sh_n_edges;
    const size_t ck = (size_t)nc * k, nbins = (size_t)n_edges + 1;
    OutPack out;
    if (int rc = out.reserve(r, {ck, ck, ck, ck, ck, (size_t)nc, ck * nbins, (size_t)nc * nbins})) return rc;
    fc::ShapesParams sp{};
    sp.log = s.log;
    sp.rows = r->d_sh_rows;
    sp.nodes = r->d_sh_nodes;
    sp.width = r->sh_width;
    sp.n_edges = n_edges;
    sp.edges = r->d_sh_edges;
    sp.area_now = out.at(0);
    sp.perim_now = out.at(1);
    sp.perim_sum = out.at(2);
    sp.pp_now = out.at(3);
    sp.pp_sum = out.at(4);
    sp.pp_min_sum = out.at(5);
    sp.pp_hist = out.at(6);
    sp.pp_min_hist = out.at(7);
    const int e = fc::launch_shapes(sp, r->stream);
    if (e) return fail(FC_ERR_HIP, std::string("compactness series: ") + hipGetErrorString((hipError_t)e));
    // (without pp_edges the kernel writes no histogram, and the check above has left no pointer to one)
    return out.fetch(r, {area_now, perim_now, perim_sum, pp_now, pp_sum, pp_min_sum, pp_hist, pp_min_hist});
}

// ---- locality-splits series (fc_splits.h, fc_splits.hip) ------------------------

int fc_splits_eval(int32_t n_loc, int32_t k, const int64_t *cells, int64_t *splits, int64_t *excess, int64_t *sq) {
    if (!cells) return fail(FC_ERR_ARG, "fc_splits_eval: null argument");
    if (n_loc < 1) return fail(FC_ERR_ARG, "fc_splits_eval: n_loc must be at least 1");
    if (k < 1 || k > fc::kMaxKGeneral) return fail(FC_ERR_ARG, "fc_splits_eval: k must be 1..32");
    int64_t s = 0, x = 0, q = 0;
    for (int32_t c = 0; c < n_loc; ++c) {
        // the locality's nodes enter its cells one by one, by the rule the device applies per flip
        int32_t parts = 0, split = 0;
        for (int32_t d = 0; d < k; ++d) {
            const int64_t cnt = cells[(size_t)c * k + d];
            if (cnt < 0 || cnt > fc::kSplitCellMax)
                return fail(FC_ERR_ARG, "fc_splits_eval: cells must be in 0 .. 65535");
            for (int32_t i = 0; i < (int32_t)cnt; ++i) {
                int32_t dp, ds;
                int64_t dq;
                fc::split_rule(i, +1, parts, dp, ds, dq);
                parts += dp;
                split += ds;
                q += dq;
            }
        }
        if (parts == 0) return fail(FC_ERR_ARG, "fc_splits_eval: locality " + std::to_string(c) + " has no node");
        s += split;
        x += parts - 1;
    }
    if (splits) *splits = s;
    if (excess) *excess = x;
    if (sq) *sq = q;
    return FC_OK;
}

int fc_run_set_localities(fc_run *r, int32_t n_loc, const int32_t *node_loc) {
    if (!r || !node_loc) return fail(FC_ERR_ARG, "fc_run_set_localities: null argument");
    if (r->p.proposal == FC_PROPOSE_RECOM && !r->d_events)
        return no_move_log("fc_run_set_localities", "the locality-splits series");
    if (!r->d_events) return fail(FC_ERR_ARG, "fc_run_set_localities: FC_DIAG_SERIES not enabled");
    const int32_t n = r->g.n, k = r->p.k;
    if (n_loc < 1 || n_loc > n) return fail(FC_ERR_ARG, "fc_run_set_localities: n_loc must be 1..n");
    std::vector<int32_t> size(n_loc, 0);
    for (int32_t u = 0; u < n; ++u) {
        if (node_loc[u] < 0 || node_loc[u] >= n_loc)
            return fail(FC_ERR_ARG, "fc_run_set_localities: label of node " + std::to_string(u) + " out of range");
        ++size[node_loc[u]];
    }
    int64_t x_max = -(int64_t)n_loc;
    for (int32_t c = 0; c < n_loc; ++c) {
        if (size[c] == 0) return fail(FC_ERR_ARG, "fc_run_set_localities: label " + std::to_string(c) + " is unused");
        x_max += std::min(size[c], k);
    }
    const int32_t x_top = (int32_t)std::min<int64_t>(x_max, fc::kSplitMaxExcess);
    if (!fc::splits_fit_lds(r->npad, k, n_loc, x_top))
        return fail(FC_ERR_UNSUPPORTED,
                    "fc_run_set_localities: a chain's image (" +
                        std::to_string(fc::splits_lds_bytes(r->npad, k, n_loc, x_top)) +
                        " bytes: assignment, cell table, integrals, histograms) does not fit 48 KB of LDS");
    if (int rc = fc_run_sync(r)) return rc;  // a reader of the previous table may still run
    r->sp_n_loc = 0;
    if (int rc = r->d_sp_loc.upload(node_loc, (size_t)n)) return rc;
    r->sp_x_max = (int32_t)x_max;
    r->sp_n_loc = n_loc;
    return FC_OK;
}

int fc_run_split_series(fc_run *r, int32_t c0, int32_t nc, int64_t *cells_now, int64_t *split_sum, int64_t *parts_sum,
                        int64_t *dlocs_sum, int64_t *sq_sum, int64_t *splits_hist, int64_t *excess_hist) {
    if (!r) return fail(FC_ERR_ARG, "fc_run_split_series: null run");
    if (int rc = check_series_call(r, "fc_run_split_series", c0, nc,
                                   {"the locality-splits series", r->sp_n_loc ? nullptr : "fc_run_set_localities"}))
        return rc;
    if (nc == 0) return FC_OK;
    SeriesCall s;
    if (int rc = open_window(r, "fc_run_split_series", c0, nc, true, s)) return rc;
    const int32_t k = r->p.k, L = r->sp_n_loc;
    const int32_t x_top = std::min(r->sp_x_max, fc::kSplitMaxExcess);
    const size_t cn = (size_t)nc;
    OutPack out;
    if (int rc = out.reserve(r, {cn * L * k, cn * L, cn * L, cn * k, cn, cn * ((size_t)L + 1), cn * ((size_t)x_top + 1)}))
        return rc;
    fc::SplitsParams sp{};
    sp.log = s.log;
    sp.node_loc = r->d_sp_loc;
    sp.n_loc = L;
    sp.x_top = x_top;
    sp.cells_now = out.at(0);
    sp.split_sum = out.at(1);
    sp.parts_sum = out.at(2);
    sp.dlocs_sum = out.at(3);
    sp.sq_sum = out.at(4);
    sp.splits_hist = out.at(5);
    sp.excess_hist = out.at(6);
    const int e = fc::launch_splits(sp, r->stream);
    if (e) return fail(FC_ERR_HIP, std::string("locality-splits series: ") + hipGetErrorString((hipError_t)e));
    return out.fetch(r, {cells_now, split_sum, parts_sum, dlocs_sum, sq_sum, splits_hist, excess_hist});
}

// ---- plan samples (fc_plans.h, fc_plans.hip) ------------------------------------

int fc_run_sample_plans(fc_run *r, int32_t c0, int32_t nc, int32_t n_times, const int64_t *times, int8_t *plans,
                        int64_t *cut, int64_t *nb, int64_t *dist0, int64_t *pops) {
    const char *const who = "fc_run_sample_plans";
    if (!r) return fail(FC_ERR_ARG, "fc_run_sample_plans: null run");
    CallRules rules;
    rules.log_pass = "sampling plans";
    if (int rc = check_series_call(r, who, c0, nc, rules)) return rc;
    if (n_times < 0) return fail(FC_ERR_ARG, "fc_run_sample_plans: n_times must be at least 0");
    if (n_times > 0 && !times) return fail(FC_ERR_ARG, "fc_run_sample_plans: null times");
    for (int32_t j = 1; j < n_times; ++j)
        if (times[j] <= times[j - 1]) return fail(FC_ERR_ARG, "fc_run_sample_plans: times must be strictly increasing");
    if (nc == 0 || n_times == 0) return FC_OK;
    SeriesCall s;
    if (int rc = open_window(r, who, c0, nc, false, s)) return rc;
    for (int32_t i = 0; i < nc; ++i) {
        const fc::ChainScalars &x = s.sc[i];
        if (times[0] < x.ser_t0)
            return fail(FC_ERR_ARG, "fc_run_sample_plans: chain " + std::to_string(c0 + i) + ": time " +
                                        std::to_string(times[0]) + " is before the window's first yield " +
                                        std::to_string(x.ser_t0));
        if (times[n_times - 1] > x.steps)
            return fail(FC_ERR_ARG, "fc_run_sample_plans: chain " + std::to_string(c0 + i) + ": time " +
                                        std::to_string(times[n_times - 1]) + " is after the chain's last yield " +
                                        std::to_string(x.steps));
    }
    const size_t cn = (size_t)nc, nt = (size_t)n_times, npad = (size_t)r->npad;
    const int32_t k = r->p.k, n = r->g.n;
    int q;
    // the staged rows are kept by the run; a larger call has to fit a tenth of the free device memory
    // (behind them, when the rows have padding, the same rows packed to n bytes)
    const size_t want = plans ? cn * nt * npad : 0;
    const size_t held = want + (plans && npad != (size_t)n ? cn * nt * (size_t)n : 0);
    if (held > r->d_pl_rows.capacity()) {
        bool fits = false;
        if ((q = fits_free_tenth(want, fits))) return q;
        if (!fits)
            return fail(FC_ERR_ARG, "fc_run_sample_plans: " + std::to_string(want) + " bytes of staged plans (" +
                                        std::to_string(nc) + " chains x " + std::to_string(n_times) + " times x " +
                                        std::to_string(npad) + ") exceed a tenth of the free device memory; " +
                                        "split the call by chains or by times");
        if ((q = r->d_pl_rows.grow(held))) return q;
    }
    if (pops && !r->d_pl_pop) {
        std::vector<int32_t> pp(npad, 0);
        std::copy(r->g.pop.begin(), r->g.pop.begin() + n, pp.begin());
        if ((q = r->d_pl_pop.upload(pp))) return q;
    }
    // the times (open_window has left the run idle)
    if ((q = r->d_pl_in.grow(nt))) return q;
    HIP_TRY(hipMemcpy(r->d_pl_in, times, nt * 8, hipMemcpyHostToDevice));
    OutPack out;
    if ((q = out.reserve(r, {cn * nt, cn * nt, cn * nt, cn * nt * k}))) return q;
    fc::PlansParams pp{};
    pp.log = s.log;
    pp.n_times = n_times;
    pp.times = r->d_pl_in;
    pp.cut0 = s.cut0;
    pp.nb0 = s.nb0;
    pp.node_pop = r->d_pl_pop;
    pp.plans = plans ? r->d_pl_rows.get() : nullptr;
    pp.cut = cut ? out.at(0) : nullptr;
    pp.nb = nb ? out.at(1) : nullptr;
    pp.dist0 = dist0 ? out.at(2) : nullptr;
    pp.pops = pops ? out.at(3) : nullptr;
    r->pl_timed = false;
    if ((q = r->pl_ev.mark(0, r->stream))) return q;
    const int e = fc::launch_plans(pp, r->stream);
    if (e) return fail(FC_ERR_HIP, std::string("plan samples: ") + hipGetErrorString((hipError_t)e));
    if ((q = r->pl_ev.mark(1, r->stream))) return q;
    // the rows, packed to n bytes: one strided copy, pitch npad -> n, on the device, then one
    // contiguous copy to the host (as every other reader's: no pitched copy into pageable memory)
    if (plans) {
        const int8_t *src = r->d_pl_rows;
        if (npad != (size_t)n) {
            int8_t *packed = r->d_pl_rows + want;
            HIP_TRY(hipMemcpy2DAsync(packed, (size_t)n, src, npad, (size_t)n, cn * nt, hipMemcpyDeviceToDevice, r->stream));
            src = packed;
        }
        HIP_TRY(hipMemcpyAsync(plans, src, cn * nt * (size_t)n, hipMemcpyDeviceToHost, r->stream));
    }
    if ((q = r->pl_ev.mark(2, r->stream))) return q;
    if (int rc = out.fetch(r, {cut, nb, dist0, pops})) return rc;
    r->pl_timed = true;
    r->pl_copied = plans != nullptr;
    return FC_OK;
}

int fc_run_sample_plans_ms(fc_run *r, float *kernel_ms, float *copy_ms) {
    if (!r) return fail(FC_ERR_ARG, "fc_run_sample_plans_ms: null run");
    if (!r->pl_timed) return fail(FC_ERR_ARG, "fc_run_sample_plans_ms: no fc_run_sample_plans call recorded");
    if (kernel_ms)
        if (int rc = r->pl_ev.elapsed(0, 1, kernel_ms)) return rc;
    if (copy_ms) {
        *copy_ms = 0.f;
        if (r->pl_copied) return r->pl_ev.elapsed(1, 2, copy_ms);
    }
    return FC_OK;
}

// ---- heat-map series (fc_heat.h, fc_heat.hip) -----------------------------------

int fc_run_heat_series(fc_run *r, int32_t c0, int32_t nc, uint32_t flags, int64_t *cut_hist, int64_t *nb_hist,
                       int64_t *cut_times, int64_t *moves, int64_t *last_move, int64_t *dwell) {
    const char *const who = "fc_run_heat_series";
    if (!r) return fail(FC_ERR_ARG, "fc_run_heat_series: null run");
    CallRules rules;
    rules.log_pass = "the heat-map series";
    if (int rc = check_series_call(r, who, c0, nc, rules)) return rc;
    if (flags & ~(uint32_t)FC_HEAT_LDS_ROWS) return fail(FC_ERR_ARG, "fc_run_heat_series: unknown flags");
    if (nc == 0) return FC_OK;
    SeriesCall s;
    if (int rc = open_window(r, who, c0, nc, true, s)) return rc;
    const int32_t n = r->g.n, k = r->p.k, E = r->g.n_edges, nbw = r->nb_w;
    int64_t *const host[fc::kHeatArrays] = {cut_hist, nb_hist, cut_times, moves, last_move, dwell};
    const size_t cn = (size_t)nc;
    size_t len[fc::kHeatArrays], total = 0;
    uint32_t mask = 0;
    for (int a = 0; a < fc::kHeatArrays; ++a) {
        len[a] = host[a] ? cn * fc::heat_row_len(a, n, k, E, nbw) : 0;
        total += len[a];
        if (host[a]) mask |= 1u << a;
    }
    if (!mask) return FC_OK;
    int q;
    // the outputs are kept by the run; a larger call has to fit a tenth of the free device memory
    if (total > r->d_ser_out.capacity()) {
        bool fits = false;
        if ((q = fits_free_tenth(total * 8, fits))) return q;
        if (!fits)
            return fail(FC_ERR_ARG, "fc_run_heat_series: " + std::to_string(total * 8) + " bytes of outputs (" +
                                        std::to_string(nc) + " chains) exceed a tenth of the free device memory; " +
                                        "split the call by chains");
    }
    // the neighbour / edge rows and the device's LDS limit: once per run
    if (!r->ht_width) {
        const int32_t W = fc::row_width(r->g.max_degree);
        if (W == 0) return fail(FC_ERR_UNSUPPORTED, "fc_run_heat_series: node degree above 16");
        std::vector<fc::RowSlot> rows;
        fc::build_rows(n, E, r->g.eu.data(), r->g.ev.data(), W, nullptr, -1, rows);
        if ((q = r->d_ht_rows.upload(rows))) return q;
        int dev = 0, optin = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess || optin <= 0)
            optin = 65536;
        r->ht_optin = optin;
        r->ht_width = W;
    }
    const size_t image = fc::heat_lds_bytes(r->npad, n, k, E, nbw, r->ht_width, mask);
    // the global-rows form unless the LDS form is asked for and the image fits (with one
    // workgroup per compute unit the LDS form measured slower)
    const int32_t form =
        (flags & FC_HEAT_LDS_ROWS) && image <= (size_t)r->ht_optin ? fc::kHeatFormLds : fc::kHeatFormGlobal;
    OutPack out;
    if ((q = out.reserve(r, {len[0], len[1], len[2], len[3], len[4], len[5]}))) return q;
    fc::HeatParams hp{};
    hp.log = s.log;
    hp.rows = r->d_ht_rows;
    hp.width = r->ht_width;
    hp.n_edges = E;
    hp.nb_width = nbw;
    hp.cut0 = s.cut0;
    hp.nb0 = s.nb0;
    hp.cut_hist = cut_hist ? out.at(0) : nullptr;
    hp.nb_hist = nb_hist ? out.at(1) : nullptr;
    hp.cut_times = cut_times ? out.at(2) : nullptr;
    hp.moves = moves ? out.at(3) : nullptr;
    hp.last_move = last_move ? out.at(4) : nullptr;
    hp.dwell = dwell ? out.at(5) : nullptr;
    r->ht_form = -1;
    if ((q = r->ht_ev.mark(0, r->stream))) return q;
    const int e = fc::launch_heat(hp, form, r->stream);
    if (e) return fail(FC_ERR_HIP, std::string("heat-map series: ") + hipGetErrorString((hipError_t)e));
    if ((q = r->ht_ev.mark(1, r->stream))) return q;
    if (int rc = out.fetch(r, {cut_hist, nb_hist, cut_times, moves, last_move, dwell})) return rc;
    r->ht_form = form;
    r->ht_lds = (int64_t)(form == fc::kHeatFormLds ? image : fc::heat_base_bytes(r->npad, r->ht_width));
    return FC_OK;
}

int fc_run_heat_series_info(fc_run *r, int32_t *form, int64_t *lds_bytes, float *kernel_ms) {
    if (!r) return fail(FC_ERR_ARG, "fc_run_heat_series_info: null run");
    if (r->ht_form < 0) return fail(FC_ERR_ARG, "fc_run_heat_series_info: no fc_run_heat_series call recorded");
    if (form) *form = r->ht_form;
    if (lds_bytes) *lds_bytes = r->ht_lds;
    return kernel_ms ? r->ht_ev.elapsed(0, 1, kernel_ms) : FC_OK;
}

// ---- short bursts (fc_burst.h, fc_burst.hip) ------------------------------------

int fc_burst_metric_init(fc_burst_metric *m, uint32_t struct_size) {
    if (!m) return fail(FC_ERR_ARG, "fc_burst_metric_init: null metric");
    if (struct_size != sizeof(fc_burst_metric))
        return fail(FC_ERR_ARG, "fc_burst_metric_init: struct_size is not sizeof(fc_burst_metric)");
    std::memset(m, 0, sizeof *m);
    m->struct_size = struct_size;
    m->kind = FC_BURST_CUT;
    m->num = 1;
    m->den = 2;
    m->maximize = 1;
    return FC_OK;
}

int fc_burst_eval(const fc_burst_metric *m, int32_t k, const int64_t *a, const int64_t *b, int64_t cut,
                  int64_t *score) {
    if (!m || !score) return fail(FC_ERR_ARG, "fc_burst_eval: null argument");
    if (const char *bad = fc::burst_metric_error(*m, 0, nullptr)) return fail(FC_ERR_ARG, std::string("fc_burst_eval: ") + bad);
    if (k < 1 || k > fc::kMaxKGeneral) return fail(FC_ERR_ARG, "fc_burst_eval: k must be 1..32");
    if (cut < 0) return fail(FC_ERR_ARG, "fc_burst_eval: negative cut");
    int64_t cnt = 0, gsum = 0;
    if (fc::burst_votes_kind(m->kind)) {
        if (!a || !b) return fail(FC_ERR_ARG, "fc_burst_eval: null tallies");
        int64_t total = 0;
        for (int32_t d = 0; d < k; ++d) {
            // (each term below 2^62 and the bound checked as the sum grows: no overflow on the way)
            if (a[d] < 0 || b[d] < 0) return fail(FC_ERR_ARG, "fc_burst_eval: negative tally");
            for (int64_t x : {a[d], b[d]}) {
                if (x >= fc::kBurstProductBound || !fc::burst_product_ok(m->den, total += x))
                    return fail(FC_ERR_ARG, "fc_burst_eval: den * (the tallies' total) reaches 2^62");
            }
        }
        for (int32_t d = 0; d < k; ++d) {
            int32_t c;
            int64_t g;
            fc::burst_district(a[d], b[d], m->num, m->den, c, g);
            cnt += c;
            gsum += g;
        }
    }
    *score = fc::burst_score(m->kind, cnt, gsum, cut);
    return FC_OK;
}

int fc_run_burst_select(fc_run *r, int32_t c0, int32_t nc, const fc_burst_metric *metric, uint32_t flags,
                        int64_t *best_score, int64_t *best_t, int64_t *start_score, int64_t *end_score,
                        int64_t *best_cut, int64_t *best_nb, int8_t *best_plan) {
    const char *const who = "fc_run_burst_select";
    if (!r || !metric) return fail(FC_ERR_ARG, "fc_run_burst_select: null argument");
    if (const char *bad = fc::burst_metric_error(*metric, 0, nullptr))
        return fail(FC_ERR_ARG, std::string("fc_run_burst_select: ") + bad);
    if (flags & ~(uint32_t)FC_BURST_REWIND) return fail(FC_ERR_ARG, "fc_run_burst_select: unknown flags");
    const bool votes = fc::burst_votes_kind(metric->kind), rewind = (flags & FC_BURST_REWIND) != 0;
    CallRules rules;
    rules.log_pass = "short bursts";
    rules.unset = votes && !r->el_n_cols ? "fc_run_set_elections" : nullptr;
    if (int rc = check_series_call(r, who, c0, nc, rules)) return rc;
    if (const char *bad = fc::burst_metric_error(*metric, r->el_n_cols, r->el_col_total))
        return fail(FC_ERR_ARG, std::string("fc_run_burst_select: ") + bad);
    if (rewind && r->p.proposal != FC_PROPOSE_RECOM)
        return fail(FC_ERR_UNSUPPORTED,
                    "fc_run_burst_select: FC_BURST_REWIND restarts ReCom chains only: a flip chain keeps derived "
                    "per-node state (foreign-neighbour counts, district tables, the current wait) that a rewind "
                    "would have to rebuild on the device");
    if (!fc::burst_fits_lds(r->npad))
        return fail(FC_ERR_UNSUPPORTED, "fc_run_burst_select: a chain's image (" +
                                            std::to_string(fc::burst_lds_bytes(r->npad)) +
                                            " bytes: assignment, tallies) does not fit 48 KB of LDS");
    if (nc == 0) return FC_OK;
    SeriesCall s;
    if (int rc = open_window(r, who, c0, nc, true, s)) return rc;
    const size_t cn = (size_t)nc, npad = (size_t)r->npad, n = (size_t)r->g.n;
    int q;
    // the staged rows (kept by the run, shared with the plan samples) and, when the rows have
    // padding, the same rows packed to n bytes behind them
    const size_t want = best_plan ? cn * npad : 0;
    const size_t held = want + (best_plan && npad != n ? cn * n : 0);
    if (held > r->d_pl_rows.capacity()) {
        bool fits = false;
        if ((q = fits_free_tenth(held, fits))) return q;
        if (!fits)
            return fail(FC_ERR_ARG, "fc_run_burst_select: " + std::to_string(held) + " bytes of staged plans (" +
                                        std::to_string(nc) + " chains) exceed a tenth of the free device memory; "
                                        "split the call by chains");
        if ((q = r->d_pl_rows.grow(held))) return q;
    }
    OutPack out;
    if ((q = out.reserve(r, {cn, cn, cn, cn, cn, cn}))) return q;
    fc::BurstParams bp{};
    bp.log = s.log;
    bp.cut0 = s.cut0;
    bp.nb0 = s.nb0;
    bp.kind = metric->kind;
    bp.maximize = metric->maximize;
    bp.num = metric->num;
    bp.den = metric->den;
    if (votes) {
        bp.cols = r->d_el_cols;
        bp.ncp = fc::votes_padded_cols(r->el_n_cols);
        bp.col_a = metric->col_a;
        bp.col_b = metric->col_b;
    }
    bp.rewind = rewind ? 1 : 0;
    bp.best_score = out.at(0);
    bp.best_t = out.at(1);
    bp.start_score = out.at(2);
    bp.end_score = out.at(3);
    bp.best_cut = out.at(4);
    bp.best_nb = out.at(5);
    bp.best_plan = best_plan ? r->d_pl_rows.get() : nullptr;
    if (rewind) {
        bp.assign = r->d_assign;
        bp.ser_a0 = r->d_ser_a0;
        bp.sc = r->d_sc;
    }
    r->bs_timed = false;
    if ((q = r->bs_ev.mark(0, r->stream))) return q;
    const int e = fc::launch_burst(bp, r->stream);
    if (e) return fail(FC_ERR_HIP, std::string("short bursts: ") + hipGetErrorString((hipError_t)e));
    if ((q = r->bs_ev.mark(1, r->stream))) return q;
    if (best_plan) {  // packed to n bytes on the device, then one contiguous copy (fc_run_sample_plans)
        const int8_t *src = r->d_pl_rows;
        if (npad != n) {
            int8_t *packed = r->d_pl_rows + want;
            HIP_TRY(hipMemcpy2DAsync(packed, n, src, npad, n, cn, hipMemcpyDeviceToDevice, r->stream));
            src = packed;
        }
        HIP_TRY(hipMemcpyAsync(best_plan, src, cn * n, hipMemcpyDeviceToHost, r->stream));
    }
    if (int rc = out.fetch(r, {best_score, best_t, start_score, end_score, best_cut, best_nb})) return rc;
    r->bs_timed = true;
    return FC_OK;
}

int fc_run_burst_select_ms(fc_run *r, float *kernel_ms) {
    if (!r || !kernel_ms) return fail(FC_ERR_ARG, "fc_run_burst_select_ms: null argument");
    if (!r->bs_timed) return fail(FC_ERR_ARG, "fc_run_burst_select_ms: no fc_run_burst_select call recorded");
    return r->bs_ev.elapsed(0, 1, kernel_ms);
}

int fc_graph_heat_rows(const fc_graph *g, int32_t *width, int32_t *nbr, int32_t *eid) {
    if (!g || !width) return fail(FC_ERR_ARG, "fc_graph_heat_rows: null argument");
    fc_graph_info gi;
    if (int rc = fc_graph_get_info(g, &gi)) return rc;
    const int32_t W = fc::row_width(gi.max_degree);
    if (W == 0) return fail(FC_ERR_UNSUPPORTED, "fc_graph_heat_rows: node degree above 16");
    *width = W;
    if (!nbr && !eid) return FC_OK;
    std::vector<int32_t> eu((size_t)gi.n_edges + 1), ev((size_t)gi.n_edges + 1);
    if (int rc = fc_graph_edges(g, eu.data(), ev.data())) return rc;
    std::vector<fc::RowSlot> rows;
    fc::build_rows(gi.n_nodes, gi.n_edges, eu.data(), ev.data(), W, nullptr, -1, rows);
    for (size_t i = 0; i < rows.size(); ++i) {
        if (nbr) nbr[i] = rows[i].nbr;
        if (eid) eid[i] = rows[i].val;
    }
    return FC_OK;
}

int fc_run_read_hist(fc_run *r, int64_t *cut_hist, int64_t *nb_hist) {
    if (!r || !cut_hist || !nb_hist) return fail(FC_ERR_ARG, "fc_run_read_hist: null argument");
    if (!r->d_cut_hist) return fail(FC_ERR_ARG, "fc_run_read_hist: FC_DIAG_HIST not enabled");
    if (int rc = fc_run_sync(r)) return rc;
    HIP_TRY(hipMemcpy(cut_hist, r->d_cut_hist, (size_t)r->n_chains * (r->g.n_edges + 1) * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(nb_hist, r->d_nb_hist, (size_t)r->n_chains * r->nb_w * 8, hipMemcpyDeviceToHost));
    return FC_OK;
}

int fc_run_read_edges(fc_run *r, int64_t *cut_times) {
    if (!r || !cut_times) return fail(FC_ERR_ARG, "fc_run_read_edges: null argument");
    if (!r->d_edge_acc) return fail(FC_ERR_ARG, "fc_run_read_edges: FC_DIAG_EDGES not enabled");
    const size_t E = r->g.n_edges, C = r->n_chains;
    std::vector<int64_t> acc(C * E);
    std::vector<int8_t> a(C * r->npad);
    std::vector<fc::ChainScalars> sc;
    if (int rc = download_scalars(r, 0, r->n_chains, sc)) return rc;
    HIP_TRY(hipMemcpy(acc.data(), r->d_edge_acc, acc.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(a.data(), r->d_assign, a.size(), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < C; ++c) {
        const int8_t *ac = &a[c * r->npad];
        const int64_t T = sc[c].steps + 1;  // yields so far
        for (size_t e = 0; e < E; ++e) {
            const bool is_cut = ac[r->g.eu[e]] != ac[r->g.ev[e]];
            // the kernels add the yield at which e turns uncut and subtract the one at which it
            // turns cut; an edge cut now is cut through the last yield
            cut_times[c * E + e] = acc[c * E + e] + (is_cut ? T : 0);
        }
    }
    return FC_OK;
}

int fc_run_read_flips(fc_run *r, int64_t *num_flips, int64_t *part_sum, int64_t *last_flipped) {
    if (!r || !num_flips || !part_sum || !last_flipped) return fail(FC_ERR_ARG, "fc_run_read_flips: null argument");
    if (!r->d_num_flips) return fail(FC_ERR_ARG, "fc_run_read_flips: FC_DIAG_FLIPS not enabled");
    const size_t n = r->g.n, C = r->n_chains;
    std::vector<int8_t> a(C * r->npad);
    std::vector<fc::ChainScalars> sc;
    if (int rc = download_scalars(r, 0, r->n_chains, sc)) return rc;
    HIP_TRY(hipMemcpy(num_flips, r->d_num_flips, C * n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(part_sum, r->d_part_sum, C * n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(last_flipped, r->d_last_flipped, C * n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(a.data(), r->d_assign, a.size(), hipMemcpyDeviceToHost));
    const int64_t lsum = (int64_t)r->labels[0] + (int64_t)r->labels[1];
    for (size_t c = 0; c < C; ++c) {
        const int64_t T = sc[c].steps + 1;
        for (size_t u = 0; u < n; ++u) {
            const int64_t lab = r->labels[a[c * r->npad + u]];
            const int64_t t_r = last_flipped[c * n + u];
            // k = 2 (fc_flip2.hip): every run of u added (L0 + L1 - 2 a_r) per yield; the last
            // run's share is -a_R t_R instead
            if (r->p.k == 2 && t_r != 0) part_sum[c * n + u] += (lab - lsum) * t_r;
            if (t_r == 0) part_sum[c * n + u] = T * lab;  // grid_chain_sec11.py:416-418
        }
    }
    return FC_OK;
}

int fc_run_read_flips_exact(fc_run *r, int64_t *flip_count, int64_t *occupancy, int64_t *last_accept) {
    if (!r || !flip_count || !occupancy || !last_accept) return fail(FC_ERR_ARG, "fc_run_read_flips_exact: null argument");
    if (!r->d_flip_count) return fail(FC_ERR_ARG, "fc_run_read_flips_exact: FC_DIAG_FLIPS_EXACT not enabled");
    const size_t n = r->g.n, C = r->n_chains;
    std::vector<int8_t> a(C * r->npad);
    std::vector<fc::ChainScalars> sc;
    if (int rc = download_scalars(r, 0, r->n_chains, sc)) return rc;
    HIP_TRY(hipMemcpy(flip_count, r->d_flip_count, C * n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(occupancy, r->d_occ_acc, C * n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(last_accept, r->d_last_accept, C * n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(a.data(), r->d_assign, a.size(), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < C; ++c) {
        // sum_t L(a_t) = L(a_0) s_1 + L(a_1)(s_2 - s_1) + ... = L(a_now) T - sum_flips (L_new - L_old) s
        const int64_t T = sc[c].steps + 1;
        for (size_t u = 0; u < n; ++u) occupancy[c * n + u] += (int64_t)r->labels[a[c * r->npad + u]] * T;
    }
    return FC_OK;
}

int fc_run_read_wait_expected(fc_run *r, double *out) {
    if (!r || !out) return fail(FC_ERR_ARG, "fc_run_read_wait_expected: null argument");
    if (!r->d_nb_hist) return fail(FC_ERR_ARG, "fc_run_read_wait_expected: FC_DIAG_HIST not enabled");
    if (int rc = fc_run_sync(r)) return rc;
    const size_t n = r->g.n, C = r->n_chains, W = (size_t)r->nb_w;
    std::vector<int64_t> h(C * W);
    HIP_TRY(hipMemcpy(h.data(), r->d_nb_hist, h.size() * 8, hipMemcpyDeviceToHost));
    // geom_wait (:147-148): np.random.geometric(p) - 1 with p = |B| / (N^k - 1): mean 1/p - 1
    const double M = std::pow((double)n, (double)r->p.k) - 1.0;
    for (size_t c = 0; c < C; ++c) {
        double s = 0.0;
        for (size_t b = 1; b < W; ++b)
            if (h[c * W + b]) s += (double)h[c * W + b] * (M / (double)b - 1.0);
        out[c] = s;
    }
    return FC_OK;
}

}  // extern "C"
