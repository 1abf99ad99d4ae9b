// C-ABI of libflipchain.so (include/flipchain.h): graph and run lifetime, initial-state
// validation and set-up on the host, kernel launches and readouts.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "fc_run.h"

struct fc_graph {
    fc::HostGraph h;
};

namespace {

constexpr int kWaveSlots = 64;
thread_local std::string g_err;
thread_local char g_seed_kname[96] = {0};  // the calling thread's last launched seed-plan instance

}  // namespace

int fc::fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

int download_scalars(fc_run *r, int32_t c0, int32_t nc, std::vector<fc::ChainScalars> &sc) {
    if (int rc = fc_run_sync(r)) return rc;
    sc.resize((size_t)nc);
    HIP_TRY(hipMemcpy(sc.data(), r->d_sc + c0, sc.size() * sizeof(sc[0]), hipMemcpyDeviceToHost));
    return FC_OK;
}

extern "C" {

const char *fc_last_error(void) { return g_err.c_str(); }

#ifndef FC_BUILD_ID
#define FC_BUILD_ID "unknown"
#endif
// the marker lets build.py read the id from the .so bytes without loading the library
static const char kBuildIdMarker[] = "FC_BUILD_ID=" FC_BUILD_ID;

const char *fc_build_id(void) { return kBuildIdMarker + 12; }

uint32_t fc_build_flags(void) {
    uint32_t f = 0;
#ifdef FC_PHASE_PROF
    f |= FC_BUILD_PHASE_PROF;
#endif
#ifdef FC_PHASE_SYNC
    f |= FC_BUILD_PHASE_SYNC;
#endif
#ifdef FC_VARIANT_BUILD
    f |= FC_BUILD_VARIANT;
#endif
    return f;
}

int fc_device_count(int32_t *n) {
    if (!n) return fail(FC_ERR_ARG, "fc_device_count: null output");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *n = 0;
        return fail(FC_ERR_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *n = c;
    return FC_OK;
}

int fc_device_pci_id(int32_t device, char *buf, int32_t cap) {
    if (!buf || cap < 13) return fail(FC_ERR_ARG, "fc_device_pci_id: null buffer or cap < 13");
    HIP_TRY(hipDeviceGetPCIBusId(buf, cap, device));
    return FC_OK;
}

int fc_graph_create(int32_t n, const int32_t *row_ptr, const int32_t *col_idx, const int32_t *pop,
                    const double *pos_xy, uint32_t flags, fc_graph **out) {
    if (!out) return fail(FC_ERR_ARG, "fc_graph_create: null output");
    *out = nullptr;
    auto *g = new (std::nothrow) fc_graph();
    if (!g) return fail(FC_ERR_NOMEM, "fc_graph_create: out of memory");
    std::string err;
    try {
        err = fc::build_host_graph(n, row_ptr, col_idx, pop, pos_xy, flags, g->h);
    } catch (const std::exception &ex) {
        err = std::string("fc_graph_create: ") + ex.what();
    }
    if (!err.empty()) {
        delete g;
        return fail(err.rfind("graph: round-1", 0) == 0 ? FC_ERR_UNSUPPORTED : FC_ERR_ARG, err);
    }
    *out = g;
    return FC_OK;
}

int fc_graph_get_info(const fc_graph *g, fc_graph_info *out) {
    if (!g || !out) return fail(FC_ERR_ARG, "fc_graph_get_info: null argument");
    out->n_nodes = g->h.n;
    out->n_edges = g->h.n_edges;
    out->ring_max = g->h.ring_max;
    out->max_degree = g->h.max_degree;
    out->n_exact = g->h.n_exact;
    out->n_gamma = g->h.n_gamma;
    out->planar = g->h.planar ? 1 : 0;
    out->outer_simple = g->h.outer_simple ? 1 : 0;
    return FC_OK;
}

int fc_graph_edges(const fc_graph *g, int32_t *eu, int32_t *ev) {
    if (!g || !eu || !ev) return fail(FC_ERR_ARG, "fc_graph_edges: null argument");
    std::copy(g->h.eu.begin(), g->h.eu.end(), eu);
    std::copy(g->h.ev.begin(), g->h.ev.end(), ev);
    return FC_OK;
}

int fc_graph_rings(const fc_graph *g, int32_t *ring, uint64_t *meta) {
    if (!g || !ring || !meta) return fail(FC_ERR_ARG, "fc_graph_rings: null argument");
    std::copy(g->h.ring.begin(), g->h.ring.end(), ring);
    std::copy(g->h.meta.begin(), g->h.meta.end(), meta);
    return FC_OK;
}

void fc_graph_destroy(fc_graph *g) { delete g; }

int fc_seed_params_init(fc_seed_params *p, uint32_t struct_size) {
    if (!p) return fail(FC_ERR_ARG, "fc_seed_params_init: null argument");
    if (struct_size != sizeof(fc_seed_params))
        return fail(FC_ERR_ARG, "fc_seed_params_init: struct_size " + std::to_string(struct_size) +
                                    " != sizeof(fc_seed_params) " + std::to_string(sizeof(fc_seed_params)) +
                                    " (the caller's flipchain.h is another version)");
    std::memset(p, 0, sizeof *p);
    p->struct_size = (uint32_t)sizeof(fc_seed_params);
    p->abi_version = FC_ABI_VERSION;
    p->k = 2;
    p->pop_lo = 0;
    p->pop_hi = INT64_MAX;
    return FC_OK;
}

int fc_graph_seed_plans(const fc_graph *gr, const fc_seed_params *p, int32_t n_plans, int8_t *assign_out,
                        fc_seed_stats *stats_out, float *kernel_ms) {
    if (!gr || !p) return fail(FC_ERR_ARG, "fc_graph_seed_plans: null argument");
    // ---- host: checks, defaults, tables (fc_plan.cpp) -------------------------------------
    const fc::HostGraph &g = gr->h;
    fc::SeedPlan sp;
    std::string err;
    if (int rc = fc::plan_seed(g, *p, n_plans, sp, err)) return fail(rc, err);
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_plans == 0) return FC_OK;
    if (!assign_out) return fail(FC_ERR_ARG, "fc_graph_seed_plans: null assign_out");
    const size_t P = (size_t)n_plans, n = (size_t)g.n, E = (size_t)g.n_edges, npad = (size_t)sp.npad;

    // ---- device ---------------------------------------------------------------------------
    HIP_TRY(hipSetDevice(p->device));
    bool fits = false;
    const size_t want = P * (npad + sizeof(fc_seed_stats)) + sp.node_recs.size() + (sp.nbe.size() + sp.eslot.size()) * 4 +
                        2 * std::max<size_t>(E, 1) * 4;
    if (int rc = fits_free_tenth(want, fits)) return rc;
    if (!fits)
        return fail(FC_ERR_NOMEM, "fc_graph_seed_plans: " + std::to_string(n_plans) + " plan rows and the graph tables (" +
                                      std::to_string(want) + " bytes) exceed a tenth of the free device memory; split the "
                                      "call (plan_id_offset keeps the plans the same)");
    DevBuf<unsigned char> d_graph;
    DevBuf<uint32_t> d_nbe, d_eslot;
    DevBuf<int32_t> d_eu, d_ev;
    DevBuf<int8_t> d_assign;
    DevBuf<fc_seed_stats> d_stats;
    int rc;
    if ((rc = d_graph.upload(sp.node_recs))) return rc;
    if ((rc = d_nbe.upload(sp.nbe))) return rc;
    if ((rc = d_eslot.upload(sp.eslot))) return rc;
    // (one entry at least, so that an edgeless graph still hands the kernel a buffer)
    if ((rc = d_eu.alloc_zero(std::max<size_t>(E, 1)))) return rc;
    if ((rc = d_ev.alloc_zero(std::max<size_t>(E, 1)))) return rc;
    if (E) {
        HIP_TRY(hipMemcpy(d_eu, g.eu.data(), E * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_ev, g.ev.data(), E * 4, hipMemcpyHostToDevice));
    }
    if ((rc = d_assign.alloc(P * npad))) return rc;
    if ((rc = d_stats.alloc(P))) return rc;
    fc::SeedParams q{};
    q.graph = d_graph;
    q.nbe = d_nbe;
    q.eslot = d_eslot;
    q.eu = d_eu;
    q.ev = d_ev;
    q.nb_d = sp.nb_d;
    q.n = g.n;
    q.n_edges = g.n_edges;
    q.n_plans = n_plans;
    q.chain_lds_bytes = sp.chain_lds_bytes;
    q.k = sp.p.k;
    q.plan_id_offset = sp.p.plan_id_offset;
    q.seed_lo = (uint32_t)sp.p.seed;
    q.seed_hi = (uint32_t)(sp.p.seed >> 32);
    q.pop_lo = sp.p.pop_lo;
    q.pop_hi = sp.p.pop_hi;
    q.pop_total = sp.pop_total;
    q.node_repeats = sp.p.node_repeats;
    q.max_attempts = sp.p.max_attempts;
    q.max_restarts = sp.p.max_restarts;
    q.assign = d_assign;
    q.stats = d_stats;
    fc::EventMarks<2> ev;
    if (kernel_ms && (rc = ev.mark(0, nullptr))) return rc;
    const int e = fc::launch_seed(q, g.ring_max, nullptr, g_seed_kname, sizeof g_seed_kname);
    if (e != 0) return fail(FC_ERR_HIP, std::string("seed kernel launch: ") + hipGetErrorString((hipError_t)e));
    if (kernel_ms && (rc = ev.mark(1, nullptr))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (kernel_ms && (rc = ev.elapsed(0, 1, kernel_ms))) return rc;
    // ---- copy back, the row padding stripped ------------------------------------------------
    std::vector<int8_t> rows(P * npad);
    HIP_TRY(hipMemcpy(rows.data(), d_assign, rows.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < P; ++i) std::memcpy(assign_out + i * n, rows.data() + i * npad, n);
    if (stats_out) HIP_TRY(hipMemcpy(stats_out, d_stats, P * sizeof(fc_seed_stats), hipMemcpyDeviceToHost));
    return FC_OK;
}

int fc_seed_kernel_name(char *buf, int32_t cap) {
    if (!buf || cap <= 0) return fail(FC_ERR_ARG, "fc_seed_kernel_name: null argument");
    std::snprintf(buf, (size_t)cap, "%s", g_seed_kname);
    return FC_OK;
}

int fc_params_init(fc_params *p, uint32_t struct_size) {
    if (!p) return fail(FC_ERR_ARG, "fc_params_init: null argument");
    if (struct_size != sizeof(fc_params))
        return fail(FC_ERR_ARG, "fc_params_init: struct_size " + std::to_string(struct_size) + " != sizeof(fc_params) " +
                                    std::to_string(sizeof(fc_params)) + " (the caller's flipchain.h is another version)");
    std::memset(p, 0, sizeof *p);
    p->struct_size = (uint32_t)sizeof(fc_params);
    p->abi_version = FC_ABI_VERSION;
    p->k = 2;
    p->base = 1.0;
    p->pop_lo = 0;
    p->pop_hi = INT32_MAX;
    p->hit_lo = 1;  // hitting-time window off (hit_lo > hit_hi)
    p->hit_hi = 0;
    p->tune_ring_table = 64;  // (0 is "no table")
    return FC_OK;
}

int32_t fc_run_n_chains(const fc_run *r) { return r ? r->n_chains : 0; }

int32_t fc_run_chain_lds_bytes(const fc_run *r) { return r ? r->chain_lds_bytes : 0; }

int32_t fc_run_nb_width(const fc_run *r) { return r ? r->nb_w : 0; }

int fc_run_diag_paths(const fc_run *r, int64_t *tally_log_cap, int64_t *tally_log_wanted, int32_t *series_staged) {
    if (!r || !tally_log_cap || !tally_log_wanted || !series_staged) return fail(FC_ERR_ARG, "fc_run_diag_paths: null argument");
    *tally_log_cap = r->tl_cap();
    *tally_log_wanted = r->tl_want;
    *series_staged = r->series_staged;
    return FC_OK;
}

int fc_run_ring_table(const fc_run *r, int32_t *classes, int32_t *in_use) {
    if (!r || !classes || !in_use) return fail(FC_ERR_ARG, "fc_run_ring_table: null argument");
    *classes = r->ring_classes;
    *in_use = r->ring_table_on ? 1 : 0;
    return FC_OK;
}

int fc_run_tally_plan(const fc_run *r, int64_t *lds_limit, int32_t *n_passes, uint32_t *lds_masks, int64_t *lds_bytes,
                      int32_t cap, uint32_t *global_mask) {
    if (!r || !lds_limit || !n_passes || !global_mask || cap < 0 || (cap > 0 && (!lds_masks || !lds_bytes)))
        return fail(FC_ERR_ARG, "fc_run_tally_plan: null argument");
    const fc::TallyPlan &pl = r->tl_plan;
    *lds_limit = pl.limit;
    *n_passes = pl.n_passes;
    *global_mask = pl.gmask;
    for (int32_t i = 0; i < pl.n_passes && i < cap; ++i) {
        lds_masks[i] = pl.lmask[i];
        lds_bytes[i] = pl.bytes[i];
    }
    return FC_OK;
}

int fc_run_create(const fc_graph *gr, const fc_params *p, int32_t n_chains, const int8_t *init_assign,
                  const double *bases, fc_run **out) {
    if (!out) return fail(FC_ERR_ARG, "fc_run_create: null output");
    *out = nullptr;
    if (!gr || !p || !init_assign || n_chains <= 0) return fail(FC_ERR_ARG, "fc_run_create: null argument or n_chains <= 0");
    // ---- host: checks, layout, tuning, initial state (fc_plan.cpp) ------------------------
    const fc::HostGraph &g = gr->h;
    fc::RunPlan plan;
    std::string err;
    if (int rc = fc::plan_run(g, *p, n_chains, init_assign, bases, plan, err)) return fail(rc, err);
    std::unique_ptr<fc_run> r(new (std::nothrow) fc_run());
    if (!r) return fail(FC_ERR_NOMEM, "fc_run_create: out of memory");
    r->g = g;
    static_cast<fc::RunShape &>(*r) = plan;
    const bool recom = p->proposal == FC_PROPOSE_RECOM;
    const size_t C = (size_t)n_chains, n = (size_t)g.n, E = (size_t)g.n_edges;

    // ---- device ---------------------------------------------------------------------------
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
    int rc;
    if ((rc = r->d_graph.upload(plan.node_recs))) return rc;
    if ((rc = r->d_ring_eid.upload(g.ring_eid))) return rc;
    if ((rc = r->d_assign.upload(plan.assign))) return rc;
    if ((rc = r->d_fcnt.upload(plan.fcnt))) return rc;
    if ((rc = r->d_popk.upload(plan.popk))) return rc;
    if ((rc = r->d_sbits.upload(plan.sbits))) return rc;
    if ((rc = r->d_nfh.upload(plan.nfh))) return rc;
    if ((rc = r->d_mcnt.upload(plan.mcnt))) return rc;
    if ((rc = r->d_ngk.upload(plan.ngk))) return rc;
    if ((rc = r->d_sc.upload(plan.sc))) return rc;
    if ((rc = r->d_thresh.upload(plan.thresh))) return rc;
    if ((rc = r->d_log1mp.upload(r->log1mp))) return rc;
    {
        uint32_t keys[fc::kPhiloxKeyWords];
        fc::philox_round_keys((uint32_t)p->seed, (uint32_t)(p->seed >> 32), keys);
        if ((rc = r->d_pkeys.upload(keys, fc::kPhiloxKeyWords))) return rc;
    }
    if ((rc = r->d_ring_table.upload(plan.ring_table))) return rc;  // (none: the buffer stays null)
    if ((rc = r->d_labels.upload(r->labels))) return rc;
    if ((rc = r->d_cut_hist.upload(plan.cut_hist))) return rc;
    if ((rc = r->d_nb_hist.upload(plan.nb_hist))) return rc;
    if (p->diag_mask & FC_DIAG_EDGES)
        if ((rc = r->d_edge_acc.alloc_zero(C * E))) return rc;
    if (p->diag_mask & FC_DIAG_FLIPS) {
        if ((rc = r->d_num_flips.alloc_zero(C * n))) return rc;
        if ((rc = r->d_part_sum.upload(plan.part_sum))) return rc;
        if ((rc = r->d_last_flipped.alloc_zero(C * n))) return rc;
    }
    if (p->diag_mask & FC_DIAG_FLIPS_EXACT) {
        if (recom) return fail(FC_ERR_UNSUPPORTED, "fc_run_create: FC_DIAG_FLIPS_EXACT is kept by the flip kernels, not ReCom");
        for (DevBuf<int64_t> *b : {&r->d_flip_count, &r->d_occ_acc, &r->d_last_accept})
            if ((rc = b->alloc_zero(C * n))) return rc;
    }
    if (r->ev_cap > 0) {  // FC_DIAG_SERIES with an event_cap
        if (E > 65535) return fail(FC_ERR_UNSUPPORTED, "fc_run_create: FC_DIAG_SERIES stores |cut| in 16 bits (E <= 65535)");
        if ((rc = r->d_events.alloc(C * (size_t)r->ev_cap))) return rc;
        if ((rc = r->d_ser_a0.alloc(plan.assign.size()))) return rc;
        HIP_TRY(hipMemcpy(r->d_ser_a0, r->d_assign, plan.assign.size(), hipMemcpyDeviceToDevice));
    }
    if (recom) {
        // (one entry at least, so that an edgeless graph still hands the kernel a buffer)
        if ((rc = r->d_eu.alloc(std::max<size_t>(E, 1)))) return rc;
        if ((rc = r->d_ev.alloc(std::max<size_t>(E, 1)))) return rc;
        if (E) {
            HIP_TRY(hipMemcpy(r->d_eu, g.eu.data(), E * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(r->d_ev, g.ev.data(), E * 4, hipMemcpyHostToDevice));
        }
        if ((rc = r->d_nbe.upload(plan.nbe))) return rc;
        if ((rc = r->d_eslot.upload(plan.eslot))) return rc;
        if ((rc = r->d_recom_thresh.upload(plan.recom_thresh))) return rc;
    }
    if (r->p.trace_chains > 0)
        if ((rc = r->d_trace.alloc((size_t)r->p.trace_chains * p->trace_cap))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    *out = r.release();
    return FC_OK;
}

int fc_run_set_tape(fc_run *r, const uint32_t *tape, int64_t n_draws) {
    if (!r) return fail(FC_ERR_ARG, "fc_run_set_tape: null run");
    if (r->d_sbits && tape && n_draws > 0)  // a tape's word 0 is a node of all n (the node-tape map)
        return fail(FC_ERR_ARG, "fc_run_set_tape: replay tapes need the node stream (FC_STREAM_NODE)");
    HIP_TRY(hipSetDevice(r->p.device));
    r->d_tape.release();
    r->tape_draws = 0;
    if (!tape || n_draws <= 0) return FC_OK;
    if (int rc = r->d_tape.upload(tape, (size_t)r->n_chains * (size_t)n_draws * 6)) return rc;
    r->tape_draws = n_draws;
    return FC_OK;
}

int fc_run_set_initial_wait(fc_run *r, const uint32_t *words) {
    if (!r || !words) return fail(FC_ERR_ARG, "fc_run_set_initial_wait: null argument");
    if (!(r->p.diag_mask & FC_DIAG_WAIT)) return fail(FC_ERR_ARG, "fc_run_set_initial_wait: FC_DIAG_WAIT is off");
    if (r->p.proposal == FC_PROPOSE_RECOM) return fail(FC_ERR_UNSUPPORTED, "fc_run_set_initial_wait: flip runs only");
    std::vector<fc::ChainScalars> sc;
    if (int rc = download_scalars(r, 0, r->n_chains, sc)) return rc;
    for (const auto &s : sc)
        if (s.steps != 0 || s.draw != 0) return fail(FC_ERR_ARG, "fc_run_set_initial_wait: a chain has stepped");
    for (int32_t c = 0; c < r->n_chains; ++c) {
        fc::ChainScalars &s = sc[c];
        const int64_t w = fc::geom_from(fc::u53(words[2 * c], words[2 * c + 1]), r->log1mp[s.nb]);
        s.sum_wait += w - s.wait_cur;  // yield #0's term
        s.wait_cur = w;
    }
    HIP_TRY(hipMemcpy(r->d_sc, sc.data(), sc.size() * sizeof(sc[0]), hipMemcpyHostToDevice));
    return FC_OK;
}

#ifdef FC_PHASE_PROF
// diagnostic build: the launch's per-chain phase cycles appended to $FC_PROF_OUT
static int dump_prof(fc_run *r, hipStream_t s) {
    if (const char *path = std::getenv("FC_PROF_OUT")) {
        std::vector<int64_t> h((size_t)r->n_chains * fc::kProfSlots);
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipMemcpy(h.data(), r->d_prof, h.size() * 8, hipMemcpyDeviceToHost));
        if (FILE *f = std::fopen(path, "ab")) {
            std::fwrite(h.data(), 8, h.size(), f);
            std::fclose(f);
        }
    }
    return FC_OK;
}
#endif

// the flip kernels' parameters of one fc_run_steps call (its per-launch fields -- eta, deal / order
// / ctime, tl_*, prof and each chunk's n_steps / max_draws -- are set by the caller)
static fc::KParams flip_params(const fc_run *r, int64_t n_steps, int64_t max_draws) {
    fc::KParams k{};
    k.graph = r->d_graph;
    k.ring_eid = r->d_ring_eid;
    k.n = r->g.n;
    k.n_edges = r->g.n_edges;
    k.n_chains = r->n_chains;
    k.k = r->p.k;
    k.popk = r->d_popk;
    k.dgraph = r->dgraph ? 1 : 0;
    k.mcnt = r->d_mcnt;
    k.ngk = r->d_ngk;
    k.wmax = r->wmax > 0 ? r->wmax : 1;
    k.wdyn = r->p.k > 2 && r->wmax <= 0 ? 1 : 0;
    k.nfh = r->d_nfh;
    k.sbits = r->d_sbits;
    k.band_step0 = 1;
    while (k.band_step0 * 2 < r->words) k.band_step0 *= 2;
    k.chain_lds_bytes = r->chain_lds_bytes;
    k.words = r->words;
    k.lab_words = fc::bfs_lab_words(r->g.n);
    k.lemire_thresh = (uint32_t)((1ull << 32) % (uint64_t)r->g.n);
    k.chain_id_offset = r->p.chain_id_offset;
    k.seed_lo = (uint32_t)r->p.seed;
    k.seed_hi = (uint32_t)(r->p.seed >> 32);
    k.pop_lo = (int32_t)r->p.pop_lo;
    k.pop_hi = (int32_t)r->p.pop_hi;
    k.n_steps = n_steps;
    k.max_draws = max_draws > 0 ? max_draws : 65536 * std::max<int64_t>(n_steps, 1);
    k.assign = r->d_assign;
    k.fcnt = r->d_fcnt;
    k.sc = r->d_sc;
    k.thresh = r->d_thresh;
    k.log1mp = r->d_log1mp;
    k.labels = r->d_labels;
    k.diag = r->p.diag_mask;
    k.flags = (r->p.flags & ~(fc::kFlagNbr4 | fc::kFlagRingTable)) | (r->nbr4 ? fc::kFlagNbr4 : 0u) |
              (r->ring_table_on ? fc::kFlagRingTable : 0u);
    k.cut_hist = r->d_cut_hist;
    k.nb_hist = r->d_nb_hist;
    k.nb_w = r->nb_w;
    k.nb_pairs = (r->p.flags & FC_FLAG_NB_PAIRS) && r->p.k > 2;
    k.edge_acc = r->d_edge_acc;
    k.num_flips = r->d_num_flips;
    k.part_sum = r->d_part_sum;
    k.last_flipped = r->d_last_flipped;
    k.flip_count = r->d_flip_count;
    k.occ_acc = r->d_occ_acc;
    k.last_accept = r->d_last_accept;
    k.trace = r->d_trace;
    k.trace_chains = r->p.trace_chains;
    k.trace_cap = r->p.trace_cap;
    k.tape = r->d_tape;
    k.tape_draws = r->tape_draws;
    k.events = r->d_events;
    k.ev_cap = r->ev_cap;
    k.hit_lo = r->p.hit_lo;
    k.hit_hi = r->p.hit_hi;
    // launch tuning (fc_params.tune_*, resolved and checked by fc_run_create; scheduling only)
    k.hit_stop = r->tune.hit_stop;
    k.par_min = r->tune.par_min;
    k.wait_q = r->tune.wait_q;
    k.wpb = r->tune.wpb;
    k.coop = r->tune.coop ? 1 : 0;
    k.variant = r->variant ? 1 : 0;
    k.accept = r->p.accept;
    k.con_valid = r->p.con_valid;
    k.con_accept = r->p.con_accept;
    if (r->variant) k.par_min = kWaveSlots + 1;  // variants commit one event at a time
    for (int i = 0; i < 3; ++i) {
        k.prio_nb[i] = r->tune.prio_div[0] > 0 && r->p.k == 2 ? k.n / r->tune.prio_div[i] : 0;
        k.prio_th[i] = r->tune.prio_th[i];
    }
    return k;
}

static fc::RecomParams recom_params(const fc_run *r, int64_t n_steps, int64_t max_draws, int64_t *prof) {
    fc::RecomParams q{};
    q.graph = r->d_graph;
    q.nbe = r->d_nbe;
    q.eslot = r->d_eslot;
    q.nb_d = r->nb_d;
    q.eu = r->d_eu;
    q.ev = r->d_ev;
    q.n = r->g.n;
    q.n_edges = r->g.n_edges;
    q.n_chains = r->n_chains;
    q.chain_lds_bytes = r->chain_lds_bytes;
    q.chain_id_offset = r->p.chain_id_offset;
    q.seed_lo = (uint32_t)r->p.seed;
    q.seed_hi = (uint32_t)(r->p.seed >> 32);
    q.pop_lo = (int32_t)r->p.pop_lo;
    q.pop_hi = (int32_t)r->p.pop_hi;
    q.pop_target = r->p.recom_pop_target;
    q.epsilon = r->p.recom_epsilon;
    q.node_repeats = r->p.recom_node_repeats > 0 ? r->p.recom_node_repeats : 1;
    q.max_attempts = r->p.recom_max_attempts > 0 ? r->p.recom_max_attempts : 10000;
    q.n_steps = n_steps;
    q.max_draws = max_draws > 0 ? max_draws : 1024 * std::max<int64_t>(n_steps, 1);
    q.assign = r->d_assign;
    q.sc = r->d_sc;
    q.accept_thresh = r->d_recom_thresh;
    q.trace = (fc_recom_record *)r->d_trace.get();
    q.trace_chains = r->p.trace_chains;
    q.trace_cap = r->p.trace_cap;
    q.prof = prof;
    return q;
}

// per-launch event pairs: a pool that grows to kMaxLaunchEvents, then a ring that keeps
// the most recent ones (an iterator stepping one launch at a time never reads timings)
static int take_event_slot(fc_run *r, size_t *slot) {
    if (r->n_launch_events < r->launch_events.size()) {
        *slot = (r->ev_head + r->n_launch_events) % r->launch_events.size();
        ++r->n_launch_events;
    } else if (r->launch_events.size() < fc::kMaxLaunchEvents) {  // pool full and not wrapped (ev_head == 0)
        hipEvent_t a, b;
        HIP_TRY(hipEventCreate(&a));
        HIP_TRY(hipEventCreate(&b));
        r->launch_events.emplace_back(a, b);
        *slot = r->launch_events.size() - 1;
        ++r->n_launch_events;
    } else {  // ring full: overwrite the oldest
        *slot = r->ev_head;
        r->ev_head = (r->ev_head + 1) % r->launch_events.size();
    }
    return FC_OK;
}

// k = 2 full diagnostics: the tally log (16 B per entry), sized for this call's launches (a
// state's entries: one per accepted flip, plus a start-state entry per batch right after a
// queue flush -- n_steps + n_steps / 8 + 256 per chain covers what the reference's sweeps
// produce; a chain whose log fills applies the rest of its launch's tallies itself) within a
// tenth of the device's free memory; launches of at most 2^23 steps (an entry holds t - t0
// in 24 bits).  Sets k.tl_* and, when the log is in use, *chunk.
static int size_tally_log(fc_run *r, int64_t n_steps, hipStream_t s, fc::KParams &k, int64_t *chunk) {
    k.tl = nullptr;
    k.tl_t0 = k.tl_len = nullptr;
    k.tl_cap = 0;
    if (!(r->p.k == 2 && (r->p.diag_mask & (FC_DIAG_HIST | FC_DIAG_FLIPS | FC_DIAG_FLIPS_EXACT | FC_DIAG_EDGES)) &&
          r->g.n < 65535 && r->g.n_edges < (1 << 24)))
        return FC_OK;
    *chunk = int64_t(1) << 23;
    const int64_t steps1 = std::min(*chunk, n_steps);
    int64_t want = steps1 + steps1 / 8 + 256;
    if (r->p.flags & FC_FLAG_TALLY_LOG_SMALL) want = std::min<int64_t>(want, 64);
    r->tl_want = want;
    if (want > r->tl_cap()) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const int64_t per_chain = (int64_t)((free_b / 10) / ((size_t)r->n_chains * 16));
        want = std::min(want, std::max<int64_t>(per_chain, 0));
        if (want > r->tl_cap()) {
            HIP_TRY(hipStreamSynchronize(s));
            if (int rc = r->d_tl.grow((size_t)r->n_chains * (size_t)want * 4)) return rc;
        }
    }
    if (!r->d_tl_len) {
        if (int rc = r->d_tl_len.alloc((size_t)r->n_chains)) return rc;
        if (int rc = r->d_tl_t0.alloc((size_t)r->n_chains)) return rc;
        HIP_TRY(hipMemsetAsync(r->d_tl_len, 0, (size_t)r->n_chains * 8, s));
    }
    if (r->tl_cap() > 0) {
        k.tl = r->d_tl;
        k.tl_t0 = r->d_tl_t0;
        k.tl_len = r->d_tl_len;
        k.tl_cap = r->tl_cap();
    }
    return FC_OK;
}

// the end of a call's launches: the closing event, the diagnostic build's dump, the timed pair
static int finish_launches(fc_run *r, const std::pair<hipEvent_t, hipEvent_t> &evp, hipStream_t s) {
    HIP_TRY(hipEventRecord(evp.second, s));
#ifdef FC_PHASE_PROF
    if (int rc = dump_prof(r, s)) return rc;
#endif
    r->ev0 = evp.first;
    r->ev1 = evp.second;
    r->timed = true;
    return FC_OK;
}

int fc_run_steps(fc_run *r, int64_t n_steps, int64_t max_draws, void *hip_stream) {
    if (!r) return fail(FC_ERR_ARG, "fc_run_steps: null run");
    if (n_steps < 0) return fail(FC_ERR_ARG, "fc_run_steps: n_steps must be >= 0");
    if (n_steps == 0) return FC_OK;
    HIP_TRY(hipSetDevice(r->p.device));
    fc::Instance inst;  // chosen per call: a tape can be set and cleared between calls
    if (!fc::choose_instance(fc::instance_facts(r->g, *r, r->d_tape, r->d_trace), inst))
        return fail(FC_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(hipErrorInvalidValue));
    fc::KParams k = flip_params(r, n_steps, max_draws);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
#ifdef FC_PHASE_PROF
    if (!r->d_prof) {
        if (int rc = r->d_prof.alloc((size_t)r->n_chains * fc::kProfSlots)) return rc;
    }
    HIP_TRY(hipMemsetAsync(r->d_prof, 0, (size_t)r->n_chains * fc::kProfSlots * 8, s));
    k.prof = r->d_prof;
#endif
    size_t slot_i;
    if (int rc = take_event_slot(r, &slot_i)) return rc;
    const auto evp = r->launch_events[slot_i];
    HIP_TRY(hipEventRecord(evp.first, s));
    if (r->p.proposal == FC_PROPOSE_RECOM) {
        const fc::RecomParams q = recom_params(r, n_steps, max_draws, k.prof);
        const int e = fc::launch_recom(q, r->d_events, r->ev_cap, inst.recom, s, r->kname, sizeof r->kname);
        if (e != 0) return fail(FC_ERR_HIP, std::string("recom kernel launch: ") + hipGetErrorString((hipError_t)e));
        return finish_launches(r, evp, s);
    }
    // the kernel keeps per-launch step and per-lane counters in 32 bits: launch in chunks
    constexpr int64_t kChunk = int64_t(1) << 24;
    if (r->p.k == 2 && k.prio_nb[0] > 0 && k.prio_th[0] >= 0.0f) {  // tune_prio_th[0] < 0: |B| rule only
        if (!r->d_eta) {
            if (int rc = r->d_eta.alloc(2)) return rc;
            HIP_TRY(hipMemsetAsync(r->d_eta, 0, 2 * sizeof(uint32_t), s));
        }
        k.eta = r->d_eta;
    }
    if (r->tune.deal) {
        if (!r->d_deal) {
            if (int rc = r->d_deal.alloc((size_t)fc::kDealKeys + 4)) return rc;
            if (int rc = r->d_order.alloc((size_t)r->n_chains)) return rc;
            if (int rc = r->d_ctime.alloc((size_t)r->n_chains)) return rc;
        }
        k.deal = r->d_deal;
        k.order = r->d_order;
        k.ctime = r->d_ctime;
    }
    int64_t chunk = kChunk;
    if (int rc = size_tally_log(r, n_steps, s, k, &chunk)) return rc;
    for (int64_t done = 0; done < n_steps; done += chunk) {
        k.n_steps = std::min(chunk, n_steps - done);
        if (max_draws <= 0) k.max_draws = 65536 * k.n_steps;
        if (k.order) {  // this launch's deal: chains by the last one's durations (first: by |B|)
            const int e = fc::launch_deal_order(r->d_ctime, r->d_sc, k.n, r->n_chains, r->deal_timed ? 1 : 0,
                                                r->d_order, r->d_deal, s);
            if (e != 0) return fail(FC_ERR_HIP, std::string("deal kernel launch: ") + hipGetErrorString((hipError_t)e));
            r->deal_timed = true;
        }
        if (k.eta) {
            k.eta_parity = (int32_t)(r->n_flip_launches++ & 1);
            HIP_TRY(hipMemsetAsync(r->d_eta + k.eta_parity, 0, sizeof(uint32_t), s));
        }
        const int e = r->p.k == 2 ? fc::launch_flip2(k, r->d_pkeys, r->d_ring_table, inst.flip2, s, r->kname, sizeof r->kname)
                                    : fc::launch_flipk(k, inst.flipk, s, r->kname, sizeof r->kname);
        if (e != 0) return fail(FC_ERR_HIP, std::string("flip kernel launch: ") + hipGetErrorString((hipError_t)e));
        if (k.tl_len) {  // the launch's logged tallies, applied and the logs emptied
            const int er = fc::launch_tally_reduce(k, r->g.ring_max, s, &r->tl_plan);
            if (er != 0) return fail(FC_ERR_HIP, std::string("tally reduce launch: ") + hipGetErrorString((hipError_t)er));
        }
    }
    return finish_launches(r, evp, s);
}

int fc_run_sync(fc_run *r) {
    if (!r) return fail(FC_ERR_ARG, "fc_run_sync: null run");
    HIP_TRY(hipSetDevice(r->p.device));
    HIP_TRY(hipDeviceSynchronize());
    return FC_OK;
}

int fc_run_last_ms(fc_run *r, float *ms) {
    if (!r || !ms) return fail(FC_ERR_ARG, "fc_run_last_ms: null argument");
    if (!r->timed) return fail(FC_ERR_ARG, "fc_run_last_ms: no launch recorded");
    HIP_TRY(hipEventSynchronize(r->ev1));
    HIP_TRY(hipEventElapsedTime(ms, r->ev0, r->ev1));
    return FC_OK;
}

int fc_run_timings(fc_run *r, float *ms, int32_t cap, int32_t *n) {
    if (!r || !n || (cap > 0 && !ms)) return fail(FC_ERR_ARG, "fc_run_timings: null argument");
    HIP_TRY(hipSetDevice(r->p.device));
    const size_t cnt = r->n_launch_events, sz = r->launch_events.size();
    if (cnt) HIP_TRY(hipEventSynchronize(r->launch_events[(r->ev_head + cnt - 1) % sz].second));
    int32_t m = 0;
    for (size_t i = 0; i < cnt && m < cap; ++i, ++m) {
        const auto &pr = r->launch_events[(r->ev_head + i) % sz];
        HIP_TRY(hipEventElapsedTime(&ms[m], pr.first, pr.second));
    }
    *n = (int32_t)cnt;
    // the next launch records into slot 0 again; fc_run_last_ms keeps reading ev0 / ev1 (the
    // most recent pair) until then
    r->n_launch_events = 0;
    r->ev_head = 0;
    return FC_OK;
}

int fc_host_register(void *ptr, int64_t bytes) {
    if (!ptr || bytes <= 0) return fail(FC_ERR_ARG, "fc_host_register: null or empty buffer");
    HIP_TRY(hipHostRegister(ptr, (size_t)bytes, hipHostRegisterDefault));
    return FC_OK;
}

int fc_host_unregister(void *ptr) {
    if (!ptr) return fail(FC_ERR_ARG, "fc_host_unregister: null buffer");
    HIP_TRY(hipHostUnregister(ptr));
    return FC_OK;
}

int fc_run_kernel_name(const fc_run *r, char *buf, int32_t cap) {
    if (!r || !buf || cap <= 0) return fail(FC_ERR_ARG, "fc_run_kernel_name: null argument");
    std::snprintf(buf, (size_t)cap, "%s", r->kname);
    return FC_OK;
}

void fc_run_destroy(fc_run *r) {
    if (!r) return;
    (void)hipSetDevice(r->p.device);
    (void)hipDeviceSynchronize();
    delete r;
}

}  // extern "C"
