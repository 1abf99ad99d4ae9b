// Checkpoint / restore of a run (fc_run_checkpoint, fc_run_restore).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "fc_run.h"

namespace {

// Version of the canonical random stream a checkpoint's chains continue on:
// 3 = round 4's k = 2 node words, four draws per purpose-3 Philox call.  A blob written under
// another stream (magic "FCCKPT02": one call per draw) is refused, not continued on a stream
// its trajectory never used.
constexpr uint32_t kStreamVersion = 3;

struct CkptHeader {
    char magic[8];          // "FCCKPT03"
    uint32_t stream_version, reserved;
    int32_t n_chains, n, n_edges, k, ring_max, proposal, npad, dgraph;
    uint32_t diag_mask;
    uint32_t chain_id_offset;
    int64_t ev_cap, payload;
    uint64_t seed, param_hash;  // the random stream and every trajectory-determining parameter
};

// (device pointer, bytes) of every buffer a checkpoint carries, in blob order
static std::vector<std::pair<void *, size_t>> ckpt_sections(fc_run *r) {
    const size_t C = (size_t)r->n_chains, n = (size_t)r->g.n, E = (size_t)r->g.n_edges, k = (size_t)r->p.k;
    const size_t R = (size_t)r->g.ring_max;
    std::vector<std::pair<void *, size_t>> v;
    v.emplace_back(r->d_assign, C * r->npad);
    v.emplace_back(r->d_sc, C * sizeof(fc::ChainScalars));
    if (r->p.proposal != FC_PROPOSE_RECOM) {
        v.emplace_back(r->d_fcnt, C * r->npad);
        v.emplace_back(r->d_popk, C * fc::kMaxKGeneral * 4);
        if (r->d_nfh) v.emplace_back(r->d_nfh, C * fc::kNfh * 4);
        if (r->d_sbits) v.emplace_back(r->d_sbits, C * (size_t)r->words * 8);
        v.emplace_back(r->d_thresh, C * (2 * R + 1) * 8);
        if (r->dgraph) {
            v.emplace_back(r->d_mcnt, C * k * k * 4);
            v.emplace_back(r->d_ngk, C * 32 * 4);
        }
    }
    if (r->d_cut_hist) v.emplace_back(r->d_cut_hist, C * (E + 1) * 8);
    if (r->d_nb_hist) v.emplace_back(r->d_nb_hist, C * (size_t)r->nb_w * 8);
    if (r->d_edge_acc) v.emplace_back(r->d_edge_acc, C * E * 8);
    if (r->d_num_flips) {
        v.emplace_back(r->d_num_flips, C * n * 8);
        v.emplace_back(r->d_part_sum, C * n * 8);
        v.emplace_back(r->d_last_flipped, C * n * 8);
    }
    if (r->d_flip_count) {
        v.emplace_back(r->d_flip_count, C * n * 8);
        v.emplace_back(r->d_occ_acc, C * n * 8);
        v.emplace_back(r->d_last_accept, C * n * 8);
    }
    if (r->d_events) {
        v.emplace_back(r->d_events, C * (size_t)r->ev_cap * sizeof(fc_event));
        v.emplace_back(r->d_ser_a0, C * r->npad);
    }
    if (r->lad_hash) {  // replica exchange: rung map, snapshots, per-slot sums and swap counters, histograms
        const size_t M = r->lad_members.size();
        v.emplace_back(r->d_slot_of, C * 4);
        v.emplace_back(r->d_chain_at, M * 4);
        v.emplace_back(r->d_lad_snap, C * fc::kRungFields * 8);
        v.emplace_back(r->d_rung, M * sizeof(fc_rung_stats));
        if (r->d_snap_cut) {
            const size_t cw2 = (E + 2) & ~(size_t)1, nw2 = ((size_t)r->nb_w + 1) & ~(size_t)1;
            v.emplace_back(r->d_snap_cut, C * cw2 * 8);
            v.emplace_back(r->d_snap_nb, C * nw2 * 8);
            v.emplace_back(r->d_rung_cut, M * cw2 * 8);
            v.emplace_back(r->d_rung_nb, M * nw2 * 8);
        }
    }
    return v;
}

// bytes after the device sections: the exchange round counter (runs with ladders only)
size_t ckpt_tail_bytes(const fc_run *r) { return r->lad_hash ? 8 : 0; }

CkptHeader ckpt_header(const fc_run *r, int64_t payload) {
    CkptHeader h{};
    std::memcpy(h.magic, "FCCKPT03", 8);
    h.stream_version = kStreamVersion;
    h.reserved = r->lad_hash;  // hash of the ladder layout (fc_run_set_ladders), 0: no ladders
    h.n_chains = r->n_chains;
    h.n = r->g.n;
    h.n_edges = r->g.n_edges;
    h.k = r->p.k;
    h.ring_max = r->g.ring_max;
    h.proposal = r->p.proposal;
    h.npad = r->npad;
    h.dgraph = r->dgraph ? 1 : 0;
    h.diag_mask = r->p.diag_mask;
    h.ev_cap = r->ev_cap;
    h.payload = payload;
    h.chain_id_offset = r->p.chain_id_offset;
    h.seed = r->p.seed;
    h.param_hash = r->param_hash;
    return h;
}

}  // namespace

extern "C" {

int fc_run_checkpoint(fc_run *r, void *buf, int64_t cap, int64_t *len) {
    if (!r || !len) return fail(FC_ERR_ARG, "fc_run_checkpoint: null argument");
    const auto secs = ckpt_sections(r);
    int64_t payload = 0;
    for (const auto &sc : secs) payload += (int64_t)sc.second;
    payload += (int64_t)ckpt_tail_bytes(r);
    const int64_t total = (int64_t)sizeof(CkptHeader) + payload;
    *len = total;
    if (!buf) return FC_OK;
    if (cap < total) return fail(FC_ERR_ARG, "fc_run_checkpoint: buffer too small (" + std::to_string(total) + " bytes needed)");
    if (int rc = fc_run_sync(r)) return rc;
    const CkptHeader h = ckpt_header(r, payload);
    unsigned char *out = (unsigned char *)buf;
    std::memcpy(out, &h, sizeof h);
    size_t off = sizeof h;
    for (const auto &sc : secs) {
        if (sc.second) HIP_TRY(hipMemcpy(out + off, sc.first, sc.second, hipMemcpyDeviceToHost));
        off += sc.second;
    }
    if (ckpt_tail_bytes(r)) std::memcpy(out + off, &r->ex_round, 8);
    return FC_OK;
}

int fc_run_restore(fc_run *r, const void *buf, int64_t len) {
    if (!r || !buf) return fail(FC_ERR_ARG, "fc_run_restore: null argument");
    if (len < (int64_t)sizeof(CkptHeader)) return fail(FC_ERR_ARG, "fc_run_restore: blob too short");
    CkptHeader h;
    std::memcpy(&h, buf, sizeof h);
    const auto secs = ckpt_sections(r);
    int64_t payload = 0;
    for (const auto &sc : secs) payload += (int64_t)sc.second;
    payload += (int64_t)ckpt_tail_bytes(r);
    const CkptHeader want = ckpt_header(r, payload);
    if (std::memcmp(h.magic, "FCCKPT02", 8) == 0)
        return fail(FC_ERR_ARG, "fc_run_restore: the checkpoint was written under an earlier random stream (FCCKPT02: one "
                                "Philox call per k = 2 node draw); its chains cannot continue on this build's stream");
    if (std::memcmp(h.magic, want.magic, 8) != 0) return fail(FC_ERR_ARG, "fc_run_restore: not a flipchain checkpoint");
    if (h.stream_version != kStreamVersion)
        return fail(FC_ERR_ARG, "fc_run_restore: the checkpoint's random-stream version (" + std::to_string(h.stream_version) +
                                    ") differs from this build's (" + std::to_string(kStreamVersion) + ")");
    if (h.reserved != want.reserved)
        return fail(FC_ERR_ARG, "fc_run_restore: the checkpoint's ladders (fc_run_set_ladders) differ from this run's");
    if (h.n_chains != want.n_chains || h.n != want.n || h.n_edges != want.n_edges || h.k != want.k ||
        h.ring_max != want.ring_max || h.proposal != want.proposal || h.npad != want.npad || h.dgraph != want.dgraph ||
        h.diag_mask != want.diag_mask || h.ev_cap != want.ev_cap || h.payload != payload)
        return fail(FC_ERR_ARG, "fc_run_restore: the checkpoint was taken from a run with another graph or fc_params");
    if (h.seed != want.seed || h.chain_id_offset != want.chain_id_offset)
        return fail(FC_ERR_ARG, "fc_run_restore: the checkpoint's seed / chain_id_offset differ from this run's "
                                "(its chains would continue on another random stream)");
    if (h.param_hash != want.param_hash)
        return fail(FC_ERR_ARG, "fc_run_restore: the checkpoint's bases / thresholds, population bounds, labels, "
                                "log(1 - p) table or accept / constraint / ReCom settings differ from this run's");
    if (len != (int64_t)sizeof(CkptHeader) + payload) return fail(FC_ERR_ARG, "fc_run_restore: blob size mismatch");
    if (int rc = fc_run_sync(r)) return rc;
    const unsigned char *in = (const unsigned char *)buf;
    size_t off = sizeof h;
    if (r->lad_hash) {  // the rung map must be a permutation inside every ladder (the kernel indexes by it)
        size_t o = off;
        for (const auto &sc : secs) {
            if (sc.first == (void *)r->d_slot_of) break;
            o += sc.second;
        }
        const size_t C = (size_t)r->n_chains, M = r->lad_members.size();
        std::vector<int32_t> so(C), ca(M);
        std::memcpy(so.data(), in + o, C * 4);
        std::memcpy(ca.data(), in + o + C * 4, M * 4);
        bool ok = true;
        for (size_t c = 0; c < C && ok; ++c) ok = so[c] >= -1 && so[c] < (int32_t)M && (so[c] < 0 || ca[so[c]] == (int32_t)c);
        for (size_t m = 0; m < M && ok; ++m)
            ok = ca[m] >= 0 && ca[m] < (int32_t)C && so[ca[m]] == (int32_t)m;
        std::vector<int32_t> home(C, -1);  // a chain stays in the ladder it was listed in
        for (size_t m = 0; m < M; ++m) home[r->lad_members[m]] = r->lad_slot_ladder[m];
        for (size_t m = 0; m < M && ok; ++m) ok = home[ca[m]] == r->lad_slot_ladder[m];
        if (!ok) return fail(FC_ERR_ARG, "fc_run_restore: the checkpoint's rung map is not a permutation of this run's ladders");
    }
    for (size_t i = 0; i < secs.size(); ++i) {
        const auto &sc = secs[i];
        if (i == 1) {  // ChainScalars: traces are outputs and restart empty
            std::vector<fc::ChainScalars> s((size_t)r->n_chains);
            std::memcpy(s.data(), in + off, sc.second);
            for (auto &x : s) x.trace_len = 0;
            HIP_TRY(hipMemcpy(sc.first, s.data(), sc.second, hipMemcpyHostToDevice));
        } else if (sc.second) {
            HIP_TRY(hipMemcpy(sc.first, in + off, sc.second, hipMemcpyHostToDevice));
        }
        off += sc.second;
    }
    if (ckpt_tail_bytes(r)) std::memcpy(&r->ex_round, in + off, 8);
    r->deal_timed = false;  // the restored chains' pace is not the last launch's
    return FC_OK;
}

}  // extern "C"
