// Replica exchange, host side (fc_ladder.h, fc_exchange.hip; DESIGN.md "Replica exchange").
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "fc_run.h"

extern "C" {

int fc_ladder_swap_threshold(double b_lo_rung, double b_hi_rung, int32_t d, uint64_t *t) {
    if (!t) return fail(FC_ERR_ARG, "fc_ladder_swap_threshold: null output");
    if (!(b_lo_rung > 0.0) || !(b_hi_rung > 0.0) || !std::isfinite(b_lo_rung) || !std::isfinite(b_hi_rung))
        return fail(FC_ERR_ARG, "fc_ladder_swap_threshold: bases must be positive and finite");
    if (d <= -(1 << fc::kLadderBits) || d >= (1 << fc::kLadderBits))
        return fail(FC_ERR_ARG, "fc_ladder_swap_threshold: |d| must be below 2^17");
    const fc::LadderPair tab = fc::ladder_pair(b_lo_rung, b_hi_rung);
    *t = fc::ladder_threshold(tab, d);
    return FC_OK;
}

int fc_run_set_ladders(fc_run *r, int32_t n_ladders, const int32_t *ladder_off, const int32_t *members,
                       uint32_t flags) {
    if (!r || !ladder_off || !members || n_ladders <= 0)
        return fail(FC_ERR_ARG, "fc_run_set_ladders: null argument or n_ladders <= 0");
    if (r->p.proposal == FC_PROPOSE_RECOM)
        return fail(FC_ERR_UNSUPPORTED, "fc_run_set_ladders: replica exchange is for flip proposals (not ReCom)");
    if (r->p.accept != FC_ACCEPT_CUT)
        return fail(FC_ERR_UNSUPPORTED, "fc_run_set_ladders: replica exchange needs FC_ACCEPT_CUT (the swap rule is "
                                        "the ratio of cut_accept's stationary weights)");
    if (r->g.n_edges >= (1 << fc::kLadderBits))
        return fail(FC_ERR_UNSUPPORTED, "fc_run_set_ladders: the swap table covers |cut| differences below 2^17 edges");
    if (r->lad_hash) return fail(FC_ERR_ARG, "fc_run_set_ladders: ladders are already set (callable once)");
    if (flags & ~FC_LADDER_HIST) return fail(FC_ERR_ARG, "fc_run_set_ladders: unknown flags");
    if ((flags & FC_LADDER_HIST) && !r->d_cut_hist)
        return fail(FC_ERR_ARG, "fc_run_set_ladders: FC_LADDER_HIST needs a run with FC_DIAG_HIST");
    const int32_t C = r->n_chains;
    if (ladder_off[0] != 0) return fail(FC_ERR_ARG, "fc_run_set_ladders: ladder_off[0] must be 0");
    for (int32_t l = 0; l < n_ladders; ++l)
        if (ladder_off[l + 1] <= ladder_off[l] || ladder_off[l + 1] > C)
            return fail(FC_ERR_ARG, "fc_run_set_ladders: ladder " + std::to_string(l) + " is empty or ladder_off is not "
                                    "increasing within n_chains (a chain belongs to at most one ladder)");
    const int32_t M = ladder_off[n_ladders];
    std::vector<int32_t> slot_of((size_t)C, -1), slot_ladder((size_t)M);
    std::vector<fc::LadderSlot> slots((size_t)M);
    std::vector<fc::LadderPair> pairs((size_t)M);
    std::vector<fc::LadderItem> items[3];
    for (int32_t l = 0; l < n_ladders; ++l) {
        const int32_t lo = ladder_off[l], hi = ladder_off[l + 1];
        for (int32_t s = lo; s < hi; ++s) {
            const int32_t c = members[s];
            if (c < 0 || c >= C)
                return fail(FC_ERR_ARG, "fc_run_set_ladders: chain index " + std::to_string(c) + " out of range");
            if (slot_of[c] >= 0)
                return fail(FC_ERR_ARG, "fc_run_set_ladders: chain " + std::to_string(c) + " is listed twice");
            if (r->pop_bounds[2 * (size_t)c] != r->pop_bounds[2 * (size_t)members[lo]] ||
                r->pop_bounds[2 * (size_t)c + 1] != r->pop_bounds[2 * (size_t)members[lo] + 1])
                return fail(FC_ERR_ARG, "fc_run_set_ladders: the chains of ladder " + std::to_string(l) +
                                            " have different population bounds (bounds are never swapped)");
            const double b = r->bases0[c];
            if (!(b > 0.0) || !std::isfinite(b))
                return fail(FC_ERR_ARG, "fc_run_set_ladders: chain " + std::to_string(c) + " has a non-positive base");
            slot_of[c] = s;
            slot_ladder[s] = l;
            slots[s].rung = s - lo;
            slots[s].gid = r->p.chain_id_offset + (uint32_t)members[lo];
        }
        for (int32_t s = lo; s < hi; ++s) {
            pairs[s] = s + 1 < hi ? fc::ladder_pair(r->bases0[members[s]], r->bases0[members[s + 1]]) : fc::LadderPair{};
            items[2].push_back({s, 0});
        }
        for (int par = 0; par < 2; ++par)  // pairs (rung, rung + 1) with rung = par (mod 2); the rest unpaired
            for (int32_t s = lo; s < hi;) {
                const bool pr = ((s - lo) & 1) == par && s + 1 < hi;
                items[par].push_back({s, pr ? 1 : 0});
                s += pr ? 2 : 1;
            }
    }
    HIP_TRY(hipSetDevice(r->p.device));
    // built into locals and moved into the run at the end: after a failure nothing of the ladders
    // stays behind, and the call may be repeated (after FC_ERR_NOMEM, without FC_LADDER_HIST)
    int rc;
    DevBuf<fc::LadderItem> d_items[3];
    DevBuf<fc::LadderSlot> d_slots;
    DevBuf<fc::LadderPair> d_pairs;
    DevBuf<int32_t> d_slot_of, d_chain_at;
    DevBuf<int64_t> d_snap, d_hist[4];  // d_hist: snapshot cut / nb, rung cut / nb
    DevBuf<fc_rung_stats> d_rung;
    for (int i = 0; i < 3; ++i)
        if ((rc = d_items[i].upload(items[i]))) return rc;
    if ((rc = d_slots.upload(slots))) return rc;
    if ((rc = d_pairs.upload(pairs))) return rc;
    if ((rc = d_slot_of.upload(slot_of))) return rc;
    if ((rc = d_chain_at.upload(members, (size_t)M))) return rc;
    // snapshots start at zero: what a chain accumulated so far (the initial yield included) goes
    // to its initial rung at the first attribution
    if ((rc = d_snap.alloc_zero((size_t)C * fc::kRungFields))) return rc;
    if ((rc = d_rung.alloc_zero((size_t)M))) return rc;
    if (flags & FC_LADDER_HIST) {
        const size_t cw2 = ((size_t)r->g.n_edges + 2) & ~(size_t)1, nw2 = ((size_t)r->nb_w + 1) & ~(size_t)1;
        const size_t counts[4] = {(size_t)C * cw2, (size_t)C * nw2, (size_t)M * cw2, (size_t)M * nw2};
        bool ok = true;
        for (int i = 0; i < 4; ++i) ok = ok && d_hist[i].alloc(counts[i]) == FC_OK;
        if (!ok) {
            (void)hipGetLastError();
            return fail(FC_ERR_NOMEM, "fc_run_set_ladders: the FC_LADDER_HIST buffers do not fit in device memory");
        }
        for (int i = 0; i < 4; ++i) HIP_TRY(hipMemset(d_hist[i], 0, counts[i] * 8));
    }
    HIP_TRY(hipDeviceSynchronize());
    for (int i = 0; i < 3; ++i) {
        r->d_lad_items[i] = std::move(d_items[i]);
        r->lad_n_items[i] = (int32_t)items[i].size();
    }
    r->d_lad_slots = std::move(d_slots);
    r->d_lad_pairs = std::move(d_pairs);
    r->d_slot_of = std::move(d_slot_of);
    r->d_chain_at = std::move(d_chain_at);
    r->d_lad_snap = std::move(d_snap);
    r->d_rung = std::move(d_rung);
    r->d_snap_cut = std::move(d_hist[0]);
    r->d_snap_nb = std::move(d_hist[1]);
    r->d_rung_cut = std::move(d_hist[2]);
    r->d_rung_nb = std::move(d_hist[3]);
    r->lad_off.assign(ladder_off, ladder_off + n_ladders + 1);
    r->lad_members.assign(members, members + M);
    r->lad_slot_ladder = slot_ladder;
    uint64_t h = fc::kFnvBasis;
    h = fnv1a(h, r->lad_off.data(), r->lad_off.size() * 4);
    h = fnv1a(h, r->lad_members.data(), r->lad_members.size() * 4);
    h = fnv1a(h, &flags, 4);
    r->lad_hash = (uint32_t)(h ^ (h >> 32));
    if (!r->lad_hash) r->lad_hash = 1;
    return FC_OK;
}

static int enqueue_exchange(fc_run *r, int which, bool do_swap, hipStream_t s) {
    fc::ExchangeParams q{};
    q.items = r->d_lad_items[which];
    q.n_items = r->lad_n_items[which];
    q.do_swap = do_swap ? 1 : 0;
    q.round = (uint32_t)r->ex_round;
    q.seed_lo = (uint32_t)r->p.seed;
    q.seed_hi = (uint32_t)(r->p.seed >> 32);
    q.slots = r->d_lad_slots;
    q.pairs = r->d_lad_pairs;
    q.slot_of = r->d_slot_of;
    q.chain_at = r->d_chain_at;
    q.sc = r->d_sc;
    q.thresh = r->d_thresh;
    q.tw = 2 * r->g.ring_max + 1;
    q.snap = r->d_lad_snap;
    q.rung = r->d_rung;
    if (r->d_snap_cut) {
        q.cut_hist = r->d_cut_hist;
        q.nb_hist = r->d_nb_hist;
        q.snap_cut = r->d_snap_cut;
        q.snap_nb = r->d_snap_nb;
        q.rung_cut = r->d_rung_cut;
        q.rung_nb = r->d_rung_nb;
        q.cut_w = r->g.n_edges + 1;
        q.nb_w = r->nb_w;
        q.cut_w2 = (q.cut_w + 1) & ~1;
        q.nb_w2 = (q.nb_w + 1) & ~1;
    }
    const int e = fc::launch_exchange(q, s);
    if (e != 0) return fail(FC_ERR_HIP, std::string("exchange kernel launch: ") + hipGetErrorString((hipError_t)e));
    return FC_OK;
}

int fc_run_exchange(fc_run *r, int32_t parity, void *hip_stream) {
    if (!r) return fail(FC_ERR_ARG, "fc_run_exchange: null run");
    if (!r->lad_hash) return fail(FC_ERR_ARG, "fc_run_exchange: no ladders (fc_run_set_ladders)");
    if (parity < -1 || parity > 1) return fail(FC_ERR_ARG, "fc_run_exchange: parity must be 0, 1 or -1 (round & 1)");
    HIP_TRY(hipSetDevice(r->p.device));
    const int par = parity < 0 ? (int)(r->ex_round & 1) : parity;
    if (int rc = enqueue_exchange(r, par, true, hip_stream ? (hipStream_t)hip_stream : r->stream)) return rc;
    ++r->ex_round;
    return FC_OK;
}

int fc_run_read_rungs(fc_run *r, int32_t *rung_of, int32_t *chain_at) {
    if (!r) return fail(FC_ERR_ARG, "fc_run_read_rungs: null run");
    if (!r->lad_hash) return fail(FC_ERR_ARG, "fc_run_read_rungs: no ladders (fc_run_set_ladders)");
    if (int rc = fc_run_sync(r)) return rc;
    if (rung_of) {
        HIP_TRY(hipMemcpy(rung_of, r->d_slot_of, (size_t)r->n_chains * 4, hipMemcpyDeviceToHost));
        for (int32_t c = 0; c < r->n_chains; ++c)
            if (rung_of[c] >= 0) rung_of[c] -= r->lad_off[r->lad_slot_ladder[rung_of[c]]];
    }
    if (chain_at) HIP_TRY(hipMemcpy(chain_at, r->d_chain_at, r->lad_members.size() * 4, hipMemcpyDeviceToHost));
    return FC_OK;
}

int fc_run_read_bases(fc_run *r, double *bases) {
    if (!r || !bases) return fail(FC_ERR_ARG, "fc_run_read_bases: null argument");
    std::copy(r->bases0.begin(), r->bases0.end(), bases);
    if (!r->lad_hash) return FC_OK;
    if (int rc = fc_run_sync(r)) return rc;
    std::vector<int32_t> so((size_t)r->n_chains);
    HIP_TRY(hipMemcpy(so.data(), r->d_slot_of, so.size() * 4, hipMemcpyDeviceToHost));
    // a slot keeps the base of the chain listed there: temperatures move, slots do not
    for (int32_t c = 0; c < r->n_chains; ++c)
        if (so[c] >= 0) bases[c] = r->bases0[r->lad_members[so[c]]];
    return FC_OK;
}

int fc_run_read_rung_stats(fc_run *r, fc_rung_stats *out, int64_t *cut_hist, int64_t *nb_hist) {
    if (!r || !out) return fail(FC_ERR_ARG, "fc_run_read_rung_stats: null argument");
    if (!r->lad_hash) return fail(FC_ERR_ARG, "fc_run_read_rung_stats: no ladders (fc_run_set_ladders)");
    if ((cut_hist || nb_hist) && !r->d_snap_cut)
        return fail(FC_ERR_ARG, "fc_run_read_rung_stats: the per-rung histograms need FC_LADDER_HIST");
    HIP_TRY(hipSetDevice(r->p.device));
    HIP_TRY(hipDeviceSynchronize());  // launches on a caller's stream included
    if (int rc = enqueue_exchange(r, 2, false, r->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(r->stream));
    const size_t M = r->lad_members.size();
    HIP_TRY(hipMemcpy(out, r->d_rung, M * sizeof(fc_rung_stats), hipMemcpyDeviceToHost));
    const size_t cw = (size_t)r->g.n_edges + 1, nw = (size_t)r->nb_w;
    if (cut_hist)
        HIP_TRY(hipMemcpy2D(cut_hist, cw * 8, r->d_rung_cut, ((cw + 1) & ~(size_t)1) * 8, cw * 8, M, hipMemcpyDeviceToHost));
    if (nb_hist)
        HIP_TRY(hipMemcpy2D(nb_hist, nw * 8, r->d_rung_nb, ((nw + 1) & ~(size_t)1) * 8, nw * 8, M, hipMemcpyDeviceToHost));
    return FC_OK;
}

}  // extern "C"
