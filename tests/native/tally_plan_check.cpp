// CPU check of the k = 2 tally reduce's pass plan (csrc/fc_tally_plan.h plan_tally_reduce), which
// launch_tally_reduce (fc_tally.hip) launches as returned (tests/test_tally_cases.py builds and
// runs it):
//   (a) against the launcher's planning loop as it stood before the plan became a header, copied
//       here literally, over every subset of the four tally diagnostics, the limits 65,536 and
//       163,840, and every pair of an n and an n_edges taken from: the values at which j arrays
//       of n (n + 1, n_edges, n_edges + 1) entries fill a limit exactly, j = 1 .. 9, and the five
//       graphs of (b), each with two entries on either side; and a coarse sweep in between;
//   (b) against a hand-written table at limit 163,840 with all nine arrays kept (CUT 8 (E + 1),
//       NB 8 (n + 1), EDGE 8 E, six of 8 n bytes; first fit in array order).
// `tally_plan_check plan DIAG N E LIMIT` prints the plan of one shape as
// "limit L gmask G passes K mask bytes mask bytes ..." (the tests' expected plans come from here).
// Prints "checked N bad B"; exits 1 on any failure.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "fc_tally_plan.h"

using namespace fc;

static long checks = 0, bad = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        ++checks;                                \
        if (!(cond)) {                           \
            if (++bad <= 20) {                   \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);        \
                std::printf("\n");               \
            }                                    \
        }                                        \
    } while (0)

// ---- launch_tally_reduce's planning loop before fc_tally_plan.h, copied literally (p.diag, p.n,
// p.n_edges and optin are the arguments; the enum is the kernel file's own) ----
namespace ref {
enum : uint32_t { TR_CUT = 1, TR_NB = 2, TR_EDGE = 4, TR_NF = 8, TR_PS = 16, TR_LF = 32, TR_FC = 64, TR_OCC = 128, TR_LA = 256 };
constexpr int kTrArrays = 9;
struct P { uint32_t diag; int32_t n, n_edges; };
static void plan(const P &p, int optin, std::vector<std::pair<uint32_t, size_t>> &passes, uint32_t &gmask) {
    uint32_t have = 0;
    if (p.diag & FC_DIAG_HIST) have |= TR_CUT | TR_NB;
    if (p.diag & FC_DIAG_EDGES) have |= TR_EDGE;
    if (p.diag & FC_DIAG_FLIPS) have |= TR_NF | TR_PS | TR_LF;
    if (p.diag & FC_DIAG_FLIPS_EXACT) have |= TR_FC | TR_OCC | TR_LA;
    auto bytes = [&](int a) -> size_t {
        return 8 * (size_t)(a == 0 ? p.n_edges + 1 : a == 1 ? p.n + 1 : a == 2 ? p.n_edges : p.n);
    };
    const size_t kPass = (size_t)optin, kMaxLds = (size_t)optin;
    passes.clear();
    gmask = 0;
    for (int a = 0; a < kTrArrays; ++a) {
        if (!((have >> a) & 1u)) continue;
        const size_t b = bytes(a);
        if (b > kMaxLds) {
            gmask |= 1u << a;
            continue;
        }
        bool put = false;
        for (auto &ps : passes)
            if (ps.second + b <= std::max(kPass, b)) {
                ps.first |= 1u << a;
                ps.second += b;
                put = true;
                break;
            }
        if (!put) passes.emplace_back(1u << a, b);
    }
    if (passes.empty()) passes.emplace_back(0u, 0);
}
}  // namespace ref

static const uint32_t kAllTallies = FC_DIAG_HIST | FC_DIAG_EDGES | FC_DIAG_FLIPS | FC_DIAG_FLIPS_EXACT;

static void against_copy(uint32_t diag, int32_t n, int32_t e, int limit) {
    std::vector<std::pair<uint32_t, size_t>> passes;
    uint32_t gmask = 0;
    ref::plan({diag, n, e}, limit, passes, gmask);
    const TallyPlan pl = plan_tally_reduce(diag, n, e, (size_t)limit);
    bool same = pl.limit == limit && pl.gmask == gmask && (size_t)pl.n_passes == passes.size();
    for (size_t i = 0; same && i < passes.size(); ++i)
        same = pl.lmask[i] == passes[i].first && (size_t)pl.bytes[i] == passes[i].second;
    CHECK(same, "diag 0x%x n %d E %d limit %d: %d passes, gmask 0x%x against the copy's %zu, 0x%x", diag, n, e, limit,
          pl.n_passes, pl.gmask, passes.size(), gmask);
    // what any plan must hold: every kept array in exactly one place, no pass above the limit
    uint32_t seen = pl.gmask;
    bool once = true;
    for (int i = 0; i < pl.n_passes; ++i) {
        once = once && !(seen & pl.lmask[i]) && pl.bytes[i] <= (int64_t)limit;
        seen |= pl.lmask[i];
        int64_t b = 0;
        for (int a = 0; a < kTrArrays; ++a)
            if ((pl.lmask[i] >> a) & 1u) b += (int64_t)tally_array_bytes(a, n, e);
        once = once && b == pl.bytes[i];
    }
    CHECK(once && seen == tally_arrays(diag), "diag 0x%x n %d E %d limit %d: arrays 0x%x placed, 0x%x kept", diag, n, e,
          limit, seen, tally_arrays(diag));
}

struct Row {
    const char *graph;
    int32_t n, e;
    uint32_t gmask;
    int n_passes;
    uint32_t lmask[kTrArrays];
    int64_t bytes[kTrArrays];
};
// limit 163,840, every tally
static const Row kTable[] = {
    {"48 x 48", 2304, 4512, 0, 2, {TR_CUT | TR_NB | TR_EDGE | TR_NF | TR_PS | TR_LF, TR_FC | TR_OCC | TR_LA}, {145936, 55296}},
    // EDGE is not in pass 0, and NF back-fills pass 0
    {"70 x 70", 4900, 9660, 0, 3, {TR_CUT | TR_NB | TR_NF, TR_EDGE | TR_PS | TR_LF, TR_FC | TR_OCC | TR_LA},
     {155696, 155680, 117600}},
    {"104 x 104", 10816, 21424, TR_CUT | TR_EDGE, 7, {TR_NB, TR_NF, TR_PS, TR_LF, TR_FC, TR_OCC, TR_LA},
     {86536, 86528, 86528, 86528, 86528, 86528, 86528}},
    // 8 n is the limit exactly; NB is 163,848 B
    {"160 x 128", 20480, 40672, TR_CUT | TR_NB | TR_EDGE, 6, {TR_NF, TR_PS, TR_LF, TR_FC, TR_OCC, TR_LA},
     {163840, 163840, 163840, 163840, 163840, 163840}},
    {"144 x 144", 20736, 41184, 511, 1, {0}, {0}},
};
static const int kLimits[] = {65536, 163840};

static void print_plan(const TallyPlan &pl) {
    std::printf("limit %lld gmask %u passes %d", (long long)pl.limit, pl.gmask, pl.n_passes);
    for (int i = 0; i < pl.n_passes; ++i) std::printf(" %u %lld", pl.lmask[i], (long long)pl.bytes[i]);
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc == 6 && !std::strcmp(argv[1], "plan")) {
        print_plan(plan_tally_reduce((uint32_t)std::strtoul(argv[2], nullptr, 0), std::atoi(argv[3]), std::atoi(argv[4]),
                                     (size_t)std::atoll(argv[5])));
        return 0;
    }
    // (b) the table
    for (const Row &r : kTable) {
        TallyPlan want;
        want.limit = 163840;
        want.n_passes = r.n_passes;
        want.gmask = r.gmask;
        for (int i = 0; i < r.n_passes; ++i) {
            want.lmask[i] = r.lmask[i];
            want.bytes[i] = r.bytes[i];
        }
        const TallyPlan got = plan_tally_reduce(kAllTallies | FC_DIAG_WAIT, r.n, r.e, 163840);
        CHECK(got == want, "table row %s: %d passes, gmask 0x%x, first pass 0x%x %lld B", r.graph, got.n_passes, got.gmask,
              got.lmask[0], (long long)got.bytes[0]);
        if (!(got == want)) print_plan(got);
    }
    // (a) the sweep
    std::set<int32_t> ns, es;
    for (int limit : kLimits)
        for (int j = 1; j <= kTrArrays; ++j)
            for (int d = -2; d <= 2; ++d) {
                ns.insert(limit / (8 * j) + d);      // j arrays of n entries fill the limit
                ns.insert(limit / (8 * j) - 1 + d);  // ... of n + 1
                es.insert(limit / (8 * j) + d);
                es.insert(limit / (8 * j) - 1 + d);
            }
    for (const Row &r : kTable)
        for (int d = -2; d <= 2; ++d) {
            ns.insert(r.n + d);
            es.insert(r.e + d);
        }
    for (int32_t v = 1; v < 70000; v = v + v / 3 + 1) {
        ns.insert(v);
        es.insert(2 * v - 1);
    }
    for (int limit : kLimits)
        for (uint32_t sub = 0; sub < 16; ++sub) {
            const uint32_t diag = FC_DIAG_WAIT | (sub & 1 ? FC_DIAG_HIST : 0u) | (sub & 2 ? FC_DIAG_EDGES : 0u) |
                                  (sub & 4 ? FC_DIAG_FLIPS : 0u) | (sub & 8 ? FC_DIAG_FLIPS_EXACT : 0u);
            for (int32_t n : ns)
                for (int32_t e : es)
                    if (n >= 1 && e >= 0) against_copy(diag, n, e, limit);
        }
    std::printf("shapes %zu x %zu\n", ns.size(), es.size());
    std::printf("checked %ld bad %ld\n", checks, bad);
    return bad ? 1 : 0;
}
