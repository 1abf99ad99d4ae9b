// CPU check of the kernel instance choice of csrc/fc_instance.h (tests/test_instances.py builds and
// runs it).  Without an argument:
//   - over every combination of the inputs the choice and its name equal the rule as the launchers
//     held it before it was stated in one place: their `if` / `switch` ladders and snprintf formats,
//     copied here literally (ref_flip2 / ref_flipk / ref_recom), fed the KParams fields that
//     flip_params filled for them; xtra implies full, mf != 0 implies km == 3, and the distinct
//     instances reached number exactly 72 (k = 2), 60 (k > 2) and 4 (ReCom);
//   - a ring width of 12 and an nsub of 3 give an error, not an instance;
//   - a table of configurations, written by hand as literals, gives the names the GPU tests assert.
// Prints `checked N bad B`; exits 1 on any mismatch.
// With a file (int32 n, nnz, row_ptr[n + 1], col_idx[nnz], pop[n], double pos[2 n], int8 assign[n],
// a k = 2 plan): builds the graph, plans a one-chain run and prints the planner's `nbr4`.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "fc_plan.h"

using namespace fc;

static long checks = 0, bad = 0;
#define CHECK(cond, ...)                   \
    do {                                   \
        ++checks;                          \
        if (!(cond)) {                     \
            if (++bad <= 20) {             \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);  \
                std::printf("\n");         \
            }                              \
        }                                  \
    } while (0)

// ---- the launchers' rule before fc_instance.h, copied literally (the launch itself left out) ----
struct RefParams {  // the KParams fields the ladders read
    const void *tape, *trace;
    uint32_t diag, flags;
    int32_t hit_lo, hit_hi, variant, all_exact, band, nsub, coop, dgraph, multi_flip;
};
static const int hipErrorInvalidValue_ref = 1;

static int ref_flip2(const RefParams &p, int ring_max, char *name, size_t name_cap) {
    const bool full = p.tape || p.trace || (p.diag & ~(uint32_t)FC_DIAG_WAIT) || p.hit_lo <= p.hit_hi || p.variant;
    const bool xtra = p.tape || p.trace || p.variant;
    const bool search = !p.all_exact || (p.flags & FC_FLAG_FORCE_BFS);
#define FC_LAUNCH2B(R, S, F, X, Y, B)                                                                      \
    do {                                                                                                    \
        if (name)                                                                                           \
            snprintf(name, name_cap, "fc::flip2_kernel<%d, %d, %s, %s, %s, %s>", R, S, F ? "true" : "false", \
                     X ? "true" : "false", Y ? "true" : "false", B ? "true" : "false");                    \
    } while (0)
#define FC_LAUNCH2(R, S, F, X, Y)                        \
    do {                                                 \
        if (p.band) FC_LAUNCH2B(R, S, F, X, Y, true);    \
        else FC_LAUNCH2B(R, S, F, X, Y, false);          \
    } while (0)
#define FC_SEARCH2(R, S, F, Y)                    \
    do {                                          \
        if (search) FC_LAUNCH2(R, S, F, true, Y);  \
        else FC_LAUNCH2(R, S, F, false, Y);        \
    } while (0)
#define FC_FULL2(R, S)                                \
    do {                                              \
        if (xtra) FC_SEARCH2(R, S, true, true);        \
        else if (full) FC_SEARCH2(R, S, true, false);  \
        else FC_SEARCH2(R, S, false, false);           \
    } while (0)
#define FC_NSUB2(R)                                \
    switch (p.nsub) {                              \
        case 1: FC_FULL2(R, 1); break;             \
        case 2: FC_FULL2(R, 2); break;             \
        case 4: FC_FULL2(R, 4); break;             \
        default: return hipErrorInvalidValue_ref;  \
    }
    if (ring_max == 8) {
        FC_NSUB2(8)
    } else if (ring_max == 16) {
        FC_NSUB2(16)
    } else {
        return hipErrorInvalidValue_ref;
    }
#undef FC_NSUB2
#undef FC_FULL2
#undef FC_SEARCH2
#undef FC_LAUNCH2
#undef FC_LAUNCH2B
    return 0;
}

static int ref_flipk(const RefParams &p, int ring_max, char *name, size_t name_cap) {
    const bool full = p.tape || p.trace || (p.diag & ~(uint32_t)FC_DIAG_WAIT) || p.hit_lo <= p.hit_hi;
#define FC_LAUNCHM(R, S, K, F, M)                                                                       \
    do {                                                                                                \
        if (name)                                                                                       \
            snprintf(name, name_cap, "fc::flip_kernel<%d, %d, %d, %s, %d>", R, S, K, F ? "true" : "false", \
                     (int)(M));                                                                         \
    } while (0)
#define FC_LAUNCH(R, S, K, F)                                                     \
    do {                                                                          \
        if (K == 3 && p.multi_flip == 2) FC_LAUNCHM(R, S, K, F, (K == 3 ? 2 : 0)); \
        else if (K == 3 && p.multi_flip) FC_LAUNCHM(R, S, K, F, (K == 3 ? 1 : 0)); \
        else FC_LAUNCHM(R, S, K, F, 0);                                            \
    } while (0)
#define FC_FULL_SWITCH(R, S, K)                          \
    do {                                                 \
        if (full) FC_LAUNCH(R, S, K, true);              \
        else FC_LAUNCH(R, S, K, false);                  \
    } while (0)
#define FC_NSUB_SWITCH(R, K)                          \
    switch (p.nsub) {                                 \
        case 1: FC_FULL_SWITCH(R, 1, K); break;       \
        case 2: FC_FULL_SWITCH(R, 2, K); break;       \
        case 4: FC_FULL_SWITCH(R, 4, K); break;       \
        default: return hipErrorInvalidValue_ref;     \
    }
    if (ring_max == 8) {
        if (p.coop) {
            FC_NSUB_SWITCH(8, 1)
        } else if (p.dgraph) {
            FC_NSUB_SWITCH(8, 3)
        } else {
            FC_NSUB_SWITCH(8, 0)
        }
    } else if (ring_max == 16) {
        if (p.coop) {
            FC_NSUB_SWITCH(16, 1)
        } else if (p.dgraph) {
            FC_NSUB_SWITCH(16, 3)
        } else {
            FC_NSUB_SWITCH(16, 0)
        }
    } else {
        return hipErrorInvalidValue_ref;
    }
#undef FC_NSUB_SWITCH
#undef FC_FULL_SWITCH
#undef FC_LAUNCH
#undef FC_LAUNCHM
    return 0;
}

static int ref_recom(const void *events, int64_t ev_cap, int ring_max, char *name, size_t name_cap) {
    const bool log = events && ev_cap > 0;
#define FC_LAUNCH_R(R)                                                                                       \
    do {                                                                                                     \
        if (name) snprintf(name, name_cap, log ? "fc::recom_log_kernel<%d>" : "fc::recom_kernel<%d>", R);    \
    } while (0)
    if (ring_max == 8) FC_LAUNCH_R(8);
    else if (ring_max == 16) FC_LAUNCH_R(16);
    else return hipErrorInvalidValue_ref;
#undef FC_LAUNCH_R
    return 0;
}

// the KParams fields as flip_params filled them from a run (fc_capi.cpp, before)
static RefParams ref_params(const InstanceFacts &f) {
    static const int buffer = 0;
    RefParams p{};
    p.tape = f.tape ? &buffer : nullptr;
    p.trace = f.trace ? &buffer : nullptr;
    p.diag = f.diag;
    p.flags = f.flags;
    p.hit_lo = f.hit_window ? 0 : 1;
    p.hit_hi = f.hit_window ? 5 : 0;
    p.variant = f.variant ? 1 : 0;
    p.all_exact = f.all_exact ? 1 : 0;
    p.band = f.band ? 1 : 0;
    p.nsub = f.nsub;
    p.coop = f.coop ? 1 : 0;
    p.dgraph = f.dgraph ? 1 : 0;
    p.multi_flip = f.multi ? f.mf_marks : 0;
    return p;
}

// the choice and its name; "" when it is refused
static std::string chosen(const InstanceFacts &f, Instance &inst) {
    char name[96] = {0};
    if (!choose_instance(f, inst)) return "";
    if (f.family == Family::kFlip2) format_instance(inst.flip2, name, sizeof name);
    else if (f.family == Family::kFlipK) format_instance(inst.flipk, name, sizeof name);
    else format_instance(inst.recom, name, sizeof name);
    return name;
}

static void check_one(const InstanceFacts &f, std::set<std::string> *seen) {
    static const int buffer = 0;
    char want[96] = {0};
    const RefParams p = ref_params(f);
    const int e = f.family == Family::kFlip2   ? ref_flip2(p, f.ring, want, sizeof want)
                  : f.family == Family::kFlipK ? ref_flipk(p, f.ring, want, sizeof want)
                                               : ref_recom(f.log ? &buffer : nullptr, f.log ? 100 : 0, f.ring, want, sizeof want);
    Instance inst;
    const std::string got = chosen(f, inst);
    CHECK(got == (e ? "" : want), "family %d ring %d nsub %d: chose '%s', the launchers' rule '%s'", (int)f.family, f.ring,
          f.nsub, got.c_str(), e ? "(refused)" : want);
    if (got.empty()) return;
    if (f.family == Family::kFlip2) {
        const Flip2Instance &i = inst.flip2;
        CHECK(!i.xtra || i.full, "%s: xtra without full", got.c_str());
        // the name is the value's: parsed back, it gives the same instance
        int r = 0, s = 0;
        char a[8], b[8], c[8], d[8];
        CHECK(std::sscanf(got.c_str(), "fc::flip2_kernel<%d, %d, %7[a-z], %7[a-z], %7[a-z], %7[a-z]>", &r, &s, a, b, c, d) == 6 &&
                  (Flip2Instance{r, s, !std::strcmp(a, "true"), !std::strcmp(b, "true"), !std::strcmp(c, "true"),
                                 !std::strcmp(d, "true")} == i),
              "%s does not spell its instance", got.c_str());
    } else if (f.family == Family::kFlipK) {
        const FlipKInstance &i = inst.flipk;
        CHECK(i.mf == 0 || i.km == 3, "%s: multi-flip without the district rule", got.c_str());
        int r = 0, s = 0, k = 0, m = 0;
        char a[8];
        CHECK(std::sscanf(got.c_str(), "fc::flip_kernel<%d, %d, %d, %7[a-z], %d>", &r, &s, &k, a, &m) == 5 &&
                  (FlipKInstance{r, s, k, !std::strcmp(a, "true"), m} == i),
              "%s does not spell its instance", got.c_str());
    } else {
        CHECK(inst.recom.ring == f.ring && inst.recom.log == f.log, "%s: not the run's ring / log", got.c_str());
    }
    if (seen) seen->insert(got);
}

static void check_exhaustive() {
    const uint32_t diags[] = {0, FC_DIAG_WAIT, FC_DIAG_HIST, FC_DIAG_EDGES, FC_DIAG_FLIPS, FC_DIAG_SERIES, FC_DIAG_FLIPS_EXACT};
    const Family families[] = {Family::kFlip2, Family::kFlipK, Family::kRecom};
    const size_t want[] = {72, 60, 4};
    for (int fi = 0; fi < 3; ++fi) {
        std::set<std::string> seen;
        for (int ring : {8, 16})
        for (int nsub : {1, 2, 4})
        for (uint32_t diag : diags)
        for (int bits = 0; bits < (1 << 11); ++bits) {  // every boolean input
            InstanceFacts f{};
            f.family = families[fi];
            f.ring = ring;
            f.nsub = nsub;
            f.diag = diag;
            f.tape = bits & 1;
            f.trace = bits & 2;
            f.variant = bits & 4;
            f.hit_window = bits & 8;
            f.all_exact = bits & 16;
            f.flags = (bits & 32 ? FC_FLAG_FORCE_BFS : 0u) | FC_FLAG_TALLY_LOG_SMALL;  // (another flag: not read)
            f.band = bits & 64;
            f.coop = bits & 128;
            f.dgraph = bits & 256;
            f.multi = bits & 512;
            f.log = bits & 1024;
            for (int marks = 0; marks <= 2; ++marks) {
                f.mf_marks = marks;
                check_one(f, &seen);
            }
        }
        CHECK(seen.size() == want[fi], "family %d reaches %zu distinct instances, not %zu", fi, seen.size(), want[fi]);
    }
}

static void check_refusals() {
    for (Family fam : {Family::kFlip2, Family::kFlipK, Family::kRecom}) {
        InstanceFacts f{};
        f.family = fam;
        f.ring = 12;
        f.nsub = 2;
        Instance inst;
        CHECK(!choose_instance(f, inst), "family %d: ring 12 is chosen an instance", (int)fam);
        check_one(f, nullptr);
        f.ring = 8;
        f.nsub = 3;
        // (the ReCom kernels take no NSUB: their launcher never read it)
        CHECK(choose_instance(f, inst) == (fam == Family::kRecom), "family %d: nsub 3", (int)fam);
        check_one(f, nullptr);
    }
}

// ---- the names the GPU tests assert, by hand ----
static InstanceFacts k2(int nsub = 4) {  // a k = 2 run on the sec11 grid: every node exact, nothing on
    InstanceFacts f{};
    f.family = Family::kFlip2;
    f.ring = 8;
    f.nsub = nsub;
    f.all_exact = true;
    return f;
}
static InstanceFacts kgt2(int ring, int nsub, bool dgraph, int mf_marks) {  // a k > 2 run, multi-flip on auto
    InstanceFacts f{};
    f.family = Family::kFlipK;
    f.ring = ring;
    f.nsub = nsub;
    f.all_exact = dgraph;
    f.dgraph = dgraph;
    f.multi = true;
    f.mf_marks = mf_marks;
    return f;
}
static InstanceFacts recom(int ring, bool log) {
    InstanceFacts f{};
    f.family = Family::kRecom;
    f.ring = ring;
    f.nsub = 4;
    f.log = log;
    f.diag = log ? FC_DIAG_SERIES : 0;
    return f;
}
template <class F> static InstanceFacts with(InstanceFacts f, F &&change) {
    change(f);
    return f;
}

static void check_table() {
    const uint32_t kAllDiag = FC_DIAG_WAIT | FC_DIAG_HIST | FC_DIAG_EDGES | FC_DIAG_FLIPS;
    const struct {
        const char *what;
        InstanceFacts f;
        const char *name;
    } rows[] = {
        {"lean sec11 k = 2", k2(), "fc::flip2_kernel<8, 4, false, false, false, false>"},
        {"FC_DIAG_WAIT only", with(k2(), [](auto &f) { f.diag = FC_DIAG_WAIT; }),
         "fc::flip2_kernel<8, 4, false, false, false, false>"},
        {"lean, one round", k2(1), "fc::flip2_kernel<8, 1, false, false, false, false>"},
        {"full diagnostics, no trace", with(k2(), [&](auto &f) { f.diag = kAllDiag; }),
         "fc::flip2_kernel<8, 4, true, false, false, false>"},
        {"FC_DIAG_HIST alone", with(k2(2), [](auto &f) { f.diag = FC_DIAG_HIST; }),
         "fc::flip2_kernel<8, 2, true, false, false, false>"},
        {"event log", with(k2(), [](auto &f) { f.diag = FC_DIAG_SERIES; f.log = true; }),
         "fc::flip2_kernel<8, 4, true, false, false, false>"},
        {"hitting-time window", with(k2(), [](auto &f) { f.hit_window = true; }),
         "fc::flip2_kernel<8, 4, true, false, false, false>"},
        {"every chain traced", with(k2(), [&](auto &f) { f.diag = kAllDiag; f.trace = true; }),
         "fc::flip2_kernel<8, 4, true, false, true, false>"},
        {"every chain traced, forced search",
         with(k2(), [&](auto &f) { f.diag = kAllDiag; f.trace = true; f.flags = FC_FLAG_FORCE_BFS; }),
         "fc::flip2_kernel<8, 4, true, true, true, false>"},
        {"replay tape", with(k2(), [](auto &f) { f.tape = true; }), "fc::flip2_kernel<8, 4, true, false, true, false>"},
        {"accept / constraint variant", with(k2(), [](auto &f) { f.variant = true; }),
         "fc::flip2_kernel<8, 4, true, false, true, false>"},
        {"forced search, lean", with(k2(), [](auto &f) { f.flags = FC_FLAG_FORCE_BFS; }),
         "fc::flip2_kernel<8, 4, false, true, false, false>"},
        {"inexact nodes (no positions)", with(k2(), [](auto &f) { f.all_exact = false; }),
         "fc::flip2_kernel<8, 4, false, true, false, false>"},
        {"16-cell rings, inexact", with(k2(), [](auto &f) { f.ring = 16; f.all_exact = false; }),
         "fc::flip2_kernel<16, 4, false, true, false, false>"},
        {"band stream", with(k2(), [](auto &f) { f.band = true; }), "fc::flip2_kernel<8, 4, false, false, false, true>"},
        {"band stream, full", with(k2(), [&](auto &f) { f.band = true; f.diag = kAllDiag; }),
         "fc::flip2_kernel<8, 4, true, false, false, true>"},
        {"C3 district rule", kgt2(8, 2, true, 2), "fc::flip_kernel<8, 2, 3, false, 2>"},
        {"C3 forced search", with(kgt2(8, 2, false, 0), [](auto &f) { f.flags = FC_FLAG_FORCE_BFS; f.all_exact = true; }),
         "fc::flip_kernel<8, 2, 0, false, 0>"},
        {"FC_FLAG_NB_PAIRS k = 4", with(kgt2(8, 2, true, 0), [](auto &f) { f.flags = FC_FLAG_NB_PAIRS; }),
         "fc::flip_kernel<8, 2, 3, false, 0>"},
        {"C4, hashed marks", kgt2(8, 2, true, 1), "fc::flip_kernel<8, 2, 3, false, 1>"},
        {"C5", kgt2(16, 4, true, 1), "fc::flip_kernel<16, 4, 3, false, 1>"},
        {"cooperative search", with(kgt2(16, 4, false, 0), [](auto &f) { f.coop = true; }),
         "fc::flip_kernel<16, 4, 1, false, 0>"},
        {"multi-flip hashed, full", with(kgt2(8, 2, true, 1), [&](auto &f) { f.diag = kAllDiag; }),
         "fc::flip_kernel<8, 2, 3, true, 1>"},
        {"multi-flip exact, full", with(kgt2(8, 2, true, 2), [&](auto &f) { f.diag = kAllDiag; }),
         "fc::flip_kernel<8, 2, 3, true, 2>"},
        {"multi-flip off", with(kgt2(8, 2, true, 2), [](auto &f) { f.multi = false; }), "fc::flip_kernel<8, 2, 3, false, 0>"},
        {"k > 2 replay tape", with(kgt2(8, 2, true, 2), [](auto &f) { f.tape = true; }), "fc::flip_kernel<8, 2, 3, true, 2>"},
        {"ReCom, 8-cell rings", recom(8, false), "fc::recom_kernel<8>"},
        {"ReCom, 16-cell rings", recom(16, false), "fc::recom_kernel<16>"},
        {"ReCom move log, 8", recom(8, true), "fc::recom_log_kernel<8>"},
        {"ReCom move log, 16", recom(16, true), "fc::recom_log_kernel<16>"},
    };
    for (const auto &row : rows) {
        Instance inst;
        const std::string got = chosen(row.f, inst);
        CHECK(got == row.name, "%s: chose '%s', expected '%s'", row.what, got.c_str(), row.name);
    }
}

// ---- the planner's four-neighbour fact of a graph file ----
static int plan_graph(const char *path) {
    FILE *fp = std::fopen(path, "rb");
    int32_t n = 0, nnz = 0;
    if (!fp || std::fread(&n, 4, 1, fp) != 1 || std::fread(&nnz, 4, 1, fp) != 1 || n <= 0 || nnz < 0) return 2;
    std::vector<int32_t> row((size_t)n + 1), col((size_t)nnz), pop((size_t)n);
    std::vector<double> pos(2 * (size_t)n);
    std::vector<int8_t> assign((size_t)n);
    if (std::fread(row.data(), 4, row.size(), fp) != row.size() || std::fread(col.data(), 4, col.size(), fp) != col.size() ||
        std::fread(pop.data(), 4, pop.size(), fp) != pop.size() || std::fread(pos.data(), 8, pos.size(), fp) != pos.size() ||
        std::fread(assign.data(), 1, assign.size(), fp) != assign.size())
        return 2;
    std::fclose(fp);
    HostGraph g;
    const std::string err = build_host_graph(n, row.data(), col.data(), pop.data(), pos.data(), 0, g);
    if (!err.empty()) {
        std::printf("graph: %s\n", err.c_str());
        return 2;
    }
    fc_params p;
    std::memset(&p, 0, sizeof p);
    p.struct_size = (uint32_t)sizeof(fc_params);
    p.abi_version = FC_ABI_VERSION;
    p.k = 2;
    p.base = 1.0;
    p.pop_hi = INT32_MAX;
    p.hit_lo = 1;
    RunPlan plan;
    std::string msg;
    if (const int rc = plan_run(g, p, 1, assign.data(), nullptr, plan, msg)) {
        std::printf("plan: %d %s\n", rc, msg.c_str());
        return 2;
    }
    Instance inst;
    std::printf("ring %d nbr4 %d instance %s\n", g.ring_max, (int)plan.nbr4,
                chosen(instance_facts(g, plan, false, false), inst).c_str());
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) return plan_graph(argv[1]);
    check_exhaustive();
    check_refusals();
    check_table();
    std::printf("checked %ld bad %ld\n", checks, bad);
    return bad ? 1 : 0;
}
