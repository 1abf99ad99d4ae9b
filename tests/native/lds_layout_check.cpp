// CPU check of the per-chain LDS layout of csrc/fc_lds.h, the ReCom and seed-plan kernels'
// (tests/test_lds_layout.py builds and runs it).  Over a grid of shapes:
//   - the regions are ascending, do not overlap and are aligned to their element size, or wider
//     where wider accesses are made (the table is this file's own), and the pointer form agrees
//     with the byte-count form;
//   - the planner's totals (the layout's end, plus the phase-counter tail in a diagnostic build,
//     rounded up to 16) equal the closed forms it used before the layout was stated in one place
//     (copied here literally, not computed through the header);
//   - the tree CSR's offsets and its 2 (n - 1) entries end at or before par, and the speculative
//     child reads past them (up to RMAX - 1 entries, fc_bipartition.h) end at or before comp,
//     inside the chain's own slice.
//   - frame_lds_bytes (the frame-series kernel's staged tables) at the shapes the series tests run,
//     the 120 x 120 one that does not fit among them; `lds_layout_check frame F R N ...` prints it
//     for any shapes (tests/test_series_cases.py asks for its case table's).
// Prints counts and the smallest npad - n from which those reads stay clear of par; exits 1 on any
// failure.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "fc_lds.h"

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

struct Region {
    const char *name;
    size_t at, elem, count;  // start, element size, elements
    size_t align;            // required alignment (>= elem where wider accesses are made)
};

// ascending, no overlap, aligned; the last region ends at `end`
static void check_regions(const char *what, const std::vector<Region> &r, size_t end, int n) {
    for (size_t i = 0; i < r.size(); ++i) {
        CHECK(r[i].at % r[i].align == 0, "%s n=%d: %s at %zu not aligned to %zu", what, n, r[i].name, r[i].at, r[i].align);
        const size_t next = i + 1 < r.size() ? r[i + 1].at : end;
        CHECK(r[i].at + r[i].elem * r[i].count <= next, "%s n=%d: %s [%zu, +%zu) runs into the next region at %zu", what,
              n, r[i].name, r[i].at, r[i].elem * r[i].count, next);
    }
}

// ---- the closed forms of the planner before fc_lds.h (fc_plan.cpp plan_lds / plan_seed,
// fc_internal.h recom_lds_bytes), copied literally ----
static const int kProfSlots_ref = 32;
static int ref_recom_lds_bytes(int n, int ring_max) { return (ring_max == 8 ? 14 : 15) * ((n + 15) & ~15); }
static int ref_recom_total(int n, int R, bool prof) {
    int chain_lds_bytes = ref_recom_lds_bytes(n, R);
    if (prof) chain_lds_bytes += kProfSlots_ref * 8;
    return (chain_lds_bytes + 15) & ~15;
}
static int ref_seed_total(int n, int R) { return (ref_recom_lds_bytes(n, R) + 15) & ~15; }

alignas(16) static unsigned char slice[1 << 18];  // a chain's slice for the pointer form

static void check_recom(int n, int R, bool prof) {
    const int npad = (n + 15) & ~15;
    const auto L = recom_lds<size_t>(0, npad, R);
    const size_t N = (size_t)npad, te = R == 8 ? 1 : 2;
    // (par lies inside the keys' 8 npad bytes: checked by itself below; tadj takes 32-bit atomics)
    std::vector<Region> r = {{"keys", L.keys, 8, N, 16}, {"comp", L.comp, 2, N, 2}, {"order", L.order, 2, N, 2},
                             {"tadj", L.tadj, te, N, 4}, {"a", L.a, 1, N, 16}};
    check_regions("recom", r, L.end, n);
    CHECK(L.par == L.keys + 6 * N && L.par % 2 == 0 && L.par + 2 * N == L.comp, "recom n=%d: par at %zu", n, L.par);
    // the planner's totals, as fc_plan.cpp forms them from the layout's end
    const size_t total = (L.end + (prof ? kProfSlots_ref * 8 : 0) + 15) & ~(size_t)15;
    CHECK((int)total == ref_recom_total(n, R, prof), "recom n=%d R=%d prof=%d: total %zu, parent %d", n, R, prof, total,
          ref_recom_total(n, R, prof));
    CHECK((((int)L.end + 15) & ~15) == ref_seed_total(n, R), "seed n=%d R=%d: end %zu, parent %d", n, R, L.end,
          ref_seed_total(n, R));
    CHECK(L.end == (size_t)(R == 8 ? 14 : 15) * N, "recom n=%d R=%d: end %zu", n, R, L.end);
    if (total <= sizeof slice) {
        const auto D = recom_lds(slice, npad, R);
        CHECK((size_t)(D.par - slice) == L.par && (size_t)(D.comp - slice) == L.comp && (size_t)(D.order - slice) == L.order &&
                  (size_t)(D.tadj - slice) == L.tadj && (size_t)(D.a - slice) == L.a && (size_t)(D.end - slice) == L.end,
              "recom n=%d: pointer form differs from the byte counts", n);
    }
}

// the tree CSR inside the keys' space (fc_bipartition.h): int16 offsets [n + 1] at keys, entries
// from int16 index recom_csr_first(n); returns whether the speculative reads stay clear of par
static bool check_csr(int n, int R) {
    const int npad = (n + 15) & ~15;
    const auto L = recom_lds<size_t>(0, npad, R);
    const size_t first = L.keys + 2 * (size_t)recom_csr_first(n);
    const size_t written = first + 2 * (size_t)(2 * (n - 1));
    const size_t read = first + 2 * (size_t)(2 * (n - 1) + R - 1);
    CHECK(L.keys + 2 * (size_t)(n + 1) <= first, "csr n=%d: offsets run into the entries", n);
    CHECK(written <= L.par, "csr n=%d R=%d: entries end at %zu, par at %zu", n, R, written, L.par);
    CHECK(read <= L.comp, "csr n=%d R=%d: reads end at %zu, comp at %zu", n, R, read, L.comp);
    return read <= L.par;
}

// frame_lds_bytes at the shapes (frame edges, toggle rows, nodes) the series tests run: the bytes
// are counted here array by array, and the largest shape is the one that does not fit
static void check_frame() {
    struct Shape {
        const char *name;
        int n_frame, n_rows, n_nodes;
        size_t want;
    };
    const Shape shapes[] = {{"sec11 frame", 152, 152, 1596, 2432 + 4864 + 3192 + 8},
                            {"65-cycle, every edge", 65, 65, 65, 1040 + 2080 + 130 + 14},
                            {"256-cycle, every edge", 256, 256, 256, 4096 + 8192 + 512},
                            {"120 x 120 grid, 256 disjoint edges", 256, 512, 14400, 0}};
    for (const Shape &s : shapes) {
        const size_t got = frame_lds_bytes(s.n_frame, s.n_rows, s.n_nodes);
        CHECK(got == s.want && got % 16 == 0, "frame %s: %zu bytes, expected %zu", s.name, got, s.want);
        std::printf("frame_lds_bytes %d %d %d = %zu (%s)\n", s.n_frame, s.n_rows, s.n_nodes, got, s.name);
    }
    CHECK(4096 + 16384 + 28800 > 48 * 1024, "the 120 x 120 shape fits after all");
    // one node either side of the 48 KiB limit
    CHECK(frame_lds_bytes(0, 0, 24576) == 49152 && frame_lds_bytes(0, 0, 24577) == 0, "48 KiB limit");
    CHECK(frame_lds_bytes(0, 0, 1) == 16 && frame_lds_bytes(1, 2, 7) == 96, "rounding up to 16");
    CHECK(frame_lds_bytes(0, 0, 32767) == 0 && frame_lds_bytes(0, 0, 32768) == 0, "n_nodes beyond the limit");
}

// `lds_layout_check frame F R N [F R N ...]`: frame_lds_bytes of the given shapes, one line each
static int print_frames(int argc, char **argv) {
    if ((argc - 2) % 3 != 0) return 2;
    for (int i = 2; i + 2 < argc; i += 3) {
        const int f = std::atoi(argv[i]), r = std::atoi(argv[i + 1]), n = std::atoi(argv[i + 2]);
        std::printf("frame_lds_bytes %d %d %d = %zu\n", f, r, n, frame_lds_bytes(f, r, n));
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "frame") return print_frames(argc, argv);
    check_frame();
    std::vector<int> ns;
    for (int n = 1; n <= 200; ++n) ns.push_back(n);
    for (int n : {1596, 2000, 4095, 4096, 10100}) ns.push_back(n);
    long shapes = 0;
    for (int n : ns)
        for (int R : {8, 16})
            for (int prof = 0; prof < 2; ++prof, ++shapes) check_recom(n, R, prof != 0);
    for (int R : {8, 16}) {
        int clear_from = 0;  // the smallest slack from which every n keeps the reads clear of par
        for (int n = 2; n <= 4096; ++n)
            if (!check_csr(n, R)) {
                const int slack = ((n + 15) & ~15) - n;
                if (slack + 1 > clear_from) clear_from = slack + 1;
            }
        std::printf("recom RMAX %d: speculative reads stay clear of par from npad - n >= %d\n", R, clear_from);
    }
    std::printf("shapes %ld checks %ld bad %ld\n", shapes, checks, bad);
    return bad ? 1 : 0;
}
