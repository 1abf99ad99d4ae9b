// The k = 2 ring-verdict table (csrc/fc_ring_table.h) of a graph file, checked on the host:
//   * every entry -- all classes x all 256 ring bytes -- against the evaluation stated the long way
//     here (the interval form of the run rule, fc_ring.h one_run, on bits & full; the byte's bits at
//     the ring length and up must not matter);
//   * class ids dense, one per distinct (length, neighbours, links), and the same for every key
//     when the nodes are visited in another order;
//   * a cap below the class count, or 0, yields no table;
//   * the planner (fc_plan.cpp): a k = 2 plan carries the table and each node's class in the upper
//     half of its record's degree word, the degree below it; with tune_ring_table 0, or a k = 4
//     plan, the records are the plain ones.
// Usage: ring_table_check <graph file>  (n, nnz, row_ptr, col_idx, pop as int32, pos as float64, a
// two-district plan as int8).  Prints "graph n <n> ring <R> nbr4 <0|1> classes <count>" and
// "checked <entries> bad <count>".
#include <cstdio>
#include <cstring>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#include "fc_plan.h"
#include "fc_ring_table.h"

using namespace fc;

static long checks = 0, bad = 0;
#define CHECK(cond, ...)               \
    do {                               \
        ++checks;                      \
        if (!(cond)) {                 \
            if (++bad <= 20) {         \
                std::printf(__VA_ARGS__); \
                std::printf("\n");     \
            }                          \
        }                              \
    } while (0)

// the slot evaluation of fc_flip2.hip's ring body, statement by statement, with the early-return
// form of the run rule
struct Verdict {
    int nA, delta;
    bool hit, s_lin, s_cyc;
};
static Verdict long_way(uint32_t bits, uint32_t Ln, uint32_t nbr, uint32_t link) {
    const uint32_t full = (1u << Ln) - 1u;
    const uint32_t inA = bits & full;
    const uint32_t nbrA = inA & nbr, tmask = nbr & ~inA;
    Verdict r;
    r.nA = __builtin_popcount(nbrA);
    r.delta = r.nA - __builtin_popcount(tmask);
    r.hit = tmask != 0u;
    // step i -> i + 1 (cyclic) is an old-district link when both cells are in A and the ring links them
    uint32_t lk = 0;
    for (uint32_t i = 0; i < Ln; ++i)
        if (((inA >> i) & 1u) && ((inA >> ((i + 1) % Ln)) & 1u) && ((link >> i) & 1u)) lk |= 1u << i;
    r.s_lin = one_run(nbrA, full & ~lk, full);
    uint32_t closing = 0;
    if (Ln >= 2 && (inA & 1u) && ((inA >> (Ln - 1)) & 1u)) closing = 1u << (Ln - 1);
    r.s_cyc = one_run(nbrA, full & ~(lk | closing), full);
    return r;
}

static int read_graph(const char *path, HostGraph &g, std::vector<int8_t> &assign) {
    FILE *fp = std::fopen(path, "rb");
    int32_t n = 0, nnz = 0;
    if (!fp || std::fread(&n, 4, 1, fp) != 1 || std::fread(&nnz, 4, 1, fp) != 1 || n <= 0 || nnz < 0) return 2;
    std::vector<int32_t> row((size_t)n + 1), col((size_t)nnz), pop((size_t)n);
    std::vector<double> pos(2 * (size_t)n);
    assign.resize((size_t)n);
    const bool ok = std::fread(row.data(), 4, row.size(), fp) == row.size() &&
                    std::fread(col.data(), 4, col.size(), fp) == col.size() &&
                    std::fread(pop.data(), 4, pop.size(), fp) == pop.size() &&
                    std::fread(pos.data(), 8, pos.size(), fp) == pos.size() &&
                    std::fread(assign.data(), 1, assign.size(), fp) == assign.size();
    std::fclose(fp);
    if (!ok) return 2;
    const std::string err = build_host_graph(n, row.data(), col.data(), pop.data(), pos.data(), 0, g);
    if (!err.empty()) {
        std::printf("graph: %s\n", err.c_str());
        return 2;
    }
    return 0;
}

static fc_params params(int k, int ring_table) {
    fc_params p;
    std::memset(&p, 0, sizeof p);
    p.struct_size = (uint32_t)sizeof(fc_params);
    p.abi_version = FC_ABI_VERSION;
    p.k = k;
    p.proposal = k == 2 ? FC_PROPOSE_BI_SIGN : FC_PROPOSE_PAIR;
    p.base = 1.0;
    p.pop_hi = INT32_MAX;
    p.hit_lo = 1;
    p.tune_ring_table = ring_table;
    return p;
}

static int32_t rec_deg(const RunPlan &plan, int32_t v) {
    int32_t d;
    std::memcpy(&d, plan.node_recs.data() + (size_t)v * sizeof(NodeRec<8>) + offsetof(NodeRec<8>, deg), 4);
    return d;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    HostGraph g;
    std::vector<int8_t> assign;
    if (const int rc = read_graph(argv[1], g, assign)) return rc;
    const int n = g.n;
    bool nbr4 = true;
    for (uint64_t m : g.meta) nbr4 = nbr4 && __builtin_popcount((uint32_t)(m >> kMetaNbrShift) & 0xffffu) <= 4;

    // ---- the table against the long way ----
    std::vector<uint16_t> cls;
    std::vector<RingEntry> table;
    const int count = build_ring_table(g.meta.data(), n, kRingTableMaxClasses, cls, table);
    std::printf("graph n %d ring %d nbr4 %d classes %d\n", n, g.ring_max, (int)nbr4, count);
    if (g.ring_max != kRingTableRmax) {  // (every graph of the test has 8-cell rings)
        std::printf("checked 0 bad 1\n");
        return 1;
    }
    CHECK((int)cls.size() == n && (int)table.size() == count * kRingTableRow, "table of %d classes: %zu class ids, %zu entries",
          count, cls.size(), table.size());
    std::map<RingClassKey, int> id_of;
    std::vector<int> members(count, 0);
    for (int v = 0; v < n && (int)cls.size() == n; ++v) {
        const RingClassKey key = ring_class_key(g.meta[v]);
        CHECK(cls[v] < count, "node %d: class %d of %d", v, (int)cls[v], count);
        if (cls[v] >= count) continue;
        ++members[cls[v]];
        const auto it = id_of.emplace(key, (int)cls[v]).first;
        CHECK(it->second == (int)cls[v], "node %d: key has classes %d and %d", v, it->second, (int)cls[v]);
    }
    CHECK((int)id_of.size() == count, "%zu distinct keys, %d classes", id_of.size(), count);
    for (int c = 0; c < count; ++c) CHECK(members[c] > 0, "class %d has no node (ids not dense)", c);
    for (const auto &kv : id_of) {
        const uint32_t Ln = kv.first[0], nbr = kv.first[1], link = kv.first[2];
        const uint32_t full = (1u << Ln) - 1u;
        for (uint32_t bits = 0; bits < (uint32_t)kRingTableRow && (int)table.size() == count * kRingTableRow; ++bits) {
            const uint32_t e = table[(size_t)kv.second * kRingTableRow + bits];
            const Verdict w = long_way(bits & full, Ln, nbr, link);
            CHECK(ring_entry_delta(e) == w.delta && ring_entry_na(e) == w.nA && ((e & kReHit) != 0) == w.hit &&
                      ((e & kReSlin) != 0) == w.s_lin && ((e & kReScyc) != 0) == w.s_cyc &&
                      (e & ~(kReDeltaMask | kReVerdicts | (0xfu << kReNaShift))) == 0u,
                  "class %d (Ln %u nbr %#x link %#x) bits %#x: entry %#x, long way delta %d nA %d hit %d lin %d cyc %d",
                  kv.second, Ln, nbr, link, bits, e, w.delta, w.nA, (int)w.hit, (int)w.s_lin, (int)w.s_cyc);
        }
    }

    // ---- the same ids for the keys under another node order (reversed, and a stride walk) ----
    for (int order = 0; order < 2; ++order) {
        std::vector<int> perm(n);
        std::iota(perm.begin(), perm.end(), 0);
        if (order == 0) {
            for (int i = 0; i < n / 2; ++i) std::swap(perm[i], perm[n - 1 - i]);
        } else {
            int step = 7;
            while (std::gcd(step, n) != 1) ++step;
            for (int i = 0; i < n; ++i) perm[i] = (int)(((long)i * step + 3) % n);
        }
        std::vector<uint64_t> meta2(n);
        for (int i = 0; i < n; ++i) meta2[i] = g.meta[perm[i]];
        std::vector<uint16_t> cls2;
        std::vector<RingEntry> table2;
        const int count2 = build_ring_table(meta2.data(), n, kRingTableMaxClasses, cls2, table2);
        CHECK(count2 == count && table2 == table, "order %d: %d classes against %d, or another table", order, count2, count);
        for (int i = 0; i < n && (int)cls2.size() == n; ++i)
            CHECK(cls2[i] == cls[perm[i]], "order %d: node %d has class %d, was %d", order, perm[i], (int)cls2[i], (int)cls[perm[i]]);
    }

    // ---- the cap ----
    for (int cap : {count - 1, 0}) {
        std::vector<uint16_t> c3;
        std::vector<RingEntry> t3;
        const int got = build_ring_table(g.meta.data(), n, cap, c3, t3);
        CHECK(got == count && c3.empty() && t3.empty(), "cap %d: count %d, %zu ids, %zu entries", cap, got, c3.size(), t3.size());
    }
    {
        std::vector<uint16_t> c3;
        std::vector<RingEntry> t3;
        const int got = build_ring_table(g.meta.data(), n, count, c3, t3);
        CHECK(got == count && c3 == cls && t3 == table, "cap %d = the count: no table", count);
    }

    // ---- the planner ----
    {
        RunPlan plan;
        std::string msg;
        const fc_params p = params(2, count);
        const int rc = plan_run(g, p, 1, assign.data(), nullptr, plan, msg);
        CHECK(rc == 0, "plan_run: %d %s", rc, msg.c_str());
        if (rc == 0) {
            CHECK(plan.ring_classes == count && plan.ring_table_on == nbr4, "plan: %d classes, table %d (nbr4 %d)",
                  plan.ring_classes, (int)plan.ring_table_on, (int)nbr4);
            CHECK(plan.ring_table_on ? plan.ring_table == table : plan.ring_table.empty(), "plan: another table");
            for (int v = 0; v < n; ++v) {
                const int32_t d = rec_deg(plan, v), deg = g.row_ptr[v + 1] - g.row_ptr[v];
                CHECK((d & 0xffff) == deg && (d >> 16) == (plan.ring_table_on ? (int)cls[v] : 0), "node %d: degree word %#x", v, d);
            }
        }
        for (int variant = 0; variant < 3; ++variant) {  // cap one short; the knob at 0; a k = 4 plan: plain records
            RunPlan q;
            fc_params p2 = params(variant == 2 ? 4 : 2, variant == 0 ? count - 1 : variant == 1 ? 0 : count);
            std::vector<int8_t> a4(assign);
            const int rc2 = plan_run(g, p2, 1, a4.data(), nullptr, q, msg);
            if (variant == 2 && rc2 != 0) continue;  // (a two-district plan is no k = 4 start: nothing to look at)
            CHECK(rc2 == 0, "plan_run variant %d: %d %s", variant, rc2, msg.c_str());
            if (rc2 != 0) continue;
            CHECK(!q.ring_table_on && q.ring_table.empty(), "variant %d: a table", variant);
            for (int v = 0; v < n; ++v)
                CHECK(rec_deg(q, v) == g.row_ptr[v + 1] - g.row_ptr[v], "variant %d node %d: degree word %#x", variant, v, rec_deg(q, v));
        }
        fc_params p3 = params(2, kRingTableMaxClasses + 1);
        RunPlan q;
        CHECK(plan_run(g, p3, 1, assign.data(), nullptr, q, msg) == FC_ERR_ARG, "tune_ring_table above the maximum was accepted");
        p3.tune_ring_table = -1;
        CHECK(plan_run(g, p3, 1, assign.data(), nullptr, q, msg) == FC_ERR_ARG, "tune_ring_table -1 was accepted");
    }
    std::printf("checked %ld bad %ld\n", checks, bad);
    return bad ? 1 : 0;
}
