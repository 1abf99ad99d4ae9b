// philox_round_keys + philox4x32_10_keys (the k = 2 flip kernel's form: round keys from a table)
// against philox4x32_10 (key schedule by two adds per round), as host code: 1,000 random
// (counter, seed) pairs, plus the all-zero and all-ones corners.  Prints "pairs N bad M".
#include <cstdint>
#include <cstdio>

#include "fc_philox.h"

static uint64_t sm64(uint64_t &s) {  // splitmix64
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int check(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    uint32_t keys[fc::kPhiloxKeyWords];
    fc::philox_round_keys(k0, k1, keys);
    const fc::Words4 a = fc::philox4x32_10(c0, c1, c2, c3, k0, k1);
    const fc::Words4 b = fc::philox4x32_10_keys(c0, c1, c2, c3, (const uint32_t *)keys);
    return !(a.x0 == b.x0 && a.x1 == b.x1 && a.x2 == b.x2 && a.x3 == b.x3);
}

int main() {
    uint64_t s = 0x5EED0009ull;
    int n = 0, bad = 0;
    for (int i = 0; i < 1000; ++i, ++n) {
        const uint64_t a = sm64(s), b = sm64(s), k = sm64(s);
        bad += check((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32), (uint32_t)k, (uint32_t)(k >> 32));
    }
    bad += check(0, 0, 0, 0, 0, 0), ++n;
    bad += check(~0u, ~0u, ~0u, ~0u, ~0u, ~0u), ++n;
    // the known-answer vector of Random123 (kat_vectors: philox4x32 10, counter and key all ones)
    {
        const fc::Words4 w = fc::philox4x32_10(~0u, ~0u, ~0u, ~0u, ~0u, ~0u);
        if (!(w.x0 == 0x408f276du && w.x1 == 0x41c83b0eu && w.x2 == 0xa20bc7c6u && w.x3 == 0x6d5451fdu)) {
            std::printf("known answer: %08x %08x %08x %08x\n", w.x0, w.x1, w.x2, w.x3);
            ++bad;
        }
    }
    std::printf("pairs %d bad %d\n", n, bad);
    return bad != 0;
}
