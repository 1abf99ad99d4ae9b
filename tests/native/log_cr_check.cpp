// log_cr (fc_philox.h: the correctly rounded logarithm the kernels take where a geometric wait's
// quotient lies within the device log's error of an integer) as host code: against inputs whose
// logarithm lies within 10^-4 ulp of a rounding tie (found by a search in 300-bit arithmetic; the
// first is the draw on which the device's own log once gave a wait one short) and corner inputs,
// with the correctly rounded values from that arithmetic; and against the host's log on two million
// inputs of the forms the kernels pass (1 - U for a 53-bit U; small and large arguments).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "fc_philox.h"

static const double kVectors[][2] = {
    {0x1.ab84e58e4bf9cp-1, -0x1.714e8b94b729ep-3},
    {0x1.fffffffffff30p-1, -0x1.a000000000055p-46},
    {0x1.fffffffffff10p-1, -0x1.e000000000071p-46},
    {0x1.ffffffffffde0p-1, -0x1.1000000000091p-44},
    {0x1.ffffffffffc20p-1, -0x1.f0000000001e1p-44},
    {0x1.ffffffffff340p-1, -0x1.9800000000515p-42},
    {0x1.ffffffffff2c0p-1, -0x1.a80000000057dp-42},
    {0x1.ffffffffff1c0p-1, -0x1.c800000000659p-42},
    {0x1.ffffffffff140p-1, -0x1.d8000000006cdp-42},
    {0x1.fffffffffd980p-1, -0x1.3400000000b95p-40},
    {0x1.fffffffffd280p-1, -0x1.6c0000000102dp-40},
    {0x1.fffffffffc380p-1, -0x1.e400000001c99p-40},
    {0x1.fffffffff4b00p-1, -0x1.6a00000003ffdp-38},
    {0x1.fffffffff4500p-1, -0x1.760000000444dp-38},
    {0x1.fffffffff2d00p-1, -0x1.a6000000056f5p-38},
    {0x1.fffffffff2700p-1, -0x1.b200000005bf9p-38},
    {0x1.fffffffff1f00p-1, -0x1.c2000000062e1p-38},
    {0x1.b4f8a1fb9c330p-5, -0x1.772c83ff28bccp+1},
    {0x1.ffffffff79c00p-1, -0x1.0c80000023339p-34},
    {0x1.997e363f476d4p-30, -0x1.4531dc54cf4fdp+4},
    {0x1.25486e16db928p-1, -0x1.1d47984eb52c4p-1},
    {0x1.7ea0ea7877c33p-1, -0x1.2a40077ec63d2p-2},
    {0x1.ffffffff32c00p-1, -0x1.9a8000005247dp-34},
    {0x1.7d62748eee210p-2, -0x1.f9af083ac056fp-1},
    {0x1.ff6a6e738ec43p-1, -0x1.2b4ed2c6cf8edp-10},
    {0x1.645ec1a40a7d6p-4, -0x1.388cc79009e37p+1},
    {0x1.75335050797d5p-43, -0x1.d6dab00c6c00cp+4},
    {0x1.91e99556b45a6p-53, -0x1.22493407f660dp+5},
    {0x1.a81b76a61b682p-2, -0x1.c3520cc0bfc6bp-1},
    {0x1.fffffff736ba0p-1, -0x1.1928c00269950p-30},
    {0x1.bb711a7caab90p-4, -0x1.1c91cdc61350cp+1},
    {0x1.fedca980b398dp-31, -0x1.4cbf0a3cbb452p+4},
    {0x1.ffcd94f2d6541p-1, -0x1.936c46970a710p-12},
    {0x1.17a91259a28d1p-16, -0x1.6010066f999b6p+3},
    {0x1.907e4e4b5d910p-26, -0x1.19305c6da9f8dp+4},
    {0x1.ceda70cbf2880p-1, -0x1.9d5886ac0168bp-4},
    {0x1.de3d0ad60b6d5p-22, -0x1.d3fa508191585p+3},
    {0x1.b2aa245a20288p-2, -0x1.b6bb365c50aaep-1},
    {0x1.38921e797d6aep-1, -0x1.f956692950061p-2},
    {0x1.6c08df6ad6a1cp-2, -0x1.08c2d20db8a5dp+0},
    {0x1.ffff1e209aa9dp-1, -0x1.c3bf2e51b6d80p-18},
    {0x1.fffd07301fbc7p-1, -0x1.7c690ac53d8a2p-16},
    {0x1.6f57e6dd78eb6p-9, -0x1.782420ac35960p+2},
    {0x1.ffffffce49c5cp-1, -0x1.8db1d2134e881p-28},
    {0x1.fffffffeb0010p-1, -0x1.4fff00006e3f6p-33},
    {0x1.ffb9c8c73f557p-1, -0x1.18f027048d00ep-11},
    {0x1.0de06fe109f1ep-52, -0x1.1fed4af426af4p+5},
    {0x1.ffff22992a4cbp-1, -0x1.bace0b2416bd0p-18},
    {0x1.02cfa2033edc0p-4, -0x1.617e54fdd9b3fp+1},
    {0x1.0000000000000p+0, 0x0.0p+0},
    {0x1.0000000000000p-1, -0x1.62e42fefa39efp-1},
    {0x1.0000000000000p-53, -0x1.25e4f7b2737fap+5},
    {0x1.fffffffffffffp-1, -0x1.0000000000000p-53},
    {0x1.6a09e667f3bcdp-1, -0x1.62e42fefa39eep-2},
    {0x1.6a09e667f3bccp-1, -0x1.62e42fefa39f1p-2},
    {0x1.8000000000000p-1, -0x1.269621134db92p-2},
    {0x1.fffffff800000p-1, -0x1.0000000200000p-30},
};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int64_t ulps_apart(double a, double b) {
    int64_t x, y;
    std::memcpy(&x, &a, 8);
    std::memcpy(&y, &b, 8);
    return x > y ? x - y : y - x;  // same sign (both logs <= 0)
}

int main() {
    int bad = 0;
    const int nv = (int)(sizeof kVectors / sizeof kVectors[0]);
    for (int i = 0; i < nv; ++i) {
        const double got = fc::log_cr(kVectors[i][0]);
        if (got != kVectors[i][1]) {
            std::printf("vector %d: log_cr(%a) = %a, correctly rounded %a\n", i, kVectors[i][0], got, kVectors[i][1]);
            ++bad;
        }
    }
    long n = 0, differ = 0, far = 0;
    for (int i = 0; i < 2000000; ++i) {
        const uint64_t r = next_u64();
        double x;
        switch (i % 3) {
            case 0: x = 1.0 - (double)(r >> 11) * 0x1p-53; break;                                  // 1 - U
            case 1: x = std::ldexp(0.5 + (double)(r >> 12) * 0x1p-53, -(int)(r & 63u) % 53); break;  // down to 2^-53
            default: x = 1.0 - std::ldexp((double)(r >> 11) * 0x1p-53, -1 - (int)(r & 31u)); break;  // near 1
        }
        if (!(x > 0.0 && x <= 1.0)) continue;
        const double a = fc::log_cr(x), b = std::log(x);
        ++n;
        if (a != b) {
            ++differ;
            if (ulps_apart(a, b) > 1) ++far;
        }
    }
    std::printf("vectors %d bad %d; random %ld differ %ld far %ld\n", nv, bad, n, differ, far);
    return bad || far ? 1 : 0;
}
