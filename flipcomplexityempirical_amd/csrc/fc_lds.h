// Where each array of a ReCom chain's (or a seed plan's) state sits in its slice of LDS, stated
// once: the ReCom and seed-plan kernels take their pointers from recom_lds (position type
// unsigned char *, from the slice's base), the planner its byte count (size_t, from 0), and
// tests/native/lds_layout_check.cpp executes it on the CPU.  Every region is derived from the one
// before it.  No HIP, no other header.
// (The flip kernels still spell their layouts out, and fc_plan.cpp their sizes: taking the pointers
// from a function like this one moved their register allocation -- more spilled scalar registers
// in 13 of the 60 k > 2 instances and in one or two of the 72 k = 2 ones, whichever form was tried.)
#pragma once
#include <cstddef>
#include <cstdint>

// FC_HD: a function of both the host and the device (spelled without HIP's __forceinline__, which
// only hip_runtime.h defines: host sources compiled as HIP include this header without it)
#if defined(__HIPCC__) || defined(__HIP__)
#define FC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define FC_HD inline
#endif

namespace fc {

// the position after n elements of type T at p: a byte count or a pointer
template <class T> FC_HD size_t lds_after(size_t p, size_t n) { return p + sizeof(T) * n; }
template <class T> FC_HD unsigned char *lds_after(unsigned char *p, int n) { return (unsigned char *)((T *)p + n); }

// 14 B per node for RMAX = 8, 15 for 16 (the kernels are latency-bound, so the chains a CU holds
// set their rate); npad: the nodes rounded up to a multiple of 16
template <class P>
struct RecomLds {
    // 8 B per node, three uses in turn: uint64 [npad] Boruvka keys; then the tree's CSR (int16
    // offsets [n + 1], then 2 (|M| - 1) int16 entries from index recom_csr_first(n)) with the int16
    // [npad] BFS parents at par, the last quarter; then int32 [npad] subtree populations (sign
    // bit: subset mark)
    P keys, par;
    P comp;      // int16 [npad] component; then level starts
    P order;     // int16 [npad] hook targets; then BFS order
    P tadj;      // uint8 (RMAX = 8) or uint16 [npad] tree edges (bit k: neighbour row entry k)
    P a;         // int8 [npad] assignment
    P end;
};
template <class P>
FC_HD RecomLds<P> recom_lds(P base, int npad, int ring_max) {
    RecomLds<P> L;
    L.keys = base;
    L.par = lds_after<uint8_t>(L.keys, 6 * (size_t)npad);
    L.comp = lds_after<uint64_t>(L.keys, npad);
    L.order = lds_after<int16_t>(L.comp, npad);
    L.tadj = lds_after<int16_t>(L.order, npad);
    L.a = ring_max == 8 ? lds_after<uint8_t>(L.tadj, npad) : lds_after<uint16_t>(L.tadj, npad);
    L.end = lds_after<int8_t>(L.a, npad);
    return L;
}
// int16 index, from keys, of the tree CSR's first entry
FC_HD int recom_csr_first(int n) { return (n + 2) & ~1; }

// The frame-series kernel (fc_series.hip) stages its tables in LDS: the frame edges' midpoints
// (double [2 n_frame]), the toggle rows (kFrameLdsWords uint64 per node that has a frame edge) and
// the node -> row index (int16 [n_nodes]).  Their bytes, or 0 when they do not fit (then the kernel
// reads them from global memory).  Host arithmetic only.
constexpr int kFrameLdsWords = 4;  // 64-bit words of a frame-edge mask: up to 256 frame edges
inline size_t frame_lds_bytes(int32_t n_frame, int32_t n_rows, int32_t n_nodes) {
    const size_t b = 16 * (size_t)n_frame + 8 * kFrameLdsWords * (size_t)n_rows + 2 * (size_t)n_nodes;
    return (b <= 48 * 1024 && n_nodes < 32768) ? (b + 15) & ~(size_t)15 : 0;
}

}  // namespace fc
