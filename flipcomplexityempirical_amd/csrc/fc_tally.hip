// tally_reduce: a launch's k = 2 tally logs (fc_tally.h) applied to the per-chain histograms,
// per-node and per-edge arrays, after the flip kernel on the same stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "fc_internal.h"
#include "fc_tally.h"

namespace fc {

// Apply every chain's tally log and reset it: one workgroup per chain, after the flip kernel on
// the same stream, so the chain's serial stream never waits on these updates.  Each pass keeps
// the arrays of its mask (TR_* bits) privatised in LDS -- zeroed, every entry of the log applied
// with LDS atomics, then added (maxed) into the chain's global rows -- and applies the arrays of
// `gmask` with global atomics (those too large for any pass).  Global atomics from a separate
// kernel, for all arrays, took 62 ms per C2 launch: the chains' rows do not stay in L2.
enum : uint32_t { TR_CUT = 1, TR_NB = 2, TR_EDGE = 4, TR_NF = 8, TR_PS = 16, TR_LF = 32, TR_FC = 64, TR_OCC = 128, TR_LA = 256 };
constexpr int kTrArrays = 9;

__device__ __forceinline__ int64_t tr_len(const KParams &p, int a) {  // entries of array a per chain
    return a == 0 ? (int64_t)p.n_edges + 1 : a == 1 ? (int64_t)p.n + 1 : a == 2 ? (int64_t)p.n_edges : (int64_t)p.n;
}
__device__ __forceinline__ int64_t *tr_row(const KParams &p, int a, int c) {  // chain c's global row
    int64_t *b = a == 0 ? p.cut_hist : a == 1 ? p.nb_hist : a == 2 ? p.edge_acc : a == 3 ? p.num_flips
               : a == 4 ? p.part_sum : a == 5 ? p.last_flipped : a == 6 ? p.flip_count : a == 7 ? p.occ_acc : p.last_accept;
    return b + (size_t)c * (size_t)tr_len(p, a);
}

template <int RMAX>
__global__ __launch_bounds__(1024) void tally_reduce_kernel(KParams p, uint32_t lmask, uint32_t gmask, int last) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *acc = (unsigned long long *)smem;
    const int c = (int)blockIdx.x;
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const int64_t len = p.tl_len[c];
    const int64_t lab0 = p.labels[0], lab1 = p.labels[1];
    // LDS offsets (in entries) of the arrays of this pass, in TR order
    int64_t off[kTrArrays];
    int64_t tot = 0;
#pragma unroll
    for (int a = 0; a < kTrArrays; ++a) {
        off[a] = tot;
        if ((lmask >> a) & 1u) tot += tr_len(p, a);
    }
    for (int64_t i = tid; i < tot; i += nt) acc[i] = 0ull;
    __syncthreads();
    const uint4 *lg = (const uint4 *)p.tl + (size_t)c * (size_t)p.tl_cap;
    const int64_t t0 = p.tl_t0[c];
    // one update: LDS when the array is in this pass, global when it is in gmask
    auto add = [&](int a, int64_t i, int64_t v) {
        if ((lmask >> a) & 1u) atomicAdd(acc + off[a] + i, (unsigned long long)v);
        else if ((gmask >> a) & 1u) atomicAdd((unsigned long long *)(tr_row(p, a, c) + i), (unsigned long long)v);
    };
    auto mx = [&](int a, int64_t i, int64_t v) {
        if ((lmask >> a) & 1u) atomicMax(acc + off[a] + i, (unsigned long long)v);
        else if ((gmask >> a) & 1u) atomicMax((unsigned long long *)(tr_row(p, a, c) + i), (unsigned long long)v);
    };
    const uint32_t want = lmask | gmask;
    // kU entries per thread in flight: their log loads, then their ring-edge loads, are issued
    // together (2.24 -> 2.11 ms per C2 launch; contiguous stretches per thread instead, so one
    // instruction's lanes carry entries from 64 stretches of the launch: 2.54 ms)
    constexpr int kU = 8;
    const bool edges = (want & TR_EDGE) != 0;
    for (int64_t b0 = tid; b0 < len; b0 += (int64_t)nt * kU) {
        uint4 e[kU];
#pragma unroll
        for (int k = 0; k < kU; ++k) {
            const int64_t i = b0 + (int64_t)k * nt;
            e[k] = i < len ? lg[i] : make_uint4(0u, 0u, 0u, 0u);
        }
        int4 er[kU][RMAX / 4];
#pragma unroll
        for (int k = 0; k < kU; ++k) {
            const int64_t i = b0 + (int64_t)k * nt;
            const bool need = edges && i < len && !((e[k].w >> 25) & 1u);
            const int4 *rp = (const int4 *)(p.ring_eid + (size_t)(e[k].z & 0xffffu) * RMAX);
#pragma unroll
            for (int j = 0; j < RMAX / 4; ++j) er[k][j] = need ? rp[j] : make_int4(-1, -1, -1, -1);
        }
#pragma unroll
        for (int k = 0; k < kU; ++k) {
            if (b0 + (int64_t)k * nt >= len) break;
            const uint4 ek = e[k];  // (tally_pack)
            const int64_t t = t0 + (int64_t)(ek.x & 0xffffffu);
            const int run = (int)((ek.x >> 24) | ((ek.y & 0xffffu) << 8));
            const uint32_t qv = ek.z, qc = (ek.w & 0xffffffu) | (((ek.w >> 24) & 1u) << 31);
            const int u = (int)(qv & 0xffffu);
            if (want & TR_CUT) add(0, (int64_t)(qc & 0x7fffffffu), run);
            if (want & TR_NB) add(1, (int64_t)(ek.y >> 16), run);
            if ((ek.w >> 25) & 1u) {  // kind 1 (tally_apply)
                if (u != 0xffff) {
                    if (want & TR_LF) mx(5, u, t + run);
                    if (want & TR_PS) add(4, u, ((qv >> 16) & 1u ? lab0 - lab1 : lab1 - lab0) * run);
                    if (want & TR_NF) add(3, u, run);
                }
                continue;
            }
            const int tg = (int)(qc >> 31);
            const int64_t lab_t = tg ? lab1 : lab0, lab_o = tg ? lab0 : lab1;
            const int64_t t_last = t + run - 1;
            if (want & TR_LF) mx(5, u, t_last);
            if (want & TR_PS) add(4, u, (lab_o - lab_t) * t_last);
            if (want & TR_NF) add(3, u, run);
            if (want & TR_FC) add(6, u, 1);
            if (want & TR_OCC) add(7, u, -(lab_t - lab_o) * t);
            if (want & TR_LA) mx(8, u, t);
            if (edges) {
                const uint32_t up = qv >> 16;
#pragma unroll
                for (int j = 0; j < RMAX / 4; ++j) {
                    const int ev[4] = {er[k][j].x, er[k][j].y, er[k][j].z, er[k][j].w};
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (ev[q] >= 0) add(2, ev[q], ((up >> (4 * j + q)) & 1u) ? -t : t);
                }
            }
        }
    }
    __syncthreads();
    // the pass's sums (maxima) into the chain's rows: one workgroup per chain, so no atomics
#pragma unroll
    for (int a = 0; a < kTrArrays; ++a) {
        if (!((lmask >> a) & 1u)) continue;
        int64_t *row = tr_row(p, a, c);
        const int64_t L = tr_len(p, a);
        const bool is_max = a == 5 || a == 8;
        // four rows' entries per thread in flight (their loads issued together)
        for (int64_t b0 = tid; b0 < L; b0 += (int64_t)nt * 4) {
            int64_t cur[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = b0 + (int64_t)k * nt;
                cur[k] = i < L ? row[i] : 0;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = b0 + (int64_t)k * nt;
                if (i >= L) break;
                const int64_t v = (int64_t)acc[off[a] + i];
                if (is_max) {
                    if (v > cur[k]) row[i] = v;
                } else if (v) {
                    row[i] = cur[k] + v;
                }
            }
        }
    }
    if (last) {
        __syncthreads();
        if (tid == 0) p.tl_len[c] = 0;
    }
}

int launch_tally_reduce(const KParams &p, int ring_max, void *stream) {
    if (!p.tl_len || p.n_chains <= 0) return (int)hipSuccess;
    // the arrays this run keeps, their per-chain bytes, packed greedily into passes of at most
    // 160 KiB of LDS (sec11 with every tally: one pass of 139 KiB, one 1024-thread workgroup per
    // CU: the log is read once); an array above 160 KiB goes to global atomics
    uint32_t have = 0;
    if (p.diag & FC_DIAG_HIST) have |= TR_CUT | TR_NB;
    if (p.diag & FC_DIAG_EDGES) have |= TR_EDGE;
    if (p.diag & FC_DIAG_FLIPS) have |= TR_NF | TR_PS | TR_LF;
    if (p.diag & FC_DIAG_FLIPS_EXACT) have |= TR_FC | TR_OCC | TR_LA;
    auto bytes = [&](int a) -> size_t {
        return 8 * (size_t)(a == 0 ? p.n_edges + 1 : a == 1 ? p.n + 1 : a == 2 ? p.n_edges : p.n);
    };
    // the device's LDS per workgroup (gfx950: 160 KiB), queried, not assumed
    int dev = 0, optin = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess || optin <= 0)
        optin = 65536;
    const size_t kPass = (size_t)optin, kMaxLds = (size_t)optin;
    std::vector<std::pair<uint32_t, size_t>> passes;
    uint32_t gmask = 0;
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
    for (size_t i = 0; i < passes.size(); ++i) {
        size_t lds = passes[i].second;
        uint32_t lmask = passes[i].first, g = i == 0 ? gmask : 0u;
        const int last = i + 1 == passes.size() ? 1 : 0;
        const void *fn = ring_max <= 8 ? (const void *)tally_reduce_kernel<8> : (const void *)tally_reduce_kernel<16>;
        if (lds > 65536 &&
            hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            // the device refuses this much dynamic LDS: the pass's arrays take the global atomics
            (void)hipGetLastError();
            g |= lmask;
            lmask = 0;
            lds = 0;
        }
        if (ring_max <= 8)
            hipLaunchKernelGGL(tally_reduce_kernel<8>, dim3(p.n_chains), dim3(1024), lds, (hipStream_t)stream, p,
                               lmask, g, last);
        else
            hipLaunchKernelGGL(tally_reduce_kernel<16>, dim3(p.n_chains), dim3(1024), lds, (hipStream_t)stream, p,
                               lmask, g, last);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return (int)hipSuccess;
}

}  // namespace fc
