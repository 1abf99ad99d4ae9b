// tally_reduce: a launch's k = 2 tally logs (fc_tally.h) applied to the per-chain histograms,
// per-node and per-edge arrays, after the flip kernel on the same stream.
#include <hip/hip_runtime.h>

#include "fc_internal.h"
#include "fc_tally.h"
#include "fc_tally_plan.h"

namespace fc {

// Apply every chain's tally log and reset it: one workgroup per chain, after the flip kernel on
// the same stream, so the chain's serial stream never waits on these updates.  Each pass keeps
// the arrays of its mask (TR_* bits) privatised in LDS -- zeroed, every entry of the log applied
// with LDS atomics, then added (maxed) into the chain's global rows -- and applies the arrays of
// `gmask` with global atomics (those too large for any pass).  Global atomics from a separate
// kernel, for all arrays, took 62 ms per C2 launch: the chains' rows do not stay in L2.
// (TR_*, kTrArrays and the pass plan: fc_tally_plan.h)

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

int launch_tally_reduce(const KParams &p, int ring_max, void *stream, TallyPlan *used) {
    if (!p.tl_len || p.n_chains <= 0) return (int)hipSuccess;
    // the device's LDS per workgroup (gfx950: 160 KiB), queried, not assumed
    int dev = 0, optin = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess || optin <= 0)
        optin = 65536;
    // the arrays this run keeps in passes of at most that much LDS (fc_tally_plan.h)
    TallyPlan pl = plan_tally_reduce(p.diag, p.n, p.n_edges, (size_t)optin);
    const uint32_t gmask = pl.gmask;
    for (int i = 0; i < pl.n_passes; ++i) {
        size_t lds = (size_t)pl.bytes[i];
        uint32_t lmask = pl.lmask[i], g = i == 0 ? gmask : 0u;
        const int last = i + 1 == pl.n_passes ? 1 : 0;
        const void *fn = ring_max <= 8 ? (const void *)tally_reduce_kernel<8> : (const void *)tally_reduce_kernel<16>;
        if (lds > 65536 &&
            hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            // the device refuses this much dynamic LDS: the pass's arrays take the global atomics
            (void)hipGetLastError();
            g |= lmask;
            lmask = 0;
            lds = 0;
            pl.gmask |= pl.lmask[i];  // the plan as launched: an empty pass, its arrays global
            pl.lmask[i] = 0;
            pl.bytes[i] = 0;
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
    if (used) *used = pl;
    return (int)hipSuccess;
}

}  // namespace fc
