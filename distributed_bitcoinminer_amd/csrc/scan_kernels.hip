// scan_kernels.hip -- the gfx950 scan kernels of the min-hash nonce search.
//
// Replaces the miner's sequential loop (cmu440/bitcoin/miner/miner.go:46-59)
// over bitcoin.Hash (cmu440/bitcoin/hash.go:13-17).  Integer-VALU bound: no
// MFMA, no LDS on the hot path, ~zero HBM traffic.
//
//   hm_tiled_kernel      persistent waves (tasks from a workgroup-level
//                        LDS dispenser); per task 64 lanes x 100 loop
//                        steps; one SHA-256 compression per nonce from the
//                        tile state (+ a constant trailer block when the
//                        padding spills); wave-uniform running min in SGPRs,
//                        refreshed by a 64-lane shuffle reduce only when some
//                        lane's H0 <= the wave's best H0.
//   hm_chained_kernel    two-block tails whose final block is wave-uniform:
//                        per lane block 0 once, then a table-driven block.
//   hm_generic_kernel    one nonce per lane with a byte-level tail builder;
//                        small or irregular segments and cross-checks.
//   hm_*_csum_kernel     checked variants (CSUM=true): also the wrapping sum
//                        of the keys and the count of nonces hashed, per wave
//                        (hm_scan_checked).
//
// This file is compiled for the device only (`--cuda-device-only -S`); the
// Makefile passes the assembly through align_loops.py (instruction placement
// of the hot loops) and links it into the code object that the
// library embeds (scan_blob.S) and device.cpp loads with hipModuleLoadData.
// Kernels are therefore looked up by their mangled names (kernel_name() in
// seg_walk.cpp).
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "scan_tasks.hpp"
#include "sha256_defs.hpp"
#include "sha_device.hpp"

namespace hm {

// ---------------------------------------------------------------------------
// Tiled scan (the hot kernel)
// ---------------------------------------------------------------------------

// CSUM: checked variant (coverage sum and count of the hashed keys).
template <int W1, bool STRADDLE, bool TRAILER, bool CSUM>
DEV void tiled_body(const TiledArgs& A) {
    const uint32_t wslot = blockIdx.x * (kBlock / kWaveSize) + uni(threadIdx.x / kWaveSize);
    WaveBest best;   // wave-uniform (SGPR)
    WaveSums sums;   // CSUM only
    __shared__ LdsQueue queue;
    lds_queue_init(&queue);

    for (;;) {
        const uint32_t task = lds_dequeue(&queue, A.counter, A.lds_shift);
        if (task >= A.ntasks) break;
        // guided sizes: whole units first, then tenths (one tens digit each)
        const TiledTask T = tiled_decode(A, task);
        tiled_task<W1, STRADDLE, TRAILER, CSUM>(
            A.rec + (size_t)T.tile * kRecWords, T.chunk, T.t1_begin, T.t1_end,
            (A.tile0 + T.tile) * A.pow10V, A.seg_lo, A.seg_hi, A.vmax, A.q, A.lane_shift,
            A.loop_shift, A.s0_loop, A.trailer_kw, best, sums);
    }
    wave_store<CSUM>(A.cand, A.sums, wslot, best, sums);
}

template <int W1, bool STRADDLE, bool TRAILER>
__global__ void HM_TILED_BOUNDS hm_tiled_kernel(const TiledArgs A) {
    tiled_body<W1, STRADDLE, TRAILER, false>(A);
}

template <int W1, bool STRADDLE, bool TRAILER>
__global__ void HM_TILED_BOUNDS hm_tiled_csum_kernel(const TiledArgs A) {
    tiled_body<W1, STRADDLE, TRAILER, true>(A);
}

// ---------------------------------------------------------------------------
// Chained scan: per lane one compression of tail block 0 per task, then one
// table-driven compression per loop value (the final block is wave-uniform).
// With an epoch (f > fe final-block digits) the loop covers the low fe digits
// and A.ebase supplies the high ones.
// ---------------------------------------------------------------------------
template <bool CSUM>
DEV void chained_body(const ChainedArgs& A) {
    const uint32_t wslot = blockIdx.x * (kBlock / kWaveSize) + uni(threadIdx.x / kWaveSize);
    WaveBest best;
    WaveSums sums;  // CSUM only
    const uint32_t per_tile = A.tpt * A.ntc;
    __shared__ LdsQueue queue;
    lds_queue_init(&queue);

    for (;;) {
        const uint32_t task = lds_dequeue(&queue, A.counter, A.lds_shift);
        if (task >= A.ntasks) break;
        // guided sizes: whole loop chunks first, then kSplit pieces of each
        const ChainedTask T = chained_decode(A, per_tile, task);
        chained_task<CSUM>(A.rec + (size_t)T.tile * kRecWords, T.chunk, T.t_begin, T.t_end,
                           (A.tile0 + T.tile) * A.pow10qf + A.ebase, A.pow10f, A.seg_lo, A.seg_hi,
                           A.vmax, A.q, A.kwt, best, sums);
    }
    wave_store<CSUM>(A.cand, A.sums, wslot, best, sums);
}

__global__ void __launch_bounds__(kBlock) hm_chained_kernel(const ChainedArgs A) {
    chained_body<false>(A);
}

__global__ void __launch_bounds__(kBlock) hm_chained_csum_kernel(const ChainedArgs A) {
    chained_body<true>(A);
}

// ---------------------------------------------------------------------------
// Generic scan: one nonce per lane, any layout
// ---------------------------------------------------------------------------
template <bool CSUM>
DEV void generic_body(const GenericArgs& A) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t bk = ~0ull, bn = 0;
    uint64_t csum = 0, ccnt = 0;  // CSUM only
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= A.count_m1;) {
        const uint64_t n = A.seg_lo + k;
        uint32_t h0, h1;
        hash_nonce(A.pw, A.r, A.d, A.nb, A.total_bits, A.mid, n, h0, h1);
        const uint64_t key = ((uint64_t)h0 << 32) | h1;
        if constexpr (CSUM) { csum += key; ++ccnt; }
        if (key < bk || (key == bk && n < bn)) { bk = key; bn = n; }
        if (A.count_m1 - k < stride) break;
        k += stride;
    }
    wave_min(bk, bn);
    const uint32_t wslot = blockIdx.x * (kBlock / kWaveSize) + threadIdx.x / kWaveSize;
    if (__lane_id() == 0) {
        A.cand[2 * wslot] = bk;
        A.cand[2 * wslot + 1] = bn;
    }
    if constexpr (CSUM) store_sums(A.sums, wslot, csum, ccnt);
}

__global__ void __launch_bounds__(kBlock) hm_generic_kernel(const GenericArgs A) {
    generic_body<false>(A);
}

__global__ void __launch_bounds__(kBlock) hm_generic_csum_kernel(const GenericArgs A) {
    generic_body<true>(A);
}

// Every tiled layout the planner can pick, plain and checked.
#define HM_TILED_INST(W, S, T)                                                 \
    template __global__ void hm_tiled_kernel<W, S, T>(const TiledArgs);        \
    template __global__ void hm_tiled_csum_kernel<W, S, T>(const TiledArgs);
HM_FOR_EACH_TILED_LAYOUT(HM_TILED_INST)
#undef HM_TILED_INST

}  // namespace hm
