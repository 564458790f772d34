// collect_kernels.hip -- the gfx950 kernels of hm_collect (ABI 1.11): EVERY
// nonce of a range whose hash is below a target, and their exact count.
//
// The share-collection form of the miner's loop (cmu440/bitcoin/miner/miner.go:
// 46-59 over bitcoin.Hash, hash.go:13-17): instead of keeping the minimum,
//   for n = lo .. hi: if Hash(msg, n) < target: emit (Hash, n).
//
//   hm_collect_tiled_kernel    the task bodies of the scan kernels
//   hm_collect_chained_kernel  (scan_tasks.hpp tiled_task / chained_task, the
//                              same dispenser and guided split) with the "all
//                              below target" reduction (WaveCollect) in place
//                              of the running minimum
//   hm_collect_generic_kernel  one nonce per lane, grid-stride steps of 64
//                              consecutive nonces per wave
//
// Device protocol: two 64-bit words per device (CollectArgs::total, ::cursor),
// both zeroed on the stream before a call's first launch, and a buffer of
// `cap` 16-byte records (cap = 0: a pure count, no buffer).
//   count    a wave counts its hits in a register (popcount of the ballot of
//            `ok`) and adds them to `total` once at exit: one agent-scope
//            atomic from one lane.  Counting touches no memory per step.
//   reserve  (cap > 0) on a step with hits one lane reserves popcount slots
//            with one agent-scope fetch_add on `cursor`; hit lane i takes slot
//            base + (hits in lanes below i) and writes (hash, nonce) there
//            with ordinary vector stores if the slot is < cap
//   full     a wave that sees a base >= cap stops reserving (wave-uniform
//            flag): the call has overflowed, the host will not read the
//            buffer, and a dense target does not serialise on one address
//            for the rest of the launch.  It keeps counting.
// No wave waits on another beyond the dispenser's existing LDS hand-off, and
// nothing here spins.
//
// The total is exact and the records complete whatever the dispatch order,
// because
//   1. a nonce is counted and recorded only if it lies in [seg_lo, seg_hi],
//      its key is < target, and its lane is not a surplus lane (the task
//      bodies clamp lanes past vmax to vmax, the generic kernel's lanes past
//      the segment end repeat the step's first nonce: such lanes hash a nonce
//      another lane already holds -- harmless to a minimum, a double count
//      here -- so take_step(WaveCollect) takes lane_ok),
//   2. every task of every launch runs and nothing is skipped; the segments,
//      launches, epochs and split pieces partition [lo, hi], so each nonce is
//      tested exactly once,
//   3. every wave adds its count and writes its records before its kernel
//      ends, and the host reads only after the stream is idle.
// The host recomputes nothing: a record carries the hash the kernel formed.
// Which slot a record lands in depends on dispatch order; the host sorts the
// records by nonce, so the answer does not.
//
// Compiled like scan_kernels.hip (device-only -S, align_loops.py, linked into
// hipminer_scan.hsaco) and looked up by mangled name (kernel_name() in
// seg_walk.cpp).
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "scan_tasks.hpp"
#include "sha256_defs.hpp"
#include "sha_device.hpp"

namespace hm {

DEV WaveCollect collect_begin(const CollectArgs& C) {
    WaveCollect c;
    c.target = C.target;
    c.thi = (uint32_t)((C.target - 1) >> 32);
    c.cursor = C.cursor;
    c.out = C.out;
    c.cap = C.cap;
    return c;
}

template <int W1, bool STRADDLE, bool TRAILER>
__global__ void HM_TILED_BOUNDS hm_collect_tiled_kernel(const CollectTiledArgs CA) {
    const TiledArgs& A = CA.t;
    WaveCollect col = collect_begin(CA.k);
    WaveSums sums;  // unused (CSUM = false)
    __shared__ LdsQueue queue;
    lds_queue_init(&queue);

    for (;;) {
        const uint32_t task = lds_dequeue(&queue, A.counter, A.lds_shift);
        if (task >= A.ntasks) break;
        const TiledTask T = tiled_decode(A, task);
        tiled_task<W1, STRADDLE, TRAILER, false>(
            A.rec + (size_t)T.tile * kRecWords, T.chunk, T.t1_begin, T.t1_end,
            (A.tile0 + T.tile) * A.pow10V, A.seg_lo, A.seg_hi, A.vmax, A.q, A.lane_shift,
            A.loop_shift, A.s0_loop, A.trailer_kw, col, sums);
    }
    wave_total(CA.k.total, col.count);
}

__global__ void __launch_bounds__(kBlock) hm_collect_chained_kernel(const CollectChainedArgs CA) {
    const ChainedArgs& A = CA.c;
    WaveCollect col = collect_begin(CA.k);
    WaveSums sums;  // unused (CSUM = false)
    const uint32_t per_tile = A.tpt * A.ntc;
    __shared__ LdsQueue queue;
    lds_queue_init(&queue);

    for (;;) {
        const uint32_t task = lds_dequeue(&queue, A.counter, A.lds_shift);
        if (task >= A.ntasks) break;
        const ChainedTask T = chained_decode(A, per_tile, task);
        chained_task<false>(A.rec + (size_t)T.tile * kRecWords, T.chunk, T.t_begin, T.t_end,
                            (A.tile0 + T.tile) * A.pow10qf + A.ebase, A.pow10f, A.seg_lo, A.seg_hi,
                            A.vmax, A.q, A.kwt, col, sums);
    }
    wave_total(CA.k.total, col.count);
}

// One nonce per lane, any layout.  Wave w of the grid takes the 64 nonces
// seg_lo + 64 w + i * stride .. + 63 in step i.
__global__ void __launch_bounds__(kBlock) hm_collect_generic_kernel(const CollectGenericArgs CA) {
    const GenericArgs& A = CA.g;
    WaveCollect col = collect_begin(CA.k);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = __lane_id();
    for (uint64_t kb = (uint64_t)blockIdx.x * blockDim.x + uni(threadIdx.x / kWaveSize) * kWaveSize;
         kb <= A.count_m1;) {
        // lanes past the segment's end repeat the step's first nonce: surplus
        const bool live = A.count_m1 - kb >= lane;
        const uint64_t n = A.seg_lo + kb + (live ? lane : 0u);
        // hash_nonce's text (sha_device.hpp), kept here as this kernel's own
        // copy: through the helper the kernel measured 1-2 % slower
        // (profiles/README.md, dedup/)
        uint32_t w[32];
        build_tail(w, A.pw, A.r, A.d, 0, n, A.nb, A.total_bits);
        uint32_t st[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) st[j] = A.mid[j];
        uint32_t m[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) m[j] = w[j];
        d_compress(st, m);
        if (A.nb == 2) {
#pragma unroll
            for (int j = 0; j < 16; ++j) m[j] = w[16 + j];
            d_compress(st, m);
        }
        // the launch's nonces are [seg_lo, seg_lo + count_m1]: no wrap
        take_step(col, wave_cand(col, st[0]), st[0], st[1], n, 0, A.seg_lo,
                  A.seg_lo + A.count_m1, live);
        if (A.count_m1 - kb < stride) break;
        kb += stride;
    }
    wave_total(CA.k.total, col.count);
}

// Every tiled layout the planner can pick.
#define HM_COLLECT_INST(W, S, T) \
    template __global__ void hm_collect_tiled_kernel<W, S, T>(const CollectTiledArgs);
HM_FOR_EACH_TILED_LAYOUT(HM_COLLECT_INST)
#undef HM_COLLECT_INST

}  // namespace hm
