// scan_k_kernels.hip -- the gfx950 kernels of hm_scan_k (ABI 1.19): the k
// lowest (hash, nonce) pairs of a range, 1 <= k <= 32, in one pass.
//
// The ranking form of the miner's loop (cmu440/bitcoin/miner/miner.go:46-59
// over bitcoin.Hash, hash.go:13-17, is k = 1): instead of one running minimum,
//   for n = lo .. hi: keep the k lexicographically smallest (Hash(msg, n), n).
//
//   hm_scan_k_tiled_kernel    the task bodies of the scan kernels
//   hm_scan_k_chained_kernel  (scan_tasks.hpp tiled_task / chained_task, the
//                             same dispenser and guided split) with the "k
//                             lowest" reduction (WaveLowK) in place of the
//                             running minimum; every task runs, there is no
//                             stop word
//   hm_scan_k_generic_kernel  one nonce per lane, grid-stride steps of 64
//                             consecutive nonces per wave
//   hm_scan_k_fold_kernel     one workgroup, enqueued behind each launch: the
//                             launch's wave lists into the device list
//
// Device protocol (kernels.hpp ScanKArgs).  A wave keeps up to 64 records in
// its own 1 KiB of LDS and a wave-uniform bound; the per-nonce cost is the one
// compare of the running minimum (scan_tasks.hpp WaveLowK has the insertion
// and the compaction).  At launch entry a wave reads the device's carried
// bound -- written by the fold of the call's earlier launches, stream-ordered
// -- and, if the device list already holds k records, starts bounded by it
// with an empty list.  At its exit it compacts once more, writes its cnt <= k
// records and cnt to its own slot of the wave-list buffer, and adds its two
// diagnostics (records inserted, compactions) to the control block, one atomic
// each from one lane.  The fold kernel's four waves stream the launch's wave
// slots, 64 records a step, through the same insertion; wave 0 opens with the
// device list as its list, and after a workgroup barrier merges the other
// three waves' lists into its own, then writes the device list (sorted, count
// <= k) and the carried bound (valid if and only if count == k).  No wave
// spins or waits on another beyond the dispenser's LDS hand-off and that one
// barrier.
//
// Invariants:
//   1. Only in-range, non-surplus nonces enter a list: take_step(WaveLowK)
//      takes seg_lo <= n <= seg_hi and lane_ok (a surplus lane repeats another
//      lane's nonce: its duplicate would sit in the list twice).
//   2. A record is dropped only when k distinct records lexicographically
//      below it are known to exist: in this wave's list at that moment (a
//      compaction keeps the k lowest; the bound is the k-th of a list that
//      held k) or in the device list folded from earlier launches (the carried
//      bound).  The test against the bound is strict, and records are distinct
//      by nonce, so the k-th record itself is never dropped by its own bound.
//   3. Every task of every launch runs, and the segments, launches, epochs and
//      split pieces partition [lo, hi]: each nonce is hashed exactly once.
//   4. Every wave writes its list and its count before its kernel ends, and
//      the fold runs behind it on the same stream.
// So the k smallest of (device list U all wave lists) are the k smallest of
// everything hashed so far, whatever the dispatch order, and the device list
// after the last fold is the device's answer.
//
// Compiled like collect_kernels.hip (device-only -S, align_loops.py, linked
// into hipminer_scan.hsaco) and looked up by mangled name (kernel_name() in
// seg_walk.cpp).
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "scan_tasks.hpp"
#include "sha256_defs.hpp"
#include "sha_device.hpp"

namespace hm {

constexpr int kWaves = kBlock / kWaveSize;
// a workgroup's wave lists: 64 slots of 2 x u64 per wave
struct LowKLists {
    uint64_t rec[kWaves][2 * kWaveSize];
};

DEV void lowk_carried(WaveLowK& w, const ScanKArgs& K) {
    if (uni64(K.ctl[kSkCount]) == K.k) {
        w.bkey = uni64(K.ctl[kSkBoundKey]);
        w.bnonce = uni64(K.ctl[kSkBoundNonce]);
        w.bhi = (uint32_t)(w.bkey >> 32);
        w.bounded = true;
    }
}

DEV WaveLowK lowk_begin(const ScanKArgs& K, LowKLists* lists) {
    WaveLowK w;
    w.k = K.k;
    w.list = lists->rec[uni(threadIdx.x / kWaveSize)];
    lowk_carried(w, K);
    return w;
}

// The wave's exit: its sorted list and count to its slot, its diagnostics to
// the control block.
DEV void lowk_end(const ScanKArgs& K, WaveLowK& w) {
    if (w.cnt) lowk_compact(w);
    const uint32_t lane = __lane_id();
    const uint32_t wslot = blockIdx.x * kWaves + uni(threadIdx.x / kWaveSize);
    if (lane < w.cnt) {  // cnt <= k <= kScanKMax
        uint64_t* out = K.wave_recs + ((size_t)wslot * kScanKMax + lane) * 2;
        out[0] = w.list[2 * lane];
        out[1] = w.list[2 * lane + 1];
    }
    if (lane == 0) K.wave_cnt[wslot] = w.cnt;
    wave_total(K.ctl + kSkInserted, w.inserted);
    wave_total(K.ctl + kSkCompactions, w.compactions);
}

template <int W1, bool STRADDLE, bool TRAILER>
__global__ void HM_TILED_BOUNDS hm_scan_k_tiled_kernel(const ScanKTiledArgs KA) {
    const TiledArgs& A = KA.t;
    __shared__ LdsQueue queue;
    __shared__ LowKLists lists;
    WaveLowK low = lowk_begin(KA.k, &lists);
    WaveSums sums;  // unused (CSUM = false)
    lds_queue_init(&queue);

    for (;;) {
        const uint32_t task = lds_dequeue(&queue, A.counter, A.lds_shift);
        if (task >= A.ntasks) break;
        const TiledTask T = tiled_decode(A, task);
        tiled_task<W1, STRADDLE, TRAILER, false>(
            A.rec + (size_t)T.tile * kRecWords, T.chunk, T.t1_begin, T.t1_end,
            (A.tile0 + T.tile) * A.pow10V, A.seg_lo, A.seg_hi, A.vmax, A.q, A.lane_shift,
            A.loop_shift, A.s0_loop, A.trailer_kw, low, sums);
    }
    lowk_end(KA.k, low);
}

__global__ void __launch_bounds__(kBlock) hm_scan_k_chained_kernel(const ScanKChainedArgs KA) {
    const ChainedArgs& A = KA.c;
    __shared__ LdsQueue queue;
    __shared__ LowKLists lists;
    WaveLowK low = lowk_begin(KA.k, &lists);
    WaveSums sums;  // unused (CSUM = false)
    const uint32_t per_tile = A.tpt * A.ntc;
    lds_queue_init(&queue);

    for (;;) {
        const uint32_t task = lds_dequeue(&queue, A.counter, A.lds_shift);
        if (task >= A.ntasks) break;
        const ChainedTask T = chained_decode(A, per_tile, task);
        chained_task<false>(A.rec + (size_t)T.tile * kRecWords, T.chunk, T.t_begin, T.t_end,
                            (A.tile0 + T.tile) * A.pow10qf + A.ebase, A.pow10f, A.seg_lo, A.seg_hi,
                            A.vmax, A.q, A.kwt, low, sums);
    }
    lowk_end(KA.k, low);
}

// One nonce per lane, any layout.  Wave w of the grid takes the 64 nonces
// seg_lo + 64 w + i * stride .. + 63 in step i.
__global__ void __launch_bounds__(kBlock) hm_scan_k_generic_kernel(const ScanKGenericArgs KA) {
    const GenericArgs& A = KA.g;
    __shared__ LowKLists lists;
    WaveLowK low = lowk_begin(KA.k, &lists);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = __lane_id();
    for (uint64_t kb = (uint64_t)blockIdx.x * blockDim.x + uni(threadIdx.x / kWaveSize) * kWaveSize;
         kb <= A.count_m1;) {
        // lanes past the segment's end repeat the step's first nonce: surplus
        const bool live = A.count_m1 - kb >= lane;
        const uint64_t n = A.seg_lo + kb + (live ? lane : 0u);
        uint32_t h0, h1;
        hash_nonce(A.pw, A.r, A.d, A.nb, A.total_bits, A.mid, n, h0, h1);
        // the launch's nonces are [seg_lo, seg_lo + count_m1]: no wrap
        take_step(low, wave_cand(low, h0), h0, h1, n, 0, A.seg_lo, A.seg_lo + A.count_m1, live);
        if (A.count_m1 - kb < stride) break;
        kb += stride;
    }
    lowk_end(KA.k, low);
}

// One fold step: the lanes with `valid` offer (key, nn).
DEV void fold_step(WaveLowK& w, bool valid, uint64_t key, uint64_t nn) {
    const bool ok = valid && (!w.bounded || lex_below(key, nn, w.bkey, w.bnonce));
    const uint64_t hits = __builtin_amdgcn_ballot_w64(ok);
    if (hits) lowk_insert(w, ok, hits, key, nn);
}

__global__ void __launch_bounds__(kBlock) hm_scan_k_fold_kernel(const ScanKFoldArgs FA) {
    const ScanKArgs& K = FA.k;
    __shared__ LowKLists lists;
    __shared__ uint32_t counts[kWaves];
    const uint32_t wave = uni(threadIdx.x / kWaveSize), lane = __lane_id();
    uint64_t* dev_list = K.ctl + kSkList;
    WaveLowK w;
    w.k = K.k;
    w.list = lists.rec[wave];
    if (wave == 0) {
        // the device list is wave 0's opening list; with k records in it the
        // compaction makes its k-th the bound
        uint32_t dcount = (uint32_t)uni64(K.ctl[kSkCount]);
        if (dcount > K.k) dcount = K.k;
        if (lane < dcount) {
            w.list[2 * lane] = dev_list[2 * lane];
            w.list[2 * lane + 1] = dev_list[2 * lane + 1];
        }
        __builtin_amdgcn_wave_barrier();
        w.cnt = dcount;
        if (dcount) lowk_compact(w);
    } else {
        lowk_carried(w, K);
    }
    // two wave slots of kScanKMax records per step
    static_assert(2 * kScanKMax == kWaveSize, "a fold step is two wave slots");
    for (uint32_t s0 = 2 * wave; s0 < FA.nwaves; s0 += 2 * kWaves) {
        const uint32_t slot = s0 + (lane >> 5), i = lane & 31u;
        const bool valid = slot < FA.nwaves && i < K.wave_cnt[slot];
        uint64_t key = 0, nn = 0;
        if (valid) {
            const uint64_t* in = K.wave_recs + ((size_t)slot * kScanKMax + i) * 2;
            key = in[0];
            nn = in[1];
        }
        fold_step(w, valid, key, nn);
    }
    if (w.cnt) lowk_compact(w);
    if (lane == 0) counts[wave] = w.cnt;
    __syncthreads();
    if (wave != 0) return;
    for (int v = 1; v < kWaves; ++v) {
        const bool valid = lane < counts[v];  // <= k <= 32
        uint64_t key = 0, nn = 0;
        if (valid) {
            key = lists.rec[v][2 * lane];
            nn = lists.rec[v][2 * lane + 1];
        }
        fold_step(w, valid, key, nn);
    }
    if (w.cnt) lowk_compact(w);
    if (lane < w.cnt) {
        dev_list[2 * lane] = w.list[2 * lane];
        dev_list[2 * lane + 1] = w.list[2 * lane + 1];
    }
    if (lane == 0) {
        K.ctl[kSkCount] = w.cnt;
        // the list's k-th record, valid if and only if count == k
        K.ctl[kSkBoundKey] = w.bkey;
        K.ctl[kSkBoundNonce] = w.bnonce;
    }
}

// Every tiled layout the planner can pick.
#define HM_SCAN_K_INST(W, S, T) \
    template __global__ void hm_scan_k_tiled_kernel<W, S, T>(const ScanKTiledArgs);
HM_FOR_EACH_TILED_LAYOUT(HM_SCAN_K_INST)
#undef HM_SCAN_K_INST

}  // namespace hm
