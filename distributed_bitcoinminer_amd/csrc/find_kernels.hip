// find_kernels.hip -- the gfx950 kernels of hm_find: the LOWEST nonce of a
// range whose hash is below a target, found without scanning the rest.
//
// The proof-of-work form of the miner's loop (cmu440/bitcoin/miner/miner.go:
// 46-59 over bitcoin.Hash, hash.go:13-17): instead of keeping the minimum,
//   for n = lo .. hi: if Hash(msg, n) < target: return n.
//
//   hm_find_tiled_kernel    the task bodies of the scan kernels
//   hm_find_chained_kernel  (scan_tasks.hpp tiled_task / chained_task, the
//                           same dispenser and guided split) with the "first
//                           below target" reduction (WaveFirst) in place of
//                           the running minimum
//   hm_find_generic_kernel  one nonce per lane; a task is one grid-stride
//                           step of a wave (64 consecutive nonces)
//
// Device protocol: one 64-bit stop word per device (FindArgs::word), set to
// MaxUint64 on the stream before a call's first launch.
//   publish  a wave whose task lowered its best nonce writes it with one
//            agent-scope atomic min (one lane), right after the task
//   skip     before each task a wave reads the word (relaxed, agent scope);
//            a task whose smallest nonce is above it is not run
//   leave    task ids are monotone in their smallest nonce -- (tile, chunk)
//            for tiled, (tile, chunk, loop chunk) for chained, the guided
//            split tail above all whole units, and a workgroup's dispenser
//            hands its waves ascending ids -- so on the first skip the wave
//            leaves its loop: every id it, or anyone, could still draw is
//            above the word too
//   exit     a launch whose smallest nonce is above the word does nothing
//   count    each wave adds the tasks it ran to FindArgs::tasks_run once
// No wave waits on another beyond the dispenser's existing LDS hand-off.
//
// hm_cancel (ABI 1.18; cancel_relay.hpp).  Wave 0 of workgroup 0
// is the launch's RELAY: at kernel entry and between its tasks (right after each
// task it ran, so before the next one it takes; the generic kernel: before each
// step) it reads the context's cancel flag (FindArgs::cancel, pinned host memory;
// one relaxed system-scope load) and, if it is set, lowers the stop word to 0,
// from where
// skip / leave / exit above end this launch and those queued behind it.  A
// word lowered so is FORGED -- 0 is not a hit -- and the invariants
// below speak of a call that was not cancelled.  The cancel invariant:
//   The word is forged only if the flag is set.  The flag is set before the
//   device can see it, and only the call's own thread clears it (at call
//   start).  Therefore the host, which tests the flag after every wait or
//   readback and BEFORE it interprets any control word, never mistakes a
//   forged word for an answer.
//
// The final word is the lowest hit whatever the dispatch order, because
//   1. only nonces n in [seg_lo, seg_hi] with Hash(msg, n) < target are
//      published (take_step(WaveFirst&)),
//   2. a task is skipped only if every nonce in it is above a value already
//      published, and the word only decreases (atomic min), so a skipped
//      task cannot hold the lowest hit,
//   3. every task that ran publishes its hit before its kernel ends.
// The host recomputes the answer's hash (host_hash): only the nonce crosses.
//
// Compiled like scan_kernels.hip (device-only -S, align_loops.py, linked into
// hipminer_scan.hsaco) and looked up by mangled name (kernel_name() in
// seg_walk.cpp).
#include <hip/hip_runtime.h>

#include "cancel_relay.hpp"
#include "kernels.hpp"
#include "scan_tasks.hpp"
#include "sha256_defs.hpp"
#include "sha_device.hpp"

namespace hm {

// The stop word, wave-uniform: one lane loads, the wave shares the value.
DEV uint64_t find_stop(const FindArgs& F) {
    uint64_t w = 0;
    if (__lane_id() == 0)
        w = __hip_atomic_load(F.word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return uni64(w);
}
DEV void find_publish(const FindArgs& F, uint64_t nonce) {
    if (__lane_id() == 0)
        __hip_atomic_fetch_min(F.word, nonce, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
DEV void find_count(const FindArgs& F, uint32_t ran) {
    if (ran && __lane_id() == 0)
        __hip_atomic_fetch_add(F.tasks_run, (uint64_t)ran, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}
DEV WaveFirst find_first(const FindArgs& F) {
    WaveFirst first;
    first.target = F.target;
    first.thi = (uint32_t)((F.target - 1) >> 32);
    return first;
}

// Before a task whose smallest nonce is task_lo: false = skip it (and leave).
// Otherwise the wave's bound drops to the published hit (nonces at or above
// it cannot win) and *before = the bound the task starts from.
DEV bool find_enter(const FindArgs& F, WaveFirst& first, uint64_t task_lo, uint64_t* before) {
    const uint64_t stop = find_stop(F);
    if (task_lo > stop) return false;
    if (stop < first.nonce) first.nonce = stop;
    *before = first.nonce;
    return true;
}

template <int W1, bool STRADDLE, bool TRAILER>
__global__ void HM_TILED_BOUNDS hm_find_tiled_kernel(const FindTiledArgs FA) {
    const TiledArgs& A = FA.t;
    const FindArgs& F = FA.f;
    WaveFirst first = find_first(F);
    WaveSums sums;  // unused (CSUM = false)
    __shared__ LdsQueue queue;
    lds_queue_init(&queue);
    uint32_t ran = 0;
    const bool relay = cancel_is_relay(F.cancel);
    cancel_relay(relay, F.cancel, F.word);
    if (find_stop(F) < F.launch_lo) return;

    for (;;) {
        const uint32_t task = lds_dequeue(&queue, A.counter, A.lds_shift);
        if (task >= A.ntasks) break;
        const TiledTask T = tiled_decode(A, task);
        const uint64_t tile_base = (A.tile0 + T.tile) * A.pow10V;
        // lane 0's first loop step: the task's smallest nonce
        const uint64_t task_lo =
            tile_base + (uint64_t)T.chunk * (kWaveSize * 100u) + T.t1_begin * 10u;
        uint64_t before;
        if (!find_enter(F, first, task_lo, &before)) break;
        tiled_task<W1, STRADDLE, TRAILER, false>(
            A.rec + (size_t)T.tile * kRecWords, T.chunk, T.t1_begin, T.t1_end, tile_base, A.seg_lo,
            A.seg_hi, A.vmax, A.q, A.lane_shift, A.loop_shift, A.s0_loop, A.trailer_kw, first, sums);
        ++ran;
        if (first.nonce < before) find_publish(F, first.nonce);
        cancel_relay(relay, F.cancel, F.word);
    }
    find_count(F, ran);
}

__global__ void __launch_bounds__(kBlock) hm_find_chained_kernel(const FindChainedArgs FA) {
    const ChainedArgs& A = FA.c;
    const FindArgs& F = FA.f;
    WaveFirst first = find_first(F);
    WaveSums sums;  // unused (CSUM = false)
    const uint32_t per_tile = A.tpt * A.ntc;
    __shared__ LdsQueue queue;
    lds_queue_init(&queue);
    uint32_t ran = 0;
    const bool relay = cancel_is_relay(F.cancel);
    cancel_relay(relay, F.cancel, F.word);
    if (find_stop(F) < F.launch_lo) return;

    for (;;) {
        const uint32_t task = lds_dequeue(&queue, A.counter, A.lds_shift);
        if (task >= A.ntasks) break;
        const ChainedTask T = chained_decode(A, per_tile, task);
        const uint64_t tile_base = (A.tile0 + T.tile) * A.pow10qf + A.ebase;
        // lane 0's first loop value: the task's smallest nonce (its lanes
        // stride pow10f, so the task reaches 63 * pow10f beyond it)
        const uint64_t task_lo = tile_base + (uint64_t)T.chunk * kWaveSize * A.pow10f + T.t_begin;
        uint64_t before;
        if (!find_enter(F, first, task_lo, &before)) break;
        chained_task<false>(A.rec + (size_t)T.tile * kRecWords, T.chunk, T.t_begin, T.t_end,
                            tile_base, A.pow10f, A.seg_lo, A.seg_hi, A.vmax, A.q, A.kwt, first,
                            sums);
        ++ran;
        if (first.nonce < before) find_publish(F, first.nonce);
        cancel_relay(relay, F.cancel, F.word);
    }
    find_count(F, ran);
}

// One nonce per lane, any layout.  Wave w of the grid takes the 64 nonces
// seg_lo + 64 w + i * stride .. + 63 in step i: ascending per wave, so the
// first step above the word ends the wave.
__global__ void __launch_bounds__(kBlock) hm_find_generic_kernel(const FindGenericArgs FA) {
    const GenericArgs& A = FA.g;
    const FindArgs& F = FA.f;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = __lane_id();
    uint32_t ran = 0;
    uint64_t best = ~0ull;  // wave-uniform
    const bool relay = cancel_is_relay(F.cancel);
    cancel_relay(relay, F.cancel, F.word);
    if (find_stop(F) < F.launch_lo) return;
    for (uint64_t kb = (uint64_t)blockIdx.x * blockDim.x + uni(threadIdx.x / kWaveSize) * kWaveSize;
         kb <= A.count_m1;) {
        cancel_relay(relay, F.cancel, F.word);
        const uint64_t stop = find_stop(F);
        if (A.seg_lo + kb > stop) break;
        if (stop < best) best = stop;
        // lanes past the segment's end repeat the step's first nonce
        const bool live = A.count_m1 - kb >= lane;
        const uint64_t n = A.seg_lo + kb + (live ? lane : 0u);
        // hash_nonce's text (sha_device.hpp), kept here as this kernel's own
        // copy: through the helper hipcc loads the whole argument block before
        // the early exit above and the kernel spills 10 more SGPRs (83 for 73)
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
        ++ran;
        const uint64_t key = ((uint64_t)st[0] << 32) | st[1];
        const bool hit = key < F.target && n < best;
        if (__builtin_amdgcn_ballot_w64(hit)) {
            uint64_t nn = hit ? n : ~0ull, zero = 0;
            wave_min(nn, zero);
            best = uni64(nn);
            find_publish(F, best);
        }
        if (A.count_m1 - kb < stride) break;
        kb += stride;
    }
    find_count(F, ran);
}

// Every tiled layout the planner can pick.
#define HM_FIND_INST(W, S, T) \
    template __global__ void hm_find_tiled_kernel<W, S, T>(const FindTiledArgs);
HM_FOR_EACH_TILED_LAYOUT(HM_FIND_INST)
#undef HM_FIND_INST

}  // namespace hm
