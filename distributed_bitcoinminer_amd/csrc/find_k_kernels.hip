// find_k_kernels.hip -- the gfx950 kernels of hm_find_k (ABI 1.16): the k
// LOWEST nonces of a range whose hash is below a target, found without
// scanning the rest.
//
// The pool form of the miner's loop (cmu440/bitcoin/miner/miner.go:46-59 over
// bitcoin.Hash, hash.go:13-17): "from nonce lo, the next k shares",
//   for n = lo .. hi: if Hash(msg, n) < target: emit (Hash, n); stop after k.
//
//   hm_find_k_tiled_kernel    the task bodies of the scan kernels
//   hm_find_k_chained_kernel  (scan_tasks.hpp tiled_task / chained_task, the
//                             same dispenser and guided split) with the "k
//                             lowest below target" reduction (WaveFirstK)
//   hm_find_k_generic_kernel  one nonce per lane; a task is one grid-stride
//                             step of a wave (64 consecutive nonces)
//
// Device protocol: five 64-bit words per device (FindKArgs::ctl: stop =
// MaxUint64, cursor = filled = maxk = tasks_run = 0, set on the stream before
// a call's first launch) and a buffer of `cap` >= k 16-byte records.
//   record   as hm_collect: on a step with hits one lane reserves popcount
//            slots with one agent-scope fetch_add on `cursor`, each hit lane
//            writes (hash, nonce) with vector stores if its slot is < cap
//   publish  right after a task (the generic kernel: a step) that put c > 0
//            records into slots < k, the largest of their nonces being mx, one
//            lane does, in this order, atomic max(maxk, mx) and
//            old = fetch_add(filled, c) (acquire-release, agent scope).  The
//            slots < k are reserved exactly once each, so exactly one wave sees
//            old + c == k: every slot < k is then written and folded into
//            maxk.  That wave loads maxk and does atomic min(stop, maxk): from
//            then on k hits with nonce <= stop exist.
//   skip     before each task a wave reads `stop` (relaxed, agent scope); a
//            task whose smallest nonce is above it is not run
//   leave    task ids are monotone in their smallest nonce (find_kernels.hip),
//            so on the first skip the wave leaves its loop
//   exit     a launch whose smallest nonce is above `stop` does nothing
//   count    each wave adds the tasks it ran to tasks_run once
// No wave waits on another beyond the dispenser's existing LDS hand-off, and
// nothing here spins.
//
// hm_cancel (ABI 1.18; cancel_relay.hpp).  Wave 0 of workgroup 0
// is the launch's RELAY: at kernel entry and between its tasks (right after each
// task it ran, so before the next one it takes; the generic kernel: before each
// step) it reads the context's cancel flag (FindKArgs::cancel, pinned host memory;
// one relaxed system-scope load) and, if it is set, lowers the stop word to 0,
// from where
// skip / leave / exit above end this launch and those queued behind it.  A
// word lowered so is FORGED -- 0 is not a hit, nor "k records at or below 0" -- and the invariants
// below speak of a call that was not cancelled.  The cancel invariant:
//   The word is forged only if the flag is set.  The flag is set before the
//   device can see it, and only the call's own thread clears it (at call
//   start).  Therefore the host, which tests the flag after every wait or
//   readback and BEFORE it interprets any control word, never mistakes a
//   forged word for an answer.
//
// The answer is exact whatever the dispatch order, because
//   1. a record is written only for an in-range, below-target, non-surplus
//      lane (take_step(WaveFirstK&), as WaveCollect's),
//   2. `stop` is only ever set to a value V such that k written records have
//      nonce <= V, and it only decreases (atomic min),
//   3. a task or launch is skipped only if its smallest nonce is above `stop`,
//      so every hit <= the k-th lowest hit lies in a task that ran, and it is
//      in the buffer unless cursor > cap,
//   4. if `stop` is never lowered, nothing was skipped and the buffer holds
//      every hit of the range.
// The host reads min(cursor, cap) records, sorts them by nonce and keeps the k
// lowest; cursor > cap sends the call down its overflow path (find_k.cpp).  A
// published maxk of MaxUint64 leaves `stop` as it is, so the top nonce needs
// no special case: it is an ordinary record.
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
DEV uint64_t find_k_stop(const FindKArgs& F) {
    uint64_t w = 0;
    if (__lane_id() == 0)
        w = __hip_atomic_load(F.ctl + kFkStop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return uni64(w);
}
DEV void find_k_publish(const FindKArgs& F, uint32_t c, uint64_t mx) {
    if (__lane_id() == 0) {
        __hip_atomic_fetch_max(F.ctl + kFkMaxk, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t old = __hip_atomic_fetch_add(F.ctl + kFkFilled, (uint64_t)c,
                                                    __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (old + c == F.k) {
            const uint64_t v =
                __hip_atomic_load(F.ctl + kFkMaxk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(F.ctl + kFkStop, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
DEV void find_k_count(const FindKArgs& F, uint32_t ran) {
    if (ran && __lane_id() == 0)
        __hip_atomic_fetch_add(F.ctl + kFkTasksRun, (uint64_t)ran, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}
DEV WaveFirstK find_k_begin(const FindKArgs& F) {
    WaveFirstK f;
    f.target = F.target;
    f.thi = (uint32_t)((F.target - 1) >> 32);
    f.cursor = F.ctl + kFkCursor;
    f.out = F.out;
    f.cap = F.cap;
    f.k = F.k;
    return f;
}

template <int W1, bool STRADDLE, bool TRAILER>
__global__ void HM_TILED_BOUNDS hm_find_k_tiled_kernel(const FindKTiledArgs KA) {
    const TiledArgs& A = KA.t;
    const FindKArgs& F = KA.f;
    WaveFirstK fk = find_k_begin(F);
    WaveSums sums;  // unused (CSUM = false)
    __shared__ LdsQueue queue;
    lds_queue_init(&queue);
    uint32_t ran = 0;
    const bool relay = cancel_is_relay(F.cancel);
    cancel_relay(relay, F.cancel, F.ctl + kFkStop);
    if (find_k_stop(F) < F.launch_lo) return;

    for (;;) {
        const uint32_t task = lds_dequeue(&queue, A.counter, A.lds_shift);
        if (task >= A.ntasks) break;
        const TiledTask T = tiled_decode(A, task);
        const uint64_t tile_base = (A.tile0 + T.tile) * A.pow10V;
        // lane 0's first loop step: the task's smallest nonce
        const uint64_t task_lo =
            tile_base + (uint64_t)T.chunk * (kWaveSize * 100u) + T.t1_begin * 10u;
        if (task_lo > find_k_stop(F)) break;
        fk.c = 0;
        fk.mx = 0;
        tiled_task<W1, STRADDLE, TRAILER, false>(
            A.rec + (size_t)T.tile * kRecWords, T.chunk, T.t1_begin, T.t1_end, tile_base, A.seg_lo,
            A.seg_hi, A.vmax, A.q, A.lane_shift, A.loop_shift, A.s0_loop, A.trailer_kw, fk, sums);
        ++ran;
        if (fk.c) find_k_publish(F, fk.c, fk.mx);
        cancel_relay(relay, F.cancel, F.ctl + kFkStop);
    }
    find_k_count(F, ran);
}

__global__ void __launch_bounds__(kBlock) hm_find_k_chained_kernel(const FindKChainedArgs KA) {
    const ChainedArgs& A = KA.c;
    const FindKArgs& F = KA.f;
    WaveFirstK fk = find_k_begin(F);
    WaveSums sums;  // unused (CSUM = false)
    const uint32_t per_tile = A.tpt * A.ntc;
    __shared__ LdsQueue queue;
    lds_queue_init(&queue);
    uint32_t ran = 0;
    const bool relay = cancel_is_relay(F.cancel);
    cancel_relay(relay, F.cancel, F.ctl + kFkStop);
    if (find_k_stop(F) < F.launch_lo) return;

    for (;;) {
        const uint32_t task = lds_dequeue(&queue, A.counter, A.lds_shift);
        if (task >= A.ntasks) break;
        const ChainedTask T = chained_decode(A, per_tile, task);
        const uint64_t tile_base = (A.tile0 + T.tile) * A.pow10qf + A.ebase;
        // lane 0's first loop value: the task's smallest nonce (its lanes
        // stride pow10f, so the task reaches 63 * pow10f beyond it)
        const uint64_t task_lo = tile_base + (uint64_t)T.chunk * kWaveSize * A.pow10f + T.t_begin;
        if (task_lo > find_k_stop(F)) break;
        fk.c = 0;
        fk.mx = 0;
        chained_task<false>(A.rec + (size_t)T.tile * kRecWords, T.chunk, T.t_begin, T.t_end,
                            tile_base, A.pow10f, A.seg_lo, A.seg_hi, A.vmax, A.q, A.kwt, fk, sums);
        ++ran;
        if (fk.c) find_k_publish(F, fk.c, fk.mx);
        cancel_relay(relay, F.cancel, F.ctl + kFkStop);
    }
    find_k_count(F, ran);
}

// One nonce per lane, any layout.  Wave w of the grid takes the 64 nonces
// seg_lo + 64 w + i * stride .. + 63 in step i: ascending per wave, so the
// first step above the stop word ends the wave.  A step is a task: it
// publishes its own records.
__global__ void __launch_bounds__(kBlock) hm_find_k_generic_kernel(const FindKGenericArgs KA) {
    const GenericArgs& A = KA.g;
    const FindKArgs& F = KA.f;
    WaveFirstK fk = find_k_begin(F);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = __lane_id();
    uint32_t ran = 0;
    const bool relay = cancel_is_relay(F.cancel);
    cancel_relay(relay, F.cancel, F.ctl + kFkStop);
    if (find_k_stop(F) < F.launch_lo) return;
    for (uint64_t kb = (uint64_t)blockIdx.x * blockDim.x + uni(threadIdx.x / kWaveSize) * kWaveSize;
         kb <= A.count_m1;) {
        cancel_relay(relay, F.cancel, F.ctl + kFkStop);
        if (A.seg_lo + kb > find_k_stop(F)) break;
        // lanes past the segment's end repeat the step's first nonce: surplus
        const bool live = A.count_m1 - kb >= lane;
        const uint64_t n = A.seg_lo + kb + (live ? lane : 0u);
        // hash_nonce's text (sha_device.hpp), this kernel's own copy as in
        // find_kernels.hip and collect_kernels.hip
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
        fk.c = 0;
        fk.mx = 0;
        // the launch's nonces are [seg_lo, seg_lo + count_m1]: no wrap
        take_step(fk, wave_cand(fk, st[0]), st[0], st[1], n, 0, A.seg_lo, A.seg_lo + A.count_m1,
                  live);
        if (fk.c) find_k_publish(F, fk.c, fk.mx);
        if (A.count_m1 - kb < stride) break;
        kb += stride;
    }
    find_k_count(F, ran);
}

// Every tiled layout the planner can pick.
#define HM_FIND_K_INST(W, S, T) \
    template __global__ void hm_find_k_tiled_kernel<W, S, T>(const FindKTiledArgs);
HM_FOR_EACH_TILED_LAYOUT(HM_FIND_K_INST)
#undef HM_FIND_K_INST

}  // namespace hm
