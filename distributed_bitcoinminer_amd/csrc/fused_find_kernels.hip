// fused_find_kernels.hip -- the fused find kernel of hm_find_many (gfx950):
// the LOWEST nonce of one request's window whose hash is below a target, every
// digit segment of the window in ONE persistent launch that exits early.
//
// The proof-of-work form of the miner's loop (cmu440/bitcoin/miner/miner.go:
// 46-59 over bitcoin.Hash, hash.go:13-17):
//   for n = lo .. hi: if Hash(msg, n) < target: return n.
// hm_find (find_kernels.hip) answers it with one launch per segment piece and
// a host round trip every four launches; at ordinary targets the hit is a few
// million nonces in, and the call is bound by those launches.  This kernel is
// hm_fused_kernel's task loop (fused_kernels.hip: task ids from one counter, a
// task id names its segment, the segment's layout is chosen by a wave-uniform
// switch) with hm_find's reduction and protocol:
//   task bodies  tiled_task / chained_task (scan_tasks.hpp) and the generic
//                640-nonce body (fused_tasks.hpp), folding into WaveFirst ("first below
//                target"); the per-nonce test is wave_cand(first, h0)
//   dispensing   the shipped scheme only: a wave's first task is its slot,
//                then a plain dequeue from the counter, which the planner
//                (hm_fused_plan_kernel) starts past every slot
//
// Device protocol: one 64-bit stop word and one tasks-run word per REQUEST
// (FindArgs::word, ::tasks_run), seeded (MaxUint64, 0) by the planner launch
// that precedes this one on the stream.
//   publish  a wave whose task lowered its best nonce writes it with one
//            agent-scope atomic min (one lane), right after the task
//   skip     before each task a wave reads the word (relaxed, agent scope);
//            a task whose smallest nonce is above it is not run
//   leave    the host orders the segments ascending by nonce, within a
//            segment ids ascend in their smallest nonce (unit, tens digit,
//            part; lane chunk, loop chunk, part; 640-nonce block), and the
//            guided-tail pieces are the highest ids, of the last tasks -- so
//            ids are monotone in their smallest nonce, and each wave draws
//            ascending ids (its slot, then the counter): on its first skip a
//            wave leaves its loop
//   count    each wave adds the tasks it ran to FindArgs::tasks_run once
// Nothing spins and no wave waits on another.
//
// hm_cancel (ABI 1.18; cancel_relay.hpp).  Wave 0 of workgroup 0
// is the launch's RELAY: at kernel entry and before each task it takes it reads
// the context's cancel flag (FindArgs::cancel, pinned host memory; one relaxed
// system-scope load) and, if it is set, lowers the stop word to 0, from where
// skip / leave / exit above end this launch and those queued behind it.  A
// word lowered so is FORGED -- 0 is not a hit -- and the invariants
// below speak of a call that was not cancelled.  The cancel invariant:
//   The word is forged only if the flag is set.  The flag is set before the
//   device can see it, and only the call's own thread clears it (at call
//   start).  Therefore the host, which tests the flag after every wait or
//   readback and BEFORE it interprets any control word, never mistakes a
//   forged word for an answer.
//
// A task's smallest nonce (task_lo) is lane 0's first loop value:
//   tiled    tile_base + chunk * 6400 + t1 * 10 + t0b
//   chained  tile_base + chunk * 64 * 10^f + tb
//   generic  seg_lo + 640 k + 64 jb
// It may be lower than the task's smallest IN-RANGE nonce (a segment that
// starts inside a lane chunk; a sum that wraps past 2^64 only looks lower),
// never higher.  It is clamped to the segment's seg_hi: an edge chunk's last
// tens digits may start past seg_hi, and a wave that skipped such a task
// against a hit in a LATER segment would leave tasks below that hit behind.
// Clamped, a skip means word < seg_hi of the task's own segment, so the word
// lies in this segment or an earlier one and every later id is above it.
//
// The final word is the lowest hit whatever the dispatch order, because
//   1. only nonces n in [seg_lo, seg_hi] with Hash(msg, n) < target are
//      published (take_step(WaveFirst&)), and never n = 2^64-1, which the
//      word cannot tell from "none": the host tests that nonce itself,
//   2. a task is skipped only if every in-range nonce of it is above a value
//      already published, and the word only decreases (atomic min), so a
//      skipped task cannot hold the lowest hit; a wave that leaves drops no
//      task (the ids it does not draw stay in the counter for the others),
//      and the ids nobody draws lie above an id some wave skipped,
//   3. every task that ran publishes its hit before the kernel ends.
// Exactness rests on the skip rule alone; leaving is the pruning.
// The host recomputes the answer's hash (host_hash): only the nonce crosses.
//
// The task decoders and the task loop are fused_tasks.hpp's, written for every fused
// batch kernel; FindWave below is
// the policy they are instantiated with (enter = skip, done = publish and
// count).  The generic body hands take_step `in` as lane_ok, which
// take_step(WaveFirst&) ignores: a duplicate cannot change a minimum.
//
// Compiled like scan_kernels.hip (device-only -S, align_loops.py, linked into
// hipminer_scan.hsaco) and looked up by mangled name (kernel_name() in
// seg_walk.cpp).
#include <hip/hip_runtime.h>

#include "cancel_relay.hpp"
#include "fused_tasks.hpp"
#include "kernels.hpp"
#include "scan_tasks.hpp"
#include "sha256_defs.hpp"
#include "sha_device.hpp"

namespace hm {

// The launch's argument block read in place from the kernarg segment (see
// fused_kernels.hip: a runtime segment index would copy a by-value parameter
// to scratch).
typedef const __attribute__((address_space(4))) FusedFindArgs FusedFindArgsK;

// The request's stop word and its wave-side state: fused_walk's policy.
struct FindWave {
    uint64_t* word;
    bool relay;  // hm_cancel: this wave relays the flag (FindArgs::cancel, read from the kernarg)
    WaveFirst first;
    uint64_t before;  // the bound the current task started from
    uint32_t ran = 0;

    DEV WaveFirst& red() { return first; }
    // Before a task whose smallest nonce is task_lo (clamped to its segment's
    // end): false = skip it (and leave).  Otherwise the wave's bound drops to
    // the published hit.
    DEV bool enter(uint64_t task_lo, uint64_t seg_hi) {
        if (relay)
            cancel_relay(true, ((FusedFindArgsK*)__builtin_amdgcn_kernarg_segment_ptr())->f.cancel,
                         word);
        uint64_t stop = 0;
        if (__lane_id() == 0)
            stop = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        stop = uni64(stop);
        if ((task_lo < seg_hi ? task_lo : seg_hi) > stop) return false;
        if (stop < first.nonce) first.nonce = stop;
        before = first.nonce;
        return true;
    }
    // After a task that ran: count it, publish a lowered bound.
    DEV void done() {
        ++ran;
        if (first.nonce < before && __lane_id() == 0)
            __hip_atomic_fetch_min(word, first.nonce, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// The argument block is the kernel's only (explicit) parameter, so it starts
// the kernarg segment.
__global__ void __launch_bounds__(kBlock) hm_fused_find_kernel(const FusedFindArgs) {
    FusedFindArgsK* P = (FusedFindArgsK*)__builtin_amdgcn_kernarg_segment_ptr();
    FindWave w;
    w.word = P->f.word;
    w.relay = cancel_is_relay(P->f.cancel);
    w.first.target = P->f.target;
    w.first.thi = (uint32_t)((P->f.target - 1) >> 32);
    fused_walk(&P->a, w);
    if (w.ran && __lane_id() == 0)
        __hip_atomic_fetch_add(P->f.tasks_run, (uint64_t)w.ran, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace hm
