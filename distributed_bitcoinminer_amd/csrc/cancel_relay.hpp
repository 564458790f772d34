// cancel_relay.hpp -- the relay wave of hm_cancel (ABI 1.18),
// shared by the four find-family kernel files (find_kernels.hip,
// find_k_kernels.hip, fused_find_kernels.hip, fused_find_k_kernels.hip).
//
// A persistent find launch owns the GPU -- its grid is occupancy-sized, so no
// second kernel could run beside it -- and the host can reach it only through
// memory.  The context's cancel flag is one word of pinned, coherent host
// memory (FindArgs::cancel / FindKArgs::cancel: the device's pointer to it).
// Wave 0 of workgroup 0 of every launch is the RELAY: at kernel entry and
// before each task it takes, it reads the flag with one relaxed system-scope
// load, and if the flag is set one lane lowers the launch's stop word to 0
// (agent-scope atomic min).  The per-segment tiled and chained kernels poll
// right after a task instead of right before the next dequeue -- the same
// points in time, one poll per task -- because there the poll costs no
// register: at the loop's top it took the tiled kernels 2 VGPRs, and seven
// hm_find_tiled_kernel instantiations from 6 waves per SIMD to 5.  From there
// the kernels' own skip / leave / exit rules end this launch and every launch
// queued behind it, whose own relay repeats the lowering (the fused launches'
// planner re-seeds the word).
//
// Every other wave pays one wave-uniform test of "am I the relay" and never
// touches host memory: one reader per launch keeps the traffic over the link
// at one 4-byte read per task of one wave.  No wave waits on anything and
// nothing spins; a null pointer means no relay.
//
// A lowered word is FORGED: 0 is not a hit, and for hm_find_k not "k records at
// or below 0".  The invariant that keeps it from ever being read as an answer:
//   The word is forged only if the flag is set.  The flag is set before the
//   device can see it, and only the call's own thread clears it (at call
//   start).  Therefore the host, which tests the flag after every wait or
//   readback and BEFORE it interprets any control word, never mistakes a
//   forged word for an answer.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "sha_device.hpp"

namespace hm {

// Wave-uniform: is this wave its launch's relay?  (cancel null: nobody is.)
DEV bool cancel_is_relay(const uint32_t* cancel) {
    return cancel != nullptr && blockIdx.x == 0 && uni(threadIdx.x / kWaveSize) == 0;
}

// The relay's poll: flag set -> the stop word drops to 0.  One lane.
DEV void cancel_relay(bool relay, const uint32_t* cancel, uint64_t* stop) {
    if (relay && __lane_id() == 0 &&
        __hip_atomic_load(cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0)
        __hip_atomic_fetch_min(stop, (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace hm
