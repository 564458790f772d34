// verify_many_kernels.hip -- the gfx950 kernel of hm_verify_many (ABI 1.14):
// the (hash, nonce) record lists of MANY messages rechecked in one launch.
//
// hm_hash_list_kernel (verify_kernels.hip) takes its message -- midstate,
// prefix words, r, bit length -- and its target from the kernarg block, so a
// launch knows one message.  A pool that serves many clients holds many small
// lists, one message each (the reference server keeps one request per client
// and gets one Result per miner chunk: cmu440/bitcoin/server/server.go:211-219,
// 273, 318-324); here the message changes INSIDE a launch:
//   job    one request, or the piece of one that a launch holds: a VerifyJob
//          record (kernels.hpp) in a device table -- the message plan, the
//          target, where its records start in the launch's packed record
//          buffer (`first`), how many there are (`n`), the index inside its
//          request of the first one (`index0`) and the request's number
//   task   64 consecutive records of ONE job; job j has ceil(n_j / 64) tasks,
//          numbered from its task0; task_job[t] names the job of task t
//
//   hm_verify_jobs_kernel   persistent, grid-stride over tasks, one task per
//                           wave step, one record per lane
//
// A wave reads task_job[t] and then the job record through a wave-uniform
// pointer, every word passed through uni(): the message sits in SGPRs for the
// task, as the kernarg block does in the list kernel.  The body is that
// kernel's: count the lane's digits, hash through the wave-uniform path when a
// ballot shows one digit count in the task and through the divergent path
// otherwise (hash_nonce, sha_device.hpp; block 1 under the exec mask of the
// nb == 2 lanes), compare with the claimed hash and the job's target.
// dec_digits and hash_tail are copies of verify_kernels.hip's (as
// fused_find_kernels.hip keeps its decoders): that file's assembly stays as
// it was.
//
// Device protocol: WaveCollect's (scan_tasks.hpp), per job.  One 64-bit `bad`
// word per job of every launch of the call and one slot cursor per device,
// zeroed on the stream before the call's first launch, and a buffer of `cap`
// 16-byte (request, index) slots (cap = 0: pure counts).
//   count    on a task with bad lanes the lowest bad lane adds the popcount of
//            the ballot to its job's `bad` word: one agent-scope atomic
//   reserve  (cap > 0) that lane also reserves popcount slots with one
//            agent-scope fetch_add on the cursor; bad lane i takes slot
//            base + (bad lanes below i) and writes (request, index0 + its
//            position in the job) there with ordinary vector stores if the
//            slot is < cap
//   full     a wave that sees a base >= cap stops reserving (wave-uniform
//            flag) and keeps counting: the call has overflowed and the host
//            will not read the buffer
// No wave waits on another and nothing here spins.
//
// The counts are exact and the refs complete whatever the dispatch order,
// because
//   1. an element is tested only by the one lane whose position is inside its
//      job: a lane at or past n_j loads nothing, stores nothing and is never
//      bad -- in particular it never reads the next job's first record, which
//      lies right behind this job's last one in the packed buffer,
//   2. tasks partition jobs, jobs partition each launch, and the host's
//      launches and device shares partition the batch, so each record is
//      tested exactly once,
//   3. every wave adds and writes before its kernel ends, and the host reads
//      only when the stream is idle.
// Which slot a ref lands in depends on dispatch order; the host sorts the
// refs by (request, index), so the answer does not.
//
// Plain HIP C++, no inline assembly.  Compiled like scan_kernels.hip
// (device-only -S, align_loops.py, linked last into hipminer_scan.hsaco) and
// looked up by mangled name (verify_many.cpp).
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "scan_tasks.hpp"
#include "sha256_defs.hpp"
#include "sha_device.hpp"

namespace hm {

constexpr uint64_t pow10_const(int k) {
    uint64_t p = 1;
    for (int i = 0; i < k; ++i) p *= 10u;
    return p;
}
template <int... K>
DEV uint32_t digits_seq(uint64_t n, std::integer_sequence<int, K...>) {
    return (1u + ... + (n >= pow10_const(K + 1) ? 1u : 0u));
}
// Decimal digits of n: 1 for n < 10 (0 included), 20 for n >= 10^19.
DEV uint32_t dec_digits(uint64_t n) {
    return digits_seq(n, std::make_integer_sequence<int, 19>{});
}

// A job's message, wave-uniform (SGPRs after uni()).
struct JobMsg {
    uint64_t bits0;
    uint32_t r;
    uint32_t pw[16];
    uint32_t mid[8];
};

// Hash(msg, n) of a nonce of d digits from the midstate.  Inlined once with d
// wave-uniform (an SGPR after uni()) and once with d per lane.
DEV uint64_t hash_tail(const JobMsg& M, uint64_t n, uint32_t d) {
    const uint32_t nb = M.r + d + 9u <= 64u ? 1u : 2u;
    uint32_t h0, h1;
    hash_nonce(M.pw, M.r, d, nb, M.bits0 + 8u * d, M.mid, n, h0, h1);
    return ((uint64_t)h0 << 32) | h1;
}

__global__ void __launch_bounds__(kBlock) hm_verify_jobs_kernel(const VerifyJobsArgs A) {
    constexpr uint32_t kWaves = kBlock / kWaveSize;
    const uint32_t nwaves = gridDim.x * kWaves;
    const uint32_t lane = __lane_id();
    bool full = false;  // a reservation of this wave began at or past cap (uniform)
    // A.ntasks < 2^17 and nwaves <= 2^15: t + nwaves does not wrap
    for (uint32_t t = blockIdx.x * kWaves + uni(threadIdx.x / kWaveSize); t < A.ntasks;
         t += nwaves) {
        // the task's job, read wave-uniformly
        const uint32_t j = uni(A.task_job[t]);
        const VerifyJob* __restrict__ J = A.jobs + j;
        JobMsg M;
        M.bits0 = uni64(J->bits0);
        M.r = uni(J->r);
#pragma unroll
        for (int k = 0; k < 16; ++k) M.pw[k] = uni(J->pw[k]);
#pragma unroll
        for (int k = 0; k < 8; ++k) M.mid[k] = uni(J->mid[k]);
        const uint64_t target = uni64(J->target);
        const uint32_t nj = uni(J->n);
        // the task's first record inside its job: below nj (lane 0 is live)
        const uint32_t pos0 = (t - uni(J->task0)) * kWaveSize;
        // lanes past the end of the JOB take no element
        const bool live = nj - pos0 > lane;
        const uint32_t pos = pos0 + lane;
        uint64_t n = 0, claimed = 0;
        if (live) {
            const size_t e = (size_t)uni(J->first) + pos;
            claimed = A.recs[2 * e];
            n = A.recs[2 * e + 1];
        }
        const uint32_t d0 = uni(dec_digits(n));
        const uint32_t d = live ? dec_digits(n) : d0;
        uint64_t key;
        if (__builtin_amdgcn_ballot_w64(d != d0) == 0) key = hash_tail(M, n, d0);
        else key = hash_tail(M, n, d);
        const bool bad = live && (key != claimed || claimed >= target);
        const uint64_t bads = __builtin_amdgcn_ballot_w64(bad);
        if (bads) {
            const uint32_t nbad = (uint32_t)__builtin_popcountll(bads);
            // bad lanes below this one: a bad lane's rank in the task
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi(
                (uint32_t)(bads >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bads, 0u));
            // the lowest bad lane counts for the task ...
            if (bad && rank == 0)
                __hip_atomic_fetch_add(A.bad + j, (uint64_t)nbad, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            if (A.cap != 0 && !full) {
                // ... and reserves its slots
                uint64_t base = 0;
                if (bad && rank == 0)
                    base = __hip_atomic_fetch_add(A.cursor, (uint64_t)nbad, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT);
                // every lane takes the reserving lane's value
                const uint32_t src = (uint32_t)__builtin_ctzll(bads);
                base = ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(base >> 32), src) << 32) |
                       __builtin_amdgcn_readlane((uint32_t)base, src);
                if (base >= A.cap) {
                    full = true;
                } else if (bad) {
                    const uint64_t slot = base + rank;
                    if (slot < A.cap) {
                        A.refs[2 * slot] = uni64(J->request);
                        A.refs[2 * slot + 1] = uni64(J->index0) + pos;
                    }
                }
            }
        }
    }
}

}  // namespace hm
