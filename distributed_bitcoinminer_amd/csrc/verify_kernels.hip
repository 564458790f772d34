// verify_kernels.hip -- the gfx950 kernel of hm_hash_many and hm_verify (ABI
// 1.12): Hash(msg, nonce) for a LIST of arbitrary nonces.
//
// The receiving side of share collection: a pool hands out work at a share
// target, miners return lists of (hash, nonce) records (what hm_collect
// produces), and the reference server believes them
// (cmu440/bitcoin/server/server.go:273 only compares the hash).  Rechecking
// means bitcoin.Hash (hash.go:13-17) at every listed nonce:
//   for i < n: hashes[i] = Hash(msg, nonces[i])                   (<false>)
//   for i < n: bad iff recs[i].hash != Hash(msg, recs[i].nonce)
//                   or recs[i].hash >= target                      (<true>)
//
//   hm_hash_list_kernel<VERIFY>  grid-stride, one list element per lane,
//                                waves of 64 consecutive elements
//
// Every other kernel of the library walks consecutive nonces of one digit
// count; here the digit count d, and with it the tail layout (where the
// digits, the 0x80 and the bit length land, and whether the tail has one
// block or two), differs from lane to lane.  Per lane: load the element,
// count its digits, build_tail (sha_device.hpp) with the lane's d,
// nb = (r + d + 9 <= 64) ? 1 : 2 and total_bits = (len + 1 + d) * 8, compress
// from the midstate -- the second block only in lanes with nb == 2 -- and form
// the key (st[0] << 32) | st[1].
//   uniform    shares of one range mostly have one digit count: when a ballot
//              shows that every live lane of the wave step has the d of lane
//              0, d is taken through uni(), build_tail's conditions on kE, e
//              and `two` are scalar and so is the branch around block 1, as
//              in hm_collect_generic_kernel
//   divergent  otherwise the same code runs with d in a VGPR: the conditions
//              become per-lane selects (every array index stays a compile-
//              time constant: no scratch), block 1 runs under the exec mask of
//              the nb == 2 lanes
// Both paths compute the same function of (nonce, d); which one a wave step
// takes changes no answer.
//
// Device protocol of <true>: WaveCollect's (scan_tasks.hpp,
// collect_kernels.hip), applied to indices.  Two 64-bit words per device
// (VerifyArgs::total, ::cursor), zeroed on the stream before a call's first
// launch, and a buffer of `cap` 64-bit indices (cap = 0: a pure count).
//   count    a wave counts its bad records in a register (popcount of the
//            ballot of `bad`) and adds them to `total` once at its exit: one
//            agent-scope atomic from one lane
//   reserve  (cap > 0) on a step with bad lanes one lane reserves popcount
//            slots with one agent-scope fetch_add on `cursor`; bad lane i
//            takes slot base + (bad lanes below i) and writes its GLOBAL
//            index (index0 + its position in the launch) there with an
//            ordinary vector store if the slot is < cap
//   full     a wave that sees a base >= cap stops reserving (wave-uniform
//            flag) and keeps counting: the call has overflowed and the host
//            will not read the buffer
// No wave waits on another and nothing here spins.
//
// The count is exact and the indices complete whatever the dispatch order,
// because
//   1. an element is hashed, stored, counted and recorded only by the one
//      lane whose position kb + lane is below n: lanes past the end of the
//      list load nothing, store nothing and are never `bad` (a clamped lane
//      repeating element 0 would count a bad record twice),
//   2. the grid-stride steps of all waves partition [0, n), and the host's
//      chunks and device shares partition the list, so each element is tested
//      exactly once,
//   3. every wave adds its count and writes its indices before its kernel
//      ends, and the host reads only after the stream is idle.
// Which slot an index lands in depends on dispatch order; the host sorts the
// indices, so the answer does not.
//
// Compiled like scan_kernels.hip (device-only -S, align_loops.py, linked into
// hipminer_scan.hsaco) and looked up by mangled name (verify.cpp).
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

// Hash(msg, n) of a nonce of d digits from the midstate.  Inlined once with d
// wave-uniform (an SGPR after uni()) and once with d per lane.
DEV uint64_t hash_tail(const VerifyArgs& A, uint64_t n, uint32_t d) {
    const uint32_t nb = A.r + d + 9u <= 64u ? 1u : 2u;
    uint32_t h0, h1;
    hash_nonce(A.pw, A.r, d, nb, A.bits0 + 8u * d, A.mid, n, h0, h1);
    return ((uint64_t)h0 << 32) | h1;
}

template <bool VERIFY>
__global__ void __launch_bounds__(kBlock) hm_hash_list_kernel(const VerifyArgs A) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t lane = __lane_id();
    uint64_t count = 0;  // the wave's bad records (uniform)
    bool full = false;   // a reservation of this wave began at or past cap (uniform)
    // A.n <= 2^22 and stride < 2^22: kb + stride does not wrap
    for (uint32_t kb = blockIdx.x * blockDim.x + uni(threadIdx.x / kWaveSize) * kWaveSize;
         kb < A.n; kb += stride) {
        // lanes past the end of the list take no element (lane 0 is live)
        const bool live = A.n - kb > lane;
        const uint32_t i = kb + lane;
        uint64_t n = 0, claimed = 0;
        if (live) {
            if constexpr (VERIFY) {
                claimed = A.in[2 * (size_t)i];
                n = A.in[2 * (size_t)i + 1];
            } else {
                n = A.in[i];
            }
        }
        const uint32_t d0 = uni(dec_digits(n));
        const uint32_t d = live ? dec_digits(n) : d0;
        uint64_t key;
        if (__builtin_amdgcn_ballot_w64(d != d0) == 0) key = hash_tail(A, n, d0);
        else key = hash_tail(A, n, d);
        if constexpr (!VERIFY) {
            if (live) A.hashes[i] = key;
        } else {
            const bool bad = live && (key != claimed || claimed >= A.target);
            const uint64_t bads = __builtin_amdgcn_ballot_w64(bad);
            if (bads) {
                const uint32_t nbad = (uint32_t)__builtin_popcountll(bads);
                count += nbad;
                if (A.cap != 0 && !full) {
                    // bad lanes below this one: a bad lane's rank in the step
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi(
                        (uint32_t)(bads >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bads, 0u));
                    // the lowest bad lane reserves the step's slots
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
                        if (slot < A.cap) A.idx[slot] = A.index0 + i;
                    }
                }
            }
        }
    }
    if constexpr (VERIFY) wave_total(A.total, count);
}

template __global__ void hm_hash_list_kernel<false>(const VerifyArgs);
template __global__ void hm_hash_list_kernel<true>(const VerifyArgs);

}  // namespace hm
