// fused_collect_kernels.hip -- the fused collect kernel of hm_collect_many
// (gfx950): EVERY nonce of one request's range whose hash is below a target,
// and their exact count, every digit segment of the range in ONE persistent
// launch.
//
// The share-collection form of the miner's loop (cmu440/bitcoin/miner/miner.go:
// 46-59 over bitcoin.Hash, hash.go:13-17):
//   for n = lo .. hi: if Hash(msg, n) < target: emit (Hash, n).
// hm_collect (collect_kernels.hip) answers it with one launch per segment
// piece on stream 0; a small range is bound by those launches.  This kernel is
// hm_fused_kernel's task loop (fused_kernels.hip: task ids from one counter, a
// task id names its segment, the segment's layout is chosen by a wave-uniform
// switch) with hm_collect's reduction and a request tag:
//   task bodies  tiled_task / chained_task (scan_tasks.hpp) and the generic
//                640-nonce body, folding into WaveCollectTag ("all below
//                target"); the per-nonce test is wave_cand: h0 <= (target-1)>>32
//   dispensing   the shipped scheme only: a wave's first task is its slot,
//                then a plain dequeue from the counter, which the planner
//                (hm_fused_plan_kernel) starts past every slot; guided-tail
//                ids >= nbig are pieces of their task
// There is no stop word and no skip: every id of every launch runs.
//
// Device protocol: one 64-bit total word per REQUEST (CollectArgs::total),
// zeroed by the planner launch that precedes this one on the stream; one
// 64-bit cursor per DEVICE (CollectArgs::cursor), zeroed once per chunk of
// requests before any of the chunk's launches; a buffer of `cap` 16-byte
// records and one of `cap` 32-bit tags, shared by the chunk's requests on the
// device (cap = 0: pure counts, no buffers).
//   count    a wave counts its hits in a register (popcount of the ballot of
//            `ok`) and adds them to the request's total once at exit: one
//            agent-scope atomic from one lane (wave_total)
//   reserve  (cap > 0) on a step with hits the lowest hit lane reserves
//            popcount slots with one agent-scope fetch_add on the cursor; hit
//            lane i takes slot base + (hits in lanes below i) and writes
//            (hash, nonce) there and the request's index to tags[slot], with
//            ordinary vector stores, if the slot is < cap
//   full     a wave that sees a base >= cap stops reserving (wave-uniform
//            flag): the call has overflowed and the host will not read the
//            buffers.  It keeps counting.
// Nothing spins and no wave waits on another.
//
// Each request's total is exact and its records complete whatever the
// dispatch order, because
//   1. a nonce is counted and recorded only if it lies in [seg_lo, seg_hi],
//      its key is < target, and its lane is not a surplus lane (the task
//      bodies clamp lanes past vmax to vmax, the generic body's lanes past
//      the segment end hash the step's first nonce again: such lanes hash a
//      nonce another lane already holds, a double count here, so
//      take_step(WaveCollectTag) takes lane_ok; in the generic body `in` is
//      both part of cand and the lane_ok),
//   2. every task of the launch runs and nothing is skipped; the segments,
//      tasks and guided pieces partition the request's [lo, hi], so each nonce
//      is tested exactly once,
//   3. every wave adds its count and writes its records and tags before its
//      kernel ends, and the host reads only after the stream is idle.
// The host recomputes nothing: a record carries the hash the kernel formed.
// Which slot a record lands in depends on dispatch order; the host groups the
// records by tag and sorts each group by nonce, so the answer does not.
//
// The task decoders and the task loop below are this file's own, templates
// over the reduction.  fused_find_kernels.hip and fused_find_k_kernels.hip take
// theirs from fused_tasks.hpp; this kernel does not, because on that header it
// measured 8-9 % slower on a single 120-B request of 10^7 nonces (and 4-8 %
// faster on batches of 8 and 64: profiles/README.md, batch_dedup/), so its
// text is held byte for byte.  A change to the walk (the slot-then-counter
// order, the guided-tail split, the segment lookup) has to be made here too.
//
// Compiled like scan_kernels.hip (device-only -S, align_loops.py, linked last
// into hipminer_scan.hsaco) and looked up by mangled name (kernel_name() in
// seg_walk.cpp).
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "scan_tasks.hpp"
#include "sha256_defs.hpp"
#include "sha_device.hpp"

namespace hm {

// The launch's argument block read in place from the kernarg segment (see
// fused_kernels.hip: a runtime segment index would copy a by-value parameter
// to scratch).
typedef const __attribute__((address_space(4))) FusedCollectArgs FusedCollectArgsK;
typedef const __attribute__((address_space(4))) FusedArgs FusedArgsK;

// "All below target" with a request tag: WaveCollect's reduction
// (scan_tasks.hpp) where the device's cursor and buffer are shared by several
// requests, so each record's slot also names its request.
struct WaveCollectTag {
    uint32_t thi;      // (target - 1) >> 32, target >= 1
    uint32_t cap;      // records the buffers hold; 0: count only
    uint64_t target;
    uint64_t* cursor;  // next free slot (agent scope)
    uint64_t* out;     // 2 x u64 per slot: (hash, nonce)
    uint32_t* tags;    // one per slot: the request
    uint32_t request;
    uint64_t count = 0;  // the wave's hits (uniform)
    bool full = false;   // a reservation of this wave began at or past cap (uniform)
};
DEV bool wave_cand(const WaveCollectTag& c, uint32_t h0) { return h0 <= c.thi; }
DEV void take_step(WaveCollectTag& c, bool cand, uint32_t h0, uint32_t h1, uint64_t nbase,
                   uint32_t off, uint64_t seg_lo, uint64_t seg_hi, bool lane_ok) {
    if (__builtin_amdgcn_ballot_w64(cand)) {
        const uint64_t key = ((uint64_t)h0 << 32) | h1;
        const uint64_t nn = nbase + off;
        const bool ok = cand && lane_ok && key < c.target && nn >= seg_lo && nn <= seg_hi;
        const uint64_t hits = __builtin_amdgcn_ballot_w64(ok);
        if (hits) {
            const uint32_t n = (uint32_t)__builtin_popcountll(hits);
            c.count += n;
            if (c.cap != 0 && !c.full) {
                // hit lanes below this one: a hit lane's rank in the step
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi(
                    (uint32_t)(hits >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hits, 0u));
                // the lowest hit lane reserves the step's slots
                uint64_t base = 0;
                if (ok && rank == 0)
                    base = __hip_atomic_fetch_add(c.cursor, (uint64_t)n, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT);
                // every lane takes the reserving lane's value
                const uint32_t src = (uint32_t)__builtin_ctzll(hits);
                base = ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(base >> 32), src) << 32) |
                       __builtin_amdgcn_readlane((uint32_t)base, src);
                if (base >= c.cap) {
                    c.full = true;
                } else if (ok) {
                    const uint64_t slot = base + rank;
                    if (slot < c.cap) {
                        c.out[2 * slot] = key;
                        c.out[2 * slot + 1] = nn;
                        c.tags[slot] = c.request;
                    }
                }
            }
        }
    }
}

// Piece `pp` of `np` of the run [b, e): [*b2, *e2) (empty when past e).
DEV void fc_piece_of(uint32_t b, uint32_t e, uint32_t pp, uint32_t np, uint32_t* b2,
                     uint32_t* e2) {
    const uint32_t len = (e - b + np - 1) / np;
    uint32_t x = b + pp * len, y = x + len;
    if (x > e) x = e;
    if (y > e) y = e;
    *b2 = x;
    *e2 = y;
}

// Tiled task k of segment S: unit, tens digit t1 and part of the units loop;
// piece pp of np of that part.
template <int W1, bool STRADDLE, bool TRAILER, typename Red>
DEV void fc_tiled(FusedArgsK* A, const FusedSeg& S, uint32_t k, uint32_t pp, uint32_t np,
                  Red& red) {
    const uint32_t per_unit = 10u * S.tpu;
    const uint32_t unit = S.unit0 + k / per_unit;
    const uint32_t rem = k - (k / per_unit) * per_unit;
    const uint32_t t1 = rem / S.tpu;
    const uint32_t part = rem - t1 * S.tpu;
    const uint32_t steps = 10u / S.tpu;
    uint32_t t0b, t0e;
    fc_piece_of(part * steps, part * steps + steps, pp, np, &t0b, &t0e);
    if (t0b >= t0e) return;  // an empty piece (uniform)
    const uint32_t tile = unit / S.tpt;
    const uint32_t chunk = unit - tile * S.tpt;
    const uint64_t tile_base = (S.tile0 + tile) * S.pow10V;
    WaveSums sums;  // unused (CSUM = false)
    const_u32* tab = (const_u32*)(A->aux + S.aux0);
    tiled_task<W1, STRADDLE, TRAILER, false>(A->rec + (size_t)(S.rec0 + tile) * kRecWords, chunk, t1,
                                             t1 + 1, tile_base, S.seg_lo, S.seg_hi, S.vmax, S.q,
                                             S.lane_shift, S.loop_shift, tab, tab + 100, red, sums,
                                             t0b, t0e);
}

// Chained task k of segment S: lane chunk, loop chunk and part of it; piece pp
// of np of that part.
template <typename Red>
DEV void fc_chained(FusedArgsK* A, const FusedSeg& S, uint32_t k, uint32_t pp, uint32_t np,
                    Red& red) {
    const uint32_t unit = S.unit0 + k / S.tpu;
    const uint32_t part = k - (k / S.tpu) * S.tpu;
    const uint32_t per_tile = S.tpt * S.ntc;
    const uint32_t tile = unit / per_tile;
    const uint32_t rem = unit - tile * per_tile;
    const uint32_t chunk = rem / S.ntc;
    const uint32_t tc = rem - chunk * S.ntc;
    const uint32_t piece = (S.tch + S.tpu - 1) / S.tpu;
    const uint32_t t_begin = tc * S.tch + part * piece;
    uint32_t t_end = tc * S.tch + S.tch;
    if (t_end > t_begin + piece) t_end = t_begin + piece;
    uint32_t tb, te;
    fc_piece_of(t_begin, t_end, pp, np, &tb, &te);
    if (tb >= te) return;  // an empty piece (uniform)
    const uint64_t tile_base = (S.tile0 + tile) * S.pow10V;
    WaveSums sums;  // unused (CSUM = false)
    chained_task<false>(A->rec + (size_t)(S.rec0 + tile) * kRecWords, chunk, tb, te, tile_base,
                        S.pow10f, S.seg_lo, S.seg_hi, S.vmax, S.q, A->aux + S.aux0, red, sums);
}

// Generic task k: nonces seg_lo + 640k + lane + 64j, j < 10 (a guided-tail
// piece: its share of the j), every tail block compressed per lane.  A lane
// past the segment's end hashes the step's first nonce again: surplus.
template <typename Red>
DEV void fc_generic(FusedArgsK* A, const FusedSeg& S, uint32_t k, uint32_t pp, uint32_t np,
                    Red& red) {
    const uint32_t lane = __lane_id();
    const uint64_t base = S.seg_lo + (uint64_t)k * 640u;
    uint32_t jb, je;
    fc_piece_of(0, 10, pp, np, &jb, &je);
    if (jb >= je) return;  // an empty piece (uniform)
    uint32_t pw[16], mid[8];
#pragma unroll
    for (int i = 0; i < 16; ++i) pw[i] = A->pw[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) mid[i] = A->mid[i];
    for (uint32_t j = jb; j < je; ++j) {
        const uint64_t nb0 = base + 64u * j;  // wave-uniform
        if (nb0 > S.seg_hi || nb0 < S.seg_lo) break;  // past the end (or wrapped)
        const uint64_t n = nb0 + lane;
        const bool in = n >= nb0 && n <= S.seg_hi;  // no wrap past 2^64-1
        uint32_t h0, h1;
        hash_nonce(pw, A->r, S.d, S.nb, S.total_bits, mid, in ? n : nb0, h0, h1);
        take_step(red, in && wave_cand(red, h0), h0, h1, nb0, lane, S.seg_lo, S.seg_hi, in);
    }
}

#define HM_FC_CASE(W, S, T) \
    case (W) * 4 + (S) * 2 + (T): fc_tiled<W, S, T>(A, S_, k, pp, np, col); break;

// The argument block is the kernel's only (explicit) parameter, so it starts
// the kernarg segment.
__global__ void __launch_bounds__(kBlock) hm_fused_collect_kernel(const FusedCollectArgs) {
    FusedCollectArgsK* P = (FusedCollectArgsK*)__builtin_amdgcn_kernarg_segment_ptr();
    FusedArgsK* A = &P->a;
    const uint32_t wslot = blockIdx.x * (kBlock / kWaveSize) + uni(threadIdx.x / kWaveSize);
    WaveCollectTag col;
    col.target = P->k.target;
    col.thi = (uint32_t)((P->k.target - 1) >> 32);
    col.cap = P->k.cap;
    col.cursor = P->k.cursor;
    col.out = P->k.out;
    col.tags = P->tags;
    col.request = P->request;
    // the first task is the wave's slot: the planner started the counter past
    // every slot
    uint32_t next = wslot;
    const uint32_t nbig = A->nbig, nparts = A->nparts;
    for (;;) {
        const uint32_t id = uni(next);
        if (id >= A->ntasks) break;
        // guided tail: ids from nbig on are pieces pp of np of their task
        uint32_t task = id, pp = 0, np = 1;
        if (id >= nbig) {
            const uint32_t q = (id - nbig) / nparts;
            pp = id - nbig - q * nparts;
            np = nparts;
            task = nbig + q;
        }
        uint32_t i = 0;
        while (i + 1 < A->nseg && task >= A->segs[i].task_end) ++i;
        const FusedSeg S_ = A->segs[i];  // scalar loads of one descriptor
        const uint32_t k = task - (i ? A->segs[i - 1].task_end : 0u);
        switch (S_.variant) {
            HM_FOR_EACH_TILED_LAYOUT(HM_FC_CASE)
            case kVarChained: fc_chained(A, S_, k, pp, np, col); break;
            default: fc_generic(A, S_, k, pp, np, col); break;
        }
        next = 0;
        if (__lane_id() == 0) next = atomicAdd(A->counter, 1u);
    }
    wave_total(P->k.total, col.count);
}

#undef HM_FC_CASE

}  // namespace hm
