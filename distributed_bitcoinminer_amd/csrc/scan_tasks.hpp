// scan_tasks.hpp -- one task of each scan kernel kind, shared by the
// per-segment kernels (scan_kernels.hip, find_kernels.hip,
// collect_kernels.hip, find_k_kernels.hip, scan_k_kernels.hip) and the fused small-request kernel
// (fused_kernels.hip): the reductions a task folds its nonces into, the task
// dispenser, the decoding of a task id, the list of tiled layouts and the
// task bodies.
//
// Replaces the miner's sequential loop (cmu440/bitcoin/miner/miner.go:46-59)
// over bitcoin.Hash (cmu440/bitcoin/hash.go:13-17) for one wave's share of
// it: 64 lanes x a run of loop values.  Each task folds its nonces into the
// wave's running (hash, nonce) minimum, which lives in SGPRs (wave-uniform)
// and is refreshed by a 64-lane reduce only when some lane may beat it
// (strict lexicographic order: ties to the lowest nonce, miner.go:56-58).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "sha256_defs.hpp"
#include "sha_device.hpp"

namespace hm {

// A wave's running minimum (uniform) and, for checked scans, its coverage
// sum and count (per lane until the final wave_sum).
struct WaveBest {
    uint32_t hi = 0xffffffffu, lo = 0xffffffffu;  // (MaxUint64, 0): miner.go:48-49
    uint64_t nonce = 0;
};
struct WaveSums {
    uint64_t sum = 0, cnt = 0;
};

// Fold one loop step's per-lane keys (h0, h1) of nonces nbase + off into
// the wave's best.  `cand` is h0 <= best.hi (the caller's one compare per
// nonce); only when some lane holds one does the 64-lane reduce run, and
// only then are the nonce and its range check formed.  Lanes outside
// [seg_lo, seg_hi] never win.  The last argument is lane_ok, false on a
// surplus lane (one that repeats another lane's nonce): a duplicate cannot
// change a minimum, so only WaveCollect below looks at it.
DEV void take_step(WaveBest& best, bool cand, uint32_t h0, uint32_t h1, uint64_t nbase,
                   uint32_t off, uint64_t seg_lo, uint64_t seg_hi, bool = true) {
    if (__builtin_amdgcn_ballot_w64(cand)) {
        uint64_t key = ((uint64_t)h0 << 32) | h1;
        uint64_t nn = nbase + off;
        const bool ok = cand && nn >= seg_lo && nn <= seg_hi;
        if (!ok) { key = ~0ull; nn = ~0ull; }
        wave_min(key, nn);
        key = uni64(key);
        nn = uni64(nn);
        const uint64_t bk = ((uint64_t)best.hi << 32) | best.lo;
        if (key < bk || (key == bk && nn < best.nonce)) {
            best.hi = (uint32_t)(key >> 32);
            best.lo = (uint32_t)key;
            best.nonce = nn;
        }
    }
}

// The per-nonce test of the default (minimum) reduction: may this key beat
// the wave's best?  One compare against a wave-uniform value.
DEV bool wave_cand(const WaveBest& best, uint32_t h0) { return h0 <= best.hi; }

// "First below target" reduction (find_kernels.hip, hm_find): the wave keeps
// the LOWEST nonce n in [seg_lo, seg_hi] with Hash(msg, n) < target instead
// of the minimum key.  The per-nonce test is h0 <= (target - 1) >> 32, one
// compare against a wave-uniform constant like the minimum's; only behind the
// ballot are the 64-bit key, key < target and the range check formed and the
// wave minimum of the nonce taken.  Nonces at or above `nonce` (the wave's
// best so far, or a lower hit another wave published) cannot win and are
// ignored.  nonce = MaxUint64: no hit.
struct WaveFirst {
    uint32_t thi;     // (target - 1) >> 32, target >= 1
    uint64_t target;
    uint64_t nonce = ~0ull;
};
DEV bool wave_cand(const WaveFirst& first, uint32_t h0) { return h0 <= first.thi; }
DEV void take_step(WaveFirst& first, bool cand, uint32_t h0, uint32_t h1, uint64_t nbase,
                   uint32_t off, uint64_t seg_lo, uint64_t seg_hi, bool) {
    if (__builtin_amdgcn_ballot_w64(cand)) {
        const uint64_t key = ((uint64_t)h0 << 32) | h1;
        uint64_t nn = nbase + off;
        const bool ok = cand && key < first.target && nn >= seg_lo && nn <= seg_hi &&
                        nn < first.nonce;
        if (!ok) nn = ~0ull;
        uint64_t zero = 0;  // wave_min orders (nonce, 0) pairs: the minimum nonce
        wave_min(nn, zero);
        nn = uni64(nn);
        if (nn < first.nonce) first.nonce = nn;
    }
}

// "All below target" reduction (collect_kernels.hip, hm_collect): the wave
// counts every nonce n in [seg_lo, seg_hi] with Hash(msg, n) < target and,
// with a record buffer (cap > 0), appends (hash, nonce) for each.  The
// per-nonce test is WaveFirst's one compare.  Behind the ballot the 64-bit
// key, key < target, the range check and lane_ok are formed -- a surplus lane
// (one that repeats another lane's nonce) is never a hit: a duplicate cannot
// hurt a minimum but would be counted twice here -- the hits of the step are
// counted in a wave-uniform register (popcount of the ballot), and one lane
// reserves that many slots with one atomic on the device's cursor, each hit
// lane taking base + its rank among the hit lanes.  A wave that sees a base
// at or past cap stops reserving: the call has overflowed and its records
// will not be read.
struct WaveCollect {
    uint32_t thi;      // (target - 1) >> 32, target >= 1
    uint32_t cap;      // records the buffer holds; 0: count only
    uint64_t target;
    uint64_t* cursor;  // next free slot (agent scope)
    uint64_t* out;     // 2 x u64 per slot: (hash, nonce)
    uint64_t count = 0;  // the wave's hits (uniform)
    bool full = false;   // a reservation of this wave began at or past cap (uniform)
};
DEV bool wave_cand(const WaveCollect& c, uint32_t h0) { return h0 <= c.thi; }
DEV void take_step(WaveCollect& c, bool cand, uint32_t h0, uint32_t h1, uint64_t nbase,
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
                    }
                }
            }
        }
    }
}

// "The k lowest below target" reduction (find_k_kernels.hip, hm_find_k):
// WaveCollect's step -- the one compare per nonce, lane_ok, one cursor
// reservation per step with hits, the `full` rule -- without the count, and
// with two wave-uniform registers the kernel resets before each task: `c`,
// how many of the task's records landed in slots below k, and `mx`, the
// largest nonce among those.  The kernel publishes both after the task; once
// all k such slots are published their largest nonce bounds the k-th lowest
// hit and becomes the stop word.
struct WaveFirstK {
    uint32_t thi;      // (target - 1) >> 32, target >= 1
    uint32_t cap;      // records the buffer holds, >= k
    uint32_t k;
    uint64_t target;
    uint64_t* cursor;  // next free slot (agent scope)
    uint64_t* out;     // 2 x u64 per slot: (hash, nonce)
    bool full = false;  // a reservation of this wave began at or past cap (uniform)
    uint32_t c = 0;     // this task's records in slots < k (uniform)
    uint64_t mx = 0;    // the largest nonce among them (uniform)
};
DEV bool wave_cand(const WaveFirstK& f, uint32_t h0) { return h0 <= f.thi; }
DEV void take_step(WaveFirstK& f, bool cand, uint32_t h0, uint32_t h1, uint64_t nbase,
                   uint32_t off, uint64_t seg_lo, uint64_t seg_hi, bool lane_ok) {
    if (__builtin_amdgcn_ballot_w64(cand)) {
        const uint64_t key = ((uint64_t)h0 << 32) | h1;
        const uint64_t nn = nbase + off;
        const bool ok = cand && lane_ok && key < f.target && nn >= seg_lo && nn <= seg_hi;
        const uint64_t hits = __builtin_amdgcn_ballot_w64(ok);
        if (hits && !f.full) {
            const uint32_t n = (uint32_t)__builtin_popcountll(hits);
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi(
                (uint32_t)(hits >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hits, 0u));
            uint64_t base = 0;
            if (ok && rank == 0)
                base = __hip_atomic_fetch_add(f.cursor, (uint64_t)n, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t src = (uint32_t)__builtin_ctzll(hits);
            base = ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(base >> 32), src) << 32) |
                   __builtin_amdgcn_readlane((uint32_t)base, src);
            if (base >= f.cap) {
                f.full = true;
            } else {
                const uint64_t slot = base + rank;
                if (ok && slot < f.cap) {
                    f.out[2 * slot] = key;
                    f.out[2 * slot + 1] = nn;
                }
                if (base < f.k) {
                    // the step's records in slots < k: their count, and their
                    // largest nonce as the wave minimum of the complements
                    uint64_t inv = ok && slot < f.k ? ~nn : ~0ull, zero = 0;
                    wave_min(inv, zero);
                    const uint64_t m = ~uni64(inv);
                    if (m > f.mx) f.mx = m;
                    const uint64_t room = f.k - base;
                    f.c += n < room ? n : (uint32_t)room;
                }
            }
        }
    }
}

// "The k lowest" reduction (scan_k_kernels.hip, hm_scan_k): the wave keeps a
// list of up to 64 (hash, nonce) records in its own 1 KiB of LDS and, once it
// knows k of them, a wave-uniform bound (key, nonce) that every later record
// must lie strictly below.  The per-nonce test is h0 <= bhi, WaveBest's one
// compare (bhi = 0xffffffff while unbounded).  Behind the ballot the 64-bit
// key, the range check, lane_ok and (key, nonce) < bound are formed, and the
// hit lanes append at cnt + their rank among the hit lanes.  A list that
// cannot take a step's hits is compacted first (lowk_compact): sorted, cut to
// its k lowest records, and the bound lowered to the k-th of them.  All the
// state but the list is wave-uniform (SGPRs).
struct WaveLowK {
    uint32_t bhi = 0xffffffffu;  // bound key >> 32 while bounded
    uint64_t bkey = ~0ull, bnonce = ~0ull;  // the bound (bounded only)
    bool bounded = false;
    uint32_t cnt = 0;  // records in the list
    uint32_t k;
    uint64_t* list;    // LDS: 64 slots of 2 x u64, this wave's own
    uint64_t inserted = 0;     // records appended (stats)
    uint32_t compactions = 0;  // (stats)
};
// (the builtin returns int: each half goes through uint32_t, or the low one
// would sign-extend into the high one)
DEV uint64_t readlane64(uint64_t x, uint32_t lane) {
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((uint32_t)(x >> 32), lane);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((uint32_t)x, lane);
    return ((uint64_t)hi << 32) | lo;
}
// The lane id, formed where it is used: everything this reduction does per
// lane sits behind the ballot, and a lane id the compiler may hoist (with the
// list address and the lane's bit mask derived from it) would live in VGPRs
// through the task bodies' hot loop.  The empty asm pins it to its block.
DEV uint32_t cold_lane_id() {
    uint32_t zero = 0;
    asm volatile("" : "+v"(zero));
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, zero));
}
DEV bool lex_below(uint64_t k, uint64_t n, uint64_t k2, uint64_t n2) {
    return k < k2 || (k == k2 && n < n2);
}
// Sort the list, keep its min(cnt, k) lowest records, lower the bound.  Lane i
// < cnt holds record i; its rank is the number of list records below it (the
// records are distinct by nonce, so the ranks are a permutation of 0..cnt-1);
// ranks < k go back to slot = rank.
DEV void lowk_compact(WaveLowK& w) {
    const uint32_t lane = cold_lane_id();
    const bool have = lane < w.cnt;
    uint64_t key = ~0ull, nn = ~0ull;
    if (have) {
        key = w.list[2 * lane];
        nn = w.list[2 * lane + 1];
    }
    // all 64 lanes, unrolled (constant lane selects): a lane at or past cnt
    // holds (MaxUint64, MaxUint64), which is below no record, so it adds to
    // no rank.  That pair is also a representable record (nonce 2^64-1
    // hashing to 2^64-1).  Such a record still ranks correctly: every other
    // record is below it, and an empty lane's equal pair is not (the test is
    // strict), so its rank is cnt - 1, the last.  Unrolled, so that the task
    // bodies' hot loop keeps no loop inside it (align_loops.py places the
    // innermost one)
    uint32_t rank = 0;
#pragma unroll
    for (int j = 0; j < kWaveSize; ++j)
        rank += lex_below(readlane64(key, j), readlane64(nn, j), key, nn) ? 1u : 0u;
    __builtin_amdgcn_wave_barrier();  // every lane holds its record before any slot is rewritten
    if (have && rank < w.k) {
        w.list[2 * rank] = key;
        w.list[2 * rank + 1] = nn;
    }
    __builtin_amdgcn_wave_barrier();
    ++w.compactions;
    if (w.cnt >= w.k) {
        w.cnt = w.k;
        // the k-th lowest: the one lane of rank k - 1
        const uint64_t kth = __builtin_amdgcn_ballot_w64(have && rank == w.k - 1);
        const uint32_t src = (uint32_t)__builtin_ctzll(kth);
        const uint64_t bk = readlane64(key, src), bn = readlane64(nn, src);
        if (!w.bounded || lex_below(bk, bn, w.bkey, w.bnonce)) {
            w.bkey = bk;
            w.bnonce = bn;
            w.bhi = (uint32_t)(bk >> 32);
            w.bounded = true;
        }
    }
}
// Append the records of the lanes in `mask` (a ballot; at most 64 - cnt lanes);
// `in` is the lane's own bit of it.
DEV void lowk_append(WaveLowK& w, uint64_t mask, bool in, uint64_t key, uint64_t nn) {
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    if (in) {
        const uint32_t slot = w.cnt + rank;
        w.list[2 * slot] = key;
        w.list[2 * slot + 1] = nn;
    }
    __builtin_amdgcn_wave_barrier();
    w.cnt += (uint32_t)__builtin_popcountll(mask);
}
// Insert the records of the lanes in `hits` (a non-empty ballot; `ok` is the
// lane's own bit of it).  If they do
// not fit into the 64 slots the list is compacted first (then cnt <= k <= 32);
// if they still do not fit they go in as two halves of at most 32 lanes with a
// compaction between.  A compaction may lower the bound below a hit that is
// still to be appended: it is appended all the same and leaves with the next
// compaction.
DEV void lowk_insert(WaveLowK& w, bool ok, uint64_t hits, uint64_t key, uint64_t nn) {
    const uint32_t n = (uint32_t)__builtin_popcountll(hits);
    w.inserted += n;
    if (w.cnt + n > (uint32_t)kWaveSize) lowk_compact(w);
    if (w.cnt + n > (uint32_t)kWaveSize) {
        const bool low_half = cold_lane_id() < 32u;
        lowk_append(w, hits & 0xffffffffull, ok && low_half, key, nn);
        lowk_compact(w);
        lowk_append(w, hits & ~0xffffffffull, ok && !low_half, key, nn);
    } else {
        lowk_append(w, hits, ok, key, nn);
    }
}
DEV bool wave_cand(const WaveLowK& w, uint32_t h0) { return h0 <= w.bhi; }
DEV void take_step(WaveLowK& w, bool cand, uint32_t h0, uint32_t h1, uint64_t nbase, uint32_t off,
                   uint64_t seg_lo, uint64_t seg_hi, bool lane_ok) {
    if (__builtin_amdgcn_ballot_w64(cand)) {
        const uint64_t key = ((uint64_t)h0 << 32) | h1;
        const uint64_t nn = nbase + off;
        const bool ok = cand && lane_ok && nn >= seg_lo && nn <= seg_hi &&
                        (!w.bounded || lex_below(key, nn, w.bkey, w.bnonce));
        const uint64_t hits = __builtin_amdgcn_ballot_w64(ok);
        if (hits) lowk_insert(w, ok, hits, key, nn);
    }
}

// The wave's count into the device total, once, at the wave's exit
// (hm_collect's hits, hm_verify's bad records).
DEV void wave_total(uint64_t* total, uint64_t count) {
    if (count && __lane_id() == 0)
        __hip_atomic_fetch_add(total, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------
// Task ids of a persistent launch (seg_walk.cpp guided_tasks): ids below nbig
// are whole units, each later unit is kSplit ids, one part each (the guided
// tail).  `task` is parts [part, part_end) of the kSplit parts of `unit`: all
// of them for a whole unit (false), one for a split unit (true).
// ---------------------------------------------------------------------------
DEV bool guided_split(uint32_t task, uint32_t nbig, uint32_t& unit, uint32_t& part,
                      uint32_t& part_end) {
    unit = task;
    part = 0;
    part_end = kSplit;
    const bool split = task >= nbig;
    if (split) {
        const uint32_t k = task - nbig;
        const uint32_t u = k / kSplit;
        unit = nbig + u;
        part = k - u * kSplit;
        part_end = part + 1;
    }
    return split;
}

// Tiled launch: a unit is one lane chunk of one tile, a part one tens digit
// of its loop, t1 in [t1_begin, t1_end).
static_assert(kSplit == 10, "a part of a tiled unit is one tens digit");
struct TiledTask {
    uint32_t tile, chunk, t1_begin, t1_end;
};
DEV TiledTask tiled_decode(const TiledArgs& A, uint32_t task) {
    // declared in this order: hipcc numbers the task loop's registers by it,
    // and the tiled kernels' text is held equal to what it was before the
    // decoders were shared.  Any order is as correct: this one only made
    // the sharing checkable byte for byte and may be dropped later
    uint32_t t1_end, t1_begin, unit;
    guided_split(task, A.nbig, unit, t1_begin, t1_end);
    const uint32_t tile = unit / A.tpt;
    return {tile, unit - tile * A.tpt, t1_begin, t1_end};
}

// Chained launch: a unit is one loop chunk (tch loop values, the last one
// ending at nloop) of one lane chunk of one tile, a part a kSplit-th of it,
// rounded up; t in [t_begin, t_end).  per_tile = A.tpt * A.ntc, formed once
// by the caller before its task loop.
struct ChainedTask {
    uint32_t tile, chunk, t_begin, t_end;
};
DEV ChainedTask chained_decode(const ChainedArgs& A, uint32_t per_tile, uint32_t task) {
    uint32_t unit, part, part_end, nparts = 1;
    if (guided_split(task, A.nbig, unit, part, part_end)) nparts = kSplit;
    const uint32_t tile = unit / per_tile;
    const uint32_t rem = unit - tile * per_tile;
    const uint32_t chunk = rem / A.ntc;
    const uint32_t tc = rem - chunk * A.ntc;
    const uint32_t piece = (A.tch + nparts - 1) / nparts;
    const uint32_t t_begin = tc * A.tch + part * piece;
    uint32_t t_end = tc * A.tch + A.tch;
    if (t_end > A.nloop) t_end = A.nloop;
    if (t_end > t_begin + piece) t_end = t_begin + piece;
    return {tile, chunk, t_begin, t_end};
}

// Every tiled layout the planner can pick (plan.cpp layout): one tail block
// with W1 = 1..13, or W1 = 13..15 followed by a constant trailer block, each
// without and with a straddling tens digit.  X(W1, STRADDLE, TRAILER); the
// kernel instantiations and the fused kernel's switch all expand this list.
#define HM_TILED_LAYOUT_S(X, W, T) X(W, false, T) X(W, true, T)
#define HM_FOR_EACH_TILED_LAYOUT(X)                                              \
    HM_TILED_LAYOUT_S(X, 1, false) HM_TILED_LAYOUT_S(X, 2, false)                \
    HM_TILED_LAYOUT_S(X, 3, false) HM_TILED_LAYOUT_S(X, 4, false)                \
    HM_TILED_LAYOUT_S(X, 5, false) HM_TILED_LAYOUT_S(X, 6, false)                \
    HM_TILED_LAYOUT_S(X, 7, false) HM_TILED_LAYOUT_S(X, 8, false)                \
    HM_TILED_LAYOUT_S(X, 9, false) HM_TILED_LAYOUT_S(X, 10, false)               \
    HM_TILED_LAYOUT_S(X, 11, false) HM_TILED_LAYOUT_S(X, 12, false)              \
    HM_TILED_LAYOUT_S(X, 13, false) HM_TILED_LAYOUT_S(X, 13, true)               \
    HM_TILED_LAYOUT_S(X, 14, true) HM_TILED_LAYOUT_S(X, 15, true)

// Launch bounds of the tiled kernels of every family.
#ifndef HM_TILED_WAVES_PER_EU
#define HM_TILED_WAVES_PER_EU 0
#endif
#if HM_TILED_WAVES_PER_EU > 0
#define HM_TILED_BOUNDS __launch_bounds__(kBlock, HM_TILED_WAVES_PER_EU)
#else
#define HM_TILED_BOUNDS __launch_bounds__(kBlock)
#endif

// Workgroup-level task dispenser (round 5; the per-segment kernels and,
// with kFusedLds, the fused one).  A wave draws a ticket from an
// LDS counter; the first ticket of each batch of kLdsBatch fetches the
// batch's task ids from the launch's queue with ONE device-scope atomic and
// publishes the base in a 4-entry LDS ring; the batch's other tickets wait
// for it there (at most one atomic's round trip, the waves of a workgroup
// rarely finish a task together).  The per-wave task granularity and the
// guided tail are unchanged; the queue sees a quarter of the atomics, which
// execute memory-side (PMC WRITE_SIZE per cfg2 launch 18.1 -> 4.6 MB; cfg2
// +0.1 %, cfg3 +1.0 %, d = 12 +0.04 % in an interleaved A/B,
// profiles/r05/experiments/lds_dispenser/).  The ring cannot be lapped: a
// batch's slot is rewritten only 4 batches (>= 16 tickets) later, and each
// of the 4 waves holds one ticket at a time.  The batch is 2^shift tasks:
// kLdsBatch by default; launches of >= 10^11 nonces (configs[3]'s d = 12
// segment) take 16 (round 6, HM_OPT_QUEUE_BATCH), since a tail imbalance of
// 16 tenth-units is nothing against their seconds of work.
constexpr uint32_t kLdsBatch = 4;
constexpr uint32_t kLdsShift = 2;  // log2(kLdsBatch)
struct LdsQueue {
    uint32_t ticket;
    uint32_t base[4];
    uint32_t ready[4];  // batch + 1 once base[batch & 3] is set
};
DEV void lds_queue_init(LdsQueue* q) {
    if (threadIdx.x == 0) {
        q->ticket = 0;
        for (int i = 0; i < 4; ++i) q->ready[i] = 0;
    }
    __syncthreads();
}
DEV uint32_t lds_dequeue(LdsQueue* q, unsigned int* counter, uint32_t shift = kLdsShift) {
    uint32_t task = 0;
    if (__lane_id() == 0) {
        const uint32_t t = atomicAdd(&q->ticket, 1u);
        const uint32_t batch = t >> shift, slot = batch & 3u;
        if (t - (batch << shift) == 0) {
            q->base[slot] = atomicAdd(counter, 1u << shift);
            __hip_atomic_store(&q->ready[slot], batch + 1, __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
            while (__hip_atomic_load(&q->ready[slot], __ATOMIC_ACQUIRE,
                                     __HIP_MEMORY_SCOPE_WORKGROUP) != batch + 1)
                __builtin_amdgcn_s_sleep(2);
        }
        task = q->base[slot] + (t - (batch << shift));
    }
    return uni(task);
}

// Lane digits: the q low decimal digits of v as ASCII bytes, least
// significant in the lowest byte.
DEV uint64_t lane_digits(uint32_t v, uint32_t q) {
    uint64_t packed = 0;
    uint32_t x = v;
    for (uint32_t k = 0; k < q; ++k) {
        const uint32_t y = x / 10u;
        packed |= (uint64_t)(0x30u + x - y * 10u) << (8u * k);
        x = y;
    }
    return packed;
}

// ---------------------------------------------------------------------------
// Tiled task: lane chunk `chunk` of the tile whose record is R (chaining
// state + final-block words, varying digits zeroed) and whose first nonce is
// tile_base; loop steps t1 in [t1_begin, t1_end) x t0 in [0, 10): one
// SHA-256 compression per nonce from the tile state (+ a constant trailer
// block, table kw, when the padding spills).  s0_loop[t1*10 + t0] = sigma0
// of the loop-digit bits of W[W1] (wave-uniform, read by scalar loads).
// t0 runs over [t0_begin, t0_end) (the fused launch's split tasks; the
// per-segment kernels take the constant defaults, so their loop is the full
// one).  Best is the reduction the task folds its nonces into: WaveBest (the
// running minimum, the default), WaveFirst (hm_find), WaveCollect
// (hm_collect), WaveFirstK (hm_find_k) or WaveLowK (hm_scan_k); each brings its wave_cand (the
// one compare per nonce) and take_step.
// ---------------------------------------------------------------------------
template <int W1, bool STRADDLE, bool TRAILER, bool CSUM, typename S0, typename KW,
          typename Best = WaveBest>
DEV void tiled_task(const uint32_t* __restrict__ R, uint32_t chunk, uint32_t t1_begin,
                    uint32_t t1_end, uint64_t tile_base, uint64_t seg_lo, uint64_t seg_hi,
                    uint32_t vmax, uint32_t q, uint32_t lane_shift, uint32_t loop_shift,
                    S0 s0_loop, KW trailer_kw, Best& best, WaveSums& sums,
                    uint32_t t0_begin = 0, uint32_t t0_end = 10) {
    static_assert(W1 >= 1 && W1 <= 15, "varying words are W[W1-1], W[W1]");
    // Lane digits may reach back into W[W1-2] (the planner does so when the
    // last two words leave room for fewer than 5 lane digits: 10^3 or 10^4
    // lane values fill 64-lane chunks only to 97.7 / 99.5 %).  W[W1-2] is
    // loop-invariant, so this changes per-task work only: the hot loop's
    // instructions are the same (profiles/r02/isa_audit.txt).
    constexpr bool L3 = W1 >= 2;
    const uint32_t lane = __lane_id();
    uint32_t st[8], W[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) st[k] = R[k];
#pragma unroll
    for (int k = 0; k < 16; ++k) W[k] = R[8 + k];

    uint32_t v = chunk * kWaveSize + lane;
    const bool lane_ok = v <= vmax;  // CSUM: surplus lanes are not counted
    v = v > vmax ? vmax : v;  // surplus lanes repeat a valid nonce
    uint64_t packed = lane_digits(v, q);
    // the lane digits as a 96-bit big-endian window W[W1-2]:W[W1-1]:W[W1]
    uint32_t Xm2 = 0, X0, X1;
    if constexpr (L3) {
        const unsigned __int128 p = (unsigned __int128)packed << lane_shift;
        Xm2 = W[W1 - 2] | (uint32_t)(p >> 64);
        X0 = W[W1 - 1] | (uint32_t)(p >> 32);
        X1 = W[W1] | (uint32_t)p;
    } else {
        packed <<= lane_shift;  // fits: q + lane_shift/8 <= 8 bytes
        X0 = W[W1 - 1] | (uint32_t)(packed >> 32);
        X1 = W[W1] | (uint32_t)packed;
    }
    const uint64_t nbase = tile_base + (uint64_t)v * 100u;
    const uint32_t s0X1 = ssig0<false>(X1);  // lane part of sigma0(W[W1])

    // only W[W1] changes from one t0 step to the next
    constexpr uint32_t VM = 1u << W1;
    for (uint32_t t1 = t1_begin; t1 < t1_end; ++t1) {
        uint32_t mw[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) mw[k] = W[k];
        if constexpr (L3) mw[W1 - 2] = Xm2;
        // loop digits: wave-uniform, in bytes that are zero in X1
        uint32_t Lt1;
        if constexpr (STRADDLE) {
            // last digit opens W[W1], the tens digit closes W[W1-1]
            mw[W1 - 1] = X0 + (0x30u + t1);
            Lt1 = 0;
        } else {
            mw[W1 - 1] = X0;
            Lt1 = (0x30u + t1) << 8;
        }
        // rounds before W[W1] and round W1 without its loop digits: per
        // t1.  Round W1 in closed form: T1 = P + L with P invariant in the
        // t0 loop, so e and a each cost one add of the uniform L there
        // (the empty asm keeps d + P and P + T2 as the two hoisted sums;
        // else P + L is shared and costs a third add per nonce).
        State s1{st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7]};
        sha_rounds_range<VM, W1, 0, W1>(s1, mw, 0);
        const uint32_t P = s1.h + bsig1<false>(s1.e) + ch(s1.e, s1.f, s1.g) + (kK[W1] + X1);
        const uint32_t T2 = bsig0<false>(s1.a) + maj(s1.a, s1.b, s1.c);
        uint32_t dP = s1.d + P, PT = P + T2;
        asm volatile("" : "+v"(dP), "+v"(PT));
        for (uint32_t t0 = t0_begin; t0 < t0_end; ++t0) {
            uint32_t m[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) m[k] = mw[k];
            const uint32_t L = STRADDLE ? (0x30u + t0) << 24 : (Lt1 | (0x30u + t0)) << loop_shift;
            // X1 and L are bit-disjoint: | is +
            m[W1] = X1 + L;
            const uint32_t s0w = s0X1 ^ s0_loop[t1 * 10u + t0];  // scalar load
            // the state after round W1: a = T1 + T2, e = d + T1
            State s{PT + L, s1.a, s1.b, s1.c, dP + L, s1.e, s1.f, s1.g};
            sha_rounds_range<VM, W1, W1 + 1, 64>(s, m, s0w);
            uint32_t h0, h1;
            if constexpr (TRAILER) {
                State o{s.a + st[0], s.b + st[1], s.c + st[2], s.d + st[3],
                        s.e + st[4], s.f + st[5], s.g + st[6], s.h + st[7]};
                State t = o;
                sha_rounds_kw(t, trailer_kw);
                h0 = t.a + o.a;
                h1 = t.b + o.b;
            } else {
                h0 = s.a + st[0];
                h1 = s.b + st[1];
            }
            if constexpr (CSUM) {
                const uint64_t n = nbase + t1 * 10u + t0;
                if (lane_ok && n >= seg_lo && n <= seg_hi) {
                    sums.sum += ((uint64_t)h0 << 32) | h1;
                    ++sums.cnt;
                }
            }
            take_step(best, wave_cand(best, h0), h0, h1, nbase, t1 * 10u + t0, seg_lo, seg_hi,
                      lane_ok);
        }
    }
}

// ---------------------------------------------------------------------------
// Chained task: per lane one compression of tail block 0 (lane digits in
// W15 and the last byte of W14) from the tile record R, then one
// table-driven compression per loop value t in [t_begin, t_end): the final
// block is wave-uniform, its K[i]+W[i] schedule row t comes from kwt (scalar
// loads).  nbase = the first nonce of the lane value (epoch included).
// ---------------------------------------------------------------------------
template <bool CSUM, typename Best = WaveBest>
DEV void chained_task(const uint32_t* __restrict__ R, uint32_t chunk, uint32_t t_begin,
                      uint32_t t_end, uint64_t tile_base, uint64_t pow10f, uint64_t seg_lo,
                      uint64_t seg_hi, uint32_t vmax, uint32_t q, const uint32_t* kwt,
                      Best& best, WaveSums& sums) {
    const uint32_t lane = __lane_id();
    uint32_t st[8], W[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) st[k] = R[k];
#pragma unroll
    for (int k = 0; k < 16; ++k) W[k] = R[8 + k];

    uint32_t v = chunk * kWaveSize + lane;
    const bool lane_ok = v <= vmax;
    v = v > vmax ? vmax : v;
    // lane digits: the last q (<= 5) bytes of tail block 0, in W15 and
    // (q = 5) the last byte of W14
    const uint64_t packed = lane_digits(v, q);
    uint32_t m[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) m[k] = W[k];
    m[14] = W[14] | (uint32_t)(packed >> 32);
    m[15] = W[15] | (uint32_t)packed;
    State s{st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7]};
    sha_rounds<3u << 14>(s, m);  // once per task: W14, W15 vary across lanes
    // chaining value into the final block (per lane)
    const State cs{s.a + st[0], s.b + st[1], s.c + st[2], s.d + st[3],
                   s.e + st[4], s.f + st[5], s.g + st[6], s.h + st[7]};
    const uint64_t nbase = tile_base + (uint64_t)v * pow10f;
    const_u32* kw = (const_u32*)(kwt + (size_t)t_begin * 64);
    for (uint32_t t = t_begin; t < t_end; ++t, kw += 64) {
        State u = cs;
        sha_rounds_kw<true>(u, kw);
        const uint32_t h0 = u.a + cs.a;
        if constexpr (CSUM) {
            const uint64_t n = nbase + t;
            if (lane_ok && n >= seg_lo && n <= seg_hi) {
                sums.sum += ((uint64_t)h0 << 32) | (u.b + cs.b);
                ++sums.cnt;
            }
        }
        take_step(best, wave_cand(best, h0), h0, u.b + cs.b, nbase, t, seg_lo, seg_hi, lane_ok);
    }
}

// Write the wave's best (and, checked, its coverage pair) to its slot.
template <bool CSUM>
DEV void wave_store(uint64_t* cand, uint64_t* sums_out, uint32_t wslot, const WaveBest& best,
                    const WaveSums& sums) {
    if (__lane_id() == 0) {
        cand[2 * wslot] = ((uint64_t)best.hi << 32) | best.lo;
        cand[2 * wslot + 1] = best.nonce;
    }
    if constexpr (CSUM) store_sums(sums_out, wslot, sums.sum, sums.cnt);
}

}  // namespace hm
