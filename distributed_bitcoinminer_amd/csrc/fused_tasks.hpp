// fused_tasks.hpp -- the task walker of the fused batch kernels, which
// fused_find_kernels.hip runs on: hm_fused_kernel's task loop
// (fused_kernels.hip: task ids from one counter, a task id names its segment,
// the segment's layout is chosen by a wave-uniform switch) as templates over a
// WAVE POLICY, the type in which a kernel file keeps its wave-side state and
// its protocol:
//   red()                    the reduction the task bodies fold into
//                            (tiled_task / chained_task / take_step,
//                            scan_tasks.hpp)
//   enter(task_lo, seg_hi)   before a task whose smallest nonce is task_lo:
//                            false = skip it, and the wave leaves its loop
//   done()                   after a task that ran
//
// A task's smallest nonce (task_lo) is lane 0's first loop value:
//   tiled    tile_base + chunk * 6400 + t1 * 10 + t0b
//   chained  tile_base + chunk * 64 * 10^f + tb
//   generic  seg_lo + 640 k + 64 jb
// It may be lower than the task's smallest IN-RANGE nonce (a segment that
// starts inside a lane chunk; a sum that wraps past 2^64 only looks lower),
// never higher.  Within a segment ids ascend in it (unit, tens digit, part;
// lane chunk, loop chunk, part; 640-nonce block), and the guided-tail pieces
// are the highest ids, of the last tasks; a wave draws ascending ids (its slot,
// then the counter, which the planner starts past every slot).  What a policy
// may conclude from that is its own file's proof.
//
// fused_kernels.hip keeps its own decoders (WaveBest and the coverage sums, no
// empty-piece return, the experiment flags): the benchmark's kernel text is
// held byte for byte.  fused_collect_kernels.hip and fused_find_k_kernels.hip
// keep copies of this walk as well: the first measured slower through this
// header on single requests, the second was not measured enough (their
// headers say).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "scan_tasks.hpp"
#include "sha256_defs.hpp"
#include "sha_device.hpp"

namespace hm {

// The launch's FusedArgs read in place from the kernarg segment (see
// fused_kernels.hip: a runtime segment index would copy a by-value parameter
// to scratch).
typedef const __attribute__((address_space(4))) FusedArgs FusedArgsK;

// Piece `pp` of `np` of the run [b, e): [*b2, *e2) (empty when past e).
DEV void ft_piece_of(uint32_t b, uint32_t e, uint32_t pp, uint32_t np, uint32_t* b2, uint32_t* e2) {
    const uint32_t len = (e - b + np - 1) / np;
    uint32_t x = b + pp * len, y = x + len;
    if (x > e) x = e;
    if (y > e) y = e;
    *b2 = x;
    *e2 = y;
}

// Each body: false = the task was skipped, the wave leaves.

// Tiled task k of segment S: unit, tens digit t1 and part of the units loop;
// piece pp of np of that part.
template <int W1, bool STRADDLE, bool TRAILER, typename Wave>
DEV bool ft_tiled(FusedArgsK* A, const FusedSeg& S, uint32_t k, uint32_t pp, uint32_t np, Wave& w) {
    const uint32_t per_unit = 10u * S.tpu;
    const uint32_t unit = S.unit0 + k / per_unit;
    const uint32_t rem = k - (k / per_unit) * per_unit;
    const uint32_t t1 = rem / S.tpu;
    const uint32_t part = rem - t1 * S.tpu;
    const uint32_t steps = 10u / S.tpu;
    uint32_t t0b, t0e;
    ft_piece_of(part * steps, part * steps + steps, pp, np, &t0b, &t0e);
    if (t0b >= t0e) return true;  // an empty piece (uniform)
    const uint32_t tile = unit / S.tpt;
    const uint32_t chunk = unit - tile * S.tpt;
    const uint64_t tile_base = (S.tile0 + tile) * S.pow10V;
    const uint64_t task_lo = tile_base + (uint64_t)chunk * (kWaveSize * 100u) + t1 * 10u + t0b;
    if (!w.enter(task_lo, S.seg_hi)) return false;
    WaveSums sums;  // unused (CSUM = false)
    const_u32* tab = (const_u32*)(A->aux + S.aux0);
    tiled_task<W1, STRADDLE, TRAILER, false>(A->rec + (size_t)(S.rec0 + tile) * kRecWords, chunk, t1,
                                             t1 + 1, tile_base, S.seg_lo, S.seg_hi, S.vmax, S.q,
                                             S.lane_shift, S.loop_shift, tab, tab + 100, w.red(),
                                             sums, t0b, t0e);
    w.done();
    return true;
}

// Chained task k of segment S: lane chunk, loop chunk and part of it; piece pp
// of np of that part.
template <typename Wave>
DEV bool ft_chained(FusedArgsK* A, const FusedSeg& S, uint32_t k, uint32_t pp, uint32_t np,
                    Wave& w) {
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
    ft_piece_of(t_begin, t_end, pp, np, &tb, &te);
    if (tb >= te) return true;  // an empty piece (uniform)
    const uint64_t tile_base = (S.tile0 + tile) * S.pow10V;
    // lane 0's first loop value (the lanes stride pow10f beyond it)
    const uint64_t task_lo = tile_base + (uint64_t)chunk * kWaveSize * S.pow10f + tb;
    if (!w.enter(task_lo, S.seg_hi)) return false;
    WaveSums sums;  // unused (CSUM = false)
    chained_task<false>(A->rec + (size_t)(S.rec0 + tile) * kRecWords, chunk, tb, te, tile_base,
                        S.pow10f, S.seg_lo, S.seg_hi, S.vmax, S.q, A->aux + S.aux0, w.red(), sums);
    w.done();
    return true;
}

// Generic task k: nonces seg_lo + 640k + lane + 64j, j < 10 (a guided-tail
// piece: its share of the j), every tail block compressed per lane.  A lane
// past the segment's end (or past 2^64-1) hashes the step's first nonce again:
// a surplus lane, so `in` is both part of cand and the lane_ok.
template <typename Wave>
DEV bool ft_generic(FusedArgsK* A, const FusedSeg& S, uint32_t k, uint32_t pp, uint32_t np,
                    Wave& w) {
    const uint32_t lane = __lane_id();
    const uint64_t base = S.seg_lo + (uint64_t)k * 640u;
    uint32_t jb, je;
    ft_piece_of(0, 10, pp, np, &jb, &je);
    if (jb >= je) return true;  // an empty piece (uniform)
    if (!w.enter(base + 64u * jb, S.seg_hi)) return false;
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
        take_step(w.red(), in && wave_cand(w.red(), h0), h0, h1, nb0, lane, S.seg_lo, S.seg_hi, in);
    }
    w.done();
    return true;
}

#define HM_FUSED_WALK_CASE(W, S, T) \
    case (W) * 4 + (S) * 2 + (T): go = ft_tiled<W, S, T>(A, S_, k, pp, np, w); break;

// One wave's share of the launch: its first task is its slot (the planner
// started the counter past every slot, so a wave draws ascending ids), then a
// plain dequeue from the counter, until the ids run out or a task is skipped.
template <typename Wave>
DEV void fused_walk(FusedArgsK* A, Wave& w) {
    uint32_t next = blockIdx.x * (kBlock / kWaveSize) + uni(threadIdx.x / kWaveSize);
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
        bool go;
        switch (S_.variant) {
            HM_FOR_EACH_TILED_LAYOUT(HM_FUSED_WALK_CASE)
            case kVarChained: go = ft_chained(A, S_, k, pp, np, w); break;
            default: go = ft_generic(A, S_, k, pp, np, w); break;
        }
        if (!go) break;
        next = 0;
        if (__lane_id() == 0) next = atomicAdd(A->counter, 1u);
    }
}

#undef HM_FUSED_WALK_CASE

}  // namespace hm
