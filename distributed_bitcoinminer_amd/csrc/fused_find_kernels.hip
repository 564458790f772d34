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
//                640-nonce body, folding into WaveFirst ("first below
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
// The task decoders below are this file's own copies of fused_kernels.hip's
// fused_tiled / fused_chained / fused_generic (they return the task's first
// loop value before running it): the shipped kernel's text is held byte for
// byte, as for the generic kernels (profiles/README.md, dedup/).
//
// Compiled like scan_kernels.hip (device-only -S, align_loops.py, linked into
// hipminer_scan.hsaco) and looked up by mangled name (kernel_name() in
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
typedef const __attribute__((address_space(4))) FusedFindArgs FusedFindArgsK;
typedef const __attribute__((address_space(4))) FusedArgs FusedArgsK;

// The request's stop word and its wave-side state.
struct FindWave {
    uint64_t* word;
    WaveFirst first;
    uint32_t ran = 0;
};

// Before a task whose smallest nonce is task_lo (clamped to its segment's
// end): false = skip it (and leave).  Otherwise the wave's bound drops to the
// published hit and *before = the bound the task starts from.
DEV bool ff_enter(FindWave& w, uint64_t task_lo, uint64_t seg_hi, uint64_t* before) {
    uint64_t stop = 0;
    if (__lane_id() == 0)
        stop = __hip_atomic_load(w.word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    stop = uni64(stop);
    if ((task_lo < seg_hi ? task_lo : seg_hi) > stop) return false;
    if (stop < w.first.nonce) w.first.nonce = stop;
    *before = w.first.nonce;
    return true;
}
// After a task that ran: count it, publish a lowered bound.
DEV void ff_done(FindWave& w, uint64_t before) {
    ++w.ran;
    if (w.first.nonce < before && __lane_id() == 0)
        __hip_atomic_fetch_min(w.word, w.first.nonce, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Piece `pp` of `np` of the run [b, e): [*b2, *e2) (empty when past e).
DEV void ff_piece_of(uint32_t b, uint32_t e, uint32_t pp, uint32_t np, uint32_t* b2,
                     uint32_t* e2) {
    const uint32_t len = (e - b + np - 1) / np;
    uint32_t x = b + pp * len, y = x + len;
    if (x > e) x = e;
    if (y > e) y = e;
    *b2 = x;
    *e2 = y;
}

// Each body: false = the task was skipped, the wave leaves.

template <int W1, bool STRADDLE, bool TRAILER>
DEV bool ff_tiled(FusedArgsK* A, const FusedSeg& S, uint32_t k, uint32_t pp, uint32_t np,
                  FindWave& w) {
    // task k: unit, tens digit t1 and part of the units loop (fused_tiled)
    const uint32_t per_unit = 10u * S.tpu;
    const uint32_t unit = S.unit0 + k / per_unit;
    const uint32_t rem = k - (k / per_unit) * per_unit;
    const uint32_t t1 = rem / S.tpu;
    const uint32_t part = rem - t1 * S.tpu;
    const uint32_t steps = 10u / S.tpu;
    uint32_t t0b, t0e;
    ff_piece_of(part * steps, part * steps + steps, pp, np, &t0b, &t0e);
    if (t0b >= t0e) return true;  // an empty piece (uniform)
    const uint32_t tile = unit / S.tpt;
    const uint32_t chunk = unit - tile * S.tpt;
    const uint64_t tile_base = (S.tile0 + tile) * S.pow10V;
    const uint64_t task_lo = tile_base + (uint64_t)chunk * (kWaveSize * 100u) + t1 * 10u + t0b;
    uint64_t before;
    if (!ff_enter(w, task_lo, S.seg_hi, &before)) return false;
    WaveSums sums;  // unused (CSUM = false)
    const_u32* tab = (const_u32*)(A->aux + S.aux0);
    tiled_task<W1, STRADDLE, TRAILER, false>(A->rec + (size_t)(S.rec0 + tile) * kRecWords, chunk, t1,
                                             t1 + 1, tile_base, S.seg_lo, S.seg_hi, S.vmax, S.q,
                                             S.lane_shift, S.loop_shift, tab, tab + 100, w.first,
                                             sums, t0b, t0e);
    ff_done(w, before);
    return true;
}

DEV bool ff_chained(FusedArgsK* A, const FusedSeg& S, uint32_t k, uint32_t pp, uint32_t np,
                    FindWave& w) {
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
    ff_piece_of(t_begin, t_end, pp, np, &tb, &te);
    if (tb >= te) return true;  // an empty piece (uniform)
    const uint64_t tile_base = (S.tile0 + tile) * S.pow10V;
    // lane 0's first loop value (the lanes stride pow10f beyond it)
    const uint64_t task_lo = tile_base + (uint64_t)chunk * kWaveSize * S.pow10f + tb;
    uint64_t before;
    if (!ff_enter(w, task_lo, S.seg_hi, &before)) return false;
    WaveSums sums;  // unused (CSUM = false)
    chained_task<false>(A->rec + (size_t)(S.rec0 + tile) * kRecWords, chunk, tb, te, tile_base,
                        S.pow10f, S.seg_lo, S.seg_hi, S.vmax, S.q, A->aux + S.aux0, w.first, sums);
    ff_done(w, before);
    return true;
}

// Generic task k: nonces seg_lo + 640k + lane + 64j, j < 10 (a guided-tail
// piece: its share of the j), every tail block compressed per lane.
DEV bool ff_generic(FusedArgsK* A, const FusedSeg& S, uint32_t k, uint32_t pp, uint32_t np,
                    FindWave& w) {
    const uint32_t lane = __lane_id();
    const uint64_t base = S.seg_lo + (uint64_t)k * 640u;
    uint32_t jb, je;
    ff_piece_of(0, 10, pp, np, &jb, &je);
    if (jb >= je) return true;  // an empty piece (uniform)
    uint64_t before;
    if (!ff_enter(w, base + 64u * jb, S.seg_hi, &before)) return false;
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
        take_step(w.first, in && wave_cand(w.first, h0), h0, h1, nb0, lane, S.seg_lo, S.seg_hi,
                  true);
    }
    ff_done(w, before);
    return true;
}

#define HM_FF_CASE(W, S, T) \
    case (W) * 4 + (S) * 2 + (T): go = ff_tiled<W, S, T>(A, S_, k, pp, np, w); break;

// The argument block is the kernel's only (explicit) parameter, so it starts
// the kernarg segment.
__global__ void __launch_bounds__(kBlock) hm_fused_find_kernel(const FusedFindArgs) {
    FusedFindArgsK* P = (FusedFindArgsK*)__builtin_amdgcn_kernarg_segment_ptr();
    FusedArgsK* A = &P->a;
    const uint32_t wslot = blockIdx.x * (kBlock / kWaveSize) + uni(threadIdx.x / kWaveSize);
    FindWave w;
    w.word = P->f.word;
    w.first.target = P->f.target;
    w.first.thi = (uint32_t)((P->f.target - 1) >> 32);
    // the first task is the wave's slot: the planner started the counter past
    // every slot, so a wave draws ascending ids
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
        bool go;
        switch (S_.variant) {
            HM_FOR_EACH_TILED_LAYOUT(HM_FF_CASE)
            case kVarChained: go = ff_chained(A, S_, k, pp, np, w); break;
            default: go = ff_generic(A, S_, k, pp, np, w); break;
        }
        if (!go) break;
        next = 0;
        if (__lane_id() == 0) next = atomicAdd(A->counter, 1u);
    }
    if (w.ran && __lane_id() == 0)
        __hip_atomic_fetch_add(P->f.tasks_run, (uint64_t)w.ran, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}

#undef HM_FF_CASE

}  // namespace hm
