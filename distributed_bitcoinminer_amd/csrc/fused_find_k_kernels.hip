// fused_find_k_kernels.hip -- the fused find_k kernel of hm_find_k_many
// (gfx950): the k LOWEST nonces of one request's window whose hash is below a
// target, every digit segment of the window in ONE persistent launch that
// exits early.
//
// The pool form of the miner's loop (cmu440/bitcoin/miner/miner.go:46-59 over
// bitcoin.Hash, hash.go:13-17): "from nonce lo, the next k shares",
//   for n = lo .. hi: if Hash(msg, n) < target: emit (Hash, n); stop after k.
// hm_find_k (find_k_kernels.hip) answers it with one launch per segment piece
// on stream 0 and a host round trip every four launches; at ordinary targets
// the k-th hit is a few million nonces in, and the call is bound by those
// launches.  This kernel is hm_fused_find_kernel's task loop
// (fused_find_kernels.hip: task ids from one counter, a task id names its
// segment, the segment's layout is chosen by a wave-uniform switch, a wave that
// skips a task leaves) with hm_find_k's reduction and publish protocol:
//   task bodies  tiled_task / chained_task (scan_tasks.hpp) and the generic
//                640-nonce body, folding into WaveFirstK ("the k lowest below
//                target"); the per-nonce test is wave_cand: h0 <= (target-1)>>32
//   dispensing   the shipped scheme only: a wave's first task is its slot,
//                then a plain dequeue from the counter, which the planner
//                (hm_fused_plan_kernel) starts past every slot; guided-tail
//                ids >= nbig are pieces of their task
//
// Device protocol: five 64-bit words per REQUEST (FindKArgs::ctl, indices
// kFk*) and the request's own slice of `cap` >= k 16-byte records
// (FindKArgs::out).  The planner launch that precedes this one on the stream
// seeds (stop, cursor) = (MaxUint64, 0); filled, maxk and tasks_run are zeroed
// on the same stream before it.
//   record   as hm_collect: on a step with hits one lane reserves popcount
//            slots with one agent-scope fetch_add on `cursor`, each hit lane
//            writes (hash, nonce) with vector stores if its slot is < cap
//   publish  c and mx are reset before each task.  Right after a task that put
//            c > 0 records into slots < k, the largest of their nonces being
//            mx, one lane does, in this order, atomic max(maxk, mx) and
//            old = fetch_add(filled, c) (acquire-release, agent scope).  The
//            slots < k are reserved exactly once each, so exactly one wave sees
//            old + c == k: every slot < k is then written and folded into
//            maxk.  That wave loads maxk and does atomic min(stop, maxk): from
//            then on k hits with nonce <= stop exist
//   skip     before each task a wave reads `stop` (relaxed, agent scope); a
//            task whose smallest nonce, clamped to its segment's end, is above
//            it is not run
//   leave    the host orders the segments ascending by nonce and ids are
//            monotone in their smallest nonce (fused_find_kernels.hip), and
//            each wave draws ascending ids (its slot, then the counter): on its
//            first skip a wave leaves its loop
//   count    each wave adds the tasks it ran to tasks_run once
// Nothing spins and no wave waits on another.
//
// hm_cancel (ABI 1.18; cancel_relay.hpp).  Wave 0 of workgroup 0
// is the launch's RELAY: at kernel entry and before each task it takes it reads
// the context's cancel flag (FindKArgs::cancel, pinned host memory; one relaxed
// system-scope load) and, if it is set, lowers the stop word to 0, from where
// skip / leave / exit above end this launch and those queued behind it.  A
// word lowered so is FORGED -- 0 is not a hit, nor "k records at or below 0" -- and the invariants
// below speak of a call that was not cancelled.  The cancel invariant:
//   The word is forged only if the flag is set.  The flag is set before the
//   device can see it, and only the call's own thread clears it (at call
//   start).  Therefore the host, which tests the flag after every wait or
//   readback and BEFORE it interprets any control word, never mistakes a
//   forged word for an answer.
//
// A task's smallest nonce (task_lo) is lane 0's first loop value, as in
// fused_find_kernels.hip; it may be lower than the task's smallest IN-RANGE
// nonce, never higher.  The skip test is min(task_lo, seg_hi) > stop.  The
// clamp is still right although `stop` is no longer the first hit but an upper
// bound of the k-th: all the argument needs is that a lowered `stop` is the
// nonce of a record, and a record is an in-range hit of the launch, so it lies
// in [seg_lo, seg_hi] of one of the launch's segments.
//   - task_lo <= seg_hi: the test is task_lo > stop, so every nonce of the
//     task is above `stop`, and so is every nonce of every later id (ids are
//     monotone in task_lo).
//   - task_lo > seg_hi (an edge chunk's last tens digits): the task holds no
//     in-range nonce at all, and it is skipped only when seg_hi > stop.  Then
//     `stop` lies in this segment or an earlier one.  Later ids of this segment
//     start above seg_hi too and hold nothing; later segments lie wholly above
//     seg_hi > stop.  Unclamped, such a task would be skipped, and the wave
//     would leave, against a `stop` in a LATER segment, with tasks below
//     `stop` still undrawn behind it.
// Either way a wave leaves only when every id it could still draw holds no
// in-range nonce at or below `stop`.
//
// Per request the answer is exact whatever the dispatch order, because
//   1. a record is written only for an in-range, below-target, non-surplus
//      lane (take_step(WaveFirstK&), as WaveCollect's), into the request's own
//      slice through the request's own cursor,
//   2. the request's `stop` is only ever set to a value V such that k written
//      records of the request have nonce <= V, and it only decreases (atomic
//      min),
//   3. a task is skipped only if each of its in-range nonces is above `stop`;
//      a wave that leaves drops no task at or below `stop` (the ids it does
//      not draw stay in the counter for the others, and the ids nobody draws
//      lie above an id some wave skipped), so every hit <= the k-th lowest hit
//      lies in a task that ran, and it is in the slice unless cursor > cap,
//   4. if `stop` is never lowered, nothing was skipped and the slice holds
//      every hit of the launch's nonces.
// The host reads min(cursor, cap) records, sorts them by nonce and keeps the k
// lowest; cursor > cap sends the request down hm_find_k's own path
// (find_k_many.cpp).  A published maxk of MaxUint64 leaves `stop` as it is, so
// the top nonce is an ordinary record.
//
// The task decoders, the task loop and the protocol helpers below are this
// file's own copies of fused_tasks.hpp's (which hm_fused_find_kernel runs on)
// and of find_k_kernels.hip's.  On fused_tasks.hpp this kernel gives the same
// answers (88 VGPRs against 87, the same occupancy), but its rates were not
// shown to lie inside the parent's (profiles/README.md, batch_dedup/), so its
// text is held byte for byte.  A change to the walk or to the leave rule has
// to be made here too.
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

// The launch's argument block read in place from the kernarg segment (see
// fused_kernels.hip: a runtime segment index would copy a by-value parameter
// to scratch).
typedef const __attribute__((address_space(4))) FusedFindKArgs FusedFindKArgsK;
typedef const __attribute__((address_space(4))) FusedArgs FusedArgsK;

// The request's control words and its wave-side state.
struct FindKWave {
    uint64_t* ctl;
    const uint32_t* cancel;  // hm_cancel: the flag, and whether this wave relays it
    bool relay;
    WaveFirstK fk;
    uint32_t ran = 0;
};

// Before a task whose smallest nonce is task_lo: false = skip it (and leave).
// Otherwise the task's c and mx start at 0.
DEV bool fk_enter(FindKWave& w, uint64_t task_lo, uint64_t seg_hi) {
    cancel_relay(w.relay, w.cancel, w.ctl + kFkStop);
    uint64_t stop = 0;
    if (__lane_id() == 0)
        stop = __hip_atomic_load(w.ctl + kFkStop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    stop = uni64(stop);
    if ((task_lo < seg_hi ? task_lo : seg_hi) > stop) return false;
    w.fk.c = 0;
    w.fk.mx = 0;
    return true;
}
// After a task that ran: count it, publish its records in slots < k
// (find_k_publish of find_k_kernels.hip).
DEV void fk_done(FindKWave& w) {
    ++w.ran;
    if (w.fk.c && __lane_id() == 0) {
        __hip_atomic_fetch_max(w.ctl + kFkMaxk, w.fk.mx, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t old = __hip_atomic_fetch_add(w.ctl + kFkFilled, (uint64_t)w.fk.c,
                                                    __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (old + w.fk.c == w.fk.k) {
            const uint64_t v =
                __hip_atomic_load(w.ctl + kFkMaxk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(w.ctl + kFkStop, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Piece `pp` of `np` of the run [b, e): [*b2, *e2) (empty when past e).
DEV void fk_piece_of(uint32_t b, uint32_t e, uint32_t pp, uint32_t np, uint32_t* b2,
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
DEV bool fk_tiled(FusedArgsK* A, const FusedSeg& S, uint32_t k, uint32_t pp, uint32_t np,
                  FindKWave& w) {
    // task k: unit, tens digit t1 and part of the units loop (fused_tiled)
    const uint32_t per_unit = 10u * S.tpu;
    const uint32_t unit = S.unit0 + k / per_unit;
    const uint32_t rem = k - (k / per_unit) * per_unit;
    const uint32_t t1 = rem / S.tpu;
    const uint32_t part = rem - t1 * S.tpu;
    const uint32_t steps = 10u / S.tpu;
    uint32_t t0b, t0e;
    fk_piece_of(part * steps, part * steps + steps, pp, np, &t0b, &t0e);
    if (t0b >= t0e) return true;  // an empty piece (uniform)
    const uint32_t tile = unit / S.tpt;
    const uint32_t chunk = unit - tile * S.tpt;
    const uint64_t tile_base = (S.tile0 + tile) * S.pow10V;
    const uint64_t task_lo = tile_base + (uint64_t)chunk * (kWaveSize * 100u) + t1 * 10u + t0b;
    if (!fk_enter(w, task_lo, S.seg_hi)) return false;
    WaveSums sums;  // unused (CSUM = false)
    const_u32* tab = (const_u32*)(A->aux + S.aux0);
    tiled_task<W1, STRADDLE, TRAILER, false>(A->rec + (size_t)(S.rec0 + tile) * kRecWords, chunk, t1,
                                             t1 + 1, tile_base, S.seg_lo, S.seg_hi, S.vmax, S.q,
                                             S.lane_shift, S.loop_shift, tab, tab + 100, w.fk,
                                             sums, t0b, t0e);
    fk_done(w);
    return true;
}

DEV bool fk_chained(FusedArgsK* A, const FusedSeg& S, uint32_t k, uint32_t pp, uint32_t np,
                    FindKWave& w) {
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
    fk_piece_of(t_begin, t_end, pp, np, &tb, &te);
    if (tb >= te) return true;  // an empty piece (uniform)
    const uint64_t tile_base = (S.tile0 + tile) * S.pow10V;
    // lane 0's first loop value (the lanes stride pow10f beyond it)
    const uint64_t task_lo = tile_base + (uint64_t)chunk * kWaveSize * S.pow10f + tb;
    if (!fk_enter(w, task_lo, S.seg_hi)) return false;
    WaveSums sums;  // unused (CSUM = false)
    chained_task<false>(A->rec + (size_t)(S.rec0 + tile) * kRecWords, chunk, tb, te, tile_base,
                        S.pow10f, S.seg_lo, S.seg_hi, S.vmax, S.q, A->aux + S.aux0, w.fk, sums);
    fk_done(w);
    return true;
}

// Generic task k: nonces seg_lo + 640k + lane + 64j, j < 10 (a guided-tail
// piece: its share of the j), every tail block compressed per lane.  A lane
// past the segment's end (or past 2^64-1) hashes the step's first nonce again:
// a surplus lane, never a record.
DEV bool fk_generic(FusedArgsK* A, const FusedSeg& S, uint32_t k, uint32_t pp, uint32_t np,
                    FindKWave& w) {
    const uint32_t lane = __lane_id();
    const uint64_t base = S.seg_lo + (uint64_t)k * 640u;
    uint32_t jb, je;
    fk_piece_of(0, 10, pp, np, &jb, &je);
    if (jb >= je) return true;  // an empty piece (uniform)
    if (!fk_enter(w, base + 64u * jb, S.seg_hi)) return false;
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
        take_step(w.fk, in && wave_cand(w.fk, h0), h0, h1, nb0, lane, S.seg_lo, S.seg_hi, in);
    }
    fk_done(w);
    return true;
}

#define HM_FFK_CASE(W, S, T) \
    case (W) * 4 + (S) * 2 + (T): go = fk_tiled<W, S, T>(A, S_, k, pp, np, w); break;

// The argument block is the kernel's only (explicit) parameter, so it starts
// the kernarg segment.
__global__ void __launch_bounds__(kBlock) hm_fused_find_k_kernel(const FusedFindKArgs) {
    FusedFindKArgsK* P = (FusedFindKArgsK*)__builtin_amdgcn_kernarg_segment_ptr();
    FusedArgsK* A = &P->a;
    const uint32_t wslot = blockIdx.x * (kBlock / kWaveSize) + uni(threadIdx.x / kWaveSize);
    FindKWave w;
    w.ctl = P->f.ctl;
    w.cancel = P->f.cancel;
    w.relay = cancel_is_relay(w.cancel);
    w.fk.target = P->f.target;
    w.fk.thi = (uint32_t)((P->f.target - 1) >> 32);
    w.fk.cursor = P->f.ctl + kFkCursor;
    w.fk.out = P->f.out;
    w.fk.cap = P->f.cap;
    w.fk.k = P->f.k;
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
            HM_FOR_EACH_TILED_LAYOUT(HM_FFK_CASE)
            case kVarChained: go = fk_chained(A, S_, k, pp, np, w); break;
            default: go = fk_generic(A, S_, k, pp, np, w); break;
        }
        if (!go) break;
        next = 0;
        if (__lane_id() == 0) next = atomicAdd(A->counter, 1u);
    }
    if (w.ran && __lane_id() == 0)
        __hip_atomic_fetch_add(w.ctl + kFkTasksRun, (uint64_t)w.ran, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}

#undef HM_FFK_CASE

}  // namespace hm
