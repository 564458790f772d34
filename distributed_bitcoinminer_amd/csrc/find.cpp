// find.cpp -- hm_find (ABI 1.10).
// ---------------------------------------------------------------------------
// hm_find: the lowest nonce of [lo, hi] whose hash is below `target`
// (find_kernels.hip has the device protocol and its three invariants).
//
// Host side.  The range is planned with plan_range; each digit segment is
// one piece (with several devices: pieces of at most kFindPieceNonces per
// device, cut at tile boundaries and split across the devices with
// partition_range; PieceWalk).  Pieces are processed in ascending order.
// Within a piece every device walks its shard's launches (SegWalk) in
// ascending order on stream 0, at most kFindLookahead in flight: it issues
// that many, waits for them (host_wait), and reads its stop word and task
// counter back (host_read).
// A launch whose smallest nonce is above the lowest hit known so far is
// never issued, and the call ends once that holds for every launch left: a
// hit is known, and all work not yet issued lies above it.  A launch
// already in flight when a hit is published exits on its first read of the
// word.
//
// Chained segments with epochs run epoch by epoch over the same tiles, so
// their launches are not ascending: launch (e, t) starts at t * 10^V +
// e * 10^fe.  The rule is applied per launch there -- within an epoch the
// tiles above the hit are dropped, and the call ends when an epoch's first
// launch is above it -- and a task's lanes stride 10^f nonces, so a hit
// prunes only the tasks that start above it: later epochs still run the
// tasks that start below the hit (their in-range nonces above it are
// ignored by the wave's bound).  That is the loss of pruning: exactness is
// unaffected.
//
// A hit at nonce MaxUint64 cannot be told from "none" in the stop word, so
// the kernels never publish it and the host tests that one nonce itself.
//
// hm_cancel (ABI 1.18, cancel.hpp): the call is cancellable from its opening to
// its return (CancelScope).  The walk tests the context's cancel flag before it
// issues each launch and after each wait and readback, before it looks at the
// words it read -- a launch's relay wave lowers the stop word to 0 once the flag
// is set, and that word is no hit (cancel_relay.hpp has the invariant).  On
// observation the streams are drained (every launch still queued exits on its
// first read of the word) and the call returns HM_ERR_CANCELLED.
//
// The walk itself -- find_walk over FindDev, find_next_step, find_issue
// (hm_internal.hpp) and find_collect -- is shared with hm_find_k (find_k.cpp),
// which runs it over its own kernels, trailer and control words.
// ---------------------------------------------------------------------------
#include "hm_internal.hpp"

namespace hm {
// The device's next launch at or below `best`, planned but not launched.
int find_next_step(hm_ctx* ctx, Device& dv, FindDev& fd, const MsgPlan& mp, Family family,
                   uint64_t best, SegStep* step, bool* have) {
    *have = false;
    for (;;) {
        if (fd.si >= fd.segs.size()) return HM_OK;
        const SegPlan& s = fd.segs[fd.si];
        if (!fd.seg_open) {
            int rc = fd.walk.open(ctx, dv, mp, 0, s, family, kFindGenericNonces);
            if (rc) return rc;
            fd.seg_open = true;
        }
        if (s.lo > best) {  // this segment and every later one lie above the hit
            fd.si = fd.segs.size();
            return HM_OK;
        }
        uint64_t base;
        if (!fd.walk.peek_base(&base)) { ++fd.si; fd.seg_open = false; continue; }
        if (base > best) {
            // the rest of this epoch is above the hit; when its first launch
            // already is, so is every later epoch
            if (fd.walk.epoch_first()) fd.walk.close();
            else fd.walk.skip_epoch();
            continue;
        }
        fd.walk.next(step);
        *have = true;
        return HM_OK;
    }
}

// Wait for the device's launches in flight and read its control words back.
int find_collect(hm_ctx* ctx, Device& dv, FindDev& fd, FindTally& tally, const uint64_t* dev_ctl,
                 int nwords) {
    HIPCHK(hipSetDevice(dv.ordinal));
    int rc = host_wait(ctx, dv.stream[0]);
    if (rc) return rc;
    rc = host_read(ctx, fd.ctl, dev_ctl, (size_t)nwords * sizeof(uint64_t));
    if (rc) return rc;
    for (const auto& ev : fd.evs) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ev.first, ev.second));
        tally.kernel_ms += ms;
    }
    fd.evs.clear();
    dv.evnext = 0;  // the events are free again
    fd.inflight = 0;
    return HM_OK;
}

int find_core(hm_ctx* ctx, const uint8_t* m, size_t mlen, uint64_t lo, uint64_t hi, uint64_t target,
              FindTally* tally_out, hm_result* out, int* found) {
    FindTally& tally = *tally_out;
    uint64_t best = ~0ull;
    if (lo <= hi && target != 0) {
        const MsgPlan mp = plan_message(m, mlen);
        for (auto& dv : ctx->devs) {
            HIPCHK(hipSetDevice(dv.ordinal));
            dv.evnext = 0;
            // the stop word starts at MaxUint64, the task counter at 0
            HIPCHK(hipMemsetAsync(dv.find_ctl, 0xff, sizeof(uint64_t), dv.stream[0]));
            HIPCHK(hipMemsetAsync(dv.find_ctl + 1, 0, sizeof(uint64_t), dv.stream[0]));
        }
        // the per-device state dies with the call: a failure only has to
        // drain the streams (drain_failed)
        std::vector<FindDev> fds(ctx->devs.size());
        int rc = find_walk(ctx, mp, lo, hi, Family::Find, &Device::find_ctl, 2, fds, tally, &best,
                           [&](Device& dv, uint64_t launch_lo) {
                               FindArgs fa;
                               fa.word = dv.find_ctl;
                               fa.tasks_run = dv.find_ctl + 1;
                               fa.target = target;
                               fa.launch_lo = launch_lo;
                               fa.cancel = cancel_ptr(ctx, dv);
                               return fa;
                           });
        if (rc) return rc;
        for (const FindDev& fd : fds) tally.run += fd.ctl[1];
    }
    hm_result res{~0ull, 0};
    int hit = 0;
    if (lo <= hi && target != 0) {
        // nonce MaxUint64 is the one the stop word cannot carry: tested here
        if (best != ~0ull || (hi == ~0ull && host_hash(m, mlen, ~0ull) < target)) {
            res.nonce = best;
            res.hash = host_hash(m, mlen, best);
            if (res.hash >= target || best < lo || best > hi) return HM_ERR_INTERNAL;
            hit = 1;
        }
    }
    *out = res;
    *found = hit;
    return HM_OK;
}

// hm_find with ctx->mu held.
int find_locked(hm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
                uint64_t target, hm_result* out, int* found) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint8_t* m;
    size_t mlen;
    int rc = begin_ranged_call(ctx, msg, len, lo, hi, t0, &m, &mlen);
    if (rc) return rc;
    CancelScope cancel(ctx, HM_CANCEL_FAMILY_FIND);
    FindTally tally;
    hm_result res;
    int hit = 0;
    rc = find_core(ctx, m, mlen, lo, hi, target, &tally, &res, &hit);
    if (rc) return cancel.end(rc);
    hm_find_stats st{};
    st.kernel_ms = tally.kernel_ms;
    st.nonces_enqueued = tally.nonces;
    st.tasks_total = tally.tasks;
    st.tasks_run = tally.run;
    st.launches = tally.launches;
    st.found = hit;
    publish(ctx, ctx->find_stats, st, t0);
    *out = res;
    *found = hit;
    return HM_OK;
}

}  // namespace hm
