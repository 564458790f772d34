// find_k.cpp -- hm_find_k (ABI 1.16).
// ---------------------------------------------------------------------------
// hm_find_k: the k lowest nonces of [lo, hi] whose hash is below `target`
// (find_k_kernels.hip has the device protocol and its four invariants).
//
// Host side.  hm_find's walk (find_walk, hm_internal.hpp; find.cpp has its
// rules): pieces in ascending order, within a piece every device walks
// its shard's launches in ascending order on stream 0, at most kFindLookahead
// in flight, and after each batch its control words are read back.  The
// pruning bound is the minimum of the devices' stop words: a device lowers its
// word to V only when k records with nonce <= V are written in its own shard,
// so any device's word bounds the k-th lowest hit of the whole range.
// Launches, epochs, segments and pieces above the bound are never issued, and
// the call ends when nothing unissued lies below it.  Each device seeks k hits
// in its own shard; the host reads every device's min(cursor, B) records,
// checks them as hm_collect does (distinct, in range, below target), sorts the
// union by nonce and keeps the k lowest.
//
// Overflow.  The record buffer holds B >= k records (default min(
// HM_COLLECT_CAP_MAX, 2k + 4096); HM_OPT_FIND_K_BUF).  At a dense target the
// tasks in flight when the stop word drops can hold more than B - k hits; then
// cursor > B on some device and records <= the k-th hit may be missing.  The
// early exit still worked -- the slots below k always exist -- so the answer
// lies in [lo, min(bound, hi)], and it is taken exactly from collect_core over
// ascending windows of that range: each sized from target / 2^64 and the hits
// still missing, halved when its total exceeds its cap, until k hits are in
// hand or the range is done.
//
// hm_cancel (ABI 1.18): as hm_find (find.cpp) -- the walk tests the cancel flag
// before each launch and after each readback, before the control words count
// for anything (a relay wave's stop = 0 is not "k records at or below 0"); the
// overflow path tests it between windows.
// ---------------------------------------------------------------------------
#include "hm_internal.hpp"

namespace hm {
namespace {

// The k lowest hits of [lo, hi] through hm_collect's path, window by window.
int find_k_windows(hm_ctx* ctx, const uint8_t* m, size_t mlen, uint64_t lo, uint64_t hi,
                   uint64_t target, size_t k, CollectTally* tally, std::vector<hm_result>* recs) {
    const size_t cap = std::min<size_t>(HM_COLLECT_CAP_MAX, 2 * k + 4096);
    const double p = (double)target / 18446744073709551616.0;  // hits per nonce
    recs->clear();
    uint64_t a = lo;
    uint64_t span = 0;  // the next window's nonces; 0: size it from p
    std::vector<hm_result> win;
    for (;;) {
        // hm_cancel: the collect kernels have no relay, so the flag is tested between windows
        // (the last one has ended: nothing is in flight)
        if (cancel_seen(ctx)) return cancel_observed(ctx, 0);
        if (span == 0) {
            // about 16 hits more than are missing, so one window usually ends the call
            const double want = ((double)(k - recs->size()) + 16.0) / p;
            span = want >= 9.0e18 ? ~0ull : std::max<uint64_t>((uint64_t)want, 64);
        }
        const uint64_t b = hi - a < span - 1 ? hi : a + (span - 1);
        uint64_t total = 0;
        int rc = collect_core(ctx, m, mlen, a, b, target, cap, tally, &win, &total);
        if (rc) return rc;
        if (total > cap) {  // denser than expected: the same start, half the nonces
            span = std::max<uint64_t>((b - a + 1) / 2, 1);
            continue;
        }
        const size_t take = std::min<size_t>(win.size(), k - recs->size());
        recs->insert(recs->end(), win.begin(), win.begin() + take);
        if (recs->size() == k || b == hi) return HM_OK;
        a = b + 1;
        span = 0;
    }
}

}  // namespace

// hm_find_k without its opening and its stats (hm_find_k_many's fallback
// takes this path too).
int find_k_core(hm_ctx* ctx, const uint8_t* m, size_t mlen, uint64_t lo, uint64_t hi,
                uint64_t target, size_t k, FindKTally* out, std::vector<hm_result>* recs) {
    int rc = HM_OK;
    const int ndev = (int)ctx->devs.size();
    FindTally& tally = out->t;
    uint64_t records = 0;
    bool overflow = false;
    uint64_t best = ~0ull;
    recs->clear();
    if (lo <= hi && target != 0) {
        const size_t B = ctx->find_k_buf ? std::max<size_t>(ctx->find_k_buf, k)
                                         : std::min<size_t>(HM_COLLECT_CAP_MAX, 2 * k + 4096);
        const MsgPlan mp = plan_message(m, mlen);
        for (auto& dv : ctx->devs) {
            HIPCHK(hipSetDevice(dv.ordinal));
            dv.evnext = 0;
            rc = collect_buffer(dv, B);
            if (rc) return rc;
            rc = ctl_block(&dv.find_k_ctl, kFkWords);
            if (rc) return rc;
            // the stop word starts at MaxUint64, the other four words at 0
            static_assert(kFkStop == 0, "the stop word is the first of the control words");
            HIPCHK(hipMemsetAsync(dv.find_k_ctl, 0xff, sizeof(uint64_t), dv.stream[0]));
            HIPCHK(hipMemsetAsync(dv.find_k_ctl + 1, 0, (kFkWords - 1) * sizeof(uint64_t),
                                  dv.stream[0]));
        }
        // the per-device state dies with the call: a failure only has to
        // drain the streams (drain_failed)
        std::vector<FindDev> fds(ndev);
        rc = find_walk(ctx, mp, lo, hi, Family::FindK, &Device::find_k_ctl, kFkWords, fds, tally,
                       &best, [&](Device& dv, uint64_t launch_lo) {
                           FindKArgs ka;
                           ka.ctl = dv.find_k_ctl;
                           ka.out = dv.collect_buf;
                           ka.target = target;
                           ka.launch_lo = launch_lo;
                           ka.cap = (uint32_t)B;
                           ka.k = (uint32_t)k;
                           ka.cancel = cancel_ptr(ctx, dv);
                           return ka;
                       });
        if (rc) return rc;
        // every stream is idle: the records of every device
        for (int i = 0; i < ndev; ++i) {
            const uint64_t cursor = fds[i].ctl[kFkCursor];
            tally.run += fds[i].ctl[kFkTasksRun];
            if (cursor > B) overflow = true;
            const size_t have = (size_t)std::min<uint64_t>(cursor, B);
            records += have;
            if (!have || overflow) continue;
            Device& dv = ctx->devs[i];
            HIPCHK(hipSetDevice(dv.ordinal));
            const size_t at = recs->size();
            recs->resize(at + have);
            rc = host_read(ctx, recs->data() + at, dv.collect_buf, have * sizeof(hm_result));
            if (rc) return rc;
        }
        CollectTally ct;
        if (overflow) {
            rc = find_k_windows(ctx, m, mlen, lo, std::min(best, hi), target, k, &ct, recs);
            if (rc) return rc;
            tally.nonces += ct.nonces;
            tally.launches += ct.launches;
            tally.kernel_ms += ct.kernel_ms;
        } else {
            rc = sort_check_records(recs, lo, hi, target);
            if (rc) return rc;
            if (recs->size() > k) recs->resize(k);
            // a lowered stop word promises k records at or below it
            if (best != ~0ull && (recs->size() < k || recs->back().nonce > best))
                return HM_ERR_INTERNAL;
        }
    }
    out->records += records;
    out->overflow = out->overflow || overflow;
    return HM_OK;
}

// hm_find_k with ctx->mu held.
int find_k_locked(hm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
                  uint64_t target, size_t k, std::vector<hm_result>* recs) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint8_t* m;
    size_t mlen;
    int rc = begin_ranged_call(ctx, msg, len, lo, hi, t0, &m, &mlen);
    if (rc) return rc;
    CancelScope cancel(ctx, HM_CANCEL_FAMILY_FIND_K);
    FindKTally kt;
    rc = find_k_core(ctx, m, mlen, lo, hi, target, k, &kt, recs);
    if (rc) return cancel.end(rc);
    const FindTally& tally = kt.t;
    hm_find_k_stats st{};
    st.kernel_ms = tally.kernel_ms;
    st.nonces_enqueued = tally.nonces;
    st.tasks_total = tally.tasks;
    st.tasks_run = tally.run;
    st.records = kt.records;
    st.launches = tally.launches;
    st.found = (int32_t)recs->size();
    st.fallback = kt.overflow ? 1 : 0;
    publish(ctx, ctx->find_k_stats, st, t0);
    return HM_OK;
}

}  // namespace hm
