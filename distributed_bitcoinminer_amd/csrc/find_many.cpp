// find_many.cpp -- hm_find_many (ABI 1.13).
// ---------------------------------------------------------------------------
// hm_find_many: hm_find's answer for each of a batch of requests
// (fused_find_kernels.hip has the device protocol and its three invariants).
//
// Host side, per chunk of at most kMaxBatch requests (BatchChunk, batch.cpp,
// plans, launches and reads back; this file has what is hm_find's):
//   window    request r's window is [lo, min(hi, lo + W - 1)], W =
//             kFusedNonces (HM_OPT_FIND_WINDOW: a test hook); the longest
//             ascending prefix of its segments that one launch can hold is
//             fused.
//   launch    the planner's `result` seed (MaxUint64, 0) is pointed at the
//             request's (stop word, tasks run) pair, then hm_fused_find_kernel.
//             No fold: the word is the answer.
//   readback  one host_read of the pairs per device.  A hit's hash is
//             recomputed (host_hash) and must qualify, as in find_core.
//   fallback  a request without a hit whose range goes on past what was fused
//             continues from the first nonce not fused through find_core (the
//             per-segment path of hm_find), one request after another.
//             HM_OPT_FUSED = 0 sends every request there.
// A hit at nonce MaxUint64 cannot be told from "none" in the stop word: the
// kernel never publishes it and the host tests that one nonce itself.
//
// hm_cancel (ABI 1.18): every fused launch has a relay wave (the planner
// re-seeds each request's word, each launch's relay lowers it again), so a
// signalled chunk ends by itself; the host tests the cancel flag after the
// chunk's wait and readback, before any word is looked at, and find_core tests
// it before each leftover's first launch (find_walk).
// ---------------------------------------------------------------------------
#include "hm_internal.hpp"

namespace hm {
namespace {

int find_chunk(hm_ctx* ctx, const hm_find_request* reqs, int n, int index0, hm_result* outs,
               int* found, hm_find_many_stats* st) {
    BatchChunk C(ctx, index0, ctx->find_window, false);
    for (int r = 0; r < n; ++r) {
        const hm_find_request& q = reqs[r];
        C.add(q.msg, q.len, q.lo, q.hi, q.target);
        outs[r] = hm_result{~0ull, 0};
        found[r] = 0;
    }
    int rc = C.prepare(&Device::find_many_ctl, (size_t)kMaxBatch * 2);
    if (rc) return rc;
    static const KernelName name = kernel_name(Family::Find, HM_KIND_FUSED, nullptr);
    FindTally fused;
    rc = C.launch<FusedFindArgs>(
        name, &fused,
        [&](int r, const BatchReq&, Device& dv, hipStream_t, FusedLaunch* fl, FusedFindArgs* ka) {
            fl->pa.result = dv.find_many_ctl + 2 * r;
            ka->f.word = dv.find_many_ctl + 2 * r;
            ka->f.tasks_run = dv.find_many_ctl + 2 * r + 1;
            ka->f.target = reqs[r].target;
            ka->f.launch_lo = reqs[r].lo;
            ka->f.cancel = cancel_ptr(ctx, dv);
            return HM_OK;
        });
    if (!rc) rc = C.finish(&Device::find_many_ctl, (size_t)2 * n, &fused);
    if (rc) return rc;
    // hm_cancel: after the wait and the readback, before any word is looked at
    if (cancel_seen(ctx)) return cancel_observed(ctx, fused.launches);
    st->nonces_enqueued += fused.nonces;
    st->tasks_total += fused.tasks;
    st->launches += fused.launches;
    st->kernel_ms += fused.kernel_ms;
    for (int r = 0; r < n; ++r) {
        const hm_find_request& q = reqs[r];
        const BatchReq& R = C.rq[r];
        if (!R.live) continue;
        uint64_t from = q.lo;
        if (R.launched) {
            st->tasks_run += C.ctl[R.dev][2 * r + 1];
            uint64_t best = C.ctl[R.dev][2 * r];
            // nonce MaxUint64 is the one the stop word cannot carry: tested here
            const bool at_max = best == ~0ull && R.fused_hi == ~0ull &&
                                host_hash(R.m, R.mlen, ~0ull) < q.target;
            if (best != ~0ull || at_max) {
                const uint64_t h = host_hash(R.m, R.mlen, best);
                if (h >= q.target || best < q.lo || best > R.fused_hi) return HM_ERR_INTERNAL;
                outs[r] = hm_result{h, best};
                found[r] = 1;
            }
            if (found[r] || R.fused_hi == q.hi) {
                ++st->fused;
                continue;
            }
            from = R.fused_hi + 1;
        }
        FindTally tally;
        rc = find_core(ctx, R.m, R.mlen, from, q.hi, q.target, &tally, &outs[r], &found[r]);
        if (rc) return rc;
        ++st->fallback;
        st->nonces_enqueued += tally.nonces;
        st->tasks_total += tally.tasks;
        st->tasks_run += tally.run;
        st->launches += tally.launches;
        st->kernel_ms += tally.kernel_ms;
    }
    return HM_OK;
}

}  // namespace

// hm_find_many with ctx->mu held.
int find_many_locked(hm_ctx* ctx, const hm_find_request* reqs, int n, hm_result* outs, int* found) {
    const auto t0 = std::chrono::steady_clock::now();
    int rc = batch_open(ctx, reqs, n, t0);
    if (rc) return rc;
    CancelScope cancel(ctx, HM_CANCEL_FAMILY_FIND_MANY);
    hm_find_many_stats st{};
    for (int c = 0; c < n; c += kMaxBatch) {
        const int m = std::min(kMaxBatch, n - c);
        // hm_cancel: nothing is in flight between chunks
        rc = cancel_seen(ctx) ? cancel_observed(ctx, 0)
                              : find_chunk(ctx, reqs + c, m, c, outs + c, found + c, &st);
        if (rc) return cancel.end(drain_streams(ctx, rc));
    }
    for (int r = 0; r < n; ++r) st.found += found[r];
    st.requests = n;
    publish(ctx, ctx->find_many_stats, st, t0);
    return HM_OK;
}

}  // namespace hm
