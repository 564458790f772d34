// collect_many.cpp -- hm_collect_many (ABI 1.15).
// ---------------------------------------------------------------------------
// hm_collect_many: hm_collect's answer for each of a batch of requests
// (fused_collect_kernels.hip has the device protocol and its three
// invariants).
//
// Host side, per chunk of at most kMaxBatch requests (BatchChunk, batch.cpp,
// plans, launches and reads back; this file has what is hm_collect's):
//   plan      a live request (lo <= hi, target != 0) of at most W nonces (W =
//             kFusedNonces; HM_OPT_COLLECT_WINDOW: a test hook) whose segments
//             fusible() accepts, ALL of them, is fused; its segments are put
//             in fused_order (costliest first, as the fused scan).  Any other
//             live request takes the fallback whole: there is no early exit,
//             so a fused prefix would buy nothing.
//   enqueue   the planner's `acc` (one word) is pointed at the request's total
//             word, which it zeroes, then hm_fused_collect_kernel.  The
//             device's one slot cursor is zeroed once per chunk on stream 0, an event is
//             recorded behind that, and every other stream the chunk uses
//             waits on the event before its first launch (the previous chunk
//             has been waited for by then).
//   readback  one host_read of the cursor and the total words per device and,
//             while the call's running sum still fits `cap`, one of `cursor`
//             records and one of their tags.  Once the running sum exceeds
//             `cap` the call has overflowed: later chunks and fallbacks run as
//             counts (cap = 0, no buffers).
//   fallback  the unfused requests run through collect_core (the per-segment
//             path of hm_collect), one after another, after the chunk's
//             readback: it uses the same record buffer.  HM_OPT_FUSED = 0
//             sends every request there.
//   assemble  the records are grouped by tag, each group sorted by nonce and
//             checked as collect_core checks its own: distinct, in range,
//             below the target; and each group's size is its request's total,
//             and a device whose records fit has cursor = the sum of its
//             totals.
// ---------------------------------------------------------------------------
#include "hm_internal.hpp"

namespace hm {
namespace {

// What the call has gathered so far.
struct Gather {
    size_t cap;
    bool overflow = false;  // the running sum exceeds cap: counts only from here on
    uint64_t sum = 0;
    std::vector<uint64_t>* totals;
    std::vector<std::vector<hm_result>> recs;  // per request, until the call overflows

    // Request i's total is known: false once the sum has wrapped.
    bool add(size_t i, uint64_t t) {
        (*totals)[i] = t;
        if (sum + t < sum) return false;
        sum += t;
        if (sum > cap && !overflow) {
            overflow = true;
            recs.clear();
            recs.shrink_to_fit();
        }
        return true;
    }
};

int collect_chunk(hm_ctx* ctx, const hm_collect_request* reqs, int n, int index0, Gather* G,
                  hm_collect_many_stats* st) {
    const int ndev = (int)ctx->devs.size();
    // the chunk's launches record only while the call's records still fit
    const size_t cap = G->overflow ? 0 : G->cap;
    BatchChunk C(ctx, index0, ctx->collect_window, true);
    for (int r = 0; r < n; ++r) {
        const hm_collect_request& q = reqs[r];
        C.add(q.msg, q.len, q.lo, q.hi, q.target);
    }
    int rc = C.prepare(&Device::collect_many_ctl, (size_t)kMaxBatch + 1);
    if (rc) return rc;
    for (int i = 0; i < ndev; ++i) {
        Device& dv = ctx->devs[i];
        if (!C.nfused[i]) continue;
        HIPCHK(hipSetDevice(dv.ordinal));
        rc = collect_buffer(dv, cap);
        if (rc) return rc;
        rc = grow_buffer(dv, &dv.collect_tags, &dv.collect_tags_cap, cap, HM_COLLECT_CAP_MAX,
                         sizeof(uint32_t));
        if (rc) return rc;
        // the cursor starts at 0 before any launch of the chunk, on any stream
        HIPCHK(hipMemsetAsync(dv.collect_many_ctl, 0, sizeof(uint64_t), dv.stream[0]));
        if (C.used(i) > 1) {
            hipEvent_t zeroed;
            rc = next_event(dv, &zeroed);
            if (rc) return rc;
            HIPCHK(hipEventRecord(zeroed, dv.stream[0]));
            for (int s = 1; s < C.used(i); ++s) HIPCHK(hipStreamWaitEvent(dv.stream[s], zeroed, 0));
        }
    }
    static const KernelName name = kernel_name(Family::Collect, HM_KIND_FUSED, nullptr);
    FindTally fused;
    rc = C.launch<FusedCollectArgs>(
        name, &fused,
        [&](int r, const BatchReq&, Device& dv, hipStream_t, FusedLaunch* fl, FusedCollectArgs* ka) {
            // the planner zeroes the request's total word
            fl->pa.acc = dv.collect_many_ctl + 1 + r;
            fl->pa.n_acc = 1;
            ka->k.total = dv.collect_many_ctl + 1 + r;
            ka->k.cursor = dv.collect_many_ctl;
            ka->k.out = cap ? dv.collect_buf : nullptr;
            ka->k.target = reqs[r].target;
            ka->k.cap = (uint32_t)cap;
            ka->tags = cap ? dv.collect_tags : nullptr;
            ka->request = (uint32_t)r;
            return HM_OK;
        });
    if (!rc) rc = C.finish(&Device::collect_many_ctl, (size_t)n + 1, &fused);
    if (rc) return rc;
    st->nonces += fused.nonces;
    st->tasks += fused.tasks;
    st->launches += fused.launches;
    st->fused += fused.launches;  // a fused request is one launch and needs nothing more
    st->kernel_ms += fused.kernel_ms;
    const std::vector<BatchReq>& rq = C.rq;
    const std::vector<std::vector<uint64_t>>& ctl = C.ctl;
    // the fused requests' totals, device by device, and their records
    std::vector<uint64_t> dev_sum(ndev, 0);
    for (int r = 0; r < n; ++r) {
        const BatchReq& R = rq[r];
        if (!R.launched) continue;
        const uint64_t t = ctl[R.dev][1 + r];
        if (dev_sum[R.dev] + t < dev_sum[R.dev]) return HM_ERR_INTERNAL;
        dev_sum[R.dev] += t;
    }
    for (int r = 0; r < n; ++r) {
        const BatchReq& R = rq[r];
        if (!R.live) { G->add((size_t)index0 + r, 0); continue; }
        if (R.launched && !G->add((size_t)index0 + r, ctl[R.dev][1 + r])) return HM_ERR_INTERNAL;
    }
    for (int i = 0; i < ndev && cap; ++i) {
        if (!C.nfused[i]) continue;
        // a device whose records all fit reserved exactly one slot per hit
        if (dev_sum[i] <= cap && ctl[i][0] != dev_sum[i]) return HM_ERR_INTERNAL;
        if (G->overflow || dev_sum[i] == 0) continue;
        Device& dv = ctx->devs[i];
        HIPCHK(hipSetDevice(dv.ordinal));
        const size_t cnt = (size_t)dev_sum[i];  // <= cap: the call's sum still fits
        std::vector<hm_result> got(cnt);
        std::vector<uint32_t> tag(cnt);
        rc = host_read(ctx, got.data(), dv.collect_buf, cnt * sizeof(hm_result));
        if (rc) return rc;
        rc = host_read(ctx, tag.data(), dv.collect_tags, cnt * sizeof(uint32_t));
        if (rc) return rc;
        for (size_t k = 0; k < cnt; ++k) {
            const uint32_t r = tag[k];
            if (r >= (uint32_t)n || !rq[r].launched || rq[r].dev != i) return HM_ERR_INTERNAL;
            G->recs[(size_t)index0 + r].push_back(got[k]);
        }
    }
    for (int r = 0; r < n && !G->overflow; ++r) {
        if (!rq[r].launched) continue;
        std::vector<hm_result>& v = G->recs[(size_t)index0 + r];
        if (v.size() != (*G->totals)[(size_t)index0 + r]) return HM_ERR_INTERNAL;
        rc = sort_check_records(&v, reqs[r].lo, reqs[r].hi, reqs[r].target);
        if (rc) return rc;
    }
    // what was not fused: hm_collect's path, whole, one request after another
    for (int r = 0; r < n; ++r) {
        const hm_collect_request& q = reqs[r];
        const BatchReq& R = rq[r];
        if (!R.live || R.launched) continue;
        CollectTally tally;
        std::vector<hm_result> recs;
        uint64_t t = 0;
        rc = collect_core(ctx, R.m, R.mlen, q.lo, q.hi, q.target, G->overflow ? 0 : G->cap,
                          &tally, &recs, &t);
        if (rc) return rc;
        if (!G->add((size_t)index0 + r, t)) return HM_ERR_INTERNAL;
        if (!G->overflow) G->recs[(size_t)index0 + r] = std::move(recs);
        ++st->fallback;
        st->nonces += tally.nonces;
        st->launches += tally.launches;
        st->kernel_ms += tally.kernel_ms;
    }
    return HM_OK;
}

}  // namespace

// hm_collect_many with ctx->mu held.
int collect_many_locked(hm_ctx* ctx, const hm_collect_request* reqs, int n, size_t cap,
                        std::vector<uint64_t>* totals, std::vector<hm_result>* recs,
                        uint64_t* total) {
    const auto t0 = std::chrono::steady_clock::now();
    int rc = batch_open(ctx, reqs, n, t0);
    if (rc) return rc;
    hm_collect_many_stats st{};
    totals->assign((size_t)n, 0);
    recs->clear();
    Gather G;
    G.cap = cap;
    G.totals = totals;
    G.recs.resize((size_t)n);
    for (int c = 0; c < n; c += kMaxBatch) {
        const int m = std::min(kMaxBatch, n - c);
        rc = collect_chunk(ctx, reqs + c, m, c, &G, &st);
        if (rc) return drain_streams(ctx, rc);
    }
    if (!G.overflow) {
        recs->reserve((size_t)G.sum);
        for (const auto& v : G.recs) recs->insert(recs->end(), v.begin(), v.end());
        if (recs->size() != G.sum) return HM_ERR_INTERNAL;
    }
    st.total = G.sum;
    st.overflow = G.overflow ? 1 : 0;
    st.requests = n;
    publish(ctx, ctx->collect_many_stats, st, t0);
    *total = G.sum;
    return HM_OK;
}

}  // namespace hm
