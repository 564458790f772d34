// collect_many.cpp -- hm_collect_many (ABI 1.15).
// ---------------------------------------------------------------------------
// hm_collect_many: hm_collect's answer for each of a batch of requests
// (fused_collect_kernels.hip has the device protocol and its three
// invariants).
//
// Host side, per chunk of at most kMaxBatch requests:
//   plan      a live request (lo <= hi, target != 0) of at most W nonces (W =
//             kFusedNonces; HM_OPT_COLLECT_WINDOW: a test hook) whose segments
//             fusible() accepts, ALL of them, is fused; its segments are put
//             in fused_order (costliest first, as the fused scan).  Any other
//             live request takes the fallback whole: there is no early exit,
//             so a fused prefix would buy nothing.
//   enqueue   request r goes whole to device r mod ndev and round-robins over
//             that device's streams; per request hm_fused_plan_kernel --
//             records, tables, the queue counter, and its `acc` (one word)
//             pointed at the request's total word, which it zeroes -- then
//             hm_fused_collect_kernel between two events.  The device's one
//             slot cursor is zeroed once per chunk on stream 0, an event is
//             recorded behind that, and every other stream the chunk uses
//             waits on the event before its first launch (the previous chunk
//             has been waited for by then).
//   readback  every request of the chunk is enqueued on every device before
//             the host waits on any: one host_wait per used stream, one
//             host_read of the cursor and the total words per device and,
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

// One request of a chunk.
struct Req {
    const uint8_t* m;
    size_t mlen;
    bool live = false;      // lo <= hi and target != 0: something to hash
    bool launched = false;  // its fused launch was enqueued
    int dev = 0;
    hipEvent_t a = nullptr, b = nullptr;
};

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

// Make dv's tag buffer hold `cap` tags, grown as collect_buffer grows the
// record buffer.
int tag_buffer(Device& dv, size_t cap) {
    if (cap <= dv.collect_tags_cap) return HM_OK;
    const size_t want =
        std::min<size_t>(std::max(cap, 2 * dv.collect_tags_cap), HM_COLLECT_CAP_MAX);
    uint32_t* b = nullptr;
    if (hipMalloc(&b, want * sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();
        return HM_ERR_NOMEM;
    }
    if (dv.collect_tags) dv.retired.push_back(dv.collect_tags);
    dv.collect_tags = b;
    dv.collect_tags_cap = want;
    return HM_OK;
}

// The records of one request, as they came: sorted by nonce, then checked.
int check_sorted(std::vector<hm_result>* recs, const hm_collect_request& q, uint64_t total) {
    if (recs->size() != total) return HM_ERR_INTERNAL;
    std::sort(recs->begin(), recs->end(),
              [](const hm_result& x, const hm_result& y) { return x.nonce < y.nonce; });
    for (size_t i = 0; i < recs->size(); ++i) {
        const hm_result& r = (*recs)[i];
        if (r.hash >= q.target || r.nonce < q.lo || r.nonce > q.hi ||
            (i > 0 && r.nonce == (*recs)[i - 1].nonce))
            return HM_ERR_INTERNAL;
    }
    return HM_OK;
}

int collect_chunk(hm_ctx* ctx, const hm_collect_request* reqs, int n, int index0, Gather* G,
                  hm_collect_many_stats* st) {
    static const uint8_t empty_msg = 0;
    const int ndev = (int)ctx->devs.size();
    const uint64_t W = ctx->collect_window ? ctx->collect_window : kFusedNonces;
    const int nstreams = std::max(1, std::min(ctx->streams, kStreams));
    // the chunk's launches record only while the call's records still fit
    const size_t cap = G->overflow ? 0 : G->cap;
    std::vector<Req> rq(n);
    std::vector<MsgPlan> mps(n);
    std::vector<std::vector<SegPlan>> segs(n);
    std::vector<int> nfused(ndev, 0);
    for (int r = 0; r < n; ++r) {
        const hm_collect_request& q = reqs[r];
        Req& R = rq[r];
        R.m = q.msg ? q.msg : &empty_msg;
        R.mlen = q.msg ? q.len : 0;
        R.live = q.lo <= q.hi && q.target != 0;
        R.dev = (index0 + r) % ndev;
        if (!R.live || !ctx->fused || q.hi - q.lo > W - 1) continue;
        mps[r] = plan_message(R.m, R.mlen);
        segs[r] = plan_range(mps[r], q.lo, q.hi, ctx->force_generic, ctx->table_digits);
        // all of its segments in one launch, or none
        if (!fusible(segs[r])) { segs[r].clear(); continue; }
        fused_order(&segs[r]);
        ++nfused[R.dev];
    }
    for (int i = 0; i < ndev; ++i) {
        Device& dv = ctx->devs[i];
        if (!nfused[i]) continue;
        HIPCHK(hipSetDevice(dv.ordinal));
        if (!dv.collect_many_ctl)
            HIPCHK(hipMalloc(&dv.collect_many_ctl, (size_t)(kMaxBatch + 1) * sizeof(uint64_t)));
        int rc = collect_buffer(dv, cap);
        if (rc) return rc;
        rc = tag_buffer(dv, cap);
        if (rc) return rc;
        const int used = std::min(nstreams, nfused[i]);
        rc = make_streams(dv, used);
        if (rc) return rc;
        // the cursor starts at 0 before any launch of the chunk, on any stream
        HIPCHK(hipMemsetAsync(dv.collect_many_ctl, 0, sizeof(uint64_t), dv.stream[0]));
        if (used > 1) {
            hipEvent_t zeroed;
            rc = next_event(dv, &zeroed);
            if (rc) return rc;
            HIPCHK(hipEventRecord(zeroed, dv.stream[0]));
            for (int s = 1; s < used; ++s) HIPCHK(hipStreamWaitEvent(dv.stream[s], zeroed, 0));
        }
    }
    static const KernelName name = kernel_name(Family::Collect, HM_KIND_FUSED, nullptr);
    std::vector<int> rr(ndev, 0);
    for (int r = 0; r < n; ++r) {
        if (segs[r].empty()) continue;
        Req& R = rq[r];
        Device& dv = ctx->devs[R.dev];
        HIPCHK(hipSetDevice(dv.ordinal));
        const int si = rr[R.dev]++ % std::min(nstreams, nfused[R.dev]);
        hipStream_t s = dv.stream[si];
        FusedCollectArgs ka;
        FusedLaunch fl;
        int rc = plan_fused(ctx, dv, mps[r], segs[r], si, kFusedStaticFirst, &fl);
        if (rc) return rc;
        // the planner zeroes the request's total word
        fl.pa.acc = dv.collect_many_ctl + 1 + r;
        fl.pa.n_acc = 1;
        ka.a = fl.fa;
        ka.k.total = dv.collect_many_ctl + 1 + r;
        ka.k.cursor = dv.collect_many_ctl;
        ka.k.out = cap ? dv.collect_buf : nullptr;
        ka.k.target = reqs[r].target;
        ka.k.cap = (uint32_t)cap;
        ka.tags = cap ? dv.collect_tags : nullptr;
        ka.request = (uint32_t)r;
        const Device::Fn* fn = nullptr;
        rc = scan_fn(dv, name.symbol, &fn);
        if (rc) return rc;
        rc = next_event(dv, &R.a);
        if (rc) return rc;
        rc = next_event(dv, &R.b);
        if (rc) return rc;
        HIPCHK(launch_fused_plan(fl.pa, s));
        HIPCHK(hipEventRecord(R.a, s));
        rc = launch_scan(*fn, ka, fl.grid, s);
        if (rc) return rc;
        HIPCHK(hipEventRecord(R.b, s));
        R.launched = true;
        st->nonces += fl.nonces;
        st->tasks += fl.fa.ntasks;
        ++st->launches;
    }
    // every device's work is queued: wait, then one read of the words each
    std::vector<std::vector<uint64_t>> ctl(ndev);
    for (int i = 0; i < ndev; ++i) {
        Device& dv = ctx->devs[i];
        if (!nfused[i]) continue;
        HIPCHK(hipSetDevice(dv.ordinal));
        for (int s = 0; s < std::min(nstreams, nfused[i]); ++s) {
            int rc = host_wait(ctx, dv.stream[s]);
            if (rc) return rc;
        }
        ctl[i].resize((size_t)n + 1);
        int rc = host_read(ctx, ctl[i].data(), dv.collect_many_ctl, ctl[i].size() * sizeof(uint64_t));
        if (rc) return rc;
    }
    for (int r = 0; r < n; ++r) {
        const Req& R = rq[r];
        if (!R.launched) continue;
        float ms = 0.f;
        HIPCHK(hipSetDevice(ctx->devs[R.dev].ordinal));
        HIPCHK(hipEventElapsedTime(&ms, R.a, R.b));
        st->kernel_ms += ms;
        ++st->fused;
    }
    for (Device& dv : ctx->devs) dv.evnext = 0;  // the events are free again
    // the fused requests' totals, device by device, and their records
    std::vector<uint64_t> dev_sum(ndev, 0);
    for (int r = 0; r < n; ++r) {
        const Req& R = rq[r];
        if (!R.launched) continue;
        const uint64_t t = ctl[R.dev][1 + r];
        if (dev_sum[R.dev] + t < dev_sum[R.dev]) return HM_ERR_INTERNAL;
        dev_sum[R.dev] += t;
    }
    for (int r = 0; r < n; ++r) {
        const Req& R = rq[r];
        if (!R.live) { G->add((size_t)index0 + r, 0); continue; }
        if (R.launched && !G->add((size_t)index0 + r, ctl[R.dev][1 + r])) return HM_ERR_INTERNAL;
    }
    for (int i = 0; i < ndev && cap; ++i) {
        if (!nfused[i]) continue;
        // a device whose records all fit reserved exactly one slot per hit
        if (dev_sum[i] <= cap && ctl[i][0] != dev_sum[i]) return HM_ERR_INTERNAL;
        if (G->overflow || dev_sum[i] == 0) continue;
        Device& dv = ctx->devs[i];
        HIPCHK(hipSetDevice(dv.ordinal));
        const size_t cnt = (size_t)dev_sum[i];  // <= cap: the call's sum still fits
        std::vector<hm_result> got(cnt);
        std::vector<uint32_t> tag(cnt);
        int rc = host_read(ctx, got.data(), dv.collect_buf, cnt * sizeof(hm_result));
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
        int rc = check_sorted(&G->recs[(size_t)index0 + r], reqs[r], (*G->totals)[(size_t)index0 + r]);
        if (rc) return rc;
    }
    // what was not fused: hm_collect's path, whole, one request after another
    for (int r = 0; r < n; ++r) {
        const hm_collect_request& q = reqs[r];
        const Req& R = rq[r];
        if (!R.live || R.launched) continue;
        CollectTally tally;
        std::vector<hm_result> recs;
        uint64_t t = 0;
        int rc = collect_core(ctx, R.m, R.mlen, q.lo, q.hi, q.target, G->overflow ? 0 : G->cap,
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
    // an abandoned context's devices may still run its timed-out work
    if (ctx->abandoned) return HM_ERR_TIMEOUT;
    {
        // auto: the floor once, the slack times every request's whole range
        std::vector<hm_request> whole(n);
        for (int r = 0; r < n; ++r)
            whole[r] = hm_request{reqs[r].msg, reqs[r].msg ? reqs[r].len : 0, reqs[r].lo, reqs[r].hi};
        call_deadline(ctx, whole.data(), n, t0);
    }
    hm_collect_many_stats st{};
    totals->assign((size_t)n, 0);
    recs->clear();
    Gather G;
    G.cap = cap;
    G.totals = totals;
    G.recs.resize((size_t)n);
    for (Device& dv : ctx->devs) dv.evnext = 0;
    for (int c = 0; c < n; c += kMaxBatch) {
        const int m = std::min(kMaxBatch, n - c);
        int rc = collect_chunk(ctx, reqs + c, m, c, &G, &st);
        if (rc) return drain_streams(ctx, rc);
    }
    if (!G.overflow) {
        recs->reserve((size_t)G.sum);
        for (const auto& v : G.recs) recs->insert(recs->end(), v.begin(), v.end());
        if (recs->size() != G.sum) return HM_ERR_INTERNAL;
    }
    st.requests = n;
    st.total = G.sum;
    st.ndev = (int)ctx->devs.size();
    st.overflow = G.overflow ? 1 : 0;
    st.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0)
                     .count();
    ctx->last_collect_many = st;
    ctx->have_collect_many_stats = true;
    *total = G.sum;
    return HM_OK;
}

}  // namespace hm
