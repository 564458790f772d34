// collect.cpp -- hm_collect (ABI 1.11).
// ---------------------------------------------------------------------------
// hm_collect: every nonce of [lo, hi] whose hash is below `target`, and their
// exact count (collect_kernels.hip has the device protocol and its three
// invariants).
//
// Host side.  The range is planned and sharded as find's (PieceWalk):
// plan_range, each digit segment one piece (several devices: pieces of
// kFindPieceNonces per device, cut at tile boundaries and split with
// partition_range), and each shard's segments are walked launch by launch
// (SegWalk).  There is no early exit, so there is no lookahead window either:
// every launch of every device is enqueued on its stream 0 before the host
// waits on any -- one host_wait per device, no mid-call syncs -- and then each
// device's total, cursor and min(total, cap) records are read back.  The
// totals are summed; if the sum fits `cap` the records are concatenated and
// sorted by nonce.
// ---------------------------------------------------------------------------
#include "hm_internal.hpp"

namespace hm {
namespace {

// One device's share of a collect call.
struct CollectDev {
    hipEvent_t first = nullptr, last = nullptr;  // around its launches
    uint64_t nonces = 0;
    int launches = 0;
};

}  // namespace

// Slots are handed out in dispatch order, the answer is in nonce order: sort,
// then every record is distinct, inside [lo, hi] and below the target.
int sort_check_records(std::vector<hm_result>* recs, uint64_t lo, uint64_t hi, uint64_t target) {
    std::sort(recs->begin(), recs->end(),
              [](const hm_result& x, const hm_result& y) { return x.nonce < y.nonce; });
    for (size_t i = 0; i < recs->size(); ++i) {
        const hm_result& r = (*recs)[i];
        if (r.hash >= target || r.nonce < lo || r.nonce > hi ||
            (i > 0 && r.nonce == (*recs)[i - 1].nonce))
            return HM_ERR_INTERNAL;
    }
    return HM_OK;
}

namespace {

// Enqueue every launch of segment s on dv's stream 0 (the device's first
// launch of the call after its `first` timing event).
int collect_segment(hm_ctx* ctx, Device& dv, CollectDev& cd, const MsgPlan& mp, const SegPlan& s,
                    const CollectArgs& ka) {
    SegWalk w;
    int rc = w.open(ctx, dv, mp, 0, s, Family::Collect, kFindGenericNonces);
    if (rc) return rc;
    SegStep step;
    while (w.next(&step)) {
        hipEvent_t start = nullptr;
        if (!cd.first) {
            rc = next_event(dv, &cd.first);
            if (rc) return rc;
            rc = next_event(dv, &cd.last);
            if (rc) return rc;
            start = cd.first;
        }
        rc = w.launch(step, ka, start, nullptr);
        if (rc) return rc;
        cd.nonces += step.nonces;
        ++cd.launches;
    }
    return HM_OK;
}

}  // namespace

// hm_collect between its opening and its stats record (hm_collect_many's
// fallback runs it too).  *recs: the records, ascending by nonce, when *total
// <= cap; empty otherwise.
int collect_core(hm_ctx* ctx, const uint8_t* m, size_t mlen, uint64_t lo, uint64_t hi,
                 uint64_t target, size_t cap, CollectTally* tally, std::vector<hm_result>* recs,
                 uint64_t* total) {
    int rc;
    const int ndev = (int)ctx->devs.size();
    std::vector<CollectDev> cds(ndev);
    uint64_t sum = 0;
    double kernel_ms = 0;
    recs->clear();
    if (lo <= hi && target != 0) {
        const MsgPlan mp = plan_message(m, mlen);
        for (auto& dv : ctx->devs) {
            HIPCHK(hipSetDevice(dv.ordinal));
            dv.evnext = 0;
            rc = collect_buffer(dv, cap);
            if (rc) return rc;
            // the total and the slot cursor start at 0
            HIPCHK(hipMemsetAsync(dv.collect_ctl, 0, 2 * sizeof(uint64_t), dv.stream[0]));
        }
        PieceWalk pieces(ctx, mp, lo, hi);
        std::vector<std::vector<SegPlan>> shards;
        while (pieces.next(&shards)) {
            for (int i = 0; i < ndev; ++i) {
                if (shards[i].empty()) continue;
                Device& dv = ctx->devs[i];
                if (hipSetDevice(dv.ordinal) != hipSuccess) return drain_failed(ctx, HM_ERR_HIP);
                CollectArgs ka;
                ka.total = dv.collect_ctl;
                ka.cursor = dv.collect_ctl + 1;
                ka.out = cap ? dv.collect_buf : nullptr;
                ka.target = target;
                ka.cap = (uint32_t)cap;
                for (const SegPlan& s : shards[i]) {
                    rc = collect_segment(ctx, dv, cds[i], mp, s, ka);
                    if (rc) return drain_failed(ctx, rc);
                }
            }
        }
        for (int i = 0; i < ndev; ++i) {
            if (!cds[i].first) continue;
            Device& dv = ctx->devs[i];
            if (hipSetDevice(dv.ordinal) != hipSuccess ||
                hipEventRecord(cds[i].last, dv.stream[0]) != hipSuccess)
                return drain_failed(ctx, HM_ERR_HIP);
        }
        // everything is enqueued: wait for each device, then read it back
        std::vector<uint64_t> dev_total(ndev, 0);
        for (int i = 0; i < ndev; ++i) {
            Device& dv = ctx->devs[i];
            if (hipSetDevice(dv.ordinal) != hipSuccess) return drain_failed(ctx, HM_ERR_HIP);
            rc = host_wait(ctx, dv.stream[0]);
            if (rc) return drain_failed(ctx, rc);
        }
        for (int i = 0; i < ndev; ++i) {
            Device& dv = ctx->devs[i];
            HIPCHK(hipSetDevice(dv.ordinal));
            uint64_t ctl[2];
            rc = host_read(ctx, ctl, dv.collect_ctl, sizeof ctl);
            if (rc) return rc;
            dev_total[i] = ctl[0];
            // a device whose records all fit reserved exactly one slot per hit
            if (cap && ctl[0] <= cap && ctl[1] != ctl[0]) return HM_ERR_INTERNAL;
            if (sum + ctl[0] < sum) return HM_ERR_INTERNAL;
            sum += ctl[0];
            if (cds[i].first) {
                float ms = 0.f;
                HIPCHK(hipEventElapsedTime(&ms, cds[i].first, cds[i].last));
                kernel_ms += ms;
            }
            dv.evnext = 0;  // the events are free again
        }
        if (sum <= cap && sum > 0) {
            recs->resize((size_t)sum);
            size_t at = 0;
            for (int i = 0; i < ndev; ++i) {
                if (!dev_total[i]) continue;
                Device& dv = ctx->devs[i];
                HIPCHK(hipSetDevice(dv.ordinal));
                rc = host_read(ctx, recs->data() + at, dv.collect_buf,
                               (size_t)dev_total[i] * sizeof(hm_result));
                if (rc) return rc;
                at += (size_t)dev_total[i];
            }
            rc = sort_check_records(recs, lo, hi, target);
            if (rc) return rc;
        }
    }
    tally->kernel_ms += kernel_ms;
    for (const CollectDev& cd : cds) {
        tally->nonces += cd.nonces;
        tally->launches += cd.launches;
    }
    *total = sum;
    return HM_OK;
}

// hm_collect with ctx->mu held.
int collect_locked(hm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
                   uint64_t target, size_t cap, std::vector<hm_result>* recs, uint64_t* total) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint8_t* m;
    size_t mlen;
    int rc = begin_ranged_call(ctx, msg, len, lo, hi, t0, &m, &mlen);
    if (rc) return rc;
    CollectTally tally;
    uint64_t sum = 0;
    rc = collect_core(ctx, m, mlen, lo, hi, target, cap, &tally, recs, &sum);
    if (rc) return rc;
    hm_collect_stats st{};
    st.kernel_ms = tally.kernel_ms;
    st.total = sum;
    st.overflow = sum > cap ? 1 : 0;
    st.nonces = tally.nonces;
    st.launches = tally.launches;
    publish(ctx, ctx->collect_stats, st, t0);
    *total = sum;
    return HM_OK;
}

}  // namespace hm
