// batch.cpp -- what hm_find_many, hm_collect_many and hm_find_k_many share on
// the host: one chunk of at most kMaxBatch requests from planning to readback
// (BatchChunk, hm_internal.hpp), and the drain after a failure.
// ---------------------------------------------------------------------------
//   plan      a null message is the empty one; a request is live when lo <= hi
//             and target != 0; request r of the call goes whole to device r
//             mod ndev.  A live request is planned with plan_range, whose
//             segments ascend by nonce.  An early-exit family fuses the longest
//             prefix of its window's segments that fusible() accepts: the tasks
//             of one launch then ascend in their smallest nonce, which the
//             kernels' "leave" rule needs (enqueue_fused orders costliest
//             first; a find must not).  A family without an early exit fuses a
//             request whole or not at all (a fused prefix would buy nothing),
//             costliest segments first, as the fused scan.
//   prepare   per device with a launch: its control block, made on first use,
//             and as many streams as it has launches (at most HM_OPT_STREAMS)
//   launch    a device's requests round-robin over its streams; per request
//             hm_fused_plan_kernel -- records, tables, the queue counter, and
//             the seed or the zeroed word the family points it at -- then the
//             family's fused kernel between two events
//   finish    every request of the chunk is enqueued on every device before
//             the host waits on any: one host_wait per used stream, then one
//             host_read of the control words per device
// ---------------------------------------------------------------------------
#include "hm_internal.hpp"

namespace hm {

BatchChunk::BatchChunk(hm_ctx* ctx, int index0, uint64_t window, bool whole)
    : ctx(ctx),
      index0(index0),
      ndev((int)ctx->devs.size()),
      nstreams(std::max(1, std::min(ctx->streams, kStreams))),
      window(window ? window : kFusedNonces),
      whole(whole),
      nfused(ndev, 0),
      ctl(ndev),
      rr(ndev, 0) {
    rq.reserve(kMaxBatch);
}

BatchReq& BatchChunk::add(const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
                          uint64_t target) {
    const uint64_t W = window;
    rq.emplace_back();
    BatchReq& R = rq.back();
    const Msg e = msg_or_empty(msg, len);
    R.m = e.p;
    R.mlen = e.len;
    R.live = lo <= hi && target != 0;
    R.dev = (index0 + (int)rq.size() - 1) % ndev;
    if (!R.live || !ctx->fused || (whole && hi - lo > W - 1)) return R;
    R.mp = plan_message(R.m, R.mlen);
    const uint64_t we = hi - lo < W - 1 ? hi : lo + (W - 1);
    std::vector<SegPlan> all = plan_range(R.mp, lo, we, ctx->force_generic, ctx->table_digits);
    if (whole) {
        // all of its segments in one launch, or none
        if (fusible(all)) {
            fused_order(&all);
            R.segs = std::move(all);
        }
    } else {
        // the longest ascending prefix one fused launch can hold
        for (const SegPlan& g : all) {
            R.segs.push_back(g);
            if (!fusible(R.segs)) { R.segs.pop_back(); break; }
        }
    }
    if (!R.segs.empty()) ++nfused[R.dev];
    return R;
}

int BatchChunk::prepare(uint64_t* Device::*ctl_buf, size_t words) {
    for (int i = 0; i < ndev; ++i) {
        Device& dv = ctx->devs[i];
        if (!nfused[i]) continue;
        HIPCHK(hipSetDevice(dv.ordinal));
        int rc = ctl_block(&(dv.*ctl_buf), words);
        if (!rc) rc = make_streams(dv, used(i));
        if (rc) return rc;
    }
    return HM_OK;
}

int BatchChunk::plan_launch(int r, const std::string& symbol, int* si, FusedLaunch* fl,
                            const Device::Fn** fn) {
    BatchReq& R = rq[r];
    Device& dv = ctx->devs[R.dev];
    HIPCHK(hipSetDevice(dv.ordinal));
    *si = rr[R.dev]++ % used(R.dev);
    int rc = plan_fused(ctx, dv, R.mp, R.segs, *si, kFusedStaticFirst, fl);
    if (rc) return rc;
    rc = scan_fn(dv, symbol, fn);
    if (rc) return rc;
    rc = next_event(dv, &R.a);
    if (rc) return rc;
    return next_event(dv, &R.b);
}

int BatchChunk::finish(uint64_t* Device::*ctl_buf, size_t words, FindTally* tally) {
    // every device's work is queued: wait, then one read of the words each
    for (int i = 0; i < ndev; ++i) {
        Device& dv = ctx->devs[i];
        if (!nfused[i]) continue;
        HIPCHK(hipSetDevice(dv.ordinal));
        for (int s = 0; s < used(i); ++s) {
            int rc = host_wait(ctx, dv.stream[s]);
            if (rc) return rc;
        }
        ctl[i].resize(words);
        int rc = host_read(ctx, ctl[i].data(), dv.*ctl_buf, words * sizeof(uint64_t));
        if (rc) return rc;
    }
    for (const BatchReq& R : rq) {
        if (!R.launched) continue;
        float ms = 0.f;
        HIPCHK(hipSetDevice(ctx->devs[R.dev].ordinal));
        HIPCHK(hipEventElapsedTime(&ms, R.a, R.b));
        tally->kernel_ms += ms;
    }
    for (Device& dv : ctx->devs) dv.evnext = 0;  // the events are free again
    return HM_OK;
}

// A failure other than a timeout leaves nothing queued: every stream a
// device has made is waited for (drain_failed: stream 0 and the events).
int drain_streams(hm_ctx* ctx, int rc) {
    if (rc == HM_ERR_TIMEOUT || ctx->abandoned) return rc;
    for (Device& dv : ctx->devs) {
        if (hipSetDevice(dv.ordinal) != hipSuccess) break;
        for (int s = 1; s < dv.nmade; ++s)
            if (host_wait(ctx, dv.stream[s]) != HM_OK) return rc;
    }
    return drain_failed(ctx, rc);
}

}  // namespace hm
