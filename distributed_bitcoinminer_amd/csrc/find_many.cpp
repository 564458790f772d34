// find_many.cpp -- hm_find_many (ABI 1.13).
// ---------------------------------------------------------------------------
// hm_find_many: hm_find's answer for each of a batch of requests
// (fused_find_kernels.hip has the device protocol and its three invariants).
//
// Host side, per chunk of at most kMaxBatch requests:
//   window    request r's window is [lo, min(hi, lo + W - 1)], W =
//             kFusedNonces (HM_OPT_FIND_WINDOW: a test hook).  It is planned
//             with plan_range, whose segments ascend by nonce, and the longest
//             prefix of them that fusible() accepts is fused: the tasks of one
//             launch then ascend in their smallest nonce, which the kernel's
//             "leave" rule needs.  (enqueue_fused orders costliest first; a
//             find must not.)
//   launch    request r goes whole to device r mod ndev and round-robins over
//             that device's streams; per request hm_fused_plan_kernel --
//             records, tables, the queue counter, and its `result` seed
//             (MaxUint64, 0) pointed at the request's (stop word, tasks run)
//             pair -- then hm_fused_find_kernel between two events.  No fold:
//             the word is the answer.
//   readback  every request of the chunk is enqueued on every device before
//             the host waits on any: one host_wait per used stream, one
//             host_read of the pairs per device.  A hit's hash is recomputed
//             (host_hash) and must qualify, as in find_core.
//   fallback  a request without a hit whose range goes on past what was fused
//             continues from the first nonce not fused through find_core (the
//             per-segment path of hm_find), one request after another.
//             HM_OPT_FUSED = 0 sends every request there.
// A hit at nonce MaxUint64 cannot be told from "none" in the stop word: the
// kernel never publishes it and the host tests that one nonce itself.
// ---------------------------------------------------------------------------
#include "hm_internal.hpp"

namespace hm {
namespace {

// One request of a chunk.
struct Req {
    const uint8_t* m;
    size_t mlen;
    bool live = false;      // lo <= hi and target != 0: something to search
    bool launched = false;  // a fused launch was enqueued
    uint64_t fused_hi = 0;  // launched: its last nonce
    int dev = 0;
    hipEvent_t a = nullptr, b = nullptr;
};

int find_chunk(hm_ctx* ctx, const hm_find_request* reqs, int n, int index0, hm_result* outs,
               int* found, hm_find_many_stats* st) {
    static const uint8_t empty_msg = 0;
    const int ndev = (int)ctx->devs.size();
    const uint64_t W = ctx->find_window ? ctx->find_window : kFusedNonces;
    const int nstreams = std::max(1, std::min(ctx->streams, kStreams));
    std::vector<Req> rq(n);
    std::vector<MsgPlan> mps(n);
    std::vector<std::vector<SegPlan>> segs(n);
    std::vector<int> nfused(ndev, 0);
    for (int r = 0; r < n; ++r) {
        const hm_find_request& q = reqs[r];
        Req& R = rq[r];
        R.m = q.msg ? q.msg : &empty_msg;
        R.mlen = q.msg ? q.len : 0;
        R.live = q.lo <= q.hi && q.target != 0;
        R.dev = (index0 + r) % ndev;
        outs[r] = hm_result{~0ull, 0};
        found[r] = 0;
        if (!R.live || !ctx->fused) continue;
        mps[r] = plan_message(R.m, R.mlen);
        const uint64_t we = q.hi - q.lo < W - 1 ? q.hi : q.lo + (W - 1);
        const std::vector<SegPlan> all =
            plan_range(mps[r], q.lo, we, ctx->force_generic, ctx->table_digits);
        // the longest ascending prefix one fused launch can hold
        for (const SegPlan& g : all) {
            segs[r].push_back(g);
            if (!fusible(segs[r])) { segs[r].pop_back(); break; }
        }
        if (!segs[r].empty()) ++nfused[R.dev];
    }
    for (int i = 0; i < ndev; ++i) {
        Device& dv = ctx->devs[i];
        if (!nfused[i]) continue;
        HIPCHK(hipSetDevice(dv.ordinal));
        if (!dv.find_many_ctl)
            HIPCHK(hipMalloc(&dv.find_many_ctl, (size_t)kMaxBatch * 2 * sizeof(uint64_t)));
        int rc = make_streams(dv, std::min(nstreams, nfused[i]));
        if (rc) return rc;
    }
    static const KernelName name = kernel_name(Family::Find, HM_KIND_FUSED, nullptr);
    std::vector<int> rr(ndev, 0);
    for (int r = 0; r < n; ++r) {
        if (segs[r].empty()) continue;
        Req& R = rq[r];
        Device& dv = ctx->devs[R.dev];
        HIPCHK(hipSetDevice(dv.ordinal));
        const int si = rr[R.dev]++ % std::min(nstreams, nfused[R.dev]);
        hipStream_t s = dv.stream[si];
        FusedFindArgs ka;
        FusedLaunch fl;
        int rc = plan_fused(ctx, dv, mps[r], segs[r], si, kFusedStaticFirst, &fl);
        if (rc) return rc;
        fl.pa.result = dv.find_many_ctl + 2 * r;
        ka.a = fl.fa;
        ka.f.word = dv.find_many_ctl + 2 * r;
        ka.f.tasks_run = dv.find_many_ctl + 2 * r + 1;
        ka.f.target = reqs[r].target;
        ka.f.launch_lo = reqs[r].lo;
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
        R.fused_hi = segs[r].back().hi;
        st->nonces_enqueued += fl.nonces;
        st->tasks_total += fl.fa.ntasks;
        ++st->launches;
    }
    // every device's work is queued: wait, then one read of the pairs each
    std::vector<std::vector<uint64_t>> ctl(ndev);
    for (int i = 0; i < ndev; ++i) {
        Device& dv = ctx->devs[i];
        if (!nfused[i]) continue;
        HIPCHK(hipSetDevice(dv.ordinal));
        for (int s = 0; s < std::min(nstreams, nfused[i]); ++s) {
            int rc = host_wait(ctx, dv.stream[s]);
            if (rc) return rc;
        }
        ctl[i].resize((size_t)2 * n);
        int rc = host_read(ctx, ctl[i].data(), dv.find_many_ctl, ctl[i].size() * sizeof(uint64_t));
        if (rc) return rc;
    }
    for (int r = 0; r < n; ++r) {
        const Req& R = rq[r];
        if (!R.launched) continue;
        float ms = 0.f;
        HIPCHK(hipSetDevice(ctx->devs[R.dev].ordinal));
        HIPCHK(hipEventElapsedTime(&ms, R.a, R.b));
        st->kernel_ms += ms;
        st->tasks_run += ctl[R.dev][2 * r + 1];
    }
    for (Device& dv : ctx->devs) dv.evnext = 0;  // the events are free again
    for (int r = 0; r < n; ++r) {
        const hm_find_request& q = reqs[r];
        const Req& R = rq[r];
        if (!R.live) continue;
        uint64_t from = q.lo;
        if (R.launched) {
            uint64_t best = ctl[R.dev][2 * r];
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
        int rc = find_core(ctx, R.m, R.mlen, from, q.hi, q.target, &tally, &outs[r], &found[r]);
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

// hm_find_many with ctx->mu held.
int find_many_locked(hm_ctx* ctx, const hm_find_request* reqs, int n, hm_result* outs, int* found) {
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
    hm_find_many_stats st{};
    for (Device& dv : ctx->devs) dv.evnext = 0;
    for (int c = 0; c < n; c += kMaxBatch) {
        const int m = std::min(kMaxBatch, n - c);
        int rc = find_chunk(ctx, reqs + c, m, c, outs + c, found + c, &st);
        if (rc) return drain_streams(ctx, rc);
    }
    st.requests = n;
    for (int r = 0; r < n; ++r) st.found += found[r];
    st.ndev = (int)ctx->devs.size();
    st.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0)
                     .count();
    ctx->last_find_many = st;
    ctx->have_find_many_stats = true;
    return HM_OK;
}

}  // namespace hm
