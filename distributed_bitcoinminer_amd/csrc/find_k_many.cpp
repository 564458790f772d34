// find_k_many.cpp -- hm_find_k_many (ABI 1.17).
// ---------------------------------------------------------------------------
// hm_find_k_many: hm_find_k's answer for each of a batch of requests
// (fused_find_k_kernels.hip has the device protocol and its four invariants).
//
// Host side, per chunk:
//   chunk     at most kMaxBatch requests, cut early so that the record slices
//             placed on any one device sum to at most HM_COLLECT_CAP_MAX
//             records.  Request i's slice is B_i = min(HM_COLLECT_CAP_MAX,
//             2 k_i + 4096) records (HM_OPT_FIND_K_BUF: max(that value, k_i)),
//             so one request always fits.  The slices of a device lie side by
//             side in its collect_buf; the control words are a per-device
//             block of kMaxBatch x kFkWords words.
//   window    exactly hm_find_many's: request r's window is [lo, min(hi, lo +
//             W - 1)], W = kFusedNonces (HM_OPT_FIND_WINDOW: a test hook),
//             planned with plan_range, whose segments ascend by nonce, and the
//             longest prefix of them that fusible() accepts is fused: the tasks
//             of one launch then ascend in their smallest nonce, which the
//             kernel's "leave" rule needs.
//   launch    request r goes whole to device r mod ndev and round-robins over
//             that device's streams; per request, on its stream: filled, maxk
//             and tasks_run zeroed, hm_fused_plan_kernel -- records, tables,
//             the queue counter, and its `result` seed (MaxUint64, 0) pointed
//             at the request's (stop, cursor) pair -- then
//             hm_fused_find_k_kernel between two events.
//   readback  every request of the chunk is enqueued on every device before
//             the host waits on any: one host_wait per used stream, one
//             host_read of the control block per device, then each request's
//             min(cursor, B_i) records.  All records are on the host before
//             any fallback starts: the fallback reuses collect_buf.
//   answer    after hm_find_k's checks (records distinct, inside [lo,
//             fused_hi], below the target; a lowered stop word has k records at
//             or below it), per request:
//               cursor > B_i      the launch overran its slice: the whole
//                                 request goes down find_k_core from lo
//               stop lowered      the k lowest records are the answer
//               stop not lowered  nothing was skipped, the records are every
//                                 hit of [lo, fused_hi]: the answer if there
//                                 are k of them (the k-th at nonce MaxUint64
//                                 leaves the word as it is) or the window ends
//                                 the range; otherwise find_k_core continues
//                                 from fused_hi + 1 for the hits still missing
//               not fused         (an empty prefix, HM_OPT_FUSED = 0) the whole
//                                 request goes down find_k_core
// find_k_core is hm_find_k's per-segment path (find_k.cpp), one request after
// another on stream 0.
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
    size_t B = 0;    // records of its slice
    size_t off = 0;  // launched: its slice's first record in the device's collect_buf
    hipEvent_t a = nullptr, b = nullptr;
};

// The records of request q's slice, if it gets a fused launch; 0: it cannot.
size_t slice_records(const hm_ctx* ctx, const hm_find_k_request& q) {
    if (!ctx->fused || q.lo > q.hi || q.target == 0) return 0;
    return ctx->find_k_buf ? std::max<size_t>(ctx->find_k_buf, q.k)
                           : std::min<size_t>(HM_COLLECT_CAP_MAX, 2 * q.k + 4096);
}

void add_tally(hm_find_k_many_stats* st, const FindKTally& kt) {
    st->nonces_enqueued += kt.t.nonces;
    st->tasks_total += kt.t.tasks;
    st->tasks_run += kt.t.run;
    st->launches += kt.t.launches;
    st->kernel_ms += kt.t.kernel_ms;
    st->records += kt.records;
}

int find_k_chunk(hm_ctx* ctx, const hm_find_k_request* reqs, int n, int index0,
                 std::vector<hm_result>* outs, hm_find_k_many_stats* st) {
    static const uint8_t empty_msg = 0;
    const int ndev = (int)ctx->devs.size();
    const uint64_t W = ctx->find_window ? ctx->find_window : kFusedNonces;
    const int nstreams = std::max(1, std::min(ctx->streams, kStreams));
    std::vector<Req> rq(n);
    std::vector<MsgPlan> mps(n);
    std::vector<std::vector<SegPlan>> segs(n);
    std::vector<int> nfused(ndev, 0);
    std::vector<size_t> slab(ndev, 0);
    for (int r = 0; r < n; ++r) {
        const hm_find_k_request& q = reqs[r];
        Req& R = rq[r];
        R.m = q.msg ? q.msg : &empty_msg;
        R.mlen = q.msg ? q.len : 0;
        R.live = q.lo <= q.hi && q.target != 0;
        R.dev = (index0 + r) % ndev;
        R.B = slice_records(ctx, q);
        outs[r].clear();
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
        if (segs[r].empty()) continue;
        ++nfused[R.dev];
        R.off = slab[R.dev];
        slab[R.dev] += R.B;
    }
    for (int i = 0; i < ndev; ++i) {
        Device& dv = ctx->devs[i];
        if (!nfused[i]) continue;
        // the caller cut the chunk so (find_k_many_locked)
        if (slab[i] > HM_COLLECT_CAP_MAX) return HM_ERR_INTERNAL;
        HIPCHK(hipSetDevice(dv.ordinal));
        if (!dv.find_k_many_ctl)
            HIPCHK(hipMalloc(&dv.find_k_many_ctl,
                             (size_t)kMaxBatch * kFkWords * sizeof(uint64_t)));
        int rc = collect_buffer(dv, slab[i]);
        if (rc) return rc;
        rc = make_streams(dv, std::min(nstreams, nfused[i]));
        if (rc) return rc;
    }
    static const KernelName name = kernel_name(Family::FindK, HM_KIND_FUSED, nullptr);
    std::vector<int> rr(ndev, 0);
    for (int r = 0; r < n; ++r) {
        if (segs[r].empty()) continue;
        Req& R = rq[r];
        Device& dv = ctx->devs[R.dev];
        HIPCHK(hipSetDevice(dv.ordinal));
        const int si = rr[R.dev]++ % std::min(nstreams, nfused[R.dev]);
        hipStream_t s = dv.stream[si];
        FusedFindKArgs ka;
        FusedLaunch fl;
        int rc = plan_fused(ctx, dv, mps[r], segs[r], si, kFusedStaticFirst, &fl);
        if (rc) return rc;
        uint64_t* ctl = dv.find_k_many_ctl + (size_t)kFkWords * r;
        // the planner seeds (stop, cursor) = (MaxUint64, 0)
        static_assert(kFkStop == 0 && kFkCursor == 1 && kFkFilled == 2 && kFkWords == 5,
                      "the planner's seed, then the words zeroed here");
        fl.pa.result = ctl;
        ka.a = fl.fa;
        ka.f.ctl = ctl;
        ka.f.out = dv.collect_buf + 2 * R.off;
        ka.f.target = reqs[r].target;
        ka.f.launch_lo = reqs[r].lo;
        ka.f.cap = (uint32_t)R.B;
        ka.f.k = (uint32_t)reqs[r].k;
        const Device::Fn* fn = nullptr;
        rc = scan_fn(dv, name.symbol, &fn);
        if (rc) return rc;
        rc = next_event(dv, &R.a);
        if (rc) return rc;
        rc = next_event(dv, &R.b);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(ctl + kFkFilled, 0, (kFkWords - kFkFilled) * sizeof(uint64_t), s));
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
        ctl[i].resize((size_t)kFkWords * n);
        int rc = host_read(ctx, ctl[i].data(), dv.find_k_many_ctl,
                           ctl[i].size() * sizeof(uint64_t));
        if (rc) return rc;
    }
    // the records of every request whose slice held them, before any fallback
    // (which writes collect_buf)
    std::vector<std::vector<hm_result>> got(n);
    for (int r = 0; r < n; ++r) {
        const Req& R = rq[r];
        if (!R.launched) continue;
        Device& dv = ctx->devs[R.dev];
        HIPCHK(hipSetDevice(dv.ordinal));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, R.a, R.b));
        st->kernel_ms += ms;
        const uint64_t* w = ctl[R.dev].data() + (size_t)kFkWords * r;
        st->tasks_run += w[kFkTasksRun];
        const uint64_t cursor = w[kFkCursor];
        if (cursor > R.B || cursor == 0) continue;
        got[r].resize((size_t)cursor);
        int rc = host_read(ctx, got[r].data(), dv.collect_buf + 2 * R.off,
                           (size_t)cursor * sizeof(hm_result));
        if (rc) return rc;
        st->records += cursor;
    }
    for (Device& dv : ctx->devs) dv.evnext = 0;  // the events are free again
    for (int r = 0; r < n; ++r) {
        const hm_find_k_request& q = reqs[r];
        const Req& R = rq[r];
        if (!R.live) continue;
        uint64_t from = q.lo;
        size_t need = q.k;
        if (R.launched) {
            const uint64_t* w = ctl[R.dev].data() + (size_t)kFkWords * r;
            const uint64_t stop = w[kFkStop];
            if (w[kFkCursor] > R.B) {
                // records at or below the k-th hit may be missing
                ++st->overflow;
            } else {
                std::vector<hm_result>& v = got[r];
                // slots are handed out in dispatch order: the answer is in nonce order
                std::sort(v.begin(), v.end(), [](const hm_result& x, const hm_result& y) {
                    return x.nonce < y.nonce;
                });
                for (size_t i = 0; i < v.size(); ++i) {
                    if (v[i].hash >= q.target || v[i].nonce < q.lo || v[i].nonce > R.fused_hi ||
                        (i > 0 && v[i].nonce == v[i - 1].nonce))
                        return HM_ERR_INTERNAL;
                }
                if (v.size() > q.k) v.resize(q.k);
                // a lowered stop word promises k records at or below it
                if (stop != ~0ull && (v.size() < q.k || v.back().nonce > stop))
                    return HM_ERR_INTERNAL;
                outs[r] = std::move(v);
                // stop not lowered: nothing was skipped, these are all of [lo, fused_hi]
                if (outs[r].size() == q.k || R.fused_hi == q.hi) {
                    ++st->fused;
                    continue;
                }
                from = R.fused_hi + 1;
                need = q.k - outs[r].size();
            }
        }
        FindKTally kt;
        std::vector<hm_result> more;
        int rc = find_k_core(ctx, R.m, R.mlen, from, q.hi, q.target, need, &kt, &more);
        if (rc) return rc;
        outs[r].insert(outs[r].end(), more.begin(), more.end());
        ++st->fallback;
        add_tally(st, kt);
    }
    return HM_OK;
}

}  // namespace

// hm_find_k_many with ctx->mu held.
int find_k_many_locked(hm_ctx* ctx, const hm_find_k_request* reqs, int n,
                       std::vector<std::vector<hm_result>>* recs) {
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
    hm_find_k_many_stats st{};
    recs->assign((size_t)n, {});
    const int ndev = (int)ctx->devs.size();
    for (Device& dv : ctx->devs) dv.evnext = 0;
    for (int c = 0; c < n;) {
        // the chunk: up to kMaxBatch requests whose slices fit each device's slab
        std::vector<size_t> slab(ndev, 0);
        int m = 0;
        while (c + m < n && m < kMaxBatch) {
            size_t& s = slab[(c + m) % ndev];
            const size_t B = slice_records(ctx, reqs[c + m]);
            if (m > 0 && s + B > HM_COLLECT_CAP_MAX) break;
            s += B;
            ++m;
        }
        int rc = find_k_chunk(ctx, reqs + c, m, c, recs->data() + c, &st);
        if (rc) return drain_streams(ctx, rc);
        c += m;
    }
    st.requests = n;
    for (int r = 0; r < n; ++r) st.found += (*recs)[r].size();
    st.ndev = ndev;
    st.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0)
                     .count();
    ctx->last_find_k_many = st;
    ctx->have_find_k_many_stats = true;
    return HM_OK;
}

}  // namespace hm
