// find_k_many.cpp -- hm_find_k_many (ABI 1.17).
// ---------------------------------------------------------------------------
// hm_find_k_many: hm_find_k's answer for each of a batch of requests
// (fused_find_k_kernels.hip has the device protocol and its four invariants).
//
// Host side, per chunk (BatchChunk, batch.cpp, plans, launches and reads back;
// this file has what is hm_find_k's):
//   chunk     at most kMaxBatch requests, cut early so that the record slices
//             placed on any one device sum to at most HM_COLLECT_CAP_MAX
//             records.  Request i's slice is B_i = min(HM_COLLECT_CAP_MAX,
//             2 k_i + 4096) records (HM_OPT_FIND_K_BUF: max(that value, k_i)),
//             so one request always fits.  The slices of a device lie side by
//             side in its collect_buf; the control words are a per-device
//             block of kMaxBatch x kFkWords words.
//   window    exactly hm_find_many's: request r's window is [lo, min(hi, lo +
//             W - 1)], W = kFusedNonces (HM_OPT_FIND_WINDOW: a test hook); the
//             longest ascending prefix of its segments that one launch can
//             hold is fused.
//   launch    per request, on its stream: filled, maxk and tasks_run zeroed,
//             the planner with its `result` seed (MaxUint64, 0) pointed at the
//             request's (stop, cursor) pair, then hm_fused_find_k_kernel.
//   readback  one host_read of the control block per device, then each request's
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
//
// hm_cancel (ABI 1.18): as hm_find_many (find_many.cpp) -- each fused launch's
// relay wave ends it, the host tests the cancel flag after the chunk's wait and
// readback, before any control word or record is looked at, and find_k_core
// tests it before each leftover's first launch and between overflow windows.
// ---------------------------------------------------------------------------
#include "hm_internal.hpp"

namespace hm {
namespace {

// A request's record slice.
struct Slice {
    size_t B = 0;    // its records
    size_t off = 0;  // fused: its first record in the device's collect_buf
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
    const int ndev = (int)ctx->devs.size();
    BatchChunk C(ctx, index0, ctx->find_window, false);
    std::vector<Slice> sl(n);
    std::vector<size_t> slab(ndev, 0);
    for (int r = 0; r < n; ++r) {
        const hm_find_k_request& q = reqs[r];
        const BatchReq& R = C.add(q.msg, q.len, q.lo, q.hi, q.target);
        sl[r].B = slice_records(ctx, q);
        outs[r].clear();
        if (R.segs.empty()) continue;
        sl[r].off = slab[R.dev];
        slab[R.dev] += sl[r].B;
    }
    int rc = C.prepare(&Device::find_k_many_ctl, (size_t)kMaxBatch * kFkWords);
    if (rc) return rc;
    for (int i = 0; i < ndev; ++i) {
        Device& dv = ctx->devs[i];
        if (!C.nfused[i]) continue;
        // the caller cut the chunk so (find_k_many_locked)
        if (slab[i] > HM_COLLECT_CAP_MAX) return HM_ERR_INTERNAL;
        HIPCHK(hipSetDevice(dv.ordinal));
        rc = collect_buffer(dv, slab[i]);
        if (rc) return rc;
    }
    static const KernelName name = kernel_name(Family::FindK, HM_KIND_FUSED, nullptr);
    FindTally fused;
    rc = C.launch<FusedFindKArgs>(
        name, &fused,
        [&](int r, const BatchReq&, Device& dv, hipStream_t s, FusedLaunch* fl, FusedFindKArgs* ka) {
            uint64_t* ctl = dv.find_k_many_ctl + (size_t)kFkWords * r;
            // the planner seeds (stop, cursor) = (MaxUint64, 0)
            static_assert(kFkStop == 0 && kFkCursor == 1 && kFkFilled == 2 && kFkWords == 5,
                          "the planner's seed, then the words zeroed here");
            fl->pa.result = ctl;
            HIPCHK(hipMemsetAsync(ctl + kFkFilled, 0, (kFkWords - kFkFilled) * sizeof(uint64_t), s));
            ka->f.ctl = ctl;
            ka->f.out = dv.collect_buf + 2 * sl[r].off;
            ka->f.target = reqs[r].target;
            ka->f.launch_lo = reqs[r].lo;
            ka->f.cap = (uint32_t)sl[r].B;
            ka->f.k = (uint32_t)reqs[r].k;
            ka->f.cancel = cancel_ptr(ctx, dv);
            return (int)HM_OK;
        });
    if (!rc) rc = C.finish(&Device::find_k_many_ctl, (size_t)kFkWords * n, &fused);
    if (rc) return rc;
    // hm_cancel: after the wait and the readback, before any word is looked at
    if (cancel_seen(ctx)) return cancel_observed(ctx, fused.launches);
    st->nonces_enqueued += fused.nonces;
    st->tasks_total += fused.tasks;
    st->launches += fused.launches;
    st->kernel_ms += fused.kernel_ms;
    // the records of every request whose slice held them, before any fallback
    // (which writes collect_buf)
    std::vector<std::vector<hm_result>> got(n);
    for (int r = 0; r < n; ++r) {
        const BatchReq& R = C.rq[r];
        if (!R.launched) continue;
        Device& dv = ctx->devs[R.dev];
        HIPCHK(hipSetDevice(dv.ordinal));
        const uint64_t* w = C.ctl[R.dev].data() + (size_t)kFkWords * r;
        st->tasks_run += w[kFkTasksRun];
        const uint64_t cursor = w[kFkCursor];
        if (cursor > sl[r].B || cursor == 0) continue;
        got[r].resize((size_t)cursor);
        rc = host_read(ctx, got[r].data(), dv.collect_buf + 2 * sl[r].off,
                       (size_t)cursor * sizeof(hm_result));
        if (rc) return rc;
        st->records += cursor;
    }
    for (int r = 0; r < n; ++r) {
        const hm_find_k_request& q = reqs[r];
        const BatchReq& R = C.rq[r];
        if (!R.live) continue;
        uint64_t from = q.lo;
        size_t need = q.k;
        if (R.launched) {
            const uint64_t* w = C.ctl[R.dev].data() + (size_t)kFkWords * r;
            const uint64_t stop = w[kFkStop];
            if (w[kFkCursor] > sl[r].B) {
                // records at or below the k-th hit may be missing
                ++st->overflow;
            } else {
                std::vector<hm_result>& v = got[r];
                // slots are handed out in dispatch order: the answer is in nonce order
                rc = sort_check_records(&v, q.lo, R.fused_hi, q.target);
                if (rc) return rc;
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
        rc = find_k_core(ctx, R.m, R.mlen, from, q.hi, q.target, need, &kt, &more);
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
    int rc = batch_open(ctx, reqs, n, t0);
    if (rc) return rc;
    CancelScope cancel(ctx, HM_CANCEL_FAMILY_FIND_K_MANY);
    hm_find_k_many_stats st{};
    recs->assign((size_t)n, {});
    const int ndev = (int)ctx->devs.size();
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
        // hm_cancel: nothing is in flight between chunks
        rc = cancel_seen(ctx) ? cancel_observed(ctx, 0)
                              : find_k_chunk(ctx, reqs + c, m, c, recs->data() + c, &st);
        if (rc) return cancel.end(drain_streams(ctx, rc));
        c += m;
    }
    for (int r = 0; r < n; ++r) st.found += (*recs)[r].size();
    st.requests = n;
    publish(ctx, ctx->find_k_many_stats, st, t0);
    return HM_OK;
}

}  // namespace hm
