// scan_k.cpp -- hm_scan_k (ABI 1.19).
// ---------------------------------------------------------------------------
// hm_scan_k: the k lexicographically smallest (Hash(msg, n), n) pairs of
// [lo, hi], 1 <= k <= HM_SCAN_K_MAX (scan_k_kernels.hip has the device
// protocol and its four invariants).
//
// Host side, as hm_collect's.  The range is planned and sharded through
// PieceWalk (each digit segment one piece; several devices: pieces of
// kFindPieceNonces per device, split with partition_range) and each shard's
// segments are walked launch by launch (SegWalk).  The whole range is always
// hashed, so nothing is pruned and nothing is waited for in between: every
// launch of every device goes onto its stream 0 up front, each followed by the
// fold kernel that merges the launch's wave lists into the device list and
// refreshes the bound the next launch's waves start from.  One host_wait per
// device; then each device's count and <= 32 records are read back, the lists
// are merged (sort by (hash, nonce), keep k) and every record is checked:
// its hash recomputed on the host, its nonce inside [lo, hi], the order
// strictly ascending, the count min(k, nonces of the range).
// ---------------------------------------------------------------------------
#include "hm_internal.hpp"

namespace hm {
namespace {

static_assert(kScanKMax == HM_SCAN_K_MAX, "kernels.hpp's copy of the limit");
constexpr size_t kWaveRecWords = (size_t)kMaxCandWaves * kScanKMax * 2;  // 16 MiB of records

// One device's share of a call.
struct ScanKDev {
    hipEvent_t first = nullptr, last = nullptr;  // around its launches
    const Device::Fn* fold = nullptr;
    uint64_t nonces = 0;
    int launches = 0;
};

// The device's control block and wave-list buffer, made on first use and kept
// until hm_close.
int scan_k_buffers(Device& dv) {
    int rc = ctl_block(&dv.scan_k_ctl, kSkWords);
    if (rc) return rc;
    if (!dv.scan_k_waves) {
        const size_t bytes = kWaveRecWords * sizeof(uint64_t) + kMaxCandWaves * sizeof(uint32_t);
        if (hipMalloc(&dv.scan_k_waves, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return HM_ERR_NOMEM;
        }
    }
    return HM_OK;
}

// Enqueue every launch of segment s on dv's stream 0, each followed by its fold.
int scan_k_segment(hm_ctx* ctx, Device& dv, ScanKDev& sd, const MsgPlan& mp, const SegPlan& s,
                   const ScanKArgs& ka) {
    SegWalk w;
    int rc = w.open(ctx, dv, mp, 0, s, Family::ScanK, kFindGenericNonces);
    if (rc) return rc;
    SegStep step;
    while (w.next(&step)) {
        hipEvent_t start = nullptr;
        if (!sd.first) {
            rc = next_event(dv, &sd.first);
            if (rc) return rc;
            rc = next_event(dv, &sd.last);
            if (rc) return rc;
            start = sd.first;
        }
        rc = w.launch(step, ka, start, nullptr);
        if (rc) return rc;
        // the launch's waves each wrote one slot: merge them into the device list
        ScanKFoldArgs fa;
        fa.k = ka;
        fa.nwaves = (uint32_t)step.grid * (kBlock / kWaveSize);
        rc = launch_scan(*sd.fold, fa, 1, dv.stream[0]);
        if (rc) return rc;
        sd.nonces += step.nonces;
        ++sd.launches;
    }
    return HM_OK;
}

bool rec_below(const hm_result& x, const hm_result& y) {
    return x.hash < y.hash || (x.hash == y.hash && x.nonce < y.nonce);
}

}  // namespace

// hm_scan_k with ctx->mu held.
int scan_k_locked(hm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
                  uint32_t k, std::vector<hm_result>* recs) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint8_t* m;
    size_t mlen;
    int rc = begin_ranged_call(ctx, msg, len, lo, hi, t0, &m, &mlen);
    if (rc) return rc;
    const int ndev = (int)ctx->devs.size();
    std::vector<ScanKDev> sds(ndev);
    hm_scan_k_stats st{};
    st.k = k;
    recs->clear();
    if (lo <= hi) {
        const MsgPlan mp = plan_message(m, mlen);
        const std::string fold_sym = "_ZN2hm21hm_scan_k_fold_kernelENS_13ScanKFoldArgsE";
        for (int i = 0; i < ndev; ++i) {
            Device& dv = ctx->devs[i];
            if (hipSetDevice(dv.ordinal) != hipSuccess) return drain_failed(ctx, HM_ERR_HIP);
            dv.evnext = 0;
            rc = scan_k_buffers(dv);
            if (rc) return drain_failed(ctx, rc);  // earlier devices have their reset queued
            rc = scan_fn(dv, fold_sym, &sds[i].fold);
            if (rc) return drain_failed(ctx, rc);
            // an empty device list, no bound, the diagnostics at 0
            if (hipMemsetAsync(dv.scan_k_ctl, 0, kSkZeroed * sizeof(uint64_t), dv.stream[0]) !=
                hipSuccess)
                return drain_failed(ctx, HM_ERR_HIP);
        }
        PieceWalk pieces(ctx, mp, lo, hi);
        std::vector<std::vector<SegPlan>> shards;
        while (pieces.next(&shards)) {
            for (int i = 0; i < ndev; ++i) {
                if (shards[i].empty()) continue;
                Device& dv = ctx->devs[i];
                if (hipSetDevice(dv.ordinal) != hipSuccess) return drain_failed(ctx, HM_ERR_HIP);
                ScanKArgs ka;
                ka.ctl = dv.scan_k_ctl;
                ka.wave_recs = dv.scan_k_waves;
                ka.wave_cnt = reinterpret_cast<uint32_t*>(dv.scan_k_waves + kWaveRecWords);
                ka.k = k;
                for (const SegPlan& s : shards[i]) {
                    rc = scan_k_segment(ctx, dv, sds[i], mp, s, ka);
                    if (rc) return drain_failed(ctx, rc);
                }
            }
        }
        for (int i = 0; i < ndev; ++i) {
            if (!sds[i].first) continue;
            Device& dv = ctx->devs[i];
            if (hipSetDevice(dv.ordinal) != hipSuccess ||
                hipEventRecord(sds[i].last, dv.stream[0]) != hipSuccess)
                return drain_failed(ctx, HM_ERR_HIP);
        }
        // everything is enqueued: wait for each device, then read it back
        for (int i = 0; i < ndev; ++i) {
            Device& dv = ctx->devs[i];
            if (hipSetDevice(dv.ordinal) != hipSuccess) return drain_failed(ctx, HM_ERR_HIP);
            rc = host_wait(ctx, dv.stream[0]);
            if (rc) return drain_failed(ctx, rc);
        }
        for (int i = 0; i < ndev; ++i) {
            Device& dv = ctx->devs[i];
            HIPCHK(hipSetDevice(dv.ordinal));
            uint64_t ctl[kSkWords];
            rc = host_read(ctx, ctl, dv.scan_k_ctl, sizeof ctl);
            if (rc) return rc;
            if (sds[i].first) {
                float ms = 0.f;
                HIPCHK(hipEventElapsedTime(&ms, sds[i].first, sds[i].last));
                st.kernel_ms += ms;
            }
            dv.evnext = 0;  // the events are free again
            if (ctl[kSkCount] > k) return HM_ERR_INTERNAL;
            for (uint64_t j = 0; j < ctl[kSkCount]; ++j)
                recs->push_back(hm_result{ctl[kSkList + 2 * j], ctl[kSkList + 2 * j + 1]});
            st.inserted += ctl[kSkInserted];
            st.compactions += ctl[kSkCompactions];
            st.nonces += sds[i].nonces;
            st.launches += sds[i].launches;
        }
        // the devices' lists into one: the k lowest of their union
        std::sort(recs->begin(), recs->end(), rec_below);
        if (recs->size() > k) recs->resize(k);
        const uint64_t span_m1 = hi - lo;
        if (recs->size() != (span_m1 >= k - 1 ? (size_t)k : (size_t)span_m1 + 1))
            return HM_ERR_INTERNAL;
        for (size_t j = 0; j < recs->size(); ++j) {
            const hm_result& r = (*recs)[j];
            if (r.nonce < lo || r.nonce > hi || r.hash != host_hash(m, mlen, r.nonce) ||
                (j > 0 && !rec_below((*recs)[j - 1], r)))
                return HM_ERR_INTERNAL;
        }
    }
    st.count = (int32_t)recs->size();
    publish(ctx, ctx->scan_k_stats, st, t0);
    return HM_OK;
}

}  // namespace hm
