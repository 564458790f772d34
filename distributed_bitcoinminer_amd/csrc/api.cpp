// api.cpp -- the hipminer C ABI (include/hipminer.h): the extern "C" entry
// points and the debug exports (include/hipminer_debug.h).
//
// Replaces, inside the Go miner process, the scan of evalRoutine
// (cmu440/bitcoin/miner/miner.go:46-59) and bitcoin.Hash
// (cmu440/bitcoin/hash.go:13-17).  Per device and per call:
//
//   host:  plan_message (midstate) -> plan_range (digit segments, layouts)
//   GPU :  per segment, on one of kStreams HIP streams
//            [tiled]   hm_tile_plan_kernel -> counter reset -> hm_tiled_kernel
//            [chained] hm_kw_table_kernel, hm_tile_plan_kernel -> hm_chained_kernel
//            [generic] hm_generic_kernel
//          -> hm_fold_kernel (per-wave candidates -> per-stream best)
//          -> join streams -> hm_fold_kernel (stream bests -> 16-B result)
//   multi-device: contiguous shards, then either a host merge of the 16-B
//          results or an RCCL all-gather of them (HM_OPT_MERGE_RCCL).
//   hm_scan_many: scan.cpp.  hm_find (ABI 1.10): find.cpp, the kernels of
//   find_kernels.hip.  hm_collect (ABI 1.11): collect.cpp, the kernels of
//   collect_kernels.hip.  All three walk a segment's launches with SegWalk
//   (seg_walk.cpp); devices, streams and host waits are device.cpp's.
//   hm_hash_many and hm_verify (ABI 1.12): verify.cpp, a list of arbitrary
//   nonces through the one kernel of verify_kernels.hip.
//   hm_find_many (ABI 1.13): find_many.cpp, one fused launch of
//   fused_find_kernels.hip per request, hm_find's path for what is left.
//   hm_verify_many (ABI 1.14): verify_many.cpp, the lists of many messages
//   through the job kernel of verify_many_kernels.hip.
//   hm_collect_many (ABI 1.15): collect_many.cpp, one fused launch of
//   fused_collect_kernels.hip per request, hm_collect's path for the rest.
//   hm_find_k (ABI 1.16): find_k.cpp over hm_find's walk, the kernels of
//   find_k_kernels.hip, hm_collect's path when its record buffer overflows.
//   hm_find_k_many (ABI 1.17): find_k_many.cpp, one fused launch of
//   fused_find_k_kernels.hip per request, hm_find_k's path for what is left.
//   The three *_many calls above share one chunk runner on the host
//   (batch.cpp); fused_tasks.hpp has the fused batch kernels' task walker
//   (hm_fused_find_kernel runs on it).  hm_cancel (ABI 1.18): cancel.hpp, the
//   flag's state machine; cancel_relay.hpp, the relay wave of the four
//   find-family kernel files.  hm_scan_k (ABI 1.19): scan_k.cpp over
//   hm_collect's walk, the kernels of scan_k_kernels.hip, a fold launch behind
//   each scan launch.  hm_find and hm_find_k share one
//   early-exit walk (find_walk), every family's stats getter is stats_out over
//   its StatsSlot of hm_ctx (both hm_internal.hpp), and guarded() and the
//   null-message rule (msg_or_empty) are plan.hpp's, shared with host_scan.cpp.
//   The scan kernels come from their own code object (scan_kernels.hip ->
//   align_loops.py -> hipminer_scan.hsaco, embedded by scan_blob.S), loaded
//   per device with hipModuleLoadData and launched with hipModuleLaunchKernel.
#include "build_id.h"  // generated: HM_BUILD_ID (distributed_bitcoinminer_amd/build_id.py)
#include "hm_internal.hpp"

using namespace hm;

// The scan kernels' code object (scan_blob.S .incbin of hipminer_scan.hsaco).
extern "C" const unsigned char hm_scan_code_object[];
extern "C" const unsigned char hm_scan_code_object_end[];

extern "C" {

uint64_t hm_hash(const uint8_t* msg, size_t len, uint64_t nonce) {
    const Msg m = msg_or_empty(msg, len);
    return host_hash(m.p, m.len, nonce);
}

// 1.1: hm_scan_many, hm_stats.dom_*; 1.2: hm_partition; 1.3: hm_scan_checked;
// 1.4: hm_stats.merge / dom_compressions_eff, HM_OPT_MERGE_RCCL at any device count;
// 1.5: hm_scan_stats_sized, HM_OPT_MERGE_RCCL refused up front for repeated ordinals;
// 1.6: hm_build_id, hm_stats.enqueue_ms / mid_call_syncs / table_grows, HM_OPT_TABLE_ROWS_CAP;
// 1.7: hm_scan_cpu, hm_scan_stats frozen at HM_STATS_SIZE_1_4 bytes;
// 1.8: HM_OPT_DEADLINE_MS / HM_ERR_TIMEOUT, hm_stats.deadline_ms, streams 1..
//      made on first use;
// 1.9: option ids 16 and 18 (rejected experiment hooks) retired:
//      hm_set_option answers HM_ERR_INVALID; the wave-timeline debug export removed;
//      test and experiment hooks and hm_debug_* prototypes moved to hipminer_debug.h
// 1.10: hm_find, hm_find_cpu, hm_find_stats_sized
// 1.11: hm_collect, hm_collect_cpu, hm_collect_stats_sized
// 1.12: hm_hash_many, hm_hash_many_cpu, hm_verify, hm_verify_cpu, hm_verify_stats_sized
// 1.13: hm_find_many, hm_find_many_cpu, hm_find_many_stats_sized, HM_OPT_FIND_WINDOW
// 1.14: hm_verify_many, hm_verify_many_cpu, hm_verify_many_stats_sized, HM_OPT_VERIFY_JOBS
// 1.15: hm_collect_many, hm_collect_many_cpu, hm_collect_many_stats_sized, HM_OPT_COLLECT_WINDOW
// 1.16: hm_find_k, hm_find_k_cpu, hm_find_k_stats_sized, HM_OPT_FIND_K_BUF
// 1.17: hm_find_k_many, hm_find_k_many_cpu, hm_find_k_many_stats_sized
// 1.18: hm_cancel, HM_ERR_CANCELLED, hm_cancel_stats_sized; debug export hm_debug_no_relay
// 1.19: hm_scan_k, hm_scan_k_cpu, hm_scan_k_stats_sized
int hm_version(void) { return (1 << 16) | 19; }

// The digest of the sources this library was built from (build_id.py), kept
// in the binary behind a tag so tools can read it without loading the library.
static const char kBuildTag[] = "hipminer-build-id:" HM_BUILD_ID;
const char* hm_build_id(void) { return kBuildTag + sizeof("hipminer-build-id:") - 1; }

int hm_partition(const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi, int n,
                 uint64_t* bounds) {
    if (n <= 0 || !bounds || (len > 0 && !msg)) return HM_ERR_INVALID;
    return guarded([&] {
        const MsgPlan mp = plan_message(msg_or_empty(msg, len));
        const std::vector<Shard> sh = partition_range(mp, lo, hi, n, false);
        for (int i = 0; i < n; ++i) {
            bounds[2 * i] = sh[i].empty ? 1 : sh[i].lo;
            bounds[2 * i + 1] = sh[i].empty ? 0 : sh[i].hi;
        }
        return (int)HM_OK;
    });
}

const char* hm_strerror(int rc) {
    switch (rc) {
        case HM_OK: return "ok";
        case HM_ERR_INVALID: return "invalid argument";
        case HM_ERR_NO_DEVICE: return "no usable HIP device";
        case HM_ERR_HIP: return "HIP runtime error (set HM_DEBUG=1 for details)";
        case HM_ERR_NOMEM: return "out of memory";
        case HM_ERR_RCCL: return "RCCL error";
        case HM_ERR_INTERNAL: return "internal planner error";
        case HM_ERR_TIMEOUT:
            return "GPU scan missed its deadline (HM_OPT_DEADLINE_MS); the context is "
                   "abandoned: close it, open a new one or scan on the host";
        case HM_ERR_CANCELLED:
            return "the call was stopped by hm_cancel; nothing was written and the context is "
                   "usable";
        default: return "unknown error";
    }
}

int hm_open(const int* devices, int ndev, hm_ctx** out) {
    if (!out || ndev < 0 || (ndev > 0 && !devices)) return HM_ERR_INVALID;
    *out = nullptr;
    return guarded([&] { return open_devices(devices, ndev, out); });
}

void hm_close(hm_ctx* ctx) {
    if (!ctx) return;
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        // an abandoned context (HM_ERR_TIMEOUT) may still have work running:
        // its streams, buffers and pinned readback slot are left to the
        // process exit rather than waited for
        if (!ctx->abandoned) {
            for (auto& dv : ctx->devs) device_free(dv);
            cancel_flag_free(ctx);
        }
    }
    delete ctx;
}

int hm_set_option(hm_ctx* ctx, int opt, int64_t value) {
    if (!ctx) return HM_ERR_INVALID;
    std::lock_guard<std::mutex> g(ctx->mu);
    if (ctx->abandoned) return HM_ERR_TIMEOUT;
    switch (opt) {
        case HM_OPT_DEADLINE_MS:
            if (value < -1) return HM_ERR_INVALID;
            ctx->deadline_opt = value;
            return HM_OK;
        case HM_OPT_FORCE_GENERIC: ctx->force_generic = value != 0; return HM_OK;
        case HM_OPT_MERGE_RCCL:
            // RCCL needs one rank per device: a context naming a device twice
            // can never merge over RCCL, so the option is refused up front
            if (value != 0 && !distinct_ordinals(ctx)) return HM_ERR_INVALID;
            ctx->merge_rccl = value != 0;
            return HM_OK;
        case HM_OPT_STREAMS:
            if (value < 1 || value > kStreams) return HM_ERR_INVALID;
            ctx->streams = (int)value;
            return HM_OK;
        case HM_OPT_TABLE_DIGITS:
            if (value < -1 || value > (int64_t)kMaxTableDigits) return HM_ERR_INVALID;
            ctx->table_digits = (int)value;
            return HM_OK;
        case HM_OPT_TABLE_ROWS_CAP:
            if (value < 0) return HM_ERR_INVALID;
            ctx->table_rows_cap = (uint64_t)value;
            return HM_OK;
        case HM_OPT_TEST_MID_SYNC:
            ctx->test_mid_sync = value != 0;
            return HM_OK;
        case HM_OPT_FUSED:
            ctx->fused = value != 0;
            return HM_OK;
        case HM_OPT_FUSED_FLAGS:
            if (value < 0 || value > 31) return HM_ERR_INVALID;
            ctx->fused_flags = (uint32_t)value;
            return HM_OK;
        case HM_OPT_FUSED_PARTS:
            if (value != 1 && value != 2 && value != 5 && value != 10) return HM_ERR_INVALID;
            ctx->fused_parts = (uint32_t)value;
            return HM_OK;
        case HM_OPT_QUEUE_BATCH:
            if (value != 0 && value != 4 && value != 8 && value != 16 && value != 32)
                return HM_ERR_INVALID;
            ctx->queue_batch = (int)value;
            return HM_OK;
        case HM_OPT_TAIL_FUSED:
            ctx->tail_fused = value != 0;
            return HM_OK;
        case HM_OPT_FUSED_TAIL:
            if (value != 1 && value != 2 && value != 5 && value != 10) return HM_ERR_INVALID;
            ctx->fused_tail = (uint32_t)value;
            return HM_OK;
        case HM_OPT_VERIFY_CHUNK:
            if (value < 0 || value > (int64_t)kVerifyChunk || value % kWaveSize != 0)
                return HM_ERR_INVALID;
            ctx->verify_chunk = (uint32_t)value;
            return HM_OK;
        case HM_OPT_VERIFY_JOBS:
            if (value < 0 || value > (int64_t)kVerifyJobsMax) return HM_ERR_INVALID;
            ctx->verify_jobs = (uint32_t)value;
            return HM_OK;
        case HM_OPT_FIND_WINDOW:
            if (value != 0 && (value < 64 || value > (int64_t)kFusedNonces)) return HM_ERR_INVALID;
            ctx->find_window = (uint64_t)value;
            return HM_OK;
        case HM_OPT_COLLECT_WINDOW:
            if (value != 0 && (value < 64 || value > (int64_t)kFusedNonces)) return HM_ERR_INVALID;
            ctx->collect_window = (uint64_t)value;
            return HM_OK;
        case HM_OPT_FIND_K_BUF:
            if (value != 0 && (value < 1 || value > (int64_t)HM_COLLECT_CAP_MAX))
                return HM_ERR_INVALID;
            ctx->find_k_buf = (uint32_t)value;
            return HM_OK;
        case HM_OPT_GRID_PER_CU:
            if (value < 0 || value > 32) return HM_ERR_INVALID;
            ctx->grid_per_cu = (int)value;
            return HM_OK;
        default: return HM_ERR_INVALID;
    }
}

int hm_scan_many(hm_ctx* ctx, const hm_request* reqs, int n, hm_result* outs) {
    if (!ctx || n < 0 || (n > 0 && (!reqs || !outs))) return HM_ERR_INVALID;
    for (int r = 0; r < n; ++r)
        if (!reqs[r].msg && reqs[r].len) return HM_ERR_INVALID;
    std::lock_guard<std::mutex> g(ctx->mu);
    return guarded([&] { return scan_many_locked(ctx, reqs, n, outs); });
}

int hm_scan(hm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
            hm_result* out) {
    if (!ctx || !out || (!msg && len)) return HM_ERR_INVALID;
    hm_request q{msg, len, lo, hi};
    return hm_scan_many(ctx, &q, 1, out);
}

int hm_scan_checked(hm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
                    hm_result* out, uint64_t* sum, uint64_t* count) {
    if (!ctx || !out || !sum || !count || (!msg && len)) return HM_ERR_INVALID;
    std::lock_guard<std::mutex> g(ctx->mu);
    hm_request q{msg, len, lo, hi};
    hm_result res;
    ctx->csum = true;
    int rc = guarded([&] { return scan_many_locked(ctx, &q, 1, &res); });
    ctx->csum = false;
    if (rc) return rc;
    uint64_t s = 0, c = 0;
    for (auto& dv : ctx->devs) {
        uint64_t a[kStreams * 2];
        HIPCHK(hipSetDevice(dv.ordinal));
        rc = host_read(ctx, a, dv.acc, sizeof a);
        if (rc) return rc;
        for (int i = 0; i < kStreams; ++i) { s += a[2 * i]; c += a[2 * i + 1]; }
    }
    *out = res;
    *sum = s;
    *count = c;
    return HM_OK;
}


int hm_find(hm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi, uint64_t target,
            hm_result* out, int* found) {
    if (!ctx || !out || !found || (!msg && len)) return HM_ERR_INVALID;
    std::lock_guard<std::mutex> g(ctx->mu);
    hm_result res;
    int hit = 0;
    int rc = guarded([&] { return find_locked(ctx, msg, len, lo, hi, target, &res, &hit); });
    if (rc) return rc;
    *out = res;
    *found = hit;
    return HM_OK;
}

int hm_find_stats_sized(const hm_ctx* ctx, hm_find_stats* out, size_t size) {
    return stats_out(ctx, &hm_ctx::find_stats, out, size, HM_FIND_STATS_SIZE_1_10);
}

int hm_find_many(hm_ctx* ctx, const hm_find_request* reqs, int n, hm_result* outs, int* found) {
    if (!ctx || n < 0 || (n > 0 && (!reqs || !outs || !found))) return HM_ERR_INVALID;
    for (int r = 0; r < n; ++r)
        if (!reqs[r].msg && reqs[r].len) return HM_ERR_INVALID;
    std::lock_guard<std::mutex> g(ctx->mu);
    std::vector<hm_result> res;
    std::vector<int> hit;
    int rc = guarded([&] {
        res.resize((size_t)n);
        hit.resize((size_t)n);
        return find_many_locked(ctx, reqs, n, res.data(), hit.data());
    });
    if (rc) return rc;
    // all n answers, or (on any failure above) none
    for (int r = 0; r < n; ++r) {
        outs[r] = res[r];
        found[r] = hit[r];
    }
    return HM_OK;
}

int hm_find_many_stats_sized(const hm_ctx* ctx, hm_find_many_stats* out, size_t size) {
    return stats_out(ctx, &hm_ctx::find_many_stats, out, size, HM_FIND_MANY_STATS_SIZE_1_13);
}

int hm_find_k(hm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
              uint64_t target, size_t k, hm_result* out, size_t* n) {
    if (!ctx || !out || !n || (!msg && len) || k == 0 || k > HM_FIND_K_MAX) return HM_ERR_INVALID;
    std::lock_guard<std::mutex> g(ctx->mu);
    std::vector<hm_result> recs;
    int rc = guarded([&] { return find_k_locked(ctx, msg, len, lo, hi, target, k, &recs); });
    if (rc) return rc;
    // nothing at or beyond out[*n] is touched
    if (!recs.empty()) memcpy(out, recs.data(), recs.size() * sizeof(hm_result));
    *n = recs.size();
    return HM_OK;
}

int hm_find_k_stats_sized(const hm_ctx* ctx, hm_find_k_stats* out, size_t size) {
    return stats_out(ctx, &hm_ctx::find_k_stats, out, size, HM_FIND_K_STATS_SIZE_1_16);
}

int hm_find_k_many(hm_ctx* ctx, const hm_find_k_request* reqs, int n, hm_result* out,
                   size_t* counts) {
    if (!ctx || n < 0 || (n > 0 && (!reqs || !out || !counts))) return HM_ERR_INVALID;
    for (int r = 0; r < n; ++r)
        if ((!reqs[r].msg && reqs[r].len) || reqs[r].k == 0 || reqs[r].k > HM_FIND_K_MAX)
            return HM_ERR_INVALID;
    std::lock_guard<std::mutex> g(ctx->mu);
    std::vector<std::vector<hm_result>> recs;
    int rc = guarded([&] { return find_k_many_locked(ctx, reqs, n, &recs); });
    if (rc) return rc;
    // all n answers, or (on any failure above) none; inside request i's slot
    // nothing at or beyond its counts[i] records is touched
    size_t off = 0;
    for (int r = 0; r < n; ++r) {
        if (!recs[r].empty()) memcpy(out + off, recs[r].data(), recs[r].size() * sizeof(hm_result));
        counts[r] = recs[r].size();
        off += reqs[r].k;
    }
    return HM_OK;
}

int hm_find_k_many_stats_sized(const hm_ctx* ctx, hm_find_k_many_stats* out, size_t size) {
    return stats_out(ctx, &hm_ctx::find_k_many_stats, out, size, HM_FIND_K_MANY_STATS_SIZE_1_17);
}

// hm_cancel: no ctx->mu, no HIP call (cancel.hpp).  An abandoned context has no call in
// flight, so it answers 0.
int hm_cancel(hm_ctx* ctx) {
    if (!ctx) return HM_ERR_INVALID;
    return ctx->cancel.request();
}

int hm_cancel_stats_sized(const hm_ctx* ctx, hm_cancel_stats* out, size_t size) {
    if (!ctx || !out || size < HM_CANCEL_STATS_SIZE_1_18) return HM_ERR_INVALID;
    const hm_cancel_stats st = const_cast<hm_ctx*>(ctx)->cancel.read();
    memcpy(out, &st, std::min(size, sizeof st));
    return HM_OK;
}

int hm_collect(hm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
               uint64_t target, hm_result* out, size_t cap, uint64_t* total) {
    if (!ctx || !total || (!msg && len) || cap > HM_COLLECT_CAP_MAX || (cap && !out))
        return HM_ERR_INVALID;
    std::lock_guard<std::mutex> g(ctx->mu);
    std::vector<hm_result> recs;
    uint64_t sum = 0;
    int rc = guarded(
        [&] { return collect_locked(ctx, msg, len, lo, hi, target, cap, &recs, &sum); });
    if (rc) return rc;
    // sum > cap: out is not written at all
    if (sum <= cap && sum) memcpy(out, recs.data(), (size_t)sum * sizeof(hm_result));
    *total = sum;
    return HM_OK;
}

int hm_collect_stats_sized(const hm_ctx* ctx, hm_collect_stats* out, size_t size) {
    return stats_out(ctx, &hm_ctx::collect_stats, out, size, HM_COLLECT_STATS_SIZE_1_11);
}

int hm_scan_k(hm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi, uint32_t k,
              hm_result* out, size_t* n) {
    if (!ctx || !out || !n || (!msg && len) || k == 0 || k > HM_SCAN_K_MAX) return HM_ERR_INVALID;
    std::lock_guard<std::mutex> g(ctx->mu);
    std::vector<hm_result> recs;
    int rc = guarded([&] { return scan_k_locked(ctx, msg, len, lo, hi, k, &recs); });
    if (rc) return rc;
    // nothing at or beyond out[*n] is touched
    if (!recs.empty()) memcpy(out, recs.data(), recs.size() * sizeof(hm_result));
    *n = recs.size();
    return HM_OK;
}

int hm_scan_k_stats_sized(const hm_ctx* ctx, hm_scan_k_stats* out, size_t size) {
    return stats_out(ctx, &hm_ctx::scan_k_stats, out, size, HM_SCAN_K_STATS_SIZE_1_19);
}

int hm_collect_many(hm_ctx* ctx, const hm_collect_request* reqs, int n, uint64_t* totals,
                    hm_result* out, size_t cap, uint64_t* total) {
    if (!ctx || n < 0 || (n > 0 && (!reqs || !totals)) || !total || cap > HM_COLLECT_CAP_MAX ||
        (cap && !out))
        return HM_ERR_INVALID;
    for (int r = 0; r < n; ++r)
        if (!reqs[r].msg && reqs[r].len) return HM_ERR_INVALID;
    std::lock_guard<std::mutex> g(ctx->mu);
    std::vector<uint64_t> per;
    std::vector<hm_result> recs;
    uint64_t sum = 0;
    int rc = guarded([&] { return collect_many_locked(ctx, reqs, n, cap, &per, &recs, &sum); });
    if (rc) return rc;
    // every total, and the records when they fit; on any failure above, nothing
    for (int r = 0; r < n; ++r) totals[r] = per[r];
    if (sum <= cap && sum) memcpy(out, recs.data(), (size_t)sum * sizeof(hm_result));
    *total = sum;
    return HM_OK;
}

int hm_collect_many_stats_sized(const hm_ctx* ctx, hm_collect_many_stats* out, size_t size) {
    return stats_out(ctx, &hm_ctx::collect_many_stats, out, size, HM_COLLECT_MANY_STATS_SIZE_1_15);
}

int hm_hash_many(hm_ctx* ctx, const uint8_t* msg, size_t len, const uint64_t* nonces, size_t n,
                 uint64_t* hashes) {
    if (!ctx || (!msg && len) || (n && (!nonces || !hashes))) return HM_ERR_INVALID;
    std::lock_guard<std::mutex> g(ctx->mu);
    std::vector<uint64_t> out;
    uint64_t bad = 0;
    int rc = guarded(
        [&] { return list_locked(ctx, msg, len, nonces, nullptr, n, 0, 0, &out, &bad); });
    if (rc) return rc;
    // all n hashes, or (on any failure above) nothing
    if (n) memcpy(hashes, out.data(), n * sizeof(uint64_t));
    return HM_OK;
}

int hm_verify(hm_ctx* ctx, const uint8_t* msg, size_t len, const hm_result* recs, size_t n,
              uint64_t target, uint64_t* bad_idx, size_t cap, uint64_t* bad) {
    if (!ctx || !bad || (!msg && len) || (n && !recs) || cap > HM_VERIFY_CAP_MAX ||
        (cap && !bad_idx))
        return HM_ERR_INVALID;
    std::lock_guard<std::mutex> g(ctx->mu);
    std::vector<uint64_t> idx;
    uint64_t sum = 0;
    int rc = guarded(
        [&] { return list_locked(ctx, msg, len, nullptr, recs, n, target, cap, &idx, &sum); });
    if (rc) return rc;
    // sum > cap: bad_idx is not written at all
    if (sum <= cap && sum) memcpy(bad_idx, idx.data(), (size_t)sum * sizeof(uint64_t));
    *bad = sum;
    return HM_OK;
}

int hm_verify_stats_sized(const hm_ctx* ctx, hm_verify_stats* out, size_t size) {
    return stats_out(ctx, &hm_ctx::verify_stats, out, size, HM_VERIFY_STATS_SIZE_1_12);
}

int hm_verify_many(hm_ctx* ctx, const hm_verify_request* reqs, int nreq, uint64_t* bad_per_req,
                   hm_bad_ref* refs, size_t cap, uint64_t* bad) {
    if (!ctx || nreq < 0 || (nreq > 0 && (!reqs || !bad_per_req)) || !bad ||
        cap > HM_VERIFY_CAP_MAX || (cap && !refs))
        return HM_ERR_INVALID;
    for (int r = 0; r < nreq; ++r)
        if ((!reqs[r].msg && reqs[r].len) || (!reqs[r].recs && reqs[r].n)) return HM_ERR_INVALID;
    std::lock_guard<std::mutex> g(ctx->mu);
    std::vector<uint64_t> per;
    std::vector<hm_bad_ref> out;
    uint64_t sum = 0;
    int rc = guarded([&] { return verify_many_locked(ctx, reqs, nreq, cap, &per, &out, &sum); });
    if (rc) return rc;
    // every count, and the refs when they fit; on any failure above, nothing
    for (int r = 0; r < nreq; ++r) bad_per_req[r] = per[r];
    if (sum <= cap && sum) memcpy(refs, out.data(), (size_t)sum * sizeof(hm_bad_ref));
    *bad = sum;
    return HM_OK;
}

int hm_verify_many_stats_sized(const hm_ctx* ctx, hm_verify_many_stats* out, size_t size) {
    return stats_out(ctx, &hm_ctx::verify_many_stats, out, size, HM_VERIFY_MANY_STATS_SIZE_1_14);
}

int hm_scan_stats(const hm_ctx* ctx, hm_stats* out) {
    // frozen at the 1.4/1.5 size (include/hipminer.h): newer fields only
    // through hm_scan_stats_sized
    return hm_scan_stats_sized(ctx, out, HM_STATS_SIZE_1_4);
}

int hm_scan_stats_sized(const hm_ctx* ctx, hm_stats* out, size_t size) {
    return stats_out(ctx, &hm_ctx::scan_stats, out, size, HM_STATS_SIZE_1_0);
}

// ---- debug exports for host-side tests (include/hipminer_debug.h) ----
// The embedded scan code object (scan_blob.S): bench.py hashes these bytes to
// match a PMC summary to the build that actually runs.
size_t hm_debug_code_object(const unsigned char** p) {
    if (p) *p = hm_scan_code_object;
    return (size_t)(hm_scan_code_object_end - hm_scan_code_object);
}

// HM_OPT_DEADLINE_MS = -1's deadline for one request on `cus` compute units
// (host-only; tests/test_abi.py checks the model without a GPU).
double hm_debug_auto_deadline_ms(const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
                                 int cus) {
    const hm_request q{msg, msg ? len : 0, lo, hi};
    try {
        return modelled_deadline_ms(&q, 1, false, 0, 4.0 * cus);
    } catch (...) {
        return -1.0;
    }
}

// Streams (hardware queues) made so far on device i of ctx (make_streams):
// 1 after hm_open, up to HM_OPT_STREAMS once calls used them; -1 if i is out
// of range.
int hm_debug_streams_made(const hm_ctx* ctx, int i) {
    if (!ctx || i < 0 || i >= (int)ctx->devs.size()) return -1;
    std::lock_guard<std::mutex> g(ctx->mu);
    return ctx->devs[i].nmade;
}

// hm_cancel's test hook: no relay wave and no host test of the flag (hm_internal.hpp
// cancel_ptr, cancel_seen), so a signalled call runs to its end.
int hm_debug_no_relay(hm_ctx* ctx, int on) {
    if (!ctx) return HM_ERR_INVALID;
    std::lock_guard<std::mutex> g(ctx->mu);
    ctx->no_relay = on != 0;
    return HM_OK;
}

// Writes up to `cap` segment descriptors as 13 x int64:
//   d, lo, hi, kind, W1, V, trailer, straddle, seg_cost (SIMD cycles / 64 nonces), lane3,
//   f (chained: final-block digits), tch (chained: loop values per unit),
//   fe (chained: table digits; f - fe epoch digits)
int hm_debug_plan(const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi, int force_generic,
                  int64_t* outv, int cap) {
    if (lo > hi) return 0;
    const MsgPlan mp = plan_message(msg_or_empty(msg, len));
    std::vector<SegPlan> segs;
    try {
        segs = plan_range(mp, lo, hi, force_generic != 0);
    } catch (...) {
        return HM_ERR_NOMEM;
    }
    int i = 0;
    for (; i < (int)segs.size() && i < cap; ++i) {
        const SegPlan& s = segs[i];
        int64_t* o = outv + 13 * i;
        o[0] = s.d; o[1] = (int64_t)s.lo; o[2] = (int64_t)s.hi; o[3] = s.kind;
        o[4] = s.W1; o[5] = s.V; o[6] = s.trailer; o[7] = s.straddle;
        o[8] = (int64_t)seg_cost(s);
        o[9] = s.lane3;
        o[10] = s.kind == HM_KIND_CHAINED ? s.f : 0;
        o[11] = s.kind == HM_KIND_CHAINED ? s.tch : 0;
        o[12] = s.kind == HM_KIND_CHAINED ? s.fe : 0;
    }
    return (int)segs.size();
}

}  // extern "C"
