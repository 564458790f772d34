// device.cpp -- device and context lifetime (hm_open / hm_close), the two
// counting helpers every host wait and synchronous readback goes through,
// the K+W table's growth, and a call's deadline.
#include "hm_internal.hpp"

// The scan kernels' code object (scan_blob.S .incbin of hipminer_scan.hsaco).
extern "C" const unsigned char hm_scan_code_object[];

namespace hm {

bool debug_on() {
    static const bool on = getenv("HM_DEBUG") != nullptr;
    return on;
}

int hip_fail(hipError_t e, const char* what) {
    if (debug_on()) fprintf(stderr, "hipminer: %s: %s\n", what, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? HM_ERR_NOMEM : HM_ERR_HIP;
}

int next_event(Device& dv, hipEvent_t* ev) {
    if (dv.evnext == dv.evpool.size()) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        dv.evpool.push_back(e);
    }
    *ev = dv.evpool[dv.evnext++];
    return HM_OK;
}

// Create streams nmade..n-1 of dv and their per-stream buffers (device
// current).  Stream 0 (the dominant kernel's segments, fused launches) runs
// at the highest priority, the others at the lowest: their workgroups only
// fill what the dominant persistent launch leaves free, i.e. its tail.
// Neither hipStreamCreate nor hipMalloc waits for queued work, so a call may
// make streams while it enqueues.
int make_streams(Device& dv, int n) {
    for (int s = dv.nmade; s < n && s < kStreams; ++s) {
        HIPCHK(hipStreamCreateWithPriority(&dv.stream[s], hipStreamNonBlocking,
                                           s == 0 ? dv.prio_hi : dv.prio_lo));
        HIPCHK(hipMalloc(&dv.rec[s], (size_t)kMaxTilesPerLaunch * kRecWords * sizeof(uint32_t)));
        HIPCHK(hipMalloc(&dv.cand[s], (size_t)kMaxCandWaves * 2 * sizeof(uint64_t)));
        HIPCHK(hipMalloc(&dv.kwt[s], (size_t)kMaxChainedTable * 64 * sizeof(uint32_t)));
        dv.kwt_rows[s] = kMaxChainedTable;
        HIPCHK(hipMalloc(&dv.aux[s], (size_t)kFusedAuxWords * sizeof(uint32_t)));
        HIPCHK(hipMalloc(&dv.counter[s], sizeof(unsigned int)));
        HIPCHK(hipMalloc(&dv.sums[s], (size_t)kMaxCandWaves * 2 * sizeof(uint64_t)));
        HIPCHK(hipEventCreateWithFlags(&dv.join[s], hipEventDisableTiming));
        dv.nmade = s + 1;
    }
    return HM_OK;
}

static int device_init(Device& dv, int ordinal) {
    dv.ordinal = ordinal;
    HIPCHK(hipSetDevice(ordinal));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, ordinal));
    dv.cus = prop.multiProcessorCount;
    HIPCHK(hipDeviceGetStreamPriorityRange(&dv.prio_lo, &dv.prio_hi));
    HIPCHK(hipModuleLoadData(&dv.mod, hm_scan_code_object));
    int rc = make_streams(dv, 1);
    if (rc) return rc;
    HIPCHK(hipEventCreateWithFlags(&dv.gate, hipEventDisableTiming));
    HIPCHK(hipEventCreate(&dv.t0));
    HIPCHK(hipMalloc(&dv.best, (size_t)kMaxBatch * kStreams * 2 * sizeof(uint64_t)));
    HIPCHK(hipMalloc(&dv.acc, (size_t)kStreams * 2 * sizeof(uint64_t)));
    HIPCHK(hipMalloc(&dv.result, (size_t)kMaxBatch * 2 * sizeof(uint64_t)));
    HIPCHK(hipMalloc(&dv.find_ctl, 2 * sizeof(uint64_t)));
    HIPCHK(hipMalloc(&dv.collect_ctl, 2 * sizeof(uint64_t)));
    // pinned readback slots of the 16-B result copies
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&dv.host_out), kMaxBatch * sizeof(hm_result),
                         hipHostMallocMapped | hipHostMallocCoherent));
    return HM_OK;
}

void device_free(Device& dv) {
    if (dv.ordinal < 0) return;
    (void)hipSetDevice(dv.ordinal);
    for (int s = 0; s < kStreams; ++s) {
        if (dv.stream[s]) (void)hipStreamSynchronize(dv.stream[s]);
    }
    if (dv.comm) ncclCommDestroy(dv.comm);
    for (int s = 0; s < kStreams; ++s) {
        if (dv.rec[s]) (void)hipFree(dv.rec[s]);
        if (dv.cand[s]) (void)hipFree(dv.cand[s]);
        if (dv.kwt[s]) (void)hipFree(dv.kwt[s]);
        if (dv.aux[s]) (void)hipFree(dv.aux[s]);
        if (dv.counter[s]) (void)hipFree(dv.counter[s]);
        if (dv.sums[s]) (void)hipFree(dv.sums[s]);
        if (dv.join[s]) (void)hipEventDestroy(dv.join[s]);
        if (s == 0 && dv.gate) (void)hipEventDestroy(dv.gate);
        if (s == 0 && dv.t0) (void)hipEventDestroy(dv.t0);
        if (dv.stream[s]) (void)hipStreamDestroy(dv.stream[s]);
    }
    for (void* t : dv.retired) (void)hipFree(t);
    dv.retired.clear();
    for (hipEvent_t e : dv.evpool) (void)hipEventDestroy(e);
    if (dv.mod) (void)hipModuleUnload(dv.mod);
    dv.fns.clear();
    if (dv.best) (void)hipFree(dv.best);
    if (dv.acc) (void)hipFree(dv.acc);
    if (dv.result) (void)hipFree(dv.result);
    if (dv.gathered) (void)hipFree(dv.gathered);
    if (dv.find_ctl) (void)hipFree(dv.find_ctl);
    if (dv.find_many_ctl) (void)hipFree(dv.find_many_ctl);
    if (dv.find_k_ctl) (void)hipFree(dv.find_k_ctl);
    if (dv.find_k_many_ctl) (void)hipFree(dv.find_k_many_ctl);
    if (dv.collect_ctl) (void)hipFree(dv.collect_ctl);
    if (dv.collect_buf) (void)hipFree(dv.collect_buf);
    if (dv.collect_many_ctl) (void)hipFree(dv.collect_many_ctl);
    if (dv.scan_k_ctl) (void)hipFree(dv.scan_k_ctl);
    if (dv.scan_k_waves) (void)hipFree(dv.scan_k_waves);
    if (dv.collect_tags) (void)hipFree(dv.collect_tags);
    if (dv.verify_ctl) (void)hipFree(dv.verify_ctl);
    if (dv.verify_in) (void)hipFree(dv.verify_in);
    if (dv.verify_idx) (void)hipFree(dv.verify_idx);
    if (dv.vm_blob) (void)hipFree(dv.vm_blob);
    if (dv.vm_ctl) (void)hipFree(dv.vm_ctl);
    if (dv.vm_refs) (void)hipFree(dv.vm_refs);
    for (uint64_t* p : dv.vm_stage)
        if (p) (void)hipHostFree(p);
    for (void* p : dv.retired_host) (void)hipHostFree(p);
    dv.retired_host.clear();
    if (dv.host_out) (void)hipHostFree(dv.host_out);
    dv.ordinal = -1;
}

// hm_cancel's flag: one word (a cache line of its own) of pinned host memory,
// mapped into every device and coherent, like dv.host_out; each device gets its
// own pointer to it.  The host writes it (cancel.hpp), a find launch's relay wave
// reads it (cancel_relay.hpp).
static int cancel_flag_init(hm_ctx* ctx) {
    HIPCHK(hipSetDevice(ctx->devs[0].ordinal));
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&ctx->cancel.flag), 64,
                         hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent));
    *ctx->cancel.flag = 0;
    for (Device& dv : ctx->devs) {
        HIPCHK(hipSetDevice(dv.ordinal));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&dv.cancel_dev), ctx->cancel.flag,
                                       0));
    }
    return HM_OK;
}

void cancel_flag_free(hm_ctx* ctx) {
    if (ctx->cancel.flag) (void)hipHostFree(ctx->cancel.flag);
    ctx->cancel.flag = nullptr;
}

int open_devices(const int* devices, int ndev, hm_ctx** out) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return HM_ERR_NO_DEVICE;
    std::vector<int> ords;
    if (ndev == 0) {
        for (int i = 0; i < count; ++i) ords.push_back(i);
    } else {
        for (int i = 0; i < ndev; ++i) {
            if (devices[i] < 0 || devices[i] >= count) return HM_ERR_INVALID;
            ords.push_back(devices[i]);
        }
    }
    hm_ctx* ctx = new (std::nothrow) hm_ctx;
    if (!ctx) return HM_ERR_NOMEM;
    int rc = HM_OK;
    try {
        ctx->devs.resize(ords.size());
        for (size_t i = 0; i < ords.size() && rc == HM_OK; ++i) rc = device_init(ctx->devs[i], ords[i]);
        if (rc == HM_OK) rc = cancel_flag_init(ctx);
    } catch (const std::bad_alloc&) {
        rc = HM_ERR_NOMEM;
    }
    if (rc) {
        for (auto& dv : ctx->devs) device_free(dv);
        cancel_flag_free(ctx);
        delete ctx;
        return rc;
    }
    *out = ctx;
    return HM_OK;
}

// One RCCL rank per device: does the context name every device once?
bool distinct_ordinals(const hm_ctx* ctx) {
    const size_t n = ctx->devs.size();
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < i; ++j)
            if (ctx->devs[i].ordinal == ctx->devs[j].ordinal) return false;
    return true;
}

// The host-blocking HIP calls of a scan call -- a stream wait and a
// synchronous readback -- go through these two helpers and nowhere else
// (device_free at hm_close is outside any call; tests/test_abi.py checks the
// sources for stray ones).  Each counts in hm_stats.mid_call_syncs when the
// call is still enqueuing work (on this or a later device): such a wait would
// hold back every launch after it.  No enqueue path calls them
// (HM_OPT_TEST_MID_SYNC makes one, so tests can see the counter work).  The
// enqueue path's only other host calls that are not async launches, event
// records or memsets are hipMalloc of a grown K+W table (hm_stats.table_grows)
// and of a context's streams 1.. on first use (make_streams), neither of
// which waits for queued work (tests/test_gpu_enqueue.py bounds enqueue_ms
// against the call's wall).  The library never calls hipFree during a call:
// it waits for the whole device, other contexts' work included.
//
// With a deadline (HM_OPT_DEADLINE_MS) the stream wait polls hipStreamQuery
// instead of blocking: spinning (yield) for the first 2 ms, then sleeping
// 100 us between queries.  Past the deadline it abandons the context and
// returns HM_ERR_TIMEOUT, so a hung or starved GPU scan cannot hold a miner
// whose LSP thread keeps heartbeating (lsp_client.cpp) -- the server would
// never reassign its chunk (server.go:326-376).
int host_wait(hm_ctx* ctx, hipStream_t st) {
    if (ctx->enqueuing) ++ctx->mid_syncs;
    if (!ctx->has_deadline) {
        HIPCHK(hipStreamSynchronize(st));
        return HM_OK;
    }
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(st);
        if (e == hipSuccess) return HM_OK;
        if (e != hipErrorNotReady) return hip_fail(e, "hipStreamQuery");
        const auto now = clk::now();
        if (now >= ctx->deadline_at) {
            ctx->abandoned = true;
            if (debug_on())
                fprintf(stderr, "hipminer: scan deadline of %.1f ms passed: context abandoned\n",
                        ctx->deadline_ms);
            return HM_ERR_TIMEOUT;
        }
        if (now - t0 < std::chrono::milliseconds(2)) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
}
int host_wait(hm_ctx* ctx, hipEvent_t ev) {
    if (ctx->enqueuing) ++ctx->mid_syncs;
    if (!ctx->has_deadline) {
        HIPCHK(hipEventSynchronize(ev));
        return HM_OK;
    }
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return HM_OK;
        if (e != hipErrorNotReady) return hip_fail(e, "hipEventQuery");
        const auto now = clk::now();
        if (now >= ctx->deadline_at) {
            ctx->abandoned = true;
            if (debug_on())
                fprintf(stderr, "hipminer: scan deadline of %.1f ms passed: context abandoned\n",
                        ctx->deadline_ms);
            return HM_ERR_TIMEOUT;
        }
        if (now - t0 < std::chrono::milliseconds(2)) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
}
int host_read(hm_ctx* ctx, void* dst, const void* src, size_t n) {
    if (ctx->enqueuing) ++ctx->mid_syncs;
    HIPCHK(hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
    return HM_OK;
}

// Make stream si's K+W table hold `rows` rows.  Grown once to the largest
// table used so far (10^5 .. 10^7 rows, up to 2.56 GB, for final blocks of
// >= 5 digits).  Work queued earlier on the stream may still read the old
// table, and hipFree would wait for the whole device (other contexts' work
// too), so the old table is retired and freed at hm_close.  Rows are powers
// of ten, so all tables a stream retires together hold < 1/9 of its current
// one (at most 0.28 GB beside a 2.56-GB table).
// Returns HM_ERR_NOMEM (with HIP's error state cleared, the old table kept)
// when the device cannot hold the table, or the HM_OPT_TABLE_ROWS_CAP test
// hook refuses it; the caller then plans smaller tables.
int kw_table_rows(hm_ctx* ctx, Device& dv, int si, uint64_t rows) {
    if (rows <= dv.kwt_rows[si]) return HM_OK;
    if (ctx->table_rows_cap && rows > ctx->table_rows_cap) return HM_ERR_NOMEM;
    uint32_t* t = nullptr;
    if (hipMalloc(&t, (size_t)rows * 64 * sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();
        return HM_ERR_NOMEM;
    }
    if (dv.kwt[si]) dv.retired.push_back(dv.kwt[si]);
    dv.kwt[si] = t;
    dv.kwt_rows[si] = rows;
    ++ctx->table_grows;
    return HM_OK;
}

// HM_OPT_DEADLINE_MS = -1 (auto): kDeadlineFloorMs plus kDeadlineSlack times
// the call's modelled kernel time -- every segment's nonces at its layout's
// measured SIMD cycles per 64 nonces (seg_cost, the model hm_partition
// balances shards with), over every SIMD of the context's distinct devices at
// the nominal 2.4 GHz.  The slack covers a GPU shared with other processes,
// a lowered clock and the fused launch's partial grid; hm_miner and the Go
// gpuminer use it so a hung or starved GPU scan is answered on the host
//  long before any healthy scan could finish that late.
constexpr double kDeadlineFloorMs = 2000.0;
constexpr double kDeadlineSlack = 8.0;

double modelled_deadline_ms(const hm_request* reqs, int n, bool force_generic, int table_digits,
                            double simds) {
    long double cycles = 0;
    for (int r = 0; r < n; ++r) {
        const hm_request& q = reqs[r];
        if (q.lo > q.hi) continue;
        const MsgPlan mp = plan_message(msg_or_empty(q.msg, q.len));
        for (const SegPlan& g : plan_range(mp, q.lo, q.hi, force_generic, table_digits))
            cycles += ((long double)(g.hi - g.lo) + 1) * seg_cost(g) / kWaveSize;
    }
    return kDeadlineFloorMs + kDeadlineSlack * (double)(cycles / (long double)simds / 2.4e6L);
}

static double auto_deadline_ms(const hm_ctx* ctx, const hm_request* reqs, int n) {
    std::vector<int> ords;
    for (const auto& dv : ctx->devs)
        if (std::find(ords.begin(), ords.end(), dv.ordinal) == ords.end()) ords.push_back(dv.ordinal);
    return modelled_deadline_ms(reqs, n, ctx->force_generic, ctx->table_digits,
                                4.0 * ctx->devs[0].cus * (double)ords.size());
}

static void set_deadline(hm_ctx* ctx, double auto_ms, std::chrono::steady_clock::time_point t0) {
    ctx->has_deadline = ctx->deadline_opt != 0;
    ctx->deadline_ms = !ctx->has_deadline ? 0.0
                       : ctx->deadline_opt > 0 ? (double)ctx->deadline_opt
                                               : auto_ms;
    if (ctx->has_deadline)
        ctx->deadline_at = t0 + std::chrono::duration_cast<std::chrono::steady_clock::duration>(
                                    std::chrono::duration<double, std::milli>(ctx->deadline_ms));
}

void call_deadline(hm_ctx* ctx, const hm_request* reqs, int n,
                   std::chrono::steady_clock::time_point t0) {
    set_deadline(ctx, ctx->deadline_opt < 0 ? auto_deadline_ms(ctx, reqs, n) : 0.0, t0);
}

// hm_hash_many, hm_verify and hm_verify_many have no range to model: auto is the same floor
// plus the same slack times a wall time per list element: the median wall of
// hm_verify over 4,192,403 records of the 120-B message, the slower of the two
// messages measured (1.6845 ms; profiles/verify/verify_rate.jsonl part (a)).
constexpr double kVerifyNsPerRecord = 0.402;

void list_deadline(hm_ctx* ctx, size_t n, std::chrono::steady_clock::time_point t0) {
    set_deadline(ctx, kDeadlineFloorMs + kDeadlineSlack * kVerifyNsPerRecord * 1e-6 * (double)n,
                 t0);
}

}  // namespace hm
