// hm_internal.hpp -- what the library's host sources share: the per-device
// state (Device), the context (hm_ctx), the constants, and the helpers each
// file exports to the others.  Not part of the ABI (include/hipminer.h).
//
//   plan.hpp      the planner; guarded() and msg_or_empty(), which host_scan.cpp shares
//   device.cpp    device and context lifetime, host_wait / host_read, K+W table growth, deadlines
//   seg_walk.cpp  one segment -> its sequence of launches (SegWalk), the argument fillers
//   scan.cpp      hm_scan_many: batching, the fused launch, merge, stats
//   find.cpp      hm_find; the early-exit walk's steps (find_walk, below, runs them)
//   find_k.cpp    hm_find_k, over the same walk
//   collect.cpp   hm_collect
//   scan_k.cpp    hm_scan_k
//   batch.cpp     the chunk runner of the three batch calls below: plan, prepare, launch, wait and read
//   find_many.cpp hm_find_many
//   find_k_many.cpp hm_find_k_many
//   collect_many.cpp hm_collect_many
//   verify.cpp    hm_hash_many, hm_verify
//   verify_many.cpp hm_verify_many
//   api.cpp       the extern "C" entry points and the debug exports
// Every family's stats record is a StatsSlot of hm_ctx: publish() fills it when
// a call succeeds, stats_out() is its hm_X_stats_sized.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/hipminer.h"
#include "../../include/hipminer_debug.h"
#include "cancel.hpp"
#include "kernels.hpp"
#include "plan.hpp"

namespace hm {

constexpr int kStreams = 4;
// Requests of at most this many nonces (≈3.6 ms of work) run their digit
// segments concurrently on all streams; larger ones use the dominant-stream
// order with tail filling (enqueue_device_batch).
constexpr uint64_t kConcurrentNonces = 1ull << 27;
// Workgroups per CU of a fused (small-request) launch: fewer waves per SIMD
// than occupancy allows (6), so a task's wall time, and with it the launch's
// tail, is about halved at < 1 % of issue rate; first tasks handed out by
// wave slot (no opening burst of queue atomics).  Interleaved A/B over
// flags x grids: profiles/r05/fused/fused_ab.jsonl.
constexpr int kFusedPerCu = 3;
constexpr uint32_t kFusedDefaultFlags = kFusedStaticFirst;
constexpr uint32_t kFusedDefaultParts = 1;  // tiled fused tasks: one tens digit (10 steps)
// Tasks one queue atomic fetches for a workgroup (scan_tasks.hpp lds_dequeue,
// log2): 4, and 16 for launches of at least kBigLaunchNonces nonces
// (HM_OPT_QUEUE_BATCH; configs[3]'s d = 12 launch: 9e11 nonces, ~24 s).
constexpr uint32_t kQueueShift = 2;
constexpr uint32_t kQueueShiftBig = 4;
constexpr uint64_t kBigLaunchNonces = 100000000000ull;
// Guided tail of a fused launch (HM_OPT_FUSED_TAIL): the tasks of the last,
// partial wave-round are cut into up to this many pieces each.
constexpr uint32_t kFusedDefaultTail = 2;
// hm_find and hm_collect (find.cpp, collect.cpp)
constexpr uint64_t kFindPieceNonces = 1ull << 40;    // per device and piece (multi-device)
constexpr uint64_t kFindGenericNonces = 1ull << 30;  // per generic launch
// hm_hash_many and hm_verify (verify.cpp): list elements per chunk and device
// (one copy in, one launch; HM_OPT_VERIFY_CHUNK)
constexpr uint32_t kVerifyChunk = 1u << 22;

struct Launch {
    hipEvent_t start, stop;
    uint64_t nonces;
    int kind;
    int grid;
    uint32_t compressions;
    double comp_eff;  // compressions per nonce the kernel executes (hm_stats)
    char kernel[64];  // kernel instantiation, as rocprofv3 names it (sans args)
};

struct Device {
    int ordinal = -1;
    int cus = 0;
    int prio_hi = 0, prio_lo = 0;  // stream priorities (stream 0 / streams 1..)
    // streams (and their buffers) made so far: stream 0 at hm_open, streams
    // 1.. on the first call that enqueues onto them (make_streams).  Each HIP
    // stream holds a hardware queue until the process exits, and the GPU
    // time-slices once a process set holds more than ~20, so a
    // context that only ever runs fused requests, or HM_OPT_STREAMS = 2,
    // never creates the others.
    int nmade = 0;
    hipStream_t stream[kStreams] = {};
    uint32_t* rec[kStreams] = {};
    uint32_t* kwt[kStreams] = {};
    uint32_t* aux[kStreams] = {};      // fused launches: s0 / trailer / K+W tables
    uint64_t kwt_rows[kStreams] = {};  // rows allocated (grown on demand, kw_table_rows)
    std::vector<void*> retired;        // tables and buffers replaced by larger ones, freed at hm_close
    uint64_t* cand[kStreams] = {};
    unsigned int* counter[kStreams] = {};
    uint64_t* sums[kStreams] = {};  // checked scans: per-wave (sum, count) slots
    uint64_t* acc = nullptr;        // checked scans: [kStreams][2] (sum, count)
    uint64_t* best = nullptr;      // [kMaxBatch][kStreams][2]: per request, per stream
    uint64_t* result = nullptr;    // [kMaxBatch][2]
    uint64_t* gathered = nullptr;  // [ndev][kMaxBatch][2] (RCCL merge)
    uint64_t* find_ctl = nullptr;  // hm_find: [0] the stop word, [1] tasks run (kernels.hpp FindArgs)
    // hm_find_many, made on first use: [kMaxBatch][2], request r's (stop word, tasks run)
    uint64_t* find_many_ctl = nullptr;
    // hm_find_k, made on first use: the kFkWords control words (kernels.hpp FindKArgs).  The
    // records go through collect_buf, which hm_collect and this call never use at once
    uint64_t* find_k_ctl = nullptr;
    // hm_find_k_many, made on first use: [kMaxBatch][kFkWords], the control words of request r of
    // a chunk.  The requests' record slices are laid side by side in collect_buf
    uint64_t* find_k_many_ctl = nullptr;
    // hm_collect: [0] total, [1] slot cursor (kernels.hpp CollectArgs), and the record buffer of
    // collect_cap records, grown when a larger cap arrives (the old one joins `retired`)
    uint64_t* collect_ctl = nullptr;
    uint64_t* collect_buf = nullptr;
    size_t collect_cap = 0;
    // hm_collect_many, made on first use: [0] the chunk's slot cursor, [1 + r] request r's total
    // (kMaxBatch + 1 words); the tag buffer of collect_tags_cap 32-bit words (the request of each
    // record slot), grown like collect_buf (grow_buffer).  The records go through collect_buf,
    // which hm_collect and this call never use at once
    uint64_t* collect_many_ctl = nullptr;
    uint32_t* collect_tags = nullptr;
    size_t collect_tags_cap = 0;
    // hm_hash_many / hm_verify, all made on first use: [0] total, [1] slot cursor (kernels.hpp
    // VerifyArgs); the chunk buffer of verify_in_bytes bytes (nonces, or 16-byte records) and the
    // index buffer of verify_idx_cap indices, grown like collect_buf
    uint64_t* verify_ctl = nullptr;
    uint64_t* verify_in = nullptr;
    size_t verify_in_bytes = 0;
    uint64_t* verify_idx = nullptr;
    size_t verify_idx_cap = 0;
    // hm_verify_many, all made on first use and grown like collect_buf: two pinned staging slots
    // (a launch's [job table | task_job | records], used alternately), the device blob they are
    // copied to, the control words ([0] slot cursor, [1 + j] the bad count of the call's job j on
    // this device) and the buffer of vm_refs_cap 16-byte refs
    uint64_t* vm_stage[2] = {};
    size_t vm_stage_bytes[2] = {};
    std::vector<void*> retired_host;  // pinned slots replaced by larger ones, freed at hm_close
    uint64_t* vm_blob = nullptr;
    size_t vm_blob_bytes = 0;
    uint64_t* vm_ctl = nullptr;
    size_t vm_ctl_words = 0;
    uint64_t* vm_refs = nullptr;
    size_t vm_refs_cap = 0;
    // hm_scan_k, both made on first use: the kSkWords control words and device list (kernels.hpp
    // ScanKArgs), and the wave-list buffer: kMaxCandWaves slots of kScanKMax records, then the
    // kMaxCandWaves 32-bit counts
    uint64_t* scan_k_ctl = nullptr;
    uint64_t* scan_k_waves = nullptr;
    hm_result* host_out = nullptr; // pinned, fine-grained [kMaxBatch]: the 16-B readback slots
    // hm_cancel: this device's pointer to the context's cancel flag (hm_ctx::cancel.flag)
    uint32_t* cancel_dev = nullptr;
    hipEvent_t join[kStreams] = {};
    hipEvent_t gate = nullptr;     // stream 0 reached its last dominant segment
    hipEvent_t t0 = nullptr;       // timing origin of the current call
    std::vector<hipEvent_t> evpool;
    size_t evnext = 0;
    std::vector<Launch> launches;
    ncclComm_t comm = nullptr;
    hipModule_t mod = nullptr;  // scan kernels (hipminer_scan.hsaco)
    struct Fn { std::string sym; hipFunction_t fn; int blocks_per_cu; };
    std::deque<Fn> fns;         // resolved on first use (stable addresses)
};

bool debug_on();
int hip_fail(hipError_t e, const char* what);

#define HIPCHK(expr)                                   \
    do {                                               \
        hipError_t e_ = (expr);                        \
        if (e_ != hipSuccess) return hm::hip_fail(e_, #expr); \
    } while (0)

// A family's stats record: the last successful call's, once there was one.
template <class T>
struct StatsSlot {
    bool have = false;
    T v{};
};

}  // namespace hm

struct hm_ctx {
    mutable std::mutex mu;
    std::vector<hm::Device> devs;
    bool force_generic = false;
    bool merge_rccl = false;
    int grid_per_cu = 0;
    int streams = hm::kStreams;  // HM_OPT_STREAMS (tail filling by default)
    int table_digits = 0;    // HM_OPT_TABLE_DIGITS (test hook; 0 = default, -1 = off)
    uint64_t table_rows_cap = 0;  // HM_OPT_TABLE_ROWS_CAP (test hook; 0 = off)
    bool test_mid_sync = false;   // HM_OPT_TEST_MID_SYNC (test hook: a host wait mid-enqueue)
    bool fused = true;            // HM_OPT_FUSED: small requests in one launch
    uint32_t fused_flags = hm::kFusedDefaultFlags;  // HM_OPT_FUSED_FLAGS (experiment hook)
    uint32_t fused_parts = hm::kFusedDefaultParts;  // HM_OPT_FUSED_PARTS (experiment hook)
    uint32_t fused_tail = hm::kFusedDefaultTail;    // HM_OPT_FUSED_TAIL (1 = no split)
    bool tail_fused = true;  // HM_OPT_TAIL_FUSED: a large request's tail segments in one fused launch
    int queue_batch = 0;     // HM_OPT_QUEUE_BATCH: 0 = auto, else tasks per queue atomic (4..32)
    uint32_t verify_chunk = 0;  // HM_OPT_VERIFY_CHUNK (test hook; 0 = kVerifyChunk)
    uint32_t verify_jobs = 0;   // HM_OPT_VERIFY_JOBS (test hook; 0 = kVerifyJobsMax)
    uint64_t find_window = 0;   // HM_OPT_FIND_WINDOW (test hook; 0 = kFusedNonces)
    uint64_t collect_window = 0;  // HM_OPT_COLLECT_WINDOW (test hook; 0 = kFusedNonces)
    uint32_t find_k_buf = 0;      // HM_OPT_FIND_K_BUF (test hook; 0 = min(cap max, 2k + 4096))
    // host waits on GPU work while the call is still enqueuing (hm_stats.mid_call_syncs)
    bool enqueuing = false;
    int32_t mid_syncs = 0;
    int32_t table_grows = 0;
    double enqueue_ms = 0;
    bool csum = false;  // inside hm_scan_checked: checked kernels + coverage sums
    // HM_OPT_DEADLINE_MS: 0 = none (the host blocks until the GPU is done),
    // > 0 = that many ms per call, -1 = auto (deadline_for).  Past the
    // deadline a call returns HM_ERR_TIMEOUT and the context is abandoned:
    // its queued work may still run, so no later call touches its devices
    // and hm_close leaks them rather than wait (SURVEY §8(b) liveness).
    int64_t deadline_opt = 0;
    bool has_deadline = false;
    std::chrono::steady_clock::time_point deadline_at{};
    double deadline_ms = 0;  // the current call's deadline (hm_stats.deadline_ms)
    bool abandoned = false;
    // hm_cancel (cancel.hpp): the flag (pinned host memory, made at hm_open), cancel_mu, whether
    // a cancellable call is in flight, the timestamp and the record.  Not guarded by `mu`.
    hm::CancelState cancel;
    bool no_relay = false;  // hm_debug_no_relay (test hook: cancel reaches neither GPU nor host)
    int merge = HM_MERGE_NONE;  // how the current call merged device results
    // every family keeps its own record: hm_find leaves the last scan's alone
    hm::StatsSlot<hm_stats> scan_stats;
    hm::StatsSlot<hm_find_stats> find_stats;
    hm::StatsSlot<hm_collect_stats> collect_stats;
    hm::StatsSlot<hm_verify_stats> verify_stats;  // hm_hash_many and hm_verify
    hm::StatsSlot<hm_find_many_stats> find_many_stats;
    hm::StatsSlot<hm_verify_many_stats> verify_many_stats;
    hm::StatsSlot<hm_collect_many_stats> collect_many_stats;
    hm::StatsSlot<hm_find_k_stats> find_k_stats;
    hm::StatsSlot<hm_find_k_many_stats> find_k_many_stats;
    hm::StatsSlot<hm_scan_k_stats> scan_k_stats;
};

namespace hm {

// hm_X_stats_sized: the first min(size, sizeof(T)) bytes of the slot's record.  A caller built
// against an older header passes its smaller struct (the layouts only ever grow at the end);
// min_size is the family's first layout.
template <class T>
int stats_out(const hm_ctx* ctx, StatsSlot<T> hm_ctx::*slot, T* out, size_t size, size_t min_size) {
    if (!ctx || !out || size < min_size) return HM_ERR_INVALID;
    std::lock_guard<std::mutex> g(ctx->mu);  // calls write their slot under the lock
    if (!(ctx->*slot).have) return HM_ERR_INVALID;
    memcpy(out, &(ctx->*slot).v, std::min(size, sizeof(T)));
    return HM_OK;
}
// The close of a successful call that began at t0 (ctx->mu held): st, with the
// two fields every family has, becomes the slot's record.
template <class T>
void publish(hm_ctx* ctx, StatsSlot<T>& slot, T st, std::chrono::steady_clock::time_point t0) {
    st.ndev = (int)ctx->devs.size();
    st.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0)
                     .count();
    slot.v = st;
    slot.have = true;
}
// A control block of `words` words on the current device, made on first use.
inline int ctl_block(uint64_t** p, size_t words) {
    if (!*p) HIPCHK(hipMalloc(p, words * sizeof(uint64_t)));
    return HM_OK;
}

// ---- device.cpp ----
int open_devices(const int* devices, int ndev, hm_ctx** out);
void device_free(Device& dv);
void cancel_flag_free(hm_ctx* ctx);  // hm_close, after every device_free
bool distinct_ordinals(const hm_ctx* ctx);
int next_event(Device& dv, hipEvent_t* ev);
int make_streams(Device& dv, int n);
int host_wait(hm_ctx* ctx, hipStream_t st);
// The same wait for one event of a stream (hm_verify_many's staging slots).
int host_wait(hm_ctx* ctx, hipEvent_t ev);
int host_read(hm_ctx* ctx, void* dst, const void* src, size_t n);
int kw_table_rows(hm_ctx* ctx, Device& dv, int si, uint64_t rows);
double modelled_deadline_ms(const hm_request* reqs, int n, bool force_generic, int table_digits,
                            double simds);
// Set the deadline of a call over `reqs` that began at t0 (HM_OPT_DEADLINE_MS).
void call_deadline(hm_ctx* ctx, const hm_request* reqs, int n,
                   std::chrono::steady_clock::time_point t0);
// Set the deadline of an hm_hash_many or hm_verify call over n list elements.
void list_deadline(hm_ctx* ctx, size_t n, std::chrono::steady_clock::time_point t0);

// ---- seg_walk.cpp ----
// Which kernels run a segment: the scan's, its checked variants, hm_find's,
// hm_collect's, hm_find_k's or hm_scan_k's.
enum class Family { Scan, ScanCsum, Find, Collect, FindK, ScanK };
// The kernel of `family` for a segment of `kind` (s: the tiled instantiation's
// template arguments; unused otherwise): its mangled name in
// hipminer_scan.hsaco and the name rocprofv3 prints (sans arguments).
struct KernelName {
    std::string symbol, display;
};
KernelName kernel_name(Family family, int kind, const SegPlan* s);
int scan_fn(Device& dv, const std::string& sym, const Device::Fn** out);
int persistent_grid(const hm_ctx* ctx, const Device& dv, int per_cu_auto, uint64_t ntasks);
void launch_units(const SegPlan& s, uint64_t t, uint64_t nt, uint64_t per_chunk, uint64_t step,
                  uint32_t* unit0, uint64_t* nunits);
uint32_t count_compressions(const SegPlan& s);
double executed_compressions(const SegPlan& s);

// Launch a scan kernel with its argument block (the kernel's only, by-value
// parameter) on `grid` workgroups of kBlock threads.
template <typename Args>
int launch_scan(const Device::Fn& f, const Args& args, int grid, hipStream_t st) {
    if (grid < 1 || (uint32_t)grid * (kBlock / kWaveSize) > kMaxCandWaves)
        return hip_fail(hipErrorInvalidValue, "scan grid");
    size_t size = sizeof(Args);
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, const_cast<Args*>(&args),
                   HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    HIPCHK(hipModuleLaunchKernel(f.fn, (unsigned)grid, 1, 1, kBlock, 1, 1, 0, st, nullptr, cfg));
    return HM_OK;
}

// One launch of a segment, as SegWalk::next yields it.
struct SegStep {
    int kind;        // HM_KIND_*: which of t, c, g is filled (cand and sums null)
    TiledArgs t;
    ChainedArgs c;
    GenericArgs g;
    // the launch's smallest nonce (a wrap past 2^64 in a segment's last tile
    // only makes it look lower: to hm_find a launch more, never one less)
    uint64_t base;
    uint64_t nonces;  // chained: the epoch's share of the tiles' nonces (an estimate)
    uint64_t nunits;  // work units kept (launch_units)
    uint32_t ntasks;  // tasks (generic: wave steps of 64 nonces)
    int grid;
    // what the stream-side prologue needs
    uint64_t tile, ntiles, epoch;
    uint32_t unit0;
};
// What follows a step's argument block in the kernel's parameter: nothing
// (scan), FindArgs, CollectArgs, FindKArgs or ScanKArgs -- the layout of
// kernels.hpp's Find*Args, Collect*Args, FindK*Args and ScanK*Args.
struct NoTrailer {};
template <typename Base, typename Trailer>
struct WithTrailer {
    Base b;
    Trailer t;
};
static_assert(sizeof(WithTrailer<TiledArgs, FindArgs>) == sizeof(FindTiledArgs) &&
              sizeof(WithTrailer<ChainedArgs, FindArgs>) == sizeof(FindChainedArgs) &&
              sizeof(WithTrailer<GenericArgs, FindArgs>) == sizeof(FindGenericArgs) &&
              sizeof(WithTrailer<TiledArgs, CollectArgs>) == sizeof(CollectTiledArgs) &&
              sizeof(WithTrailer<ChainedArgs, CollectArgs>) == sizeof(CollectChainedArgs) &&
              sizeof(WithTrailer<GenericArgs, CollectArgs>) == sizeof(CollectGenericArgs) &&
              sizeof(WithTrailer<TiledArgs, FindKArgs>) == sizeof(FindKTiledArgs) &&
              sizeof(WithTrailer<ChainedArgs, FindKArgs>) == sizeof(FindKChainedArgs) &&
              sizeof(WithTrailer<GenericArgs, FindKArgs>) == sizeof(FindKGenericArgs) &&
              sizeof(WithTrailer<TiledArgs, ScanKArgs>) == sizeof(ScanKTiledArgs) &&
              sizeof(WithTrailer<ChainedArgs, ScanKArgs>) == sizeof(ScanKChainedArgs) &&
              sizeof(WithTrailer<GenericArgs, ScanKArgs>) == sizeof(ScanKGenericArgs));

// A resumable cursor over the launches of one segment on one device and
// stream.  Generic segments run in chunks of `generic_chunk` nonces; tiled ones
// in windows of at most max_launch_tiles tiles; chained ones in epochs (one
// K+W table each) of such windows: epoch-major, then ascending tiles.  next()
// only plans a launch; launch() puts it, after its prologue, on the stream.
struct SegWalk {
    // Start on segment seg; generic_chunk = 0: the whole segment in one launch.
    // A chained segment gets its table here (chained_table: on a device short
    // of memory the walk's private copy of the plan has more, smaller epochs).
    int open(hm_ctx* ctx, Device& dv, const MsgPlan& mp, int si, const SegPlan& seg, Family family,
             uint64_t generic_chunk);
    // The next launch, advancing past it; false: none left.
    bool next(SegStep* step);
    // hm_find's pruning: the next launch's `base` without advancing (false:
    // none left); whether that launch is its epoch's first; drop the rest of
    // the epoch, or of the segment.
    bool peek_base(uint64_t* base) const;
    bool epoch_first() const { return s.kind != HM_KIND_GENERIC && t == s.tile_lo; }
    void skip_epoch() { ++e; t = s.tile_lo; }
    void close() { e = nep; }
    // Enqueue a step: its prologue (K+W table when the epoch on the stream
    // changes, tile records, queue-counter reset), then the family's kernel
    // with the step's argument block followed by `trailer`, between the events
    // `start` and `stop` (either may be null: not recorded).
    template <typename Trailer>
    int launch(const SegStep& step, const Trailer& trailer, hipEvent_t start, hipEvent_t stop);

    SegPlan s;        // the segment as it runs
    KernelName name;  // the kernel that runs it

private:
    int prologue(const SegStep& step);
    template <typename Base, typename Trailer>
    int launch_args(const Base& base, const Trailer& trailer, const SegStep& step,
                    hipEvent_t start, hipEvent_t stop);

    hm_ctx* ctx = nullptr;
    Device* dv = nullptr;
    const MsgPlan* mp = nullptr;
    const Device::Fn* fn = nullptr;
    int si = 0;
    uint64_t chunk_m1 = 0;     // generic: nonces per launch - 1
    uint64_t nep = 0;          // epochs (1 unless chained); e == nep: no launch left
    uint64_t nloop = 0;        // chained: table rows = loop values per lane and epoch
    uint64_t max_tiles = 0;
    uint32_t kw[64] = {};      // the trailer block's K+W (zeros without a trailer)
    uint64_t e = 0, t = 0, g = 0;    // cursor: epoch, tile, generic nonce
    uint64_t table_epoch = ~0ull;    // chained: epoch of the K+W table on the stream
};

template <typename Base, typename Trailer>
int SegWalk::launch_args(const Base& base, const Trailer& trailer, const SegStep& step,
                         hipEvent_t start, hipEvent_t stop) {
    hipStream_t st = dv->stream[si];
    int rc = prologue(step);
    if (rc) return rc;
    if (start) HIPCHK(hipEventRecord(start, st));
    if constexpr (std::is_same_v<Trailer, NoTrailer>) {
        rc = launch_scan(*fn, base, step.grid, st);
    } else {
        rc = launch_scan(*fn, WithTrailer<Base, Trailer>{base, trailer}, step.grid, st);
    }
    if (rc) return rc;
    if (stop) HIPCHK(hipEventRecord(stop, st));
    return HM_OK;
}

template <typename Trailer>
int SegWalk::launch(const SegStep& step, const Trailer& trailer, hipEvent_t start,
                    hipEvent_t stop) {
    switch (step.kind) {
        case HM_KIND_TILED: return launch_args(step.t, trailer, step, start, stop);
        case HM_KIND_CHAINED: return launch_args(step.c, trailer, step, start, stop);
        default: return launch_args(step.g, trailer, step, start, stop);
    }
}

// The pieces hm_find and hm_collect cut [lo, hi] into, in ascending order:
// each digit segment is one piece; with several devices, pieces of at most
// kFindPieceNonces per device, cut at tile boundaries and split across the
// devices with partition_range.
struct PieceWalk {
    PieceWalk(const hm_ctx* ctx, const MsgPlan& mp, uint64_t lo, uint64_t hi);
    // The next piece: (*shards)[i] = device i's segments (none: no share of
    // this piece).  false: no piece left.
    bool next(std::vector<std::vector<SegPlan>>* shards);

private:
    const hm_ctx* ctx;
    const MsgPlan& mp;
    std::vector<SegPlan> segs;
    size_t i = 0;
    uint64_t a = 0;  // the next piece's first nonce
};

// The opening of an hm_find or hm_collect call that began at t0: a null
// message is the empty one (*m, *mlen), the call's deadline is set; refuses an
// abandoned context.
int begin_ranged_call(hm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
                      std::chrono::steady_clock::time_point t0, const uint8_t** m, size_t* mlen);
// A find, collect, hash_many, verify or verify_many that fails part-way with rc leaves nothing behind: every
// device's stream 0 is waited for (launches still queued use its record,
// table, counter and control buffers) and its timing events are free again.
// After a timeout the context is abandoned and nothing is waited for, as for
// a scan.  Returns rc.
int drain_failed(hm_ctx* ctx, int rc);

// ---- hm_cancel: the call's side (cancel.hpp has the state machine and its rules) ----
// A cancellable call -- hm_find, hm_find_k, hm_find_many, hm_find_k_many -- from just after its
// opening (begin_ranged_call, batch_open) to its return, ctx->mu held: the flag is cleared and
// the call is in flight for hm_cancel while the scope lives.  The call returns through end(rc);
// a cancelled call whose drain missed the deadline is a timeout (the context is abandoned).
struct CancelScope {
    CancelScope(hm_ctx* ctx, int family) : ctx(ctx) { ctx->cancel.begin(family); }
    ~CancelScope() { ctx->cancel.finish(rc); }
    CancelScope(const CancelScope&) = delete;
    CancelScope& operator=(const CancelScope&) = delete;
    int end(int r) { return rc = r == HM_ERR_CANCELLED && ctx->abandoned ? HM_ERR_TIMEOUT : r; }

private:
    hm_ctx* ctx;
    int rc = HM_OK;
};
// What a find-family launch gets as FindArgs::cancel / FindKArgs::cancel.
inline const uint32_t* cancel_ptr(const hm_ctx* ctx, const Device& dv) {
    return ctx->no_relay ? nullptr : dv.cancel_dev;
}
// The host's test of the flag: after every wait or readback and BEFORE any control word is
// interpreted (a set flag means the words may be forged, cancel_relay.hpp), and before work is
// issued.
inline bool cancel_seen(const hm_ctx* ctx) { return !ctx->no_relay && ctx->cancel.seen(); }
// The flag was seen with `inflight` launches queued or running: HM_ERR_CANCELLED, which the
// caller returns through drain_failed / drain_streams.
inline int cancel_observed(hm_ctx* ctx, int inflight) {
    ctx->cancel.observed(inflight);
    return HM_ERR_CANCELLED;
}

// ---- scan.cpp: the fused launch, shared with batch.cpp ----
bool fusible(const std::vector<SegPlan>& segs);
// The task order of a fused launch without an early exit: costliest layout
// first, larger segments first (the launch ends on its cheapest tasks).
void fused_order(std::vector<SegPlan>* segs);
// A fused launch as plan_fused lays it out.  The caller sets the outputs
// (pa.result, pa.acc, pa.n_acc; fa.cand, fa.sums) and launches.
struct FusedLaunch {
    FusedPlanArgs pa;
    FusedArgs fa;
    int grid;
    uint64_t nonces;
    uint32_t comp_max;  // hm_stats: compressions per nonce, the largest of the segments
    double comp_eff;    // and those executed, nonce-weighted
};
int plan_fused(hm_ctx* ctx, Device& dv, const MsgPlan& mp, const std::vector<SegPlan>& segs, int si,
               uint32_t flags, FusedLaunch* out);

// ---- find.cpp: hm_find without its opening and its stats, for hm_find_many's fallback ----
struct FindTally {
    uint64_t nonces = 0, tasks = 0, run = 0;
    int launches = 0;
    double kernel_ms = 0;
};
// The lowest nonce of [lo, hi] whose hash is below target, on stream 0 through
// the per-segment find kernels: *res and *hit as hm_find returns them, the
// work added to *tally.  The call's deadline is already set; on failure the
// streams are drained (drain_failed).
int find_core(hm_ctx* ctx, const uint8_t* m, size_t mlen, uint64_t lo, uint64_t hi, uint64_t target,
              FindTally* tally, hm_result* res, int* hit);

// ---- find.cpp: the early-exit walk, shared with find_k.cpp ----
constexpr int kFindLookahead = 4;  // launches in flight per device
// One device's walk through its shard of a piece.
struct FindDev {
    std::vector<SegPlan> segs;  // the shard's segments (one digit count: one)
    size_t si = 0;
    bool seg_open = false;      // `walk` is on segs[si]
    SegWalk walk;
    int inflight = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> evs;
    uint64_t ctl[kFkWords] = {~0ull};  // last readback of the call's control words ([0]: stop)
};
// Plan the device's next launch whose smallest nonce is <= best (the pruning
// bound; MaxUint64 = none), opening segments with `family`'s kernels; a pruned
// launch is dropped.  false in *have: nothing left to issue in this piece.
int find_next_step(hm_ctx* ctx, Device& dv, FindDev& fd, const MsgPlan& mp, Family family,
                   uint64_t best, SegStep* step, bool* have);
// Issue that launch with the trailer make(step.base) between two timing events
// and count it.  *issued = false: nothing left to issue in this piece.
template <typename Make>
int find_issue(hm_ctx* ctx, Device& dv, FindDev& fd, const MsgPlan& mp, Family family,
               uint64_t best, FindTally& tally, bool* issued, Make&& make) {
    *issued = false;
    SegStep step;
    bool have = false;
    int rc = find_next_step(ctx, dv, fd, mp, family, best, &step, &have);
    if (rc || !have) return rc;
    hipEvent_t a, b;
    rc = next_event(dv, &a);
    if (rc) return rc;
    rc = next_event(dv, &b);
    if (rc) return rc;
    fd.evs.push_back({a, b});
    rc = fd.walk.launch(step, make(step.base), a, b);
    if (rc) return rc;
    tally.nonces += step.nonces;
    tally.tasks += step.ntasks;
    ++tally.launches;
    ++fd.inflight;
    *issued = true;
    return HM_OK;
}
// Wait for the device's launches in flight and read the call's first `nwords`
// control words at dev_ctl back into fd.ctl.
int find_collect(hm_ctx* ctx, Device& dv, FindDev& fd, FindTally& tally, const uint64_t* dev_ctl,
                 int nwords);
// The walk of hm_find and hm_find_k over [lo, hi] (find.cpp has the rules): pieces in ascending
// order; within a piece each device issues up to kFindLookahead launches of `family` with the
// trailer make(dv, launch_lo), then its first `nwords` control words at dv.*ctl are read back
// into fds[i].ctl and *best, the pruning bound, is lowered to word 0, the stop word.  It ends
// once *best is set or nothing is left.  The caller has reset the control words on stream 0.
// Every failure leaves through drain_failed.
template <typename Make>
int find_walk(hm_ctx* ctx, const MsgPlan& mp, uint64_t lo, uint64_t hi, Family family,
              uint64_t* Device::*ctl, int nwords, std::vector<FindDev>& fds, FindTally& tally,
              uint64_t* best, Make&& make) {
    static_assert(kFkStop == 0, "the stop word is the first of the control words");
    const int ndev = (int)ctx->devs.size();
    *best = ~0ull;
    PieceWalk pieces(ctx, mp, lo, hi);
    std::vector<std::vector<SegPlan>> shards;
    // hm_cancel: the flag is tested before each launch is issued and after each find_collect,
    // before the control words it read are looked at (they may be forged)
    auto in_flight = [&] {
        int n = 0;
        for (const FindDev& fd : fds) n += fd.inflight;
        return n;
    };
    // later pieces lie above a hit (hm_find_k: above every record written so far, the bound
    // among them)
    while (*best == ~0ull && pieces.next(&shards)) {
        for (int i = 0; i < ndev; ++i) {
            fds[i].segs = std::move(shards[i]);
            fds[i].si = 0;
            fds[i].seg_open = false;
        }
        for (;;) {
            bool any = false;
            for (int i = 0; i < ndev; ++i) {
                Device& dv = ctx->devs[i];
                if (hipSetDevice(dv.ordinal) != hipSuccess) return drain_failed(ctx, HM_ERR_HIP);
                while (fds[i].inflight < kFindLookahead) {
                    if (cancel_seen(ctx))
                        return drain_failed(ctx, cancel_observed(ctx, in_flight()));
                    bool issued = false;
                    int rc = find_issue(ctx, dv, fds[i], mp, family, *best, tally, &issued,
                                        [&](uint64_t launch_lo) { return make(dv, launch_lo); });
                    if (rc) return drain_failed(ctx, rc);
                    if (!issued) break;
                }
                any = any || fds[i].inflight > 0;
            }
            if (!any) break;
            for (int i = 0; i < ndev; ++i) {
                if (!fds[i].inflight) continue;
                Device& dv = ctx->devs[i];
                const int waited_for = in_flight();
                int rc = find_collect(ctx, dv, fds[i], tally, dv.*ctl, nwords);
                if (rc) return drain_failed(ctx, rc);
                if (cancel_seen(ctx)) return drain_failed(ctx, cancel_observed(ctx, waited_for));
                *best = std::min(*best, fds[i].ctl[0]);
            }
        }
    }
    return HM_OK;
}

// ---- find_k.cpp: hm_find_k without its opening and its stats, for hm_find_k_many's fallback ----
struct FindKTally {
    FindTally t;           // launches, tasks and kernel time, the overflow path's included
    uint64_t records = 0;  // records read back (min(cursor, buffer) summed over devices)
    bool overflow = false; // a device's buffer overflowed: the answer came from the overflow path
};
// The k lowest hits of [lo, hi], on stream 0 through the per-segment find_k
// kernels: *recs as hm_find_k returns it, the work added to *tally.  The
// call's deadline is already set; on failure the streams are drained
// (drain_failed).
int find_k_core(hm_ctx* ctx, const uint8_t* m, size_t mlen, uint64_t lo, uint64_t hi,
                uint64_t target, size_t k, FindKTally* tally, std::vector<hm_result>* recs);

// ---- collect.cpp: hm_collect without its opening and its stats, for hm_collect_many's fallback ----
struct CollectTally {
    uint64_t nonces = 0;
    int launches = 0;
    double kernel_ms = 0;
};
// Every nonce of [lo, hi] whose hash is below target, on stream 0 through the
// per-segment collect kernels: *recs and *total as collect_locked returns
// them, the work added to *tally.  The call's deadline is already set.
int collect_core(hm_ctx* ctx, const uint8_t* m, size_t mlen, uint64_t lo, uint64_t hi,
                 uint64_t target, size_t cap, CollectTally* tally, std::vector<hm_result>* recs,
                 uint64_t* total);
// Records as a device handed them out, in dispatch order: sorted by nonce, then
// HM_ERR_INTERNAL on a duplicate, a nonce outside [lo, hi] or a hash at or
// above target.
int sort_check_records(std::vector<hm_result>* recs, uint64_t lo, uint64_t hi, uint64_t target);

// ---- batch.cpp: one chunk of hm_find_many, hm_collect_many or hm_find_k_many ----
// One request of a chunk.
struct BatchReq {
    const uint8_t* m;  // a null message is the empty one
    size_t mlen;
    bool live = false;      // lo <= hi and target != 0: something to hash
    bool launched = false;  // its fused launch was enqueued
    uint64_t fused_hi = 0;  // launched: the last nonce of the launch
    int dev = 0;            // (index0 + r) mod ndev
    MsgPlan mp;
    std::vector<SegPlan> segs;  // what its fused launch holds; none: not fused
    hipEvent_t a = nullptr, b = nullptr;
};
// A chunk of at most kMaxBatch requests, from planning to readback.  The
// family's file drives it: add() per request, prepare(), launch(), finish();
// what lies between and after them (buffers, answers, fallbacks) is the
// family's own.  Every device is enqueued before the host waits on any.
struct BatchChunk {
    // Requests index0.. of the call; a fused launch holds at most `window`
    // nonces.  whole = false (an early-exit family): the longest prefix of the
    // window's segments, ascending by nonce, that fusible() accepts.  whole =
    // true: a request of at most `window` nonces all of whose segments
    // fusible() accepts, in fused_order; any other request is not fused.
    BatchChunk(hm_ctx* ctx, int index0, uint64_t window, bool whole);
    // Plan the chunk's next request.
    BatchReq& add(const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi, uint64_t target);
    // The streams device i's launches round-robin over.
    int used(int i) const { return std::min(nstreams, nfused[i]); }
    // Each device with a launch: its control block Device::*ctl of `words`
    // words (made on first use) and its streams.
    int prepare(uint64_t* Device::*ctl, size_t words);
    // Enqueue every fused request, each on its device's next stream: the
    // planner, then the family's fused kernel `name` on an Args block, between the
    // request's two events.  fill(r, R, dv, stream, &fl, &ka) sets the planner's
    // outputs (fl.pa.result / acc / n_acc) and ka but ka.a, and may enqueue
    // onto the stream what must precede the planner.  The launches' nonces,
    // tasks and count are added to *tally.
    template <typename Args, typename Fill>
    int launch(const KernelName& name, FindTally* tally, Fill&& fill);
    // Wait for every used stream of every device, then read the first `words`
    // words of each device's control block into ctl[i]; the launches' event
    // times are added to tally->kernel_ms and the events are free again.
    int finish(uint64_t* Device::*ctl, size_t words, FindTally* tally);

    hm_ctx* ctx;
    int index0, ndev, nstreams;
    uint64_t window;
    bool whole;
    std::vector<BatchReq> rq;
    std::vector<int> nfused;                 // per device: requests with a launch
    std::vector<std::vector<uint64_t>> ctl;  // per device: the control words read back

private:
    // Request r's stream and plan; *fn = the family's kernel.
    int plan_launch(int r, const std::string& symbol, int* si, FusedLaunch* fl,
                    const Device::Fn** fn);
    std::vector<int> rr;  // per device: launches so far
};

template <typename Args, typename Fill>
int BatchChunk::launch(const KernelName& name, FindTally* tally, Fill&& fill) {
    for (int r = 0; r < (int)rq.size(); ++r) {
        BatchReq& R = rq[r];
        if (R.segs.empty()) continue;
        Device& dv = ctx->devs[R.dev];
        int si;
        FusedLaunch fl;
        const Device::Fn* fn = nullptr;
        int rc = plan_launch(r, name.symbol, &si, &fl, &fn);
        if (rc) return rc;
        hipStream_t s = dv.stream[si];
        Args ka;
        rc = fill(r, R, dv, s, &fl, &ka);
        if (rc) return rc;
        ka.a = fl.fa;
        HIPCHK(launch_fused_plan(fl.pa, s));
        HIPCHK(hipEventRecord(R.a, s));
        rc = launch_scan(*fn, ka, fl.grid, s);
        if (rc) return rc;
        HIPCHK(hipEventRecord(R.b, s));
        R.launched = true;
        R.fused_hi = R.segs.back().hi;
        tally->nonces += fl.nonces;
        tally->tasks += fl.fa.ntasks;
        ++tally->launches;
    }
    return HM_OK;
}

// The opening of a batch call that began at t0: refuses an abandoned context,
// sets the call's deadline over every request's whole range, frees the events.
template <typename Req>
int batch_open(hm_ctx* ctx, const Req* reqs, int n, std::chrono::steady_clock::time_point t0) {
    // an abandoned context's devices may still run its timed-out work
    if (ctx->abandoned) return HM_ERR_TIMEOUT;
    // auto: the floor once, the slack times every request's whole range
    std::vector<hm_request> whole(n);
    for (int r = 0; r < n; ++r)
        whole[r] = hm_request{reqs[r].msg, reqs[r].msg ? reqs[r].len : 0, reqs[r].lo, reqs[r].hi};
    call_deadline(ctx, whole.data(), n, t0);
    for (Device& dv : ctx->devs) dv.evnext = 0;
    return HM_OK;
}
// A batch call that fails with rc leaves nothing queued: unless rc is a
// timeout, every stream the devices have made is waited for, then
// drain_failed (stream 0 and the events).  Returns rc.
int drain_streams(hm_ctx* ctx, int rc);

// ---- scan.cpp, find.cpp, collect.cpp, verify.cpp: the entry points' bodies, ctx->mu held ----
int scan_many_locked(hm_ctx* ctx, const hm_request* reqs, int n, hm_result* outs);
int find_locked(hm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
                uint64_t target, hm_result* out, int* found);
// hm_find_many: outs[i], found[i] for i < n, all written or (on failure) none.
int find_many_locked(hm_ctx* ctx, const hm_find_request* reqs, int n, hm_result* outs, int* found);
int collect_locked(hm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
                   uint64_t target, size_t cap, std::vector<hm_result>* recs, uint64_t* total);
// hm_scan_k: *recs = the min(k, nonces of [lo, hi]) lowest (hash, nonce) pairs, ascending.
int scan_k_locked(hm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
                  uint32_t k, std::vector<hm_result>* recs);
// hm_collect_many: (*totals)[i] for i < n, *total their sum, and *recs (every
// record, request-major, ascending by nonce inside a request) when *total <=
// cap; empty otherwise.
// hm_find_k: *recs = the min(k, hits) lowest records, ascending by nonce.
int find_k_locked(hm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
                  uint64_t target, size_t k, std::vector<hm_result>* recs);
int collect_many_locked(hm_ctx* ctx, const hm_collect_request* reqs, int n, size_t cap,
                        std::vector<uint64_t>* totals, std::vector<hm_result>* recs,
                        uint64_t* total);
// hm_find_k_many: (*recs)[i] = what find_k_locked gives for reqs[i], i < n.
int find_k_many_locked(hm_ctx* ctx, const hm_find_k_request* reqs, int n,
                       std::vector<std::vector<hm_result>>* recs);
// hm_hash_many (recs null: `list` holds n nonces, *out gets the n hashes) and
// hm_verify (recs: n records; *out gets the bad indices, ascending, when
// *bad <= cap and stays empty otherwise).
int list_locked(hm_ctx* ctx, const uint8_t* msg, size_t len, const uint64_t* nonces,
                const hm_result* recs, size_t n, uint64_t target, size_t cap,
                std::vector<uint64_t>* out, uint64_t* bad);
// Make *buf hold `want` units of `unit` bytes of device memory (*have: what it
// holds now).  A larger one replaces it -- at least twice the old size, at most
// `most` units, so all the buffers a device retires together are smaller than
// its current one -- and the old one is kept until hm_close, as the K+W tables
// are (hipFree would wait for the whole device).
template <typename T>
int grow_buffer(Device& dv, T** buf, size_t* have, size_t want, size_t most, size_t unit) {
    if (want <= *have) return HM_OK;
    const size_t size = std::min(std::max(want, 2 * *have), std::max(most, want));
    T* b = nullptr;
    if (hipMalloc(&b, size * unit) != hipSuccess) {
        (void)hipGetLastError();
        return HM_ERR_NOMEM;
    }
    if (*buf) dv.retired.push_back(*buf);
    *buf = b;
    *have = size;
    return HM_OK;
}
// Make dv's record buffer (hm_collect, hm_find_k and their batch forms) hold `cap` records.
inline int collect_buffer(Device& dv, size_t cap) {
    return grow_buffer(dv, &dv.collect_buf, &dv.collect_cap, cap, HM_COLLECT_CAP_MAX,
                       sizeof(hm_result));
}
// hm_verify_many: per[i] for i < nreq, *refs (the bad (request, index) pairs,
// ascending, when *bad <= cap; empty otherwise) and *bad.
int verify_many_locked(hm_ctx* ctx, const hm_verify_request* reqs, int nreq, size_t cap,
                       std::vector<uint64_t>* per, std::vector<hm_bad_ref>* refs, uint64_t* bad);

}  // namespace hm
