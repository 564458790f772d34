// seg_walk.cpp -- from a planned segment to its launches: the kernel names,
// the launch geometry (grid, guided task list, edge trimming), the argument
// blocks, and SegWalk, the one walk hm_scan, hm_find and hm_collect all take
// through a segment's chunks, tile windows and epochs.  PieceWalk and the two
// small helpers at the end are what hm_find and hm_collect share beyond that.
#include "hm_internal.hpp"

namespace hm {

KernelName kernel_name(Family family, int kind, const SegPlan* s) {
    static const char* const layouts[] = {"generic", "tiled", "chained", "fused"};
    static const char* const args[] = {"GenericArgs", "TiledArgs", "ChainedArgs", "FusedArgs"};
    const int li = kind == HM_KIND_TILED ? 1 : kind == HM_KIND_CHAINED ? 2 : kind == HM_KIND_FUSED ? 3 : 0;
    const char* pre = family == Family::Find      ? "find_"
                      : family == Family::Collect ? "collect_"
                      : family == Family::FindK   ? "find_k_"
                      : family == Family::ScanK   ? "scan_k_"
                                                  : "";
    const char* arg_pre = family == Family::Find      ? "Find"
                          : family == Family::Collect ? "Collect"
                          : family == Family::FindK   ? "FindK"
                          : family == Family::ScanK   ? "ScanK"
                                                      : "";
    std::string fn = std::string("hm_") + pre + layouts[li] +
                     (family == Family::ScanCsum ? "_csum" : "") + "_kernel";
    std::string arg = std::string(arg_pre) + args[li];
    if (family == Family::Find && kind == HM_KIND_FUSED) {  // fused_find_kernels.hip
        fn = "hm_fused_find_kernel";
        arg = "FusedFindArgs";
    }
    if (family == Family::Collect && kind == HM_KIND_FUSED) {  // fused_collect_kernels.hip
        fn = "hm_fused_collect_kernel";
        arg = "FusedCollectArgs";
    }
    if (family == Family::FindK && kind == HM_KIND_FUSED) {  // fused_find_k_kernels.hip
        fn = "hm_fused_find_k_kernel";
        arg = "FusedFindKArgs";
    }
    char targs[48] = "", shown[48] = "";
    if (kind == HM_KIND_TILED) {  // hm_*tiled*_kernel<W1, STRADDLE, TRAILER>
        snprintf(targs, sizeof targs, "ILi%dELb%dELb%dEEEv", s->W1, s->straddle ? 1 : 0,
                 s->trailer ? 1 : 0);
        snprintf(shown, sizeof shown, "<%d, %s, %s>", s->W1, s->straddle ? "true" : "false",
                 s->trailer ? "true" : "false");
    }
    KernelName k;
    // void hm::fn[<...>](hm::arg), Itanium-mangled
    k.symbol = "_ZN2hm" + std::to_string(fn.size()) + fn + (targs[0] ? targs : "E") + "NS_" +
               std::to_string(arg.size()) + arg + "E";
    k.display = fn + shown;
    return k;
}

// Resolve a scan kernel of dv's module (cached with its occupancy).
int scan_fn(Device& dv, const std::string& sym, const Device::Fn** out) {
    for (const auto& f : dv.fns)
        if (f.sym == sym) { *out = &f; return HM_OK; }
    Device::Fn f{sym, nullptr, 0};
    HIPCHK(hipModuleGetFunction(&f.fn, dv.mod, sym.c_str()));
    HIPCHK(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&f.blocks_per_cu, f.fn, kBlock, 0));
    dv.fns.push_back(f);
    *out = &dv.fns.back();
    return HM_OK;
}

// log2 of the tasks per queue atomic of a per-segment launch over `nonces`.
static uint32_t queue_shift(const hm_ctx* ctx, uint64_t nonces) {
    if (ctx->queue_batch > 0) return (uint32_t)__builtin_ctz((unsigned)ctx->queue_batch);
    return nonces >= kBigLaunchNonces ? kQueueShiftBig : kQueueShift;
}

uint32_t count_compressions(const SegPlan& s) {
    // SHA-256 compressions per nonce after the host midstate (SURVEY §8d "C").
    return s.nb;
}

// Compressions per nonce the segment's scan kernel executes: the algorithmic
// C minus what is hoisted out of the per-nonce loop (hm_stats.dom_compressions_eff).
// The chained kernel's launches count their block-0 compressions exactly
// (one per task and lane, scan.cpp enqueue_segment), guided-split pieces included.
double executed_compressions(const SegPlan& s) {
    switch (s.kind) {
        case HM_KIND_TILED:  // a two-block tail's block 0 is compressed per tile by the planner
            return s.trailer ? 2.0 : 1.0;
        default:
            return (double)s.nb;
    }
}

int persistent_grid(const hm_ctx* ctx, const Device& dv, int per_cu_auto, uint64_t ntasks) {
    int per_cu = ctx->grid_per_cu > 0 ? ctx->grid_per_cu : per_cu_auto;
    if (per_cu <= 0) per_cu = 1;
    uint64_t grid = (uint64_t)per_cu * (uint64_t)dv.cus;
    const uint64_t waves_per_block = kBlock / kWaveSize;
    grid = std::min<uint64_t>(grid, (ntasks + waves_per_block - 1) / waves_per_block);
    grid = std::min<uint64_t>(grid, kMaxCandWaves / waves_per_block);
    return (int)std::max<uint64_t>(grid, 1);
}

// Guided task list of a persistent launch over `nunits` work units: the
// last ~one unit per wave of the grid is split into kSplit tasks.  Returns
// the task-id count; *nbig = units dequeued whole.
static uint32_t guided_tasks(uint64_t nunits, int grid, uint32_t* nbig) {
    const uint64_t waves = (uint64_t)grid * (kBlock / kWaveSize);
    const uint64_t small = std::min<uint64_t>(nunits, waves);
    *nbig = (uint32_t)(nunits - small);
    return (uint32_t)(nunits - small + kSplit * small);
}

// Grid and guided task list of a persistent launch over `nunits` units: the
// split is planned against the occupancy-sized grid, then the grid is cut to
// the task count (one wave per task at most).  A launch with fewer units than
// the GPU has waves splits every unit, and sizing its grid by tasks rather
// than units gives each task its own wave: a segment of 10^4..10^7 nonces is
// latency-bound (one wave runs its tasks' SHA chains back to back), so this
// cuts such launches from ≈270-390 µs to tens of µs (config 1's request).
static int plan_launch(const hm_ctx* ctx, const Device& dv, int per_cu_auto, uint64_t nunits,
                       uint32_t* ntasks, uint32_t* nbig) {
    const int cap = persistent_grid(ctx, dv, per_cu_auto, 1ull << 40);  // occupancy-sized
    *ntasks = guided_tasks(nunits, cap, nbig);
    return persistent_grid(ctx, dv, per_cu_auto, *ntasks);
}

// Units of a launch over tiles [t, t+nt) (unit = lane chunk x `per_chunk`
// loop chunks; lane value v of a tile covers nonces base + v*step + [0, step)):
// the lane chunks of the first tile wholly below s.lo and of the last tile
// wholly above s.hi are skipped, so shards and segments that start or end
// inside a tile hash no out-of-range nonces beyond their edge chunks.
// *unit0 = the first unit kept, *nunits = the count kept.
void launch_units(const SegPlan& s, uint64_t t, uint64_t nt, uint64_t per_chunk, uint64_t step,
                  uint32_t* unit0, uint64_t* nunits) {
    const uint64_t P = s.pow10V;
    const uint64_t per_tile = (uint64_t)s.tpt * per_chunk;
    uint64_t first = 0, last = nt * per_tile - 1;
    const uint64_t b0 = t * P;  // <= s.hi: every tile of the launch meets [lo, hi]
    if (s.lo > b0) first = (s.lo - b0) / step / kWaveSize * per_chunk;
    const uint64_t bl = (t + nt - 1) * P;
    if (s.hi - bl < P - 1)
        last = (nt - 1) * per_tile + ((s.hi - bl) / step / kWaveSize + 1) * per_chunk - 1;
    *unit0 = (uint32_t)first;
    *nunits = last - first + 1;
}

// nonces of [t*P, (t+nt)*P - 1] ∩ [lo, hi] (P = nonces per tile)
static uint64_t tile_span_nonces(const SegPlan& s, uint64_t t, uint64_t nt) {
    const uint64_t a = std::max(s.lo, t * s.pow10V);
    const bool wraps = (t + nt) > (~0ull) / s.pow10V;
    const uint64_t b = wraps ? s.hi : std::min(s.hi, (t + nt) * s.pow10V - 1);
    return b - a + 1;
}

// ---------------------------------------------------------------------------
// Argument blocks of the per-segment launches, filled from a SegPlan for
// SegWalk::next, so a layout or argument change is made once.  The output
// fields (cand, sums) are left null: only the scan sets them.
// ---------------------------------------------------------------------------
// The tile planner's arguments for tiles [t, t + nt) of s on stream si.  The
// chained layout keeps tail block 0 raw (fb = 0): its compression is per lane.
static PlanArgs plan_args(const Device& dv, const MsgPlan& mp, const SegPlan& s, int si,
                          uint64_t t, uint64_t nt) {
    PlanArgs pa;
    pa.rec = dv.rec[si];
    pa.tile0 = t;
    pa.pow10V = s.pow10V;
    pa.total_bits = s.total_bits;
    pa.ntiles = (uint32_t)nt;
    pa.V = s.V;
    pa.d = s.d;
    pa.r = mp.r;
    pa.fb = s.kind == HM_KIND_CHAINED ? 0 : s.fb;
    pa.nb = s.nb;
    memcpy(pa.pw, mp.pw, sizeof pa.pw);
    memcpy(pa.mid, mp.mid, sizeof pa.mid);
    return pa;
}

// A tiled launch over tiles [t, t + nt) of s, but for its task list
// (plan_tasks); kw = the trailer block's K+W (zeros without a trailer).
// *unit0, *nunits: the units kept (launch_units).
static void tiled_args(const hm_ctx* ctx, const Device& dv, const SegPlan& s, int si, uint64_t t,
                       uint64_t nt, const uint32_t kw[64], TiledArgs& ta, uint32_t* unit0,
                       uint64_t* nunits) {
    ta.rec = dv.rec[si];
    ta.counter = dv.counter[si];
    ta.cand = nullptr;
    ta.sums = nullptr;
    ta.tile0 = t;
    ta.pow10V = s.pow10V;
    ta.seg_lo = s.lo;
    ta.seg_hi = s.hi;
    launch_units(s, t, nt, 1, 100, unit0, nunits);
    ta.tpt = s.tpt;
    ta.vmax = (uint32_t)(pow10_u64(s.q) - 1);
    ta.q = s.q;
    ta.lane_shift = s.lane_shift;
    ta.loop_shift = s.loop_shift;
    ta.lds_shift = queue_shift(ctx, tile_span_nonces(s, t, nt));
    memcpy(ta.trailer_kw, kw, sizeof ta.trailer_kw);
    tiled_loop_sigma0(s, ta.s0_loop);
}

// A chained launch over tiles [t, t + nt) of s in epoch e of nep, but for
// its task list.
static void chained_args(const hm_ctx* ctx, const Device& dv, const SegPlan& s, int si, uint64_t t,
                         uint64_t nt, uint64_t e, uint64_t nep, ChainedArgs& ca, uint32_t* unit0,
                         uint64_t* nunits) {
    const uint64_t nloop = pow10_u64(s.fe);
    ca.rec = dv.rec[si];
    ca.kwt = dv.kwt[si];
    ca.counter = dv.counter[si];
    ca.cand = nullptr;
    ca.sums = nullptr;
    ca.tile0 = t;
    ca.pow10qf = s.pow10V;
    ca.pow10f = pow10_u64(s.f);
    ca.ebase = e * nloop;
    ca.nloop = (uint32_t)nloop;
    ca.seg_lo = s.lo;
    ca.seg_hi = s.hi;
    launch_units(s, t, nt, s.ntc, pow10_u64(s.f), unit0, nunits);
    ca.tpt = s.tpt;
    ca.ntc = s.ntc;
    ca.tch = s.tch;
    ca.vmax = (uint32_t)(pow10_u64(s.q) - 1);
    ca.q = s.q;
    ca.lds_shift = queue_shift(ctx, tile_span_nonces(s, t, nt) / nep);
}

// A generic launch over the count_m1 + 1 nonces from lo of segment s.
static void generic_args(const MsgPlan& mp, const SegPlan& s, uint64_t lo, uint64_t count_m1,
                         GenericArgs& ga) {
    ga.cand = nullptr;
    ga.sums = nullptr;
    ga.seg_lo = lo;
    ga.count_m1 = count_m1;
    ga.total_bits = s.total_bits;
    ga.d = s.d;
    ga.r = mp.r;
    ga.nb = s.nb;
    memcpy(ga.pw, mp.pw, sizeof ga.pw);
    memcpy(ga.mid, mp.mid, sizeof ga.mid);
}
static int generic_grid(const Device& dv, uint64_t count_m1) {
    const uint64_t need = count_m1 / kBlock + 1;
    const uint64_t cap = (uint64_t)(kMaxCandWaves / (kBlock / kWaveSize));
    return (int)std::min<uint64_t>(need, std::min<uint64_t>(cap, (uint64_t)dv.cus * 8));
}

// Grid and guided task list of a persistent launch of fn over nunits units
// from unit0.  Task ids start at unit0 (the queue counter too, queue_tasks):
// the kernels map a task below nbig to that unit, so the skipped units are
// never dequeued.  *ntasks, *nbig: the launch's argument fields (unit0
// included); *count: the tasks themselves.
static int plan_tasks(const hm_ctx* ctx, const Device& dv, const Device::Fn& fn, uint64_t nunits,
                      uint32_t unit0, uint32_t* ntasks, uint32_t* nbig, uint32_t* count) {
    const int grid = plan_launch(ctx, dv, fn.blocks_per_cu, nunits, ntasks, nbig);
    *count = *ntasks;
    *ntasks += unit0;
    *nbig += unit0;
    return grid;
}
// The queue counter's reset on stream si to the launch's first task id.
static int queue_tasks(const Device& dv, int si, uint32_t unit0) {
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)dv.counter[si], (int)unit0, 1, dv.stream[si]));
    return HM_OK;
}

// Make stream si's K+W table hold segment s's 10^fe rows.  A device short of
// memory for the planned table gets smaller tables and more epochs: the same
// nonces on the same kernel, more launches (s.fe, s.tch, s.ntc shrink).
static int chained_table(hm_ctx* ctx, Device& dv, int si, SegPlan& s) {
    if (s.fe < 1 || s.fe > kMaxTableDigits || s.fe > s.f) return HM_ERR_INTERNAL;
    int rc;
    while ((rc = kw_table_rows(ctx, dv, si, pow10_u64(s.fe))) == HM_ERR_NOMEM && s.fe > 1) {
        --s.fe;
        s.tch = (uint32_t)std::min<uint64_t>(s.tch, pow10_u64(s.fe));
        s.ntc = (uint32_t)(pow10_u64(s.fe) / s.tch);
    }
    return rc;
}
// Tiles one launch of s may cover.
static uint64_t max_launch_tiles(const SegPlan& s) {
    const uint64_t per_tile = s.kind == HM_KIND_CHAINED ? (uint64_t)s.tpt * s.ntc : s.tpt;
    return std::min<uint64_t>(kMaxTilesPerLaunch, 0x7fffffffull / per_tile);
}

int SegWalk::open(hm_ctx* ctx_, Device& dv_, const MsgPlan& mp_, int si_, const SegPlan& seg,
                  Family family, uint64_t generic_chunk) {
    ctx = ctx_;
    dv = &dv_;
    mp = &mp_;
    si = si_;
    s = seg;
    chunk_m1 = generic_chunk - 1;  // 0: no limit
    nep = 1;
    nloop = 0;
    memset(kw, 0, sizeof kw);
    if (s.kind == HM_KIND_CHAINED) {
        int rc = chained_table(ctx, dv_, si, s);
        if (rc) return rc;
        nloop = pow10_u64(s.fe);       // table rows = loop values per lane
        nep = pow10_u64(s.f - s.fe);   // epochs: the final block's high digits
    } else if (s.kind == HM_KIND_TILED && s.trailer) {
        trailer_kw(s, kw);
    }
    if (s.kind != HM_KIND_GENERIC) max_tiles = max_launch_tiles(s);
    e = 0;
    t = s.tile_lo;
    g = s.lo;
    table_epoch = ~0ull;
    name = kernel_name(family, s.kind, &s);
    return scan_fn(dv_, name.symbol, &fn);
}

bool SegWalk::peek_base(uint64_t* base) const {
    if (e >= nep) return false;
    *base = std::max(s.lo, s.kind == HM_KIND_GENERIC ? g : t * s.pow10V + e * nloop);
    return true;
}

bool SegWalk::next(SegStep* o) {
    if (!peek_base(&o->base)) return false;
    o->kind = s.kind;
    if (s.kind == HM_KIND_GENERIC) {
        const uint64_t count_m1 = std::min<uint64_t>(s.hi - g, chunk_m1);
        generic_args(*mp, s, g, count_m1, o->g);
        o->nonces = count_m1 + 1;  // generic segments are far below 2^64
        o->nunits = count_m1 / kWaveSize + 1;  // a task: one wave step of 64 nonces
        o->ntasks = (uint32_t)o->nunits;
        o->grid = generic_grid(*dv, count_m1);
        if (s.hi - g == count_m1) close();
        else g += count_m1 + 1;
        return true;
    }
    const uint64_t nt = std::min<uint64_t>(max_tiles, s.tile_hi - t + 1);
    // the epochs split every lane value's nonces evenly: the launch's share
    // of its tiles' nonces (stats only, an estimate)
    const uint64_t span = tile_span_nonces(s, t, nt);
    o->nonces = span / nep + (e + 1 == nep ? span % nep : 0);
    o->tile = t;
    o->ntiles = nt;
    o->epoch = e;
    if (s.kind == HM_KIND_CHAINED) {
        chained_args(ctx, *dv, s, si, t, nt, e, nep, o->c, &o->unit0, &o->nunits);
        o->grid = plan_tasks(ctx, *dv, *fn, o->nunits, o->unit0, &o->c.ntasks, &o->c.nbig, &o->ntasks);
    } else {
        tiled_args(ctx, *dv, s, si, t, nt, kw, o->t, &o->unit0, &o->nunits);
        o->grid = plan_tasks(ctx, *dv, *fn, o->nunits, o->unit0, &o->t.ntasks, &o->t.nbig, &o->ntasks);
    }
    t += nt;
    // the epoch's last window, or the tile index wrapped (cannot happen for d <= 20)
    if (t == 0 || t > s.tile_hi) skip_epoch();
    return true;
}

int SegWalk::prologue(const SegStep& step) {
    if (step.kind == HM_KIND_GENERIC) return HM_OK;
    hipStream_t st = dv->stream[si];
    if (step.kind == HM_KIND_CHAINED && table_epoch != step.epoch) {
        HIPCHK(launch_kw_table(dv->kwt[si], s.f, s.fe, step.epoch * nloop, s.total_bits, st));
        table_epoch = step.epoch;
    }
    HIPCHK(launch_tile_plan(plan_args(*dv, *mp, s, si, step.tile, step.ntiles), st));
    return queue_tasks(*dv, si, step.unit0);
}

PieceWalk::PieceWalk(const hm_ctx* ctx_, const MsgPlan& mp_, uint64_t lo, uint64_t hi)
    : ctx(ctx_), mp(mp_), segs(plan_range(mp_, lo, hi, ctx_->force_generic, ctx_->table_digits)) {
    if (!segs.empty()) a = segs[0].lo;
}

bool PieceWalk::next(std::vector<std::vector<SegPlan>>* shards) {
    if (i >= segs.size()) return false;
    const SegPlan& seg = segs[i];
    const int ndev = (int)ctx->devs.size();
    uint64_t span = ~0ull;  // one device: the segment is one piece
    if (ndev > 1) {
        span = kFindPieceNonces * (uint64_t)ndev;
        if (seg.pow10V > 1) span = std::max<uint64_t>(span / seg.pow10V, 1) * seg.pow10V;
    }
    // pieces end at multiples of span (tile boundaries)
    const uint64_t k = a / span;
    const uint64_t b =
        ndev == 1 || k >= ~0ull / span ? seg.hi : std::min(seg.hi, (k + 1) * span - 1);
    const std::vector<Shard> sh = partition_range(mp, a, b, ndev, ctx->force_generic);
    shards->assign(ndev, {});
    for (int d = 0; d < ndev; ++d)
        if (!sh[d].empty)
            (*shards)[d] = plan_range(mp, sh[d].lo, sh[d].hi, ctx->force_generic, ctx->table_digits);
    if (b != seg.hi) a = b + 1;
    else if (++i < segs.size()) a = segs[i].lo;
    return true;
}

int begin_ranged_call(hm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
                      std::chrono::steady_clock::time_point t0, const uint8_t** m, size_t* mlen) {
    // an abandoned context's devices may still run its timed-out work
    if (ctx->abandoned) return HM_ERR_TIMEOUT;
    const Msg e = msg_or_empty(msg, len);
    *m = e.p;
    *mlen = e.len;
    const hm_request whole{*m, *mlen, lo, hi};  // auto models the whole range
    call_deadline(ctx, &whole, 1, t0);
    return HM_OK;
}

int drain_failed(hm_ctx* ctx, int rc) {
    if (rc == HM_ERR_TIMEOUT || ctx->abandoned) return rc;
    for (Device& dv : ctx->devs) {
        if (hipSetDevice(dv.ordinal) == hipSuccess && host_wait(ctx, dv.stream[0]) != HM_OK) break;
        dv.evnext = 0;
    }
    return rc;
}

}  // namespace hm
