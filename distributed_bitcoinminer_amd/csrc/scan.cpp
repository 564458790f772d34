// scan.cpp -- hm_scan_many: per device and request, the segments onto the
// streams (one fused launch for a small request, else SegWalk launch by
// launch), the merge of the devices' results, and hm_stats.
#include "hm_internal.hpp"

namespace hm {
namespace {

// Enqueue one segment on stream `si`, launch by launch (SegWalk; a generic
// segment is one launch); records its launches for stats.
// `best` = the request's [kStreams][2] running bests; this stream folds into best + 2*si.
int enqueue_segment(hm_ctx* ctx, Device& dv, const MsgPlan& mp, const SegPlan& seg, int si,
                    uint64_t* best) {
    hipStream_t st = dv.stream[si];
    SegWalk w;
    int rc = w.open(ctx, dv, mp, si, seg, ctx->csum ? Family::ScanCsum : Family::Scan, 0);
    if (rc) return rc;
    uint64_t* sums = ctx->csum ? dv.sums[si] : nullptr;
    SegStep step;
    while (w.next(&step)) {
        switch (step.kind) {
            case HM_KIND_TILED: step.t.cand = dv.cand[si]; step.t.sums = sums; break;
            case HM_KIND_CHAINED: step.c.cand = dv.cand[si]; step.c.sums = sums; break;
            default: step.g.cand = dv.cand[si]; step.g.sums = sums; break;
        }
        Launch L;
        rc = next_event(dv, &L.start);
        if (rc) return rc;
        rc = next_event(dv, &L.stop);
        if (rc) return rc;
        L.nonces = step.nonces;
        L.kind = step.kind;
        snprintf(L.kernel, sizeof L.kernel, "%s", w.name.display.c_str());
        L.grid = step.grid;
        L.compressions = count_compressions(w.s);
        // chained: every task compresses its lanes' tail block 0 once; the final
        // block runs once per lane and loop value: nunits * tch values per lane
        L.comp_eff = step.kind == HM_KIND_CHAINED
                         ? 1.0 + (double)step.ntasks / ((double)step.nunits * (double)w.s.tch)
                         : executed_compressions(w.s);
        rc = w.launch(step, NoTrailer{}, L.start, L.stop);
        if (rc) return rc;
        HIPCHK(launch_fold(dv.cand[si], (uint32_t)step.grid * (kBlock / kWaveSize), best + 2 * si,
                           st));
        if (ctx->csum)
            HIPCHK(launch_sum_fold(dv.sums[si], (uint32_t)step.grid * (kBlock / kWaveSize),
                                   dv.acc + 2 * si, st));
        dv.launches.push_back(L);
    }
    return HM_OK;
}

}  // namespace

// Fused launch (kernels.hpp, fused_kernels.hip): can all of a request's
// segments run in one launch?  Up to kFusedNonces nonces and 20 segments;
// tiled and generic segments always, chained ones with one table of f <= 4
// digits (no epochs) whose rows fit the stream's aux buffer.
bool fusible(const std::vector<SegPlan>& segs) {
    if (segs.empty() || segs.size() > (size_t)kMaxFusedSegs) return false;
    long double n = 0;
    uint64_t rows = 0, tiles = 0;
    for (const auto& g : segs) {
        n += (long double)(g.hi - g.lo) + 1;
        if (g.kind == HM_KIND_CHAINED) {
            if (g.f > kMaxChainedF || g.fe != g.f) return false;
            rows += pow10_u64(g.f);
        }
        if (g.kind != HM_KIND_GENERIC) tiles += g.tile_hi - g.tile_lo + 1;
    }
    return n <= (long double)kFusedNonces && rows <= kFusedKwRows && tiles <= kMaxTilesPerLaunch;
}

// What a fused launch of `segs`, in that task order, on stream si is: the
// planner's and the kernel's argument blocks (segment descriptors, tasks,
// guided tail, the counter's start), the grid and the stats figures.
int plan_fused(hm_ctx* ctx, Device& dv, const MsgPlan& mp, const std::vector<SegPlan>& segs, int si,
               uint32_t flags, FusedLaunch* out) {
    FusedPlanArgs& pa = out->pa;
    memset(&pa, 0, sizeof pa);
    FusedArgs& fa = out->fa;
    memset(&fa, 0, sizeof fa);
    pa.rec = dv.rec[si];
    pa.aux = dv.aux[si];
    pa.counter = dv.counter[si];
    pa.r = mp.r;
    memcpy(pa.pw, mp.pw, sizeof pa.pw);
    memcpy(pa.mid, mp.mid, sizeof pa.mid);
    fa.rec = dv.rec[si];
    fa.aux = dv.aux[si];
    fa.counter = dv.counter[si];
    fa.r = mp.r;
    memcpy(fa.pw, mp.pw, sizeof fa.pw);
    memcpy(fa.mid, mp.mid, sizeof fa.mid);
    uint64_t tasks = 0, jobs = 0, nonces = 0;
    uint32_t rec_next = 0, aux_next = 0, comp_max = 1;
    std::vector<double> ce_base(segs.size()), seg_units(segs.size());  // chained C_eff inputs
    std::vector<uint64_t> seg_cnt(segs.size());
    for (size_t i = 0; i < segs.size(); ++i) {
        const SegPlan& g = segs[i];
        FusedSeg& S = fa.segs[i];
        FusedPlanSeg& P = pa.segs[i];
        const uint64_t cnt = g.hi - g.lo + 1;  // one digit count: far below 2^64
        S.seg_lo = g.lo;
        S.seg_hi = g.hi;
        S.total_bits = g.total_bits;
        S.d = g.d;
        S.nb = g.nb;
        P.total_bits = g.total_bits;
        P.d = g.d;
        P.nb = g.nb;
        P.T = g.T;
        P.V = g.V;
        P.straddle = g.straddle;
        P.loop_shift = g.loop_shift;
        P.f = g.f;
        uint64_t seg_tasks = 0, seg_jobs = 0;
        double ce = (double)g.nb;
        if (g.kind == HM_KIND_TILED || g.kind == HM_KIND_CHAINED) {
            const bool ch = g.kind == HM_KIND_CHAINED;
            const uint64_t nt = g.tile_hi - g.tile_lo + 1;
            uint32_t unit0;
            uint64_t nunits;
            launch_units(g, g.tile_lo, nt, ch ? g.ntc : 1, ch ? pow10_u64(g.f) : 100, &unit0, &nunits);
            S.tile0 = P.tile0 = g.tile_lo;
            S.pow10V = P.pow10V = g.pow10V;
            S.rec0 = P.rec0 = rec_next;
            S.aux0 = P.aux0 = aux_next;
            S.unit0 = unit0;
            S.tpt = g.tpt;
            S.vmax = (uint32_t)(pow10_u64(g.q) - 1);
            S.q = g.q;
            P.ntiles = (uint32_t)nt;
            rec_next += (uint32_t)nt;
            if (ch) {
                S.variant = P.variant = kVarChained;
                S.pow10f = pow10_u64(g.f);
                S.ntc = g.ntc;
                S.tch = g.tch;
                S.tpu = (g.tch + kFusedChainedPiece - 1) / kFusedChainedPiece;
                P.fb = 0;  // tail block 0 kept raw: its compression is per lane
                seg_tasks = nunits * S.tpu;
                seg_jobs = nt + pow10_u64(g.f);
                aux_next += (uint32_t)pow10_u64(g.f) * 64;
                // 1 + block-0 compressions per loop value: one per task (and
                // per guided-tail piece, added below)
                ce = 1.0;
                seg_units[i] = (double)nunits * (double)g.tch;
            } else {
                S.variant = P.variant = (uint32_t)(g.W1 * 4 + (g.straddle ? 2 : 0) + (g.trailer ? 1 : 0));
                S.lane_shift = g.lane_shift;
                S.loop_shift = g.loop_shift;
                S.tpu = ctx->fused_parts;
                P.fb = g.fb;
                seg_tasks = nunits * 10 * ctx->fused_parts;
                seg_jobs = nt + 100 + (g.trailer ? 1 : 0);
                aux_next += 100 + (g.trailer ? 64 : 0);
                ce = executed_compressions(g);
            }
        } else {
            S.variant = P.variant = kVarGeneric;
            seg_tasks = (cnt + 639) / 640;
        }
        tasks += seg_tasks;
        jobs += seg_jobs;
        S.task_end = (uint32_t)tasks;
        P.job_end = (uint32_t)jobs;
        nonces += cnt;
        comp_max = std::max(comp_max, g.nb);
        ce_base[i] = ce;
        seg_cnt[i] = cnt;
    }
    // guided tail: waves that start together on equal tasks finish their
    // rounds together, so the launch ends on a partial round of
    // tasks mod waves tasks, with most of the GPU idle for a whole task's
    // time.  Those last tasks (the cheapest layouts, queued last) run as
    // pieces instead: the most pieces each (<= fused_tail; 10, 5, 2) that
    // still fit one round of the grid.  Splitting more (a whole round) costs
    // more than it saves: every piece is one more atomic on the launch's one
    // queue counter, which saturates (profiles/r06/experiments/fused_tail/).
    const uint64_t cap_waves =
        (uint64_t)persistent_grid(ctx, dv, kFusedPerCu, 1ull << 40) * (kBlock / kWaveSize);
    const uint64_t nsplit = tasks % cap_waves;
    uint32_t nparts = 1;
    for (uint32_t p : {10u, 5u, 2u})
        if (p <= ctx->fused_tail && nsplit * p <= cap_waves) { nparts = p; break; }
    const uint64_t nbig = nparts > 1 ? tasks - nsplit : tasks;
    const uint64_t ids = nbig + (nparts > 1 ? nsplit * nparts : 0);
    if (ids >= (1ull << 31) || jobs >= (1ull << 31) || aux_next > kFusedAuxWords)
        return HM_ERR_INTERNAL;  // excluded by fusible()
    double comp_w = 0;  // executed compressions x nonces (hm_stats)
    for (size_t i = 0; i < segs.size(); ++i) {
        double ce = ce_base[i];
        if (seg_units[i] > 0) {  // chained: block 0 per task, and per piece of a split task
            const uint64_t a = i ? fa.segs[i - 1].task_end : 0, b = fa.segs[i].task_end;
            const uint64_t split =
                nparts > 1 && b > std::max(a, nbig) ? b - std::max(a, nbig) : 0;
            ce += (double)(b - a + split * (nparts - 1)) / seg_units[i];
        }
        comp_w += ce * (double)seg_cnt[i];
    }
    fa.ntasks = (uint32_t)ids;
    fa.nbig = (uint32_t)nbig;
    fa.nparts = nparts > 1 ? nparts : 1;
    fa.nseg = pa.nseg = (uint32_t)segs.size();
    pa.njobs = (uint32_t)jobs;
    // small launches: few waves per SIMD keep a task short, so the launch's
    // tail is short (kFusedPerCu = 3 workgroups per CU, profiles/r05/fused/)
    out->grid = persistent_grid(ctx, dv, kFusedPerCu, ids);
    fa.flags = flags;
    // with static first tasks the queue starts past every wave slot
    pa.counter0 = (flags & kFusedStaticFirst) ? (uint32_t)out->grid * (kBlock / kWaveSize) : 0;
    out->nonces = nonces;
    out->comp_max = comp_max;
    out->comp_eff = comp_w / (double)nonces;
    return HM_OK;
}

namespace {

// Per-task cost rank of a segment's layout in the fused launch: the queue
// hands out the costly tasks first, so the launch ends on the cheapest ones.
int fused_rank(const SegPlan& g) {
    if (g.kind == HM_KIND_CHAINED) return 0;   // 64 lanes x up to 100 blocks
    if (g.kind == HM_KIND_GENERIC) return 1;   // 640 nonces, full tail compressions
    return g.trailer ? 2 : 3;                  // 640 nonces, 2 or 1 compressions
}

}  // namespace

void fused_order(std::vector<SegPlan>* segs) {
    std::stable_sort(segs->begin(), segs->end(), [](const SegPlan& a, const SegPlan& b) {
        if (fused_rank(a) != fused_rank(b)) return fused_rank(a) < fused_rank(b);
        return a.hi - a.lo > b.hi - b.lo;
    });
}

namespace {

// Enqueue every segment of one request as ONE fused launch on stream si:
// hm_fused_plan_kernel (records, tables, counter; and, when `seed_best`, the
// (MaxUint64, 0) seed of *best and zeroed coverage sums) -> hm_fused_kernel
// -> hm_fold_kernel into *best.  Tasks are ordered costliest layout first,
// larger segments first.
int enqueue_fused(hm_ctx* ctx, Device& dv, const MsgPlan& mp, std::vector<SegPlan> segs, int si,
                  uint64_t* best, bool seed_best) {
    hipStream_t st = dv.stream[si];
    fused_order(&segs);
    FusedLaunch fl;
    int rc = plan_fused(ctx, dv, mp, segs, si, ctx->fused_flags, &fl);
    if (rc) return rc;
    FusedPlanArgs& pa = fl.pa;
    FusedArgs& fa = fl.fa;
    pa.result = seed_best ? best : nullptr;
    // a lone request (seed_best) also zeroes every stream's coverage sums,
    // which hm_scan_checked adds up; in a batch they were zeroed up front
    // and hold the other requests' sums
    pa.acc = ctx->csum && seed_best ? dv.acc : nullptr;
    pa.n_acc = 2 * kStreams;
    fa.cand = dv.cand[si];
    fa.sums = ctx->csum ? dv.sums[si] : nullptr;
    const Device::Fn* fn = nullptr;
    // built once: a fused request's whole enqueue is ~10 us
    static const KernelName names[2] = {kernel_name(Family::Scan, HM_KIND_FUSED, nullptr),
                                        kernel_name(Family::ScanCsum, HM_KIND_FUSED, nullptr)};
    const KernelName& name = names[ctx->csum ? 1 : 0];
    rc = scan_fn(dv, name.symbol, &fn);
    if (rc) return rc;
    const int grid = fl.grid;
    HIPCHK(launch_fused_plan(pa, st));
    Launch L;
    rc = next_event(dv, &L.start);
    if (rc) return rc;
    rc = next_event(dv, &L.stop);
    if (rc) return rc;
    L.nonces = fl.nonces;
    L.kind = HM_KIND_FUSED;
    snprintf(L.kernel, sizeof L.kernel, "%s", name.display.c_str());
    L.grid = grid;
    L.compressions = fl.comp_max;
    L.comp_eff = fl.comp_eff;
    HIPCHK(hipEventRecord(L.start, st));
    rc = launch_scan(*fn, fa, grid, st);
    if (rc) return rc;
    HIPCHK(hipEventRecord(L.stop, st));
    HIPCHK(launch_fold(dv.cand[si], (uint32_t)grid * (kBlock / kWaveSize), best, st));
    if (ctx->csum)
        HIPCHK(launch_sum_fold(dv.sums[si], (uint32_t)grid * (kBlock / kWaveSize), dv.acc + 2 * si,
                               st));
    dv.launches.push_back(L);
    return HM_OK;
}

struct DevReq {
    const MsgPlan* mp;
    uint64_t lo, hi;
    bool empty;
};

// Enqueue a batch of scans on one device; request r's result lands in
// dv.result + 2r.  All segments of all requests are queued before any sync.
// `first`: the call's first chunk, which records the timing origin dv.t0
// (every launch of an hm_scan_many call is timed against it).
int enqueue_device_batch(hm_ctx* ctx, Device& dv, const std::vector<DevReq>& reqs, bool first) {
    HIPCHK(hipSetDevice(dv.ordinal));
    const int n = (int)reqs.size();
    hipStream_t s0 = dv.stream[0];
    if (first) HIPCHK(hipEventRecord(dv.t0, s0));
    // one small request (config 1, short server chunks): the fused launch on
    // stream 0 alone, its planner seeding the result slot -- nothing else
    // runs between the call's first launch and the 16-B readback
    if (n == 1 && !reqs[0].empty && ctx->fused && !ctx->test_mid_sync) {
        std::vector<SegPlan> segs = plan_range(*reqs[0].mp, reqs[0].lo, reqs[0].hi,
                                               ctx->force_generic, ctx->table_digits);
        if (fusible(segs))
            return enqueue_fused(ctx, dv, *reqs[0].mp, segs, 0, dv.result, true);
    }
    // streams == 1: every segment in order on stream 0, so kernels never
    // overlap and per-kernel timings match rocprofv3 exactly.  streams > 1:
    // the segments run by the request's dominant kernel instantiation (most
    // nonces) go first, in order, on stream 0 (high priority); the others
    // are queued on the low-priority streams 1.., gated on stream 0 reaching
    // its last dominant segment: they start together with that launch, get
    // workgroup slots only as its persistent waves retire, and so run in its
    // tail instead of after it.  Small requests (<= kConcurrentNonces) skip
    // that order: all their segments run at once on all streams.
    const int nstreams = std::max(1, std::min(ctx->streams, kStreams));
    // instantiation key per segment
    auto key = [](const SegPlan& g) {
        return g.kind * 1000 + g.W1 * 4 + (g.straddle ? 2 : 0) + (g.trailer ? 1 : 0);
    };
    struct ReqPlan {
        std::vector<SegPlan> segs;
        int dom = -1;            // the key with the most nonces
        long double total = 0;   // nonces
        bool fused = false;      // the whole request in one fused launch
        std::vector<SegPlan> tail;  // segments off the dominant key (large requests)
        bool tail_fused = false;    // ... run as one fused launch
    };
    // plan every request first: the streams the batch needs are made (once
    // per context, make_streams) before anything is queued on them
    std::vector<ReqPlan> plans(n);
    int used = 1, nfused = 0;
    for (int r = 0; r < n; ++r) {
        if (reqs[r].empty) continue;
        ReqPlan& P = plans[r];
        P.segs = plan_range(*reqs[r].mp, reqs[r].lo, reqs[r].hi, ctx->force_generic,
                            ctx->table_digits);
        std::vector<std::pair<int, long double>> load;
        for (const auto& g : P.segs) {
            const long double cnt = (long double)(g.hi - g.lo) + 1;
            auto it = std::find_if(load.begin(), load.end(),
                                   [&](const auto& p) { return p.first == key(g); });
            if (it == load.end()) load.push_back({key(g), cnt});
            else it->second += cnt;
        }
        long double most = -1;
        for (const auto& p : load) {
            P.total += p.second;
            if (p.second > most) { most = p.second; P.dom = p.first; }
        }
        P.fused = ctx->fused && fusible(P.segs);
        if (P.fused) {
            used = std::max(used, std::min(nstreams, ++nfused));
        } else if (P.total <= (long double)kConcurrentNonces) {
            used = std::max(used, std::min(nstreams, (int)P.segs.size()));
        } else {
            // segments off the dominant key run in its tail: as ONE fused
            // launch when they fit it (cfg2's d <= 8, cfg3's trailer
            // segments), else one launch each on the tail streams
            for (const auto& g : P.segs)
                if (key(g) != P.dom) P.tail.push_back(g);
            P.tail_fused = ctx->fused && ctx->tail_fused && fusible(P.tail);
            const int off = P.tail_fused ? 1 : (int)P.tail.size();
            used = std::max(used, std::min(nstreams, 1 + off));
        }
    }
    const int ns = used;  // streams this batch enqueues onto (<= nstreams)
    {
        int rc = make_streams(dv, ns);
        if (rc) return rc;
    }
    HIPCHK(launch_init_best(dv.best, (uint32_t)(n * kStreams), s0));
    HIPCHK(launch_init_best(dv.result, (uint32_t)n, s0));
    if (ctx->csum) HIPCHK(hipMemsetAsync(dv.acc, 0, kStreams * 2 * sizeof(uint64_t), s0));
    HIPCHK(hipEventRecord(dv.join[0], s0));
    for (int s = 1; s < ns; ++s) HIPCHK(hipStreamWaitEvent(dv.stream[s], dv.join[0], 0));
    if (ctx->test_mid_sync) {  // HM_OPT_TEST_MID_SYNC: a host wait mid-enqueue, counted
        int rc = host_wait(ctx, s0);
        if (rc) return rc;
    }
    int rr = 0;
    for (int r = 0; r < n; ++r) {
        if (reqs[r].empty) continue;
        const std::vector<SegPlan>& segs = plans[r].segs;
        const int dom = plans[r].dom;
        uint64_t* best = dv.best + (size_t)r * kStreams * 2;
        if (plans[r].fused) {
            // a small request of a batch: one fused launch on the next stream
            const int si = rr++ % ns;
            int rc = enqueue_fused(ctx, dv, *reqs[r].mp, segs, si, best + 2 * si, false);
            if (rc) return rc;
            continue;
        }
        if (ns > 1 && plans[r].total <= (long double)kConcurrentNonces) {
            // a small request (config 1's [0, 10^7+1], short server chunks):
            // its launches are latency-bound, so every segment goes onto the
            // streams round-robin, ungated, largest first: the host enqueues
            // a segment every ~25 us, and the largest one should not be the
            // last to start
            std::vector<size_t> order(segs.size());
            for (size_t i = 0; i < order.size(); ++i) order[i] = i;
            std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
                return segs[a].hi - segs[a].lo > segs[b].hi - segs[b].lo;
            });
            for (size_t i : order) {
                int rc = enqueue_segment(ctx, dv, *reqs[r].mp, segs[i], rr++ % ns, best);
                if (rc) return rc;
            }
            continue;
        }
        size_t last_dom = 0;
        for (size_t i = 0; i < segs.size(); ++i)
            if (key(segs[i]) == dom) last_dom = i;
        for (int pass = 0; pass < (ns > 1 ? 2 : 1); ++pass) {
            if (pass == 1)
                for (int q = 1; q < ns; ++q)
                    HIPCHK(hipStreamWaitEvent(dv.stream[q], dv.gate, 0));
            if (pass == 1 && plans[r].tail_fused) {
                // every tail segment in one fused launch on a tail stream
                const int si = 1 + (rr++ % (ns - 1));
                int rc = enqueue_fused(ctx, dv, *reqs[r].mp, plans[r].tail, si, best + 2 * si,
                                       false);
                if (rc) return rc;
                continue;
            }
            for (size_t i = 0; i < segs.size(); ++i) {
                int si = 0;
                if (ns > 1) {
                    const bool is_dom = key(segs[i]) == dom;
                    if (is_dom != (pass == 0)) continue;
                    if (!is_dom) si = 1 + (rr++ % (ns - 1));
                    if (is_dom && i == last_dom) HIPCHK(hipEventRecord(dv.gate, dv.stream[0]));
                }
                int rc = enqueue_segment(ctx, dv, *reqs[r].mp, segs[i], si, best);
                if (rc) return rc;
            }
        }
    }
    for (int s = 1; s < ns; ++s) {
        HIPCHK(hipEventRecord(dv.join[s], dv.stream[s]));
        HIPCHK(hipStreamWaitEvent(s0, dv.join[s], 0));
    }
    for (int r = 0; r < n; ++r)
        HIPCHK(launch_fold(dv.best + (size_t)r * kStreams * 2, kStreams, dv.result + 2 * r, s0));
    return HM_OK;
}

bool lex_less(uint64_t k1, uint64_t n1, uint64_t k2, uint64_t n2) {
    return k1 < k2 || (k1 == k2 && n1 < n2);
}

// All-gather every device's n 16-B results over RCCL; device 0 folds them.
// Runs for any device count, including one (a 1-rank communicator), so the
// path the 8-GPU context takes is exercised on a 1-GPU box.
int rccl_merge(hm_ctx* ctx, int nreq) {
    const int n = (int)ctx->devs.size();
    if (!ctx->devs[0].comm) {
        std::vector<ncclComm_t> comms(n);
        std::vector<int> ords(n);
        for (int i = 0; i < n; ++i) ords[i] = ctx->devs[i].ordinal;
        if (ncclCommInitAll(comms.data(), n, ords.data()) != ncclSuccess) return HM_ERR_RCCL;
        for (int i = 0; i < n; ++i) {
            ctx->devs[i].comm = comms[i];
            HIPCHK(hipSetDevice(ctx->devs[i].ordinal));
            HIPCHK(hipMalloc(&ctx->devs[i].gathered, (size_t)n * kMaxBatch * 2 * sizeof(uint64_t)));
        }
    }
    if (ncclGroupStart() != ncclSuccess) return HM_ERR_RCCL;
    for (int i = 0; i < n; ++i) {
        Device& dv = ctx->devs[i];
        HIPCHK(hipSetDevice(dv.ordinal));
        if (ncclAllGather(dv.result, dv.gathered, (size_t)2 * nreq, ncclUint64, dv.comm,
                          dv.stream[0]) != ncclSuccess) {
            ncclGroupEnd();
            return HM_ERR_RCCL;
        }
    }
    if (ncclGroupEnd() != ncclSuccess) return HM_ERR_RCCL;
    // gathered[d][r][2]: request r's candidates are strided by nreq pairs
    Device& d0 = ctx->devs[0];
    HIPCHK(hipSetDevice(d0.ordinal));
    HIPCHK(launch_init_best(d0.result, (uint32_t)nreq, d0.stream[0]));
    for (int r = 0; r < nreq; ++r)
        HIPCHK(launch_fold(d0.gathered + 2 * r, (uint32_t)n, d0.result + 2 * r, d0.stream[0],
                           (uint32_t)nreq));
    return HM_OK;
}

// One chunk (<= kMaxBatch requests) of hm_scan_many.
int scan_chunk(hm_ctx* ctx, const hm_request* reqs, int nreq, hm_result* outs, bool first) {
    const int ndev = (int)ctx->devs.size();
    // one RCCL rank per device (hm_set_option refuses the option otherwise);
    // checked again here, before any work is enqueued
    if (ctx->merge_rccl && !distinct_ordinals(ctx)) return HM_ERR_INVALID;
    std::vector<MsgPlan> plans(nreq);
    std::vector<std::vector<DevReq>> per_dev(ndev, std::vector<DevReq>(nreq));
    for (int r = 0; r < nreq; ++r) {
        const hm_request& q = reqs[r];
        plans[r] = plan_message(msg_or_empty(q.msg, q.len));
        // contiguous shards of equal modelled cost
        const std::vector<Shard> sh =
            partition_range(plans[r], q.lo, q.hi, ndev, ctx->force_generic);
        for (int i = 0; i < ndev; ++i) {
            DevReq& dr = per_dev[i][r];
            dr.mp = &plans[r];
            dr.empty = sh[i].empty;
            dr.lo = sh[i].empty ? 0 : sh[i].lo;
            dr.hi = sh[i].empty ? 0 : sh[i].hi;
        }
    }
    // every device's work is enqueued before the host waits on any of it
    const auto te = std::chrono::steady_clock::now();
    ctx->enqueuing = true;
    for (int i = 0; i < ndev; ++i) {
        int rc = enqueue_device_batch(ctx, ctx->devs[i], per_dev[i], first);
        if (rc) { ctx->enqueuing = false; return rc; }
    }
    ctx->enqueuing = false;
    ctx->enqueue_ms +=
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - te).count();
    if (ctx->merge_rccl) {
        int rc = rccl_merge(ctx, nreq);
        if (rc) return rc;
        ctx->merge = HM_MERGE_RCCL;
        Device& d0 = ctx->devs[0];
        HIPCHK(hipSetDevice(d0.ordinal));
        HIPCHK(hipMemcpyAsync(d0.host_out, d0.result, nreq * sizeof(hm_result),
                              hipMemcpyDeviceToHost, d0.stream[0]));
        for (auto& dv : ctx->devs) {
            HIPCHK(hipSetDevice(dv.ordinal));
            int rc = host_wait(ctx, dv.stream[0]);
            if (rc) return rc;
        }
        for (int r = 0; r < nreq; ++r) outs[r] = d0.host_out[r];
        return HM_OK;
    }
    ctx->merge = ndev > 1 ? HM_MERGE_HOST : HM_MERGE_NONE;
    for (auto& dv : ctx->devs) {
        HIPCHK(hipSetDevice(dv.ordinal));
        HIPCHK(hipMemcpyAsync(dv.host_out, dv.result, nreq * sizeof(hm_result),
                              hipMemcpyDeviceToHost, dv.stream[0]));
    }
    for (int r = 0; r < nreq; ++r) outs[r] = hm_result{~0ull, 0};
    for (auto& dv : ctx->devs) {
        HIPCHK(hipSetDevice(dv.ordinal));
        int rc = host_wait(ctx, dv.stream[0]);
        if (rc) return rc;
        for (int r = 0; r < nreq; ++r)
            if (lex_less(dv.host_out[r].hash, dv.host_out[r].nonce, outs[r].hash, outs[r].nonce))
                outs[r] = dv.host_out[r];
    }
    return HM_OK;
}

}  // namespace

// hm_scan_many with ctx->mu held.
int scan_many_locked(hm_ctx* ctx, const hm_request* reqs, int n, hm_result* outs) {
    const auto t0 = std::chrono::steady_clock::now();
    // an abandoned context's devices may still run its timed-out work
    if (ctx->abandoned) return HM_ERR_TIMEOUT;
    call_deadline(ctx, reqs, n, t0);
    std::vector<hm_result> res(n);
    for (auto& dv : ctx->devs) {
        dv.evnext = 0;
        dv.launches.clear();
    }
    ctx->mid_syncs = 0;
    ctx->table_grows = 0;
    ctx->enqueue_ms = 0;
    uint64_t total = 0;
    for (int r = 0; r < n; ++r)
        if (reqs[r].lo <= reqs[r].hi) total += reqs[r].hi - reqs[r].lo + 1;  // wraps for 2^64
    ctx->merge = HM_MERGE_NONE;
    for (int c = 0; c < n; c += kMaxBatch) {
        const int m = std::min(kMaxBatch, n - c);
        int rc = scan_chunk(ctx, reqs + c, m, res.data() + c, c == 0);
        if (rc) return rc;
    }
    // stats
    hm_stats st{};
    st.nonces = total;
    // aggregate per kernel instantiation; the dominant one has the most nonces
    struct Agg { std::string name; double ms = 0; uint64_t nonces = 0; int launches = 0;
                 int kind = 0, grid = 0; uint32_t comp = 0; double comp_eff = 0;
                 uint64_t big = 0; };
    std::vector<Agg> aggs;
    for (auto& dv : ctx->devs) {
        // kernel_ms: time during which some scan kernel ran on this device
        // (union of the launches' event intervals; launches on several
        // streams overlap)
        std::vector<std::pair<float, float>> iv;
        for (auto& L : dv.launches) {
            float a = 0.f, b = 0.f;
            HIPCHK(hipEventElapsedTime(&a, dv.t0, L.start));
            HIPCHK(hipEventElapsedTime(&b, dv.t0, L.stop));
            iv.push_back({a, b});
        }
        std::sort(iv.begin(), iv.end());
        float cur_a = 0.f, cur_b = -1.f;
        for (const auto& x : iv) {
            if (x.first > cur_b) {
                if (cur_b > cur_a) st.kernel_ms += cur_b - cur_a;
                cur_a = x.first;
                cur_b = x.second;
            } else if (x.second > cur_b) {
                cur_b = x.second;
            }
        }
        if (cur_b > cur_a) st.kernel_ms += cur_b - cur_a;
        for (auto& L : dv.launches) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, L.start, L.stop));
            st.launches += 1;
            Agg* a = nullptr;
            for (auto& x : aggs)
                if (x.name == L.kernel) a = &x;
            if (!a) { aggs.push_back(Agg{}); a = &aggs.back(); a->name = L.kernel; }
            a->ms += ms;
            a->nonces += L.nonces;
            a->launches += 1;
            a->kind = L.kind;
            a->comp = std::max(a->comp, L.compressions);
            a->comp_eff += L.comp_eff * (double)L.nonces;  // nonce-weighted mean below
            if (L.nonces > a->big) { a->big = L.nonces; a->grid = L.grid; }
        }
    }
    for (auto& a : aggs) {
        if (a.nonces > st.dom_nonces) {
            st.dom_nonces = a.nonces;
            st.dom_kernel_ms = a.ms;
            st.dom_compressions = a.comp;
            st.dom_compressions_eff = a.nonces ? a.comp_eff / (double)a.nonces : 0.0;
            st.dom_kind = a.kind;
            st.dom_grid = a.grid;
            st.dom_launches = a.launches;
            snprintf(st.dom_kernel, sizeof st.dom_kernel, "%s", a.name.c_str());
        }
    }
    st.merge = ctx->merge;
    st.enqueue_ms = ctx->enqueue_ms;
    st.mid_call_syncs = ctx->mid_syncs;
    st.table_grows = ctx->table_grows;
    st.deadline_ms = ctx->deadline_ms;
    publish(ctx, ctx->scan_stats, st, t0);
    for (int r = 0; r < n; ++r) outs[r] = res[r];
    return HM_OK;
}

}  // namespace hm
