// verify_many.cpp -- hm_verify_many (ABI 1.14).
// ---------------------------------------------------------------------------
// Which (hash, nonce) records of MANY lists, each with its own message and
// target, are bad: hm_verify's answer for every request of a batch, from as
// few launches as hold them (verify_many_kernels.hip has the job and task
// tables, the device protocol and its three invariants).
//
// Host side.  plan_message per request.  The concatenation of all requests'
// records -- the flattened sequence -- is cut contiguously across the
// context's devices in even shares by record count; a cut may fall inside a
// request.  Each share is walked in order and packed into launches: a launch
// closes when it holds kVerifyChunk records (HM_OPT_VERIFY_CHUNK) or
// kVerifyJobsMax jobs (HM_OPT_VERIFY_JOBS), a request is cut where a launch
// fills (the job's index0 carries the offset) and a request without records
// makes no job.
//
// Per launch the host packs [job table | task_job | records] into one of the
// device's two pinned staging slots and issues, on stream 0, ONE copy of the
// blob and the kernel, with events around both.  The slots alternate; a slot
// is refilled only after the copy that last read it has completed (that wait
// honours the deadline), so the first two launches of every device are
// enqueued before the host waits on anything: the launches are walked
// round-robin over the devices.  The one device blob is reused: the stream
// orders a launch's copy after the previous launch's kernel.  Then one
// host_wait per device and the readback of its count words, cursor and refs;
// the pieces' counts are summed per request, the refs sorted by (request,
// index).
//
// The caller's memory is pageable and is neither registered nor altered: the
// packing pass reads it, and that pass is why a single large list is better
// served by hm_verify (DESIGN.md §3e has the measured rates).
// ---------------------------------------------------------------------------
#include "hm_internal.hpp"

namespace hm {
namespace {

const char* kJobsKernel = "_ZN2hm21hm_verify_jobs_kernelENS_14VerifyJobsArgsE";

// A job before it is packed: records [off, off + n) of request `req`.
struct Piece {
    uint32_t req;
    uint32_t n;
    size_t off;
};

struct VmLaunch {
    size_t job0 = 0;  // the launch's first job among the device's
    uint32_t njobs = 0, nrec = 0, ntasks = 0;
    // byte offsets in the blob (the job table is at 0)
    size_t task_off() const { return (size_t)njobs * sizeof(VerifyJob); }
    size_t rec_off() const {
        return (task_off() + (size_t)ntasks * sizeof(uint32_t) + 15) & ~(size_t)15;
    }
    size_t bytes() const { return rec_off() + (size_t)nrec * sizeof(hm_result); }
};

// One device's share of a call: flattened records [lo, hi).
struct VmDev {
    uint64_t lo = 0, hi = 0;
    std::vector<Piece> jobs;
    std::vector<VmLaunch> launches;
    std::vector<hipEvent_t> ev;  // per launch: before the copy, after it, after the kernel
    const Device::Fn* fn = nullptr;
};

// A pinned staging slot of at least `want` bytes: grown by at least doubling,
// the old one kept until hm_close.
int grow_stage(Device& dv, int slot, size_t want) {
    if (want <= dv.vm_stage_bytes[slot]) return HM_OK;
    const size_t size = std::max(want, 2 * dv.vm_stage_bytes[slot]);
    void* p = nullptr;
    if (hipHostMalloc(&p, size, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return HM_ERR_NOMEM;
    }
    if (dv.vm_stage[slot]) dv.retired_host.push_back(dv.vm_stage[slot]);
    dv.vm_stage[slot] = static_cast<uint64_t*>(p);
    dv.vm_stage_bytes[slot] = size;
    return HM_OK;
}

// Cut share [lo, hi) of the flattened sequence (start[i]: request i's first
// position; start[nreq]: the total) into jobs and launches.
void pack_share(const std::vector<uint64_t>& start, uint32_t chunk, uint32_t maxjobs, VmDev* vd) {
    // the request holding position lo
    int r = (int)(std::upper_bound(start.begin(), start.end(), vd->lo) - start.begin()) - 1;
    uint64_t pos = vd->lo;
    VmLaunch cur;
    while (pos < vd->hi) {
        while (start[r + 1] <= pos) ++r;  // past requests without records too
        const uint64_t end = std::min<uint64_t>(start[r + 1], vd->hi);
        const uint32_t n = (uint32_t)std::min<uint64_t>(end - pos, chunk - cur.nrec);
        vd->jobs.push_back(Piece{(uint32_t)r, n, (size_t)(pos - start[r])});
        ++cur.njobs;
        cur.nrec += n;
        cur.ntasks += (n + kWaveSize - 1) / kWaveSize;
        pos += n;
        if (cur.nrec == chunk || cur.njobs == maxjobs) {
            vd->launches.push_back(cur);
            VmLaunch next;
            next.job0 = cur.job0 + cur.njobs;
            cur = next;
        }
    }
    if (cur.njobs) vd->launches.push_back(cur);
}

// Launch k of a device into its staging slot.
void fill_slot(const hm_verify_request* reqs, const std::vector<MsgPlan>& plans, const VmDev& vd,
               const VmLaunch& L, uint8_t* blob) {
    VerifyJob* jobs = reinterpret_cast<VerifyJob*>(blob);
    uint32_t* task_job = reinterpret_cast<uint32_t*>(blob + L.task_off());
    uint8_t* recs = blob + L.rec_off();
    uint32_t first = 0, task = 0;
    for (uint32_t j = 0; j < L.njobs; ++j) {
        const Piece& p = vd.jobs[L.job0 + j];
        const MsgPlan& mp = plans[p.req];
        VerifyJob& J = jobs[j];
        J.target = reqs[p.req].target;
        J.bits0 = (mp.len + 1) * 8;
        J.index0 = p.off;
        J.request = p.req;
        J.first = first;
        J.n = p.n;
        J.task0 = task;
        J.r = mp.r;
        memcpy(J.pw, mp.pw, sizeof J.pw);
        memcpy(J.mid, mp.mid, sizeof J.mid);
        memcpy(recs + (size_t)first * sizeof(hm_result), reqs[p.req].recs + p.off,
               (size_t)p.n * sizeof(hm_result));
        const uint32_t nt = (p.n + kWaveSize - 1) / kWaveSize;
        for (uint32_t t = 0; t < nt; ++t) task_job[task + t] = j;
        first += p.n;
        task += nt;
    }
}

}  // namespace

int verify_many_locked(hm_ctx* ctx, const hm_verify_request* reqs, int nreq, size_t cap,
                       std::vector<uint64_t>* per, std::vector<hm_bad_ref>* refs, uint64_t* bad) {
    const auto t0 = std::chrono::steady_clock::now();
    // an abandoned context's devices may still run its timed-out work
    if (ctx->abandoned) return HM_ERR_TIMEOUT;
    const int ndev = (int)ctx->devs.size();
    const uint32_t chunk = ctx->verify_chunk ? ctx->verify_chunk : kVerifyChunk;
    const uint32_t maxjobs = ctx->verify_jobs ? ctx->verify_jobs : kVerifyJobsMax;
    per->assign((size_t)nreq, 0);
    refs->clear();
    // the flattened sequence: request i holds positions [start[i], start[i + 1])
    std::vector<uint64_t> start((size_t)nreq + 1, 0);
    for (int i = 0; i < nreq; ++i) {
        if (reqs[i].n > UINT64_MAX - start[i]) return HM_ERR_INVALID;
        start[i + 1] = start[i] + reqs[i].n;
    }
    const uint64_t total = start[nreq];
    list_deadline(ctx, (size_t)total, t0);
    std::vector<VmDev> vds(ndev);
    uint64_t sum = 0, tasks = 0;
    int launches = 0;
    double kernel_ms = 0, copy_ms = 0;
    if (total > 0) {
        std::vector<MsgPlan> plans((size_t)nreq);
        for (int i = 0; i < nreq; ++i)
            if (reqs[i].n) plans[i] = plan_message(msg_or_empty(reqs[i].msg, reqs[i].len));
        typedef unsigned __int128 u128;
        size_t most = 0;  // launches of the busiest device
        for (int i = 0; i < ndev; ++i) {
            VmDev& vd = vds[i];
            vd.lo = (uint64_t)((u128)total * (unsigned)i / (unsigned)ndev);
            vd.hi = (uint64_t)((u128)total * (unsigned)(i + 1) / (unsigned)ndev);
            pack_share(start, chunk, maxjobs, &vd);
            most = std::max(most, vd.launches.size());
        }
        // every buffer a device needs, before anything is enqueued
        for (int i = 0; i < ndev; ++i) {
            Device& dv = ctx->devs[i];
            VmDev& vd = vds[i];
            HIPCHK(hipSetDevice(dv.ordinal));
            dv.evnext = 0;
            if (vd.launches.empty()) continue;
            size_t bytes = 0;
            for (const VmLaunch& L : vd.launches) bytes = std::max(bytes, L.bytes());
            const size_t any = ~(size_t)0;  // no upper bound: at least doubled
            int rc = grow_buffer(dv, &dv.vm_blob, &dv.vm_blob_bytes, bytes, any, 1);
            for (size_t k = 0; !rc && k < std::min<size_t>(2, vd.launches.size()); ++k)
                rc = grow_stage(dv, (int)k, bytes);
            if (!rc)
                rc = grow_buffer(dv, &dv.vm_ctl, &dv.vm_ctl_words, 1 + vd.jobs.size(),
                                 any / sizeof(uint64_t), sizeof(uint64_t));
            if (!rc)
                rc = grow_buffer(dv, &dv.vm_refs, &dv.vm_refs_cap, cap, HM_VERIFY_CAP_MAX,
                                 sizeof(hm_bad_ref));
            if (rc) return rc;
        }
        for (int i = 0; i < ndev; ++i) {
            Device& dv = ctx->devs[i];
            VmDev& vd = vds[i];
            if (vd.launches.empty()) continue;
            if (hipSetDevice(dv.ordinal) != hipSuccess) return drain_failed(ctx, HM_ERR_HIP);
            const int rc = scan_fn(dv, kJobsKernel, &vd.fn);
            if (rc) return drain_failed(ctx, rc);
            // the cursor and every job's count start at 0
            if (hipMemsetAsync(dv.vm_ctl, 0, (1 + vd.jobs.size()) * sizeof(uint64_t),
                               dv.stream[0]) != hipSuccess)
                return drain_failed(ctx, HM_ERR_HIP);
        }
        // launch k of every device, then launch k + 1: two launches per device
        // are enqueued everywhere before the host first waits for a slot
        for (size_t k = 0; k < most; ++k) {
            for (int i = 0; i < ndev; ++i) {
                Device& dv = ctx->devs[i];
                VmDev& vd = vds[i];
                if (k >= vd.launches.size()) continue;
                const VmLaunch& L = vd.launches[k];
                if (hipSetDevice(dv.ordinal) != hipSuccess) return drain_failed(ctx, HM_ERR_HIP);
                hipStream_t st = dv.stream[0];
                const int slot = (int)(k & 1);
                int rc = HM_OK;
                // the copy of launch k - 2 read this slot: it must be over
                if (k >= 2) rc = host_wait(ctx, vd.ev[3 * (k - 2) + 1]);
                if (rc) return drain_failed(ctx, rc);
                uint8_t* stage = reinterpret_cast<uint8_t*>(dv.vm_stage[slot]);
                fill_slot(reqs, plans, vd, L, stage);
                hipEvent_t e[3] = {};
                for (int x = 0; x < 3; ++x) {
                    rc = next_event(dv, &e[x]);
                    if (rc) return drain_failed(ctx, rc);
                    vd.ev.push_back(e[x]);
                }
                uint8_t* blob = reinterpret_cast<uint8_t*>(dv.vm_blob);
                VerifyJobsArgs ka{};
                ka.jobs = reinterpret_cast<const VerifyJob*>(blob);
                ka.task_job = reinterpret_cast<const uint32_t*>(blob + L.task_off());
                ka.recs = reinterpret_cast<const uint64_t*>(blob + L.rec_off());
                ka.bad = dv.vm_ctl + 1 + L.job0;
                ka.cursor = dv.vm_ctl;
                ka.refs = cap ? dv.vm_refs : nullptr;
                ka.ntasks = L.ntasks;
                ka.cap = (uint32_t)cap;
                const uint64_t blocks = ((uint64_t)L.ntasks + kBlock / kWaveSize - 1) /
                                        (kBlock / kWaveSize);
                const int grid = (int)std::min<uint64_t>(
                    std::min<uint64_t>(blocks, kMaxCandWaves / (kBlock / kWaveSize)),
                    (uint64_t)std::max(1, vd.fn->blocks_per_cu) * (uint64_t)dv.cus);
                if (hipEventRecord(e[0], st) != hipSuccess ||
                    hipMemcpyAsync(blob, stage, L.bytes(), hipMemcpyHostToDevice, st) !=
                        hipSuccess ||
                    hipEventRecord(e[1], st) != hipSuccess)
                    return drain_failed(ctx, HM_ERR_HIP);
                rc = launch_scan(*vd.fn, ka, grid, st);
                if (rc) return drain_failed(ctx, rc);
                if (hipEventRecord(e[2], st) != hipSuccess) return drain_failed(ctx, HM_ERR_HIP);
                ++launches;
                tasks += L.ntasks;
            }
        }
        // everything is enqueued: wait for each device, then read it back
        for (int i = 0; i < ndev; ++i) {
            if (vds[i].launches.empty()) continue;
            Device& dv = ctx->devs[i];
            if (hipSetDevice(dv.ordinal) != hipSuccess) return drain_failed(ctx, HM_ERR_HIP);
            const int rc = host_wait(ctx, dv.stream[0]);
            if (rc) return drain_failed(ctx, rc);
        }
        std::vector<uint64_t> dev_total(ndev, 0);
        std::vector<uint64_t> ctl;
        for (int i = 0; i < ndev; ++i) {
            Device& dv = ctx->devs[i];
            const VmDev& vd = vds[i];
            if (vd.launches.empty()) continue;
            HIPCHK(hipSetDevice(dv.ordinal));
            ctl.resize(1 + vd.jobs.size());
            const int rc = host_read(ctx, ctl.data(), dv.vm_ctl, ctl.size() * sizeof(uint64_t));
            if (rc) return rc;
            for (size_t j = 0; j < vd.jobs.size(); ++j) {
                // no more bad records than the piece has records
                if (ctl[1 + j] > vd.jobs[j].n) return HM_ERR_INTERNAL;
                (*per)[vd.jobs[j].req] += ctl[1 + j];
                dev_total[i] += ctl[1 + j];
            }
            // a device whose refs all fit reserved exactly one slot per bad record
            if (cap && dev_total[i] <= cap && ctl[0] != dev_total[i]) return HM_ERR_INTERNAL;
            sum += dev_total[i];
            for (size_t k = 0; k + 3 <= vd.ev.size(); k += 3) {
                float ms = 0.f;
                HIPCHK(hipEventElapsedTime(&ms, vd.ev[k], vd.ev[k + 1]));
                copy_ms += ms;
                HIPCHK(hipEventElapsedTime(&ms, vd.ev[k + 1], vd.ev[k + 2]));
                kernel_ms += ms;
            }
            dv.evnext = 0;  // the events are free again
        }
        if (sum <= cap && sum > 0) {
            refs->resize((size_t)sum);
            size_t at = 0;
            for (int i = 0; i < ndev; ++i) {
                if (!dev_total[i]) continue;
                Device& dv = ctx->devs[i];
                HIPCHK(hipSetDevice(dv.ordinal));
                const size_t cnt = (size_t)dev_total[i];
                const int rc = host_read(ctx, refs->data() + at, dv.vm_refs, cnt * sizeof(hm_bad_ref));
                if (rc) return rc;
                // slots are handed out in dispatch order: the answer is ascending
                std::sort(refs->begin() + at, refs->begin() + at + cnt,
                          [](const hm_bad_ref& a, const hm_bad_ref& b) {
                              return a.request != b.request ? a.request < b.request
                                                            : a.index < b.index;
                          });
                // a device's refs are distinct and lie in its pieces: in a
                // real request, inside its list, at a flattened position of
                // the device's share (the shares ascend, so the concatenation
                // is sorted)
                for (size_t k = at; k < at + cnt; ++k) {
                    const hm_bad_ref& x = (*refs)[k];
                    if (x.request >= (uint64_t)nreq || x.index >= reqs[x.request].n)
                        return HM_ERR_INTERNAL;
                    const uint64_t pos = start[x.request] + x.index;
                    if (pos < vds[i].lo || pos >= vds[i].hi) return HM_ERR_INTERNAL;
                    if (k > at && x.request == (*refs)[k - 1].request &&
                        x.index == (*refs)[k - 1].index)
                        return HM_ERR_INTERNAL;
                }
                at += cnt;
            }
        }
    }
    hm_verify_many_stats vs{};
    vs.kernel_ms = kernel_ms;
    vs.copy_ms = copy_ms;
    vs.records = total;
    vs.bad = sum;
    vs.tasks = tasks;
    vs.requests = nreq;
    vs.launches = launches;
    vs.copies = launches;  // one blob per launch
    vs.overflow = sum > cap ? 1 : 0;
    publish(ctx, ctx->verify_many_stats, vs, t0);
    *bad = sum;
    return HM_OK;
}

}  // namespace hm
