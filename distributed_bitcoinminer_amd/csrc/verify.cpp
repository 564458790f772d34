// verify.cpp -- hm_hash_many and hm_verify (ABI 1.12).
// ---------------------------------------------------------------------------
// Hash(msg, nonce) at a LIST of arbitrary nonces (hm_hash_many), and which
// (hash, nonce) records of a list are wrong for msg or not below a target
// (hm_verify): one kernel template for both (verify_kernels.hip has the
// per-lane layout, the device protocol and its three invariants).
//
// Host side.  plan_message gives the midstate; the list is cut contiguously
// across the context's devices in even shares, each share into chunks of at
// most kVerifyChunk elements (HM_OPT_VERIFY_CHUNK).  Per chunk, on the
// device's stream 0: copy the chunk in, launch the kernel (verify: with the
// global index of the chunk's first record), and for hm_hash_many copy the
// hashes out (they were written in place, over the nonces).  The one chunk
// buffer is reused: the stream orders a chunk's copy in after the previous
// chunk's kernel and copy out.  Every device's work is enqueued before the
// host waits on any -- one host_wait per device -- and then each device's
// total, cursor and indices are read back, the totals summed, the indices
// concatenated and sorted.
//
// The caller's memory is pageable and is neither registered nor altered: the
// copies are hipMemcpyAsync between it and the chunk buffer, which the
// runtime stages through its own pinned buffers (DESIGN.md "Recheck a list"
// has the measured split between copies and kernel).
// ---------------------------------------------------------------------------
#include "hm_internal.hpp"

namespace hm {
namespace {

// _ZN2hm19hm_hash_list_kernelILb{0,1}EEEvNS_10VerifyArgsE
const char* list_kernel_symbol(bool verify) {
    return verify ? "_ZN2hm19hm_hash_list_kernelILb1EEEvNS_10VerifyArgsE"
                  : "_ZN2hm19hm_hash_list_kernelILb0EEEvNS_10VerifyArgsE";
}

// One device's share of a call: list elements [lo, hi).
struct ListDev {
    size_t lo = 0, hi = 0;
    std::vector<hipEvent_t> ev;  // per chunk: before the copy in, the launch, after it[, after the copy out]
    int launches = 0;
};

}  // namespace

int list_locked(hm_ctx* ctx, const uint8_t* msg, size_t len, const uint64_t* nonces,
                const hm_result* recs, size_t n, uint64_t target, size_t cap,
                std::vector<uint64_t>* out, uint64_t* bad) {
    const auto t0 = std::chrono::steady_clock::now();
    // an abandoned context's devices may still run its timed-out work
    if (ctx->abandoned) return HM_ERR_TIMEOUT;
    const Msg m = msg_or_empty(msg, len);
    list_deadline(ctx, n, t0);
    const bool verify = recs != nullptr;
    const size_t unit = verify ? sizeof(hm_result) : sizeof(uint64_t);
    const uint8_t* src = verify ? reinterpret_cast<const uint8_t*>(recs)
                                : reinterpret_cast<const uint8_t*>(nonces);
    const int ndev = (int)ctx->devs.size();
    const size_t chunk = ctx->verify_chunk ? ctx->verify_chunk : kVerifyChunk;
    const int evs_per_chunk = verify ? 3 : 4;
    std::vector<ListDev> lds(ndev);
    uint64_t sum = 0;
    double kernel_ms = 0, copy_ms = 0;
    out->clear();
    if (n > 0) {
        if (!verify) out->resize(n);
        const MsgPlan mp = plan_message(m);
        typedef unsigned __int128 u128;
        for (int i = 0; i < ndev; ++i) {
            lds[i].lo = (size_t)((u128)n * (unsigned)i / (unsigned)ndev);
            lds[i].hi = (size_t)((u128)n * (unsigned)(i + 1) / (unsigned)ndev);
        }
        for (int i = 0; i < ndev; ++i) {
            Device& dv = ctx->devs[i];
            HIPCHK(hipSetDevice(dv.ordinal));
            dv.evnext = 0;
            const size_t share = lds[i].hi - lds[i].lo;
            if (!share) continue;
            int rc = grow_buffer(dv, &dv.verify_in, &dv.verify_in_bytes, std::min(share, chunk) * unit,
                                 (size_t)kVerifyChunk * sizeof(hm_result), 1);
            if (rc) return rc;
            if (verify) {
                rc = grow_buffer(dv, &dv.verify_idx, &dv.verify_idx_cap, cap, HM_VERIFY_CAP_MAX,
                                 sizeof(uint64_t));
                if (!rc) rc = ctl_block(&dv.verify_ctl, 2);
                if (rc) return rc;
            }
        }
        for (int i = 0; i < ndev; ++i) {
            Device& dv = ctx->devs[i];
            ListDev& ld = lds[i];
            if (ld.lo == ld.hi) continue;
            if (hipSetDevice(dv.ordinal) != hipSuccess) return drain_failed(ctx, HM_ERR_HIP);
            hipStream_t st = dv.stream[0];
            const Device::Fn* fn = nullptr;
            int rc = scan_fn(dv, list_kernel_symbol(verify), &fn);
            if (rc) return drain_failed(ctx, rc);
            // the total and the slot cursor start at 0
            if (verify &&
                hipMemsetAsync(dv.verify_ctl, 0, 2 * sizeof(uint64_t), st) != hipSuccess)
                return drain_failed(ctx, HM_ERR_HIP);
            VerifyArgs ka{};
            ka.in = dv.verify_in;
            ka.hashes = verify ? nullptr : dv.verify_in;
            ka.total = verify ? dv.verify_ctl : nullptr;
            ka.cursor = verify ? dv.verify_ctl + 1 : nullptr;
            ka.idx = verify && cap ? dv.verify_idx : nullptr;
            ka.target = target;
            ka.bits0 = ((uint64_t)m.len + 1) * 8;
            ka.cap = (uint32_t)cap;
            ka.r = mp.r;
            memcpy(ka.pw, mp.pw, sizeof ka.pw);
            memcpy(ka.mid, mp.mid, sizeof ka.mid);
            for (size_t a = ld.lo; a < ld.hi; a += chunk) {
                const size_t cn = std::min(chunk, ld.hi - a);
                hipEvent_t e[4] = {};
                for (int k = 0; k < evs_per_chunk; ++k) {
                    rc = next_event(dv, &e[k]);
                    if (rc) return drain_failed(ctx, rc);
                    ld.ev.push_back(e[k]);
                }
                ka.index0 = a;
                ka.n = (uint32_t)cn;
                const uint64_t blocks = (cn + kBlock - 1) / kBlock;
                const int grid = (int)std::min<uint64_t>(
                    blocks, (uint64_t)std::max(1, fn->blocks_per_cu) * (uint64_t)dv.cus);
                if (hipEventRecord(e[0], st) != hipSuccess ||
                    hipMemcpyAsync(dv.verify_in, src + a * unit, cn * unit, hipMemcpyHostToDevice,
                                   st) != hipSuccess ||
                    hipEventRecord(e[1], st) != hipSuccess)
                    return drain_failed(ctx, HM_ERR_HIP);
                rc = launch_scan(*fn, ka, grid, st);
                if (rc) return drain_failed(ctx, rc);
                ++ld.launches;
                if (hipEventRecord(e[2], st) != hipSuccess) return drain_failed(ctx, HM_ERR_HIP);
                if (!verify &&
                    (hipMemcpyAsync(out->data() + a, dv.verify_in, cn * sizeof(uint64_t),
                                    hipMemcpyDeviceToHost, st) != hipSuccess ||
                     hipEventRecord(e[3], st) != hipSuccess))
                    return drain_failed(ctx, HM_ERR_HIP);
            }
        }
        // everything is enqueued: wait for each device, then read it back
        for (int i = 0; i < ndev; ++i) {
            if (lds[i].lo == lds[i].hi) continue;
            Device& dv = ctx->devs[i];
            if (hipSetDevice(dv.ordinal) != hipSuccess) return drain_failed(ctx, HM_ERR_HIP);
            const int rc = host_wait(ctx, dv.stream[0]);
            if (rc) return drain_failed(ctx, rc);
        }
        std::vector<uint64_t> dev_total(ndev, 0);
        for (int i = 0; i < ndev; ++i) {
            Device& dv = ctx->devs[i];
            const ListDev& ld = lds[i];
            if (ld.lo == ld.hi) continue;
            HIPCHK(hipSetDevice(dv.ordinal));
            if (verify) {
                uint64_t ctl[2];
                const int rc = host_read(ctx, ctl, dv.verify_ctl, sizeof ctl);
                if (rc) return rc;
                dev_total[i] = ctl[0];
                // no more bad records than records; a device whose indices
                // all fit reserved exactly one slot per bad record
                if (ctl[0] > ld.hi - ld.lo) return HM_ERR_INTERNAL;
                if (cap && ctl[0] <= cap && ctl[1] != ctl[0]) return HM_ERR_INTERNAL;
                sum += ctl[0];
            }
            for (size_t k = 0; k + evs_per_chunk <= ld.ev.size(); k += evs_per_chunk) {
                float ms = 0.f;
                HIPCHK(hipEventElapsedTime(&ms, ld.ev[k], ld.ev[k + 1]));
                copy_ms += ms;
                HIPCHK(hipEventElapsedTime(&ms, ld.ev[k + 1], ld.ev[k + 2]));
                kernel_ms += ms;
                if (!verify) {
                    HIPCHK(hipEventElapsedTime(&ms, ld.ev[k + 2], ld.ev[k + 3]));
                    copy_ms += ms;
                }
            }
            dv.evnext = 0;  // the events are free again
        }
        if (verify && sum <= cap && sum > 0) {
            out->resize((size_t)sum);
            size_t at = 0;
            for (int i = 0; i < ndev; ++i) {
                if (!dev_total[i]) continue;
                Device& dv = ctx->devs[i];
                HIPCHK(hipSetDevice(dv.ordinal));
                const int rc = host_read(ctx, out->data() + at, dv.verify_idx,
                                         (size_t)dev_total[i] * sizeof(uint64_t));
                if (rc) return rc;
                // slots are handed out in dispatch order: the answer is ascending
                std::sort(out->begin() + at, out->begin() + at + (size_t)dev_total[i]);
                // a device's indices are distinct and lie in its share (the
                // shares ascend, so the concatenation is sorted and < n)
                for (size_t k = at; k < at + (size_t)dev_total[i]; ++k) {
                    const uint64_t x = (*out)[k];
                    if (x < lds[i].lo || x >= lds[i].hi || (k > at && x == (*out)[k - 1]))
                        return HM_ERR_INTERNAL;
                }
                at += (size_t)dev_total[i];
            }
        }
    }
    hm_verify_stats vs{};
    vs.kernel_ms = kernel_ms;
    vs.copy_ms = copy_ms;
    vs.records = n;
    vs.bad = sum;
    vs.overflow = verify && sum > cap ? 1 : 0;
    for (const ListDev& ld : lds) vs.launches += ld.launches;
    publish(ctx, ctx->verify_stats, vs, t0);
    *bad = sum;
    return HM_OK;
}

}  // namespace hm
