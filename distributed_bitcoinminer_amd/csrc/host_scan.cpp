// host_scan.cpp -- hm_scan_cpu, hm_find_cpu, hm_find_many_cpu, hm_collect_cpu,
// hm_collect_many_cpu, hm_hash_many_cpu, hm_verify_cpu, hm_verify_many_cpu and
// hm_find_k_cpu:
// the min-hash scan, the first-below-target search (ABI 1.10) and its batch
// form (ABI 1.13), the all-below-target collection (ABI 1.11) and its batch
// form (ABI 1.15), the recheck of a list (ABI 1.12) and of the lists of many
// messages (ABI 1.14), the k-lowest-below-target search (ABI 1.16) and
// hm_scan_k_cpu, the k lowest hashes of a range (ABI 1.19), on the host's
// cores.
//
// SURVEY §8(b)'s liveness path.  The reference miner always answers a
// Request with a Result (cmu440/bitcoin/miner/miner.go:60-62); a GPU miner
// whose device is missing or failed keeps that contract by scanning here,
// bit-identically to hm_scan: the lexicographic min of (Hash(msg, n), n) over
// the INCLUSIVE [lo, hi] (miner.go:46-59 over bitcoin.Hash, hash.go:13-17),
// seeded (2^64-1, 0).
//
// Work split: `threads` contiguous, near-equal chunks of [lo, hi], one
// std::thread each, merged lexicographically (the merge is associative and
// ties go to the lowest nonce, so the split does not change the answer).
// Per chunk and digit segment: the planner's midstate over the constant
// message blocks (plan_message), the tail bytes built once, the decimal
// digits incremented in place, and a two-block tail's first block
// recompressed only when a carry reaches it.  The compression uses the x86
// SHA extensions when the CPU has them (HM_CPU_NO_SHA=1 forces the portable
// C compression, for tests), else the planner's h_compress.
#include <sched.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

#include "../../include/hipminer.h"
#include "plan.hpp"
#include "sha256_defs.hpp"

namespace hm {
namespace {

struct Best {
    uint64_t key = ~0ull, nonce = 0;  // miner.go:48-49
    void take(uint64_t k, uint64_t n) {
        if (k < key || (k == key && n < nonce)) { key = k; nonce = n; }
    }
};

inline uint32_t load_be32(const uint8_t* p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return __builtin_bswap32(v);
}

// Portable compression of one 64-byte block from `st` into `out`.
void compress_c(const uint32_t st[8], const uint8_t* blk, uint32_t out[8]) {
    uint32_t m[16];
    for (int i = 0; i < 16; ++i) m[i] = load_be32(blk + 4 * i);
    for (int i = 0; i < 8; ++i) out[i] = st[i];
    h_compress(out, m);
}

#if defined(__x86_64__)
// The same compression with the SHA extensions.  The state lives in two
// registers as (A, B, E, F) and (C, D, G, H), the order sha256rnds2 takes;
// each sha256rnds2 runs two rounds on the two low dwords of its message
// operand (W[i] + K[i] already added), so four rounds take two of them with
// the message shifted by 8 bytes in between.  Schedule: W[t..t+3] =
// msg2(msg1(W[t-16..], W[t-12..]) + W[t-7..t-4], W[t-4..]).
__attribute__((target("sha,sse4.1,ssse3"))) void compress_ni(const uint32_t st[8],
                                                             const uint8_t* blk,
                                                             uint32_t out[8]) {
    const __m128i bswap = _mm_set_epi64x(0x0c0d0e0f08090a0bll, 0x0405060700010203ll);
    __m128i dcba = _mm_loadu_si128(reinterpret_cast<const __m128i*>(st));      // lanes a b c d
    __m128i hgfe = _mm_loadu_si128(reinterpret_cast<const __m128i*>(st + 4));  // lanes e f g h
    const __m128i cdab = _mm_shuffle_epi32(dcba, 0xB1);                       // b a d c
    const __m128i efgh = _mm_shuffle_epi32(hgfe, 0x1B);                       // h g f e
    __m128i abef = _mm_alignr_epi8(cdab, efgh, 8);                            // f e b a
    __m128i cdgh = _mm_blend_epi16(efgh, cdab, 0xF0);                         // h g d c
    const __m128i abef0 = abef, cdgh0 = cdgh;
    __m128i w[4];
    for (int i = 0; i < 4; ++i)
        w[i] = _mm_shuffle_epi8(_mm_loadu_si128(reinterpret_cast<const __m128i*>(blk + 16 * i)),
                                bswap);
    for (int q = 0; q < 16; ++q) {
        __m128i cur;
        if (q < 4) {
            cur = w[q];
        } else {
            // w[q & 3] holds W[4q-16 ..]; the others the three groups after it
            const __m128i a = w[q & 3], b = w[(q + 1) & 3], c = w[(q + 2) & 3], d = w[(q + 3) & 3];
            const __m128i t = _mm_add_epi32(_mm_sha256msg1_epu32(a, b), _mm_alignr_epi8(d, c, 4));
            cur = _mm_sha256msg2_epu32(t, d);
            w[q & 3] = cur;
        }
        __m128i kw = _mm_add_epi32(cur, _mm_loadu_si128(reinterpret_cast<const __m128i*>(kK + 4 * q)));
        cdgh = _mm_sha256rnds2_epu32(cdgh, abef, kw);
        kw = _mm_shuffle_epi32(kw, 0x0E);
        abef = _mm_sha256rnds2_epu32(abef, cdgh, kw);
    }
    abef = _mm_add_epi32(abef, abef0);
    cdgh = _mm_add_epi32(cdgh, cdgh0);
    const __m128i feba = _mm_shuffle_epi32(abef, 0x1B);                 // a b e f
    const __m128i dchg = _mm_shuffle_epi32(cdgh, 0xB1);                 // g h c d
    dcba = _mm_blend_epi16(feba, dchg, 0xF0);                           // a b c d
    hgfe = _mm_alignr_epi8(dchg, feba, 8);                              // e f g h
    _mm_storeu_si128(reinterpret_cast<__m128i*>(out), dcba);
    _mm_storeu_si128(reinterpret_cast<__m128i*>(out + 4), hgfe);
}
#endif

typedef void (*CompressFn)(const uint32_t[8], const uint8_t*, uint32_t[8]);

CompressFn pick_compress() {
    const char* off = getenv("HM_CPU_NO_SHA");
    if (off && *off && strcmp(off, "0") != 0) return compress_c;
#if defined(__x86_64__)
    __builtin_cpu_init();
    if (__builtin_cpu_supports("sha") && __builtin_cpu_supports("sse4.1")) return compress_ni;
#endif
    return compress_c;
}

// The tail blocks of nonce x (d digits) behind the midstate: r prefix bytes,
// the digits, 0x80, zeros and the 64-bit bit length fill tail[0 .. 64 * nb).
// Returns nb (1 or 2); the last digit is tail[r + d - 1].
uint32_t build_tail(const MsgPlan& mp, uint64_t x, uint32_t d, uint8_t tail[128]) {
    const uint32_t r = mp.r, T = r + d;
    memset(tail, 0, 128);
    for (uint32_t i = 0; i < r; ++i) tail[i] = (uint8_t)(mp.pw[i / 4] >> (24 - 8 * (i % 4)));
    for (uint32_t k = 0; k < d; ++k) {
        tail[T - 1 - k] = (uint8_t)('0' + x % 10);
        x /= 10;
    }
    tail[T] = 0x80;
    const uint32_t nb = T + 9 <= 64 ? 1 : 2;
    const uint64_t bits = (mp.len + 1 + d) * 8;
    for (int i = 0; i < 8; ++i) tail[64 * nb - 1 - i] = (uint8_t)(bits >> (8 * i));
    return nb;
}

// Walk [a, b] (a <= b, one thread) in ascending order, every digit segment of
// it in turn: visit(key, nonce) per nonce; a true return ends the walk.
template <typename Visit>
void walk_chunk(const MsgPlan& mp, uint64_t a, uint64_t b, CompressFn compress, Visit&& visit) {
    for (uint32_t d = digits_u64(a); d <= digits_u64(b); ++d) {
        const uint64_t dlo = d == 1 ? 0 : pow10_u64(d - 1);
        const uint64_t dhi = d == 20 ? ~0ull : pow10_u64(d) - 1;
        const uint64_t slo = std::max(a, dlo), shi = std::min(b, dhi);
        if (slo > shi) continue;
        uint8_t tail[128];
        const uint32_t nb = build_tail(mp, slo, d, tail), T = mp.r + d;
        const uint8_t* last = tail + 64 * (nb - 1);
        uint32_t s0[8];  // state entering the last tail block
        if (nb == 2) compress(mp.mid, tail, s0);
        else memcpy(s0, mp.mid, sizeof s0);
        const uint64_t count_m1 = shi - slo;
        for (uint64_t i = 0;; ++i) {
            uint32_t o[8];
            compress(s0, last, o);
            if (visit(((uint64_t)o[0] << 32) | o[1], slo + i)) return;
            if (i == count_m1) break;
            // next nonce: increment the ASCII digits in place (no carry out:
            // every nonce of the segment has d digits)
            uint32_t p = T - 1;
            while (tail[p] == '9') tail[p--] = '0';
            ++tail[p];
            if (nb == 2 && p < 64) compress(mp.mid, tail, s0);
        }
    }
}

// Scan [a, b]: the lexicographic minimum of the walk.
void scan_chunk(const MsgPlan& mp, uint64_t a, uint64_t b, CompressFn compress, Best* out) {
    Best best;
    walk_chunk(mp, a, b, compress, [&](uint64_t k, uint64_t n) {
        best.take(k, n);
        return false;
    });
    *out = best;
}

// hm_find_cpu's shared state.  Threads take ascending windows of kFindWindow
// nonces from `next`, fold the first hit of a window into `best` (atomic
// minimum; `hit` tells a hit at nonce MaxUint64 from none) and stop taking
// windows that start above it.  The three invariants of the GPU protocol
// (find_kernels.hip) hold here too: only in-range nonces with key < target
// reach `best`; a window is left out only when all of it lies above a value
// already in `best`, which only decreases; every window a thread walked has
// folded its hit before the threads are joined.
constexpr uint64_t kFindWindow = 1ull << 14;
struct FindShared {
    std::atomic<uint64_t> next{0};
    std::atomic<uint64_t> best{~0ull};
    std::atomic<bool> hit{false};
};

void find_worker(const MsgPlan& mp, uint64_t lo, uint64_t hi, uint64_t target, uint64_t nwin,
                 CompressFn compress, FindShared* sh) {
    for (;;) {
        const uint64_t w = sh->next.fetch_add(1, std::memory_order_relaxed);
        if (w >= nwin) return;
        const uint64_t a = lo + w * kFindWindow;  // w < nwin: no wrap
        if (a > sh->best.load(std::memory_order_relaxed)) return;  // so is every later window
        const uint64_t b = hi - a < kFindWindow - 1 ? hi : a + (kFindWindow - 1);
        walk_chunk(mp, a, b, compress, [&](uint64_t k, uint64_t n) {
            if (k >= target) return false;
            uint64_t cur = sh->best.load(std::memory_order_relaxed);
            while (n < cur && !sh->best.compare_exchange_weak(cur, n, std::memory_order_relaxed)) {}
            sh->hit.store(true, std::memory_order_relaxed);
            return true;  // ascending: the window's first hit is its lowest
        });
    }
}

// hm_find_k_cpu's shared state.  Threads take ascending windows of kFindWindow
// nonces from `next`, as find_worker does, and keep a window's hits (the first
// k at most: a window cannot give the answer more) until its end; then, under
// `mu`, they join `recs`, which is cut back to its k lowest nonces whenever it
// holds more.  Once `recs` holds k, `bound` drops to the largest nonce among
// them: k hits at or below it are known, so windows that start above it are
// not begun and a window's walk ends at its first nonce above it.  `bound`
// only decreases, and a window is left out only above a value already in it:
// every hit at or below the k-th lowest lies in a window that was walked to
// that hit, whatever the order the threads ran in.
struct FindKShared {
    std::atomic<uint64_t> next{0};
    std::atomic<uint64_t> bound{~0ull};
    std::mutex mu;
    std::vector<hm_result> recs;  // under mu
    bool failed = false;          // under mu: out of memory
};

void find_k_worker(const MsgPlan& mp, uint64_t lo, uint64_t hi, uint64_t target, size_t k,
                   uint64_t nwin, CompressFn compress, FindKShared* sh) {
    const auto by_nonce = [](const hm_result& x, const hm_result& y) { return x.nonce < y.nonce; };
    std::vector<hm_result> mine;
    for (;;) {
        const uint64_t w = sh->next.fetch_add(1, std::memory_order_relaxed);
        if (w >= nwin) return;
        const uint64_t a = lo + w * kFindWindow;  // w < nwin: no wrap
        const uint64_t bound = sh->bound.load(std::memory_order_relaxed);
        if (a > bound) return;  // so is every later window
        const uint64_t b = hi - a < kFindWindow - 1 ? hi : a + (kFindWindow - 1);
        try {
            mine.clear();
            walk_chunk(mp, a, b, compress, [&](uint64_t key, uint64_t n) {
                if (key >= target) return false;
                if (n > bound) return true;  // ascending: so is the rest of the window
                mine.push_back(hm_result{key, n});
                return mine.size() == k;
            });
            if (mine.empty()) continue;
            std::lock_guard<std::mutex> g(sh->mu);
            sh->recs.insert(sh->recs.end(), mine.begin(), mine.end());
            if (sh->recs.size() >= k) {
                std::nth_element(sh->recs.begin(), sh->recs.begin() + (k - 1), sh->recs.end(),
                                 by_nonce);
                sh->recs.resize(k);
                // under mu the k-th lowest nonce held only decreases
                sh->bound.store(sh->recs[k - 1].nonce, std::memory_order_relaxed);
            }
        } catch (...) {
            std::lock_guard<std::mutex> g(sh->mu);
            sh->failed = true;
            return;
        }
    }
}

// hm_collect_cpu's share of one thread: the records of its contiguous chunk,
// ascending (the walk's order), and their count.  Once the chunk alone holds
// more than `cap` hits the call has overflowed and its records will not be
// returned: the thread stops storing and keeps counting.
struct CollectPart {
    std::vector<hm_result> recs;
    uint64_t count = 0;
    bool failed = false;  // out of memory
};

void collect_chunk(const MsgPlan& mp, uint64_t a, uint64_t b, uint64_t target, size_t cap,
                   CompressFn compress, CollectPart* out) {
    try {
        walk_chunk(mp, a, b, compress, [&](uint64_t k, uint64_t n) {
            if (k < target && ++out->count <= cap) out->recs.push_back(hm_result{k, n});
            return false;
        });
    } catch (...) {
        out->failed = true;
    }
}

// hm_scan_k_cpu's share of one thread: the k lowest (key, nonce) records of its
// contiguous chunk, ascending.  A full list is tested against its k-th record
// first -- one compare per nonce, as the running minimum's -- and only a record
// lexicographically below it is inserted.
struct LowK {
    hm_result rec[HM_SCAN_K_MAX] = {};
    uint32_t cnt = 0;
    void take(uint32_t k, uint64_t key, uint64_t n) {
        if (cnt == k) {
            const hm_result& last = rec[k - 1];
            if (key > last.hash || (key == last.hash && n > last.nonce)) return;
        }
        uint32_t i = cnt < k ? cnt++ : k - 1;
        for (; i > 0 && (key < rec[i - 1].hash || (key == rec[i - 1].hash && n < rec[i - 1].nonce));
             --i)
            rec[i] = rec[i - 1];
        rec[i] = hm_result{key, n};
    }
};

void scan_k_chunk(const MsgPlan& mp, uint64_t a, uint64_t b, uint32_t k, CompressFn compress,
                  LowK* out) {
    LowK low;
    walk_chunk(mp, a, b, compress, [&](uint64_t key, uint64_t n) {
        low.take(k, key, n);
        return false;
    });
    *out = low;
}

// Hash(msg, n) of one nonce from the midstate: the tail bytes of walk_chunk,
// built for n alone, and one or two compressions.
uint64_t hash_from_mid(const MsgPlan& mp, uint64_t n, CompressFn compress) {
    uint8_t tail[128];
    const uint32_t nb = build_tail(mp, n, digits_u64(n), tail);
    uint32_t s[8], o[8];
    if (nb == 2) compress(mp.mid, tail, s);
    else memcpy(s, mp.mid, sizeof s);
    compress(s, tail + 64 * (nb - 1), o);
    return ((uint64_t)o[0] << 32) | o[1];
}

// hm_verify_cpu's share of one thread: the bad indices of its contiguous part
// of the list, ascending, and their count; like CollectPart, it stops storing
// once the part alone holds more than `cap` and keeps counting.
struct VerifyPart {
    std::vector<uint64_t> idx;
    uint64_t count = 0;
    bool failed = false;  // out of memory
};

void hash_part(const MsgPlan& mp, const uint64_t* nonces, size_t a, size_t b, CompressFn compress,
               uint64_t* hashes) {
    for (size_t i = a; i < b; ++i) hashes[i] = hash_from_mid(mp, nonces[i], compress);
}

void verify_part(const MsgPlan& mp, const hm_result* recs, size_t a, size_t b, uint64_t target,
                 size_t cap, CompressFn compress, VerifyPart* out) {
    try {
        for (size_t i = a; i < b; ++i) {
            const bool bad = recs[i].hash >= target ||
                             recs[i].hash != hash_from_mid(mp, recs[i].nonce, compress);
            if (bad && ++out->count <= cap) out->idx.push_back(i);
        }
    } catch (...) {
        out->failed = true;
    }
}

// hm_verify_many_cpu's share of one thread: positions [a, b) of the flattened
// record sequence (start[i]: request i's first position).  Per request it
// touches, the bad count of its part of that request, in order; the bad
// (request, index) pairs ascending, stored as VerifyPart stores its indices.
struct VerifyManyPart {
    std::vector<std::pair<size_t, uint64_t>> counts;  // (request, bad records of it in this part)
    std::vector<hm_bad_ref> refs;
    uint64_t count = 0;
    bool failed = false;  // out of memory
};

void verify_many_part(const hm_verify_request* reqs, const std::vector<MsgPlan>& plans,
                      const std::vector<uint64_t>& start, size_t a, size_t b, size_t cap,
                      CompressFn compress, VerifyManyPart* out) {
    try {
        size_t r = (size_t)(std::upper_bound(start.begin(), start.end(), (uint64_t)a) -
                            start.begin()) - 1;
        size_t pos = a;
        while (pos < b) {
            while (start[r + 1] <= pos) ++r;  // past requests without records too
            const size_t end = std::min<size_t>((size_t)start[r + 1], b);
            const hm_verify_request& q = reqs[r];
            uint64_t bad_here = 0;
            for (size_t i = pos - (size_t)start[r]; i < end - (size_t)start[r]; ++i) {
                const bool bad = q.recs[i].hash >= q.target ||
                                 q.recs[i].hash != hash_from_mid(plans[r], q.recs[i].nonce, compress);
                if (!bad) continue;
                ++bad_here;
                if (++out->count <= cap) out->refs.push_back(hm_bad_ref{r, i});
            }
            out->counts.emplace_back(r, bad_here);
            pos = end;
        }
    } catch (...) {
        out->failed = true;
    }
}

// Default thread count: the CPUs this process may run on.  A GPU box's
// per-GPU share is an affinity set inside a machine whose
// hardware_concurrency() counts every CPU, many times more.
unsigned default_threads() {
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) {
        const int c = CPU_COUNT(&set);
        if (c > 0) return (unsigned)c;
    }
    return std::max(1u, std::thread::hardware_concurrency());
}

// Run work(t, a, b) over [0, n) cut into contiguous, near-equal parts, one
// thread each (the last part on the calling thread); lists below 1024
// elements per thread use fewer.  prepare(parts) runs first, so the caller
// can size its per-part state.
template <typename Prepare, typename Work>
int over_list(size_t n, int threads, Prepare&& prepare, Work&& work) {
    unsigned nt = threads > 0 ? (unsigned)threads : default_threads();
    nt = std::min(nt, 1024u);
    if (n < (size_t)nt * 1024) nt = (unsigned)std::max<size_t>(1, n / 1024);
    prepare(nt);
    std::vector<std::thread> pool;
    pool.reserve(nt);
    const size_t per = n / nt, extra = n % nt;
    size_t start = 0;
    int rc = HM_OK;
    for (unsigned t = 0; t < nt; ++t) {
        const size_t a = start, b = start + per + (t < extra ? 1 : 0);
        start = b;
        if (t + 1 == nt) {
            work(t, a, b);  // the calling thread
            break;
        }
        try {
            pool.emplace_back(work, t, a, b);
        } catch (...) {  // no thread: join the started ones before failing
            rc = HM_ERR_INTERNAL;
            break;
        }
    }
    for (auto& th : pool) th.join();
    return rc;
}

// The same over the nonces of [lo, hi] (lo <= hi; up to 2^64 of them, so the
// count is 128-bit): work(t, a, b) over the inclusive [a, b], contiguous,
// near-equal and ascending in t; ranges below 4096 nonces per thread use fewer.
template <typename Prepare, typename Work>
int over_range(uint64_t lo, uint64_t hi, int threads, Prepare&& prepare, Work&& work) {
    typedef unsigned __int128 u128;
    const u128 count = (u128)(hi - lo) + 1;
    unsigned n = threads > 0 ? (unsigned)threads : default_threads();
    n = std::min(n, 1024u);
    if (count < (u128)n * 4096) n = (unsigned)std::max<u128>(1, count / 4096);
    prepare(n);
    std::vector<std::thread> pool;
    pool.reserve(n);
    const u128 per = count / n, extra = count % n;
    u128 start = 0;
    int rc = HM_OK;
    for (unsigned t = 0; t < n; ++t) {
        const u128 len_t = per + (t < extra ? 1 : 0);
        const uint64_t a = lo + (uint64_t)start, b = lo + (uint64_t)(start + len_t - 1);
        start += len_t;
        if (t + 1 == n) {
            work(t, a, b);  // the calling thread
            break;
        }
        try {
            pool.emplace_back(work, t, a, b);
        } catch (...) {  // no thread: join the started ones before failing
            rc = HM_ERR_INTERNAL;
            break;
        }
    }
    for (auto& th : pool) th.join();
    return rc;
}

// hm_find_cpu's and hm_find_k_cpu's pool over the (hi - lo) / kFindWindow + 1
// <= 2^50 windows of [lo, hi]: worker(nwin) on at most one thread per window,
// the last on the calling thread.  The workers share the windows, so threads
// that fail to start are made up for by the started ones and the caller.
template <typename Worker>
void over_windows(uint64_t lo, uint64_t hi, int threads, Worker&& worker) {
    const uint64_t nwin = (hi - lo) / kFindWindow + 1;
    unsigned n = threads > 0 ? (unsigned)threads : default_threads();
    n = (unsigned)std::min<uint64_t>(std::min(n, 1024u), nwin);
    std::vector<std::thread> pool;
    pool.reserve(n);
    for (unsigned t = 0; t + 1 < n; ++t) {
        try {
            pool.emplace_back(worker, nwin);
        } catch (...) {
            break;
        }
    }
    worker(nwin);  // the calling thread
    for (auto& th : pool) th.join();
}

}  // namespace
}  // namespace hm

extern "C" int hm_scan_cpu(const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi, int threads,
                           hm_result* out) {
    using namespace hm;
    if (!out || (!msg && len)) return HM_ERR_INVALID;
    return guarded([&] {
        if (lo > hi) {
            *out = hm_result{~0ull, 0};
            return HM_OK;
        }
        const MsgPlan mp = plan_message(msg_or_empty(msg, len));
        const CompressFn compress = pick_compress();
        std::vector<Best> part;
        const int rc = over_range(
            lo, hi, threads, [&](unsigned parts) { part.resize(parts); },
            [&](unsigned t, uint64_t a, uint64_t b) { scan_chunk(mp, a, b, compress, &part[t]); });
        if (rc) return rc;
        Best best;
        for (const Best& p : part) best.take(p.key, p.nonce);
        *out = hm_result{best.key, best.nonce};
        return HM_OK;
    });
}

extern "C" int hm_find_cpu(const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
                           uint64_t target, int threads, hm_result* out, int* found) {
    using namespace hm;
    if (!out || !found || (!msg && len)) return HM_ERR_INVALID;
    return guarded([&] {
        if (lo > hi || target == 0) {
            *out = hm_result{~0ull, 0};
            *found = 0;
            return HM_OK;
        }
        const Msg m = msg_or_empty(msg, len);
        const MsgPlan mp = plan_message(m);
        const CompressFn compress = pick_compress();
        FindShared sh;
        over_windows(lo, hi, threads, [&](uint64_t nwin) {
            find_worker(mp, lo, hi, target, nwin, compress, &sh);
        });
        if (sh.hit.load()) {
            const uint64_t nn = sh.best.load();
            *out = hm_result{host_hash(m.p, m.len, nn), nn};
            *found = 1;
        } else {
            *out = hm_result{~0ull, 0};
            *found = 0;
        }
        return HM_OK;
    });
}

extern "C" int hm_find_k_cpu(const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
                             uint64_t target, size_t k, int threads, hm_result* out, size_t* n) {
    using namespace hm;
    if (!out || !n || (!msg && len) || k == 0 || k > HM_FIND_K_MAX) return HM_ERR_INVALID;
    return guarded([&] {
        if (lo > hi || target == 0) {
            *n = 0;
            return HM_OK;
        }
        const MsgPlan mp = plan_message(msg_or_empty(msg, len));
        const CompressFn compress = pick_compress();
        FindKShared sh;
        over_windows(lo, hi, threads, [&](uint64_t nwin) {
            find_k_worker(mp, lo, hi, target, k, nwin, compress, &sh);
        });
        if (sh.failed) return HM_ERR_NOMEM;
        std::sort(sh.recs.begin(), sh.recs.end(),
                  [](const hm_result& x, const hm_result& y) { return x.nonce < y.nonce; });
        if (!sh.recs.empty()) memcpy(out, sh.recs.data(), sh.recs.size() * sizeof(hm_result));
        *n = sh.recs.size();
        return HM_OK;
    });
}

// hm_find_many's answers on the host (ABI 1.13): hm_find_cpu request by
// request; all n outputs are written, or none.
extern "C" int hm_find_many_cpu(const hm_find_request* reqs, int n, int threads, hm_result* outs,
                                int* found) {
    if (n < 0 || (n > 0 && (!reqs || !outs || !found))) return HM_ERR_INVALID;
    for (int r = 0; r < n; ++r)
        if (!reqs[r].msg && reqs[r].len) return HM_ERR_INVALID;
    return hm::guarded([&] {
        std::vector<hm_result> res((size_t)n);
        std::vector<int> hit((size_t)n);
        for (int r = 0; r < n; ++r) {
            const hm_find_request& q = reqs[r];
            const int rc = hm_find_cpu(q.msg, q.msg ? q.len : 0, q.lo, q.hi, q.target, threads,
                                       &res[r], &hit[r]);
            if (rc) return rc;
        }
        for (int r = 0; r < n; ++r) {
            outs[r] = res[r];
            found[r] = hit[r];
        }
        return HM_OK;
    });
}

// hm_find_k_many's answers on the host (ABI 1.17): hm_find_k_cpu request by
// request; all outputs are written, or none.
extern "C" int hm_find_k_many_cpu(const hm_find_k_request* reqs, int n, int threads,
                                  hm_result* out, size_t* counts) {
    if (n < 0 || (n > 0 && (!reqs || !out || !counts))) return HM_ERR_INVALID;
    for (int r = 0; r < n; ++r)
        if ((!reqs[r].msg && reqs[r].len) || reqs[r].k == 0 || reqs[r].k > HM_FIND_K_MAX)
            return HM_ERR_INVALID;
    return hm::guarded([&] {
        std::vector<std::vector<hm_result>> res((size_t)n);
        for (int r = 0; r < n; ++r) {
            const hm_find_k_request& q = reqs[r];
            // one buffer of k records at a time: what is kept is the hits
            std::vector<hm_result> buf(q.k);
            size_t got = 0;
            const int rc = hm_find_k_cpu(q.msg, q.msg ? q.len : 0, q.lo, q.hi, q.target, q.k,
                                         threads, buf.data(), &got);
            if (rc) return rc;
            res[r].assign(buf.begin(), buf.begin() + got);
        }
        size_t off = 0;
        for (int r = 0; r < n; ++r) {
            if (!res[r].empty())
                memcpy(out + off, res[r].data(), res[r].size() * sizeof(hm_result));
            counts[r] = res[r].size();
            off += reqs[r].k;
        }
        return HM_OK;
    });
}

extern "C" int hm_collect_cpu(const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi,
                              uint64_t target, int threads, hm_result* out, size_t cap,
                              uint64_t* total) {
    using namespace hm;
    if (!total || (!msg && len) || cap > HM_COLLECT_CAP_MAX || (cap && !out))
        return HM_ERR_INVALID;
    return guarded([&] {
        if (lo > hi || target == 0) {
            *total = 0;
            return HM_OK;
        }
        const MsgPlan mp = plan_message(msg_or_empty(msg, len));
        const CompressFn compress = pick_compress();
        // contiguous, near-equal chunks in ascending order, as hm_scan_cpu's
        std::vector<CollectPart> part;
        const int rc = over_range(
            lo, hi, threads, [&](unsigned parts) { part.resize(parts); },
            [&](unsigned t, uint64_t a, uint64_t b) {
                collect_chunk(mp, a, b, target, cap, compress, &part[t]);
            });
        if (rc) return rc;
        uint64_t sum = 0;
        for (const CollectPart& p : part) {
            if (p.failed) return HM_ERR_NOMEM;
            sum += p.count;  // <= hi - lo + 1; 2^64 hits of [0, 2^64-1] are beyond any run
        }
        if (sum <= cap) {
            // the chunks ascend and each is ascending: so is the concatenation
            size_t at = 0;
            for (const CollectPart& p : part) {
                if (!p.recs.empty()) memcpy(out + at, p.recs.data(), p.recs.size() * sizeof(hm_result));
                at += p.recs.size();
            }
        }
        *total = sum;
        return HM_OK;
    });
}

extern "C" int hm_scan_k_cpu(const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi, uint32_t k,
                             int threads, hm_result* out, size_t* n) {
    using namespace hm;
    if (!out || !n || (!msg && len) || k == 0 || k > HM_SCAN_K_MAX) return HM_ERR_INVALID;
    return guarded([&] {
        if (lo > hi) {
            *n = 0;
            return HM_OK;
        }
        const MsgPlan mp = plan_message(msg_or_empty(msg, len));
        const CompressFn compress = pick_compress();
        // contiguous, near-equal chunks, as hm_scan_cpu's; the k lowest of the
        // chunks' lists are the k lowest of the range
        std::vector<LowK> part;
        const int rc = over_range(
            lo, hi, threads, [&](unsigned parts) { part.resize(parts); },
            [&](unsigned t, uint64_t a, uint64_t b) {
                scan_k_chunk(mp, a, b, k, compress, &part[t]);
            });
        if (rc) return rc;
        LowK all;
        for (const LowK& p : part)
            for (uint32_t i = 0; i < p.cnt; ++i) all.take(k, p.rec[i].hash, p.rec[i].nonce);
        // nothing at or beyond out[*n] is touched
        memcpy(out, all.rec, all.cnt * sizeof(hm_result));
        *n = all.cnt;
        return HM_OK;
    });
}

extern "C" int hm_collect_many_cpu(const hm_collect_request* reqs, int n, int threads,
                                   uint64_t* totals, hm_result* out, size_t cap,
                                   uint64_t* total) {
    if (n < 0 || (n > 0 && (!reqs || !totals)) || !total || cap > HM_COLLECT_CAP_MAX ||
        (cap && !out))
        return HM_ERR_INVALID;
    for (int r = 0; r < n; ++r)
        if (!reqs[r].msg && reqs[r].len) return HM_ERR_INVALID;
    return hm::guarded([&] {
        // request-major: request r's records go behind those of the requests
        // before it, into what is left of `cap`; once one does not fit the call
        // has overflowed and the rest are counts
        std::vector<uint64_t> per((size_t)n, 0);
        std::vector<hm_result> all(cap);
        uint64_t sum = 0;
        for (int r = 0; r < n; ++r) {
            const hm_collect_request& q = reqs[r];
            const size_t room = sum <= cap ? cap - (size_t)sum : 0;
            const int rc = hm_collect_cpu(q.msg, q.msg ? q.len : 0, q.lo, q.hi, q.target, threads,
                                          room ? all.data() + sum : nullptr, room, &per[r]);
            if (rc) return rc;
            if (sum + per[r] < sum) return HM_ERR_INTERNAL;
            sum += per[r];
        }
        // all outputs from here on, none before
        for (int r = 0; r < n; ++r) totals[r] = per[r];
        if (sum <= cap && sum) memcpy(out, all.data(), (size_t)sum * sizeof(hm_result));
        *total = sum;
        return HM_OK;
    });
}

extern "C" int hm_hash_many_cpu(const uint8_t* msg, size_t len, const uint64_t* nonces, size_t n,
                                int threads, uint64_t* hashes) {
    using namespace hm;
    if ((!msg && len) || (n && (!nonces || !hashes))) return HM_ERR_INVALID;
    return guarded([&] {
        if (n == 0) return HM_OK;
        const MsgPlan mp = plan_message(msg_or_empty(msg, len));
        const CompressFn compress = pick_compress();
        // every element is written by exactly one thread; a failed start of a
        // thread leaves a prefix written, so the answer goes through a copy
        std::vector<uint64_t> out(n);
        const int rc = over_list(
            n, threads, [](unsigned) {},
            [&](unsigned, size_t a, size_t b) { hash_part(mp, nonces, a, b, compress, out.data()); });
        if (rc) return rc;
        memcpy(hashes, out.data(), n * sizeof(uint64_t));
        return HM_OK;
    });
}

extern "C" int hm_verify_cpu(const uint8_t* msg, size_t len, const hm_result* recs, size_t n,
                             uint64_t target, int threads, uint64_t* bad_idx, size_t cap,
                             uint64_t* bad) {
    using namespace hm;
    if (!bad || (!msg && len) || (n && !recs) || cap > HM_VERIFY_CAP_MAX || (cap && !bad_idx))
        return HM_ERR_INVALID;
    return guarded([&] {
        if (n == 0) {
            *bad = 0;
            return HM_OK;
        }
        const MsgPlan mp = plan_message(msg_or_empty(msg, len));
        const CompressFn compress = pick_compress();
        std::vector<VerifyPart> part;
        const int rc = over_list(
            n, threads, [&](unsigned parts) { part.resize(parts); },
            [&](unsigned t, size_t a, size_t b) {
                verify_part(mp, recs, a, b, target, cap, compress, &part[t]);
            });
        if (rc) return rc;
        uint64_t sum = 0;
        for (const VerifyPart& p : part) {
            if (p.failed) return HM_ERR_NOMEM;
            sum += p.count;  // <= n
        }
        if (sum <= cap) {
            // the parts ascend and each is ascending: so is the concatenation
            size_t at = 0;
            for (const VerifyPart& p : part) {
                if (!p.idx.empty()) memcpy(bad_idx + at, p.idx.data(), p.idx.size() * sizeof(uint64_t));
                at += p.idx.size();
            }
        }
        *bad = sum;
        return HM_OK;
    });
}

extern "C" int hm_verify_many_cpu(const hm_verify_request* reqs, int nreq, int threads,
                                  uint64_t* bad_per_req, hm_bad_ref* refs, size_t cap,
                                  uint64_t* bad) {
    using namespace hm;
    if (nreq < 0 || (nreq > 0 && (!reqs || !bad_per_req)) || !bad || cap > HM_VERIFY_CAP_MAX ||
        (cap && !refs))
        return HM_ERR_INVALID;
    for (int r = 0; r < nreq; ++r)
        if ((!reqs[r].msg && reqs[r].len) || (!reqs[r].recs && reqs[r].n)) return HM_ERR_INVALID;
    return guarded([&] {
        // the flattened sequence: request i holds positions [start[i], start[i + 1])
        std::vector<uint64_t> start((size_t)nreq + 1, 0);
        for (int i = 0; i < nreq; ++i) {
            if (reqs[i].n > SIZE_MAX - start[i]) return HM_ERR_INVALID;
            start[i + 1] = start[i] + reqs[i].n;
        }
        const size_t total = (size_t)start[nreq];
        std::vector<uint64_t> per((size_t)nreq, 0);
        std::vector<VerifyManyPart> part;
        uint64_t sum = 0;
        if (total > 0) {
            std::vector<MsgPlan> plans((size_t)nreq);
            for (int i = 0; i < nreq; ++i)
                if (reqs[i].n) plans[i] = plan_message(msg_or_empty(reqs[i].msg, reqs[i].len));
            const CompressFn compress = pick_compress();
            const int rc = over_list(
                total, threads, [&](unsigned parts) { part.resize(parts); },
                [&](unsigned t, size_t a, size_t b) {
                    verify_many_part(reqs, plans, start, a, b, cap, compress, &part[t]);
                });
            if (rc) return rc;
            for (const VerifyManyPart& p : part) {
                if (p.failed) return HM_ERR_NOMEM;
                for (const auto& c : p.counts) per[c.first] += c.second;
                sum += p.count;  // <= total
            }
        }
        // all outputs from here on, none before
        for (int i = 0; i < nreq; ++i) bad_per_req[i] = per[i];
        if (sum <= cap) {
            // the parts ascend and each is ascending: so is the concatenation
            size_t at = 0;
            for (const VerifyManyPart& p : part) {
                if (!p.refs.empty())
                    memcpy(refs + at, p.refs.data(), p.refs.size() * sizeof(hm_bad_ref));
                at += p.refs.size();
            }
        }
        *bad = sum;
        return HM_OK;
    });
}
